"""Times the voxel down-sampling on the extract_pcd cloud of the 256-frame 640x480 map that tools/map_correction_time.py builds (the
reference's TSDF parameters), with its colours and normals, at h = 0.005 m and h = 0.05 m: the whole voxel_down_sample call (bounds and its
read-back, the table fills, the four launches, the scan, the read-backs of m and of the status word), its four kernels one by one, and
beside it what a user composes from torch today -- the same fp64 voxel keys, torch.unique(key, return_inverse=True) and an fp64
index_add_ of the nine columns and the counts, which sorts every point and sums in floating-point atomics.  HIP events, one warm-up, then
three passes; every pass is printed.  Reported, not asserted.

    python tools/voxel_down_sample_time.py [--out profiles/voxel_down_sample_time.txt] [--label TEXT]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_correction_time as M  # noqa: E402
from bodyslam_amd import _lib as L  # noqa: E402
from bodyslam_amd import pointcloud as PC  # noqa: E402
from bodyslam_amd.tsdf import BATCH_MAX, TSDF, PinholeCameraIntrinsic  # noqa: E402

PASSES = 3
SIZES = (0.005, 0.05)


def passes(fn, before=None):
    """one warm-up, then PASSES timed runs -> their times in ms; `before` runs outside the events"""
    ms = []
    for r in range(1 + PASSES):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if r >= 1:
            ms.append(e0.elapsed_time(e1))
    return ms


def show(ms, scale=1.0, unit="ms"):
    return f"{float(np.median(ms)) * scale:9.3f} {unit} (passes: " + ", ".join(f"{v * scale:.3f}" for v in ms) + ")"


def torch_composition(pts, attrs, origin, h):
    """what a user writes today -> (points, attributes, counts) per unique key, rows in key order"""
    v = torch.floor((pts.to(torch.float64) - origin) / h).to(torch.int64)
    key = (v[:, 2] << 42) | (v[:, 1] << 21) | v[:, 0]
    uniq, inverse = torch.unique(key, return_inverse=True)
    m = uniq.numel()
    sums = torch.zeros(m, 3 + attrs.shape[1], dtype=torch.float64, device=pts.device)
    sums.index_add_(0, inverse, torch.cat([pts, attrs], 1).to(torch.float64))
    counts = torch.zeros(m, dtype=torch.float64, device=pts.device)
    counts.index_add_(0, inverse, torch.ones(pts.shape[0], dtype=torch.float64, device=pts.device))
    mean = (sums / counts[:, None]).to(torch.float32)
    return mean[:, :3], mean[:, 3:], counts


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_down_sample_time.txt"))
    ap.add_argument("--label", default="", help="a line put in front of the report")
    a = ap.parse_args()
    L.init(0)
    dev = torch.device("cuda", 0)
    intr = PinholeCameraIntrinsic(M.W, M.H, *M.K)
    rgbds, poses = M.sequence(dev)
    tsdf = TSDF()
    for j0 in range(0, M.N, BATCH_MAX):
        tsdf.build_3D_map_batch(rgbds[j0:j0 + BATCH_MAX], intr, poses[j0:j0 + BATCH_MAX])
    tsdf.sync()
    pcd = tsdf.extract_pcd(host=False)
    cloud, colors, normals = pcd.points.contiguous(), pcd.colors.contiguous(), pcd.normals.contiguous()
    n = int(cloud.shape[0])
    del rgbds, tsdf
    raw = torch.empty(8, dtype=torch.int32, device=dev)
    L.pc_bounds(cloud, raw)
    lo, hi, n_finite = PC._decode_bounds(raw.cpu().numpy().view(np.uint32))
    lines = ([a.label] if a.label else []) + [
        f"voxel down-sampling on {torch.cuda.get_device_name(0)}: the extract_pcd cloud of {M.N} frames of {M.W}x{M.H} (TSDF 1 mm / 0.1 m / 32^3 / stride 8), "
        f"{n} points ({n_finite} finite) with colours and normals, extent {' x '.join(f'{v:.3f}' for v in (hi - lo))} m; HIP events, one warm-up, then "
        f"{PASSES} passes: the median and every pass"]
    i32 = dict(dtype=torch.int32, device=dev)
    for h in SIZES:
        state = {}

        def whole():
            state["r"] = PC.voxel_down_sample(cloud, h, colors=colors, normals=normals)

        ms_new = passes(whole)
        r = state["r"]
        m = int(r.points.shape[0])
        lines.append(f"h = {h} m: {m} voxels, largest count {int(r.counts.max())}, table of {PC.voxel_table_slots(n)} slots")
        lines.append(f"  voxel_down_sample, the whole call            {show(ms_new)}")
        origin, shift = PC.voxel_geometry(lo, hi, h)
        o_dev = torch.from_numpy(origin).to(dev)
        attrs = torch.cat([colors, normals], 1)

        def composed():
            state["t"] = torch_composition(cloud, attrs, o_dev, h)

        ms_old = passes(composed)
        lines.append(f"  torch.unique + fp64 index_add_ (today)       {show(ms_old)}  [{int(state['t'][2].numel())} voxels]")
        spread = max(max(ms_new) - min(ms_new), max(ms_old) - min(ms_old))
        verdict = "faster" if np.median(ms_new) < np.median(ms_old) - spread else "slower" if np.median(ms_new) > np.median(ms_old) + spread else \
            "the same within the spread of the passes"
        lines.append(f"  the new path is {verdict} (ratio of the medians {np.median(ms_old) / np.median(ms_new):.2f}, spread {spread:.3f} ms)")
        # the four kernels one by one, on the tensors the call builds
        slots = PC.voxel_table_slots(n)
        keys, first = torch.empty(slots, dtype=torch.int64, device=dev), torch.empty(slots, **i32)
        slot, leader, flag, row = (torch.empty(n, **i32) for _ in range(4))
        status = torch.zeros(1, **i32)

        def fill():
            keys.fill_(L.PC_VOXEL_EMPTY_KEY)
            first.fill_(L.PC_VOXEL_NO_POINT)

        ms = passes(lambda: L.pc_voxel_assign(cloud, origin, h, keys, first, slot, status), before=fill)
        lines.append(f"  bs_pc_voxel_assign                           {show(ms, 1e3, 'us')}")
        ms = passes(lambda: L.pc_voxel_flags(slot, first, leader, flag))
        lines.append(f"  bs_pc_voxel_flags                            {show(ms, 1e3, 'us')}")
        rank = torch.cumsum(flag, 0).to(torch.int32)
        assert int(rank[-1]) == m
        sums, counts, first_index = torch.empty(m, 9, dtype=torch.int64, device=dev), torch.empty(m, **i32), torch.empty(m, **i32)

        def zero():
            sums.zero_()
            counts.zero_()

        ms = passes(lambda: L.pc_voxel_accumulate(cloud, colors, normals, origin, shift, leader, rank, sums, counts, first_index, row, status), before=zero)
        lines.append(f"  bs_pc_voxel_accumulate, 9 terms              {show(ms, 1e3, 'us')}")
        out = [torch.empty(m, 3, dtype=torch.float32, device=dev) for _ in range(3)]
        ms = passes(lambda: L.pc_voxel_finish(cloud, colors, normals, sums, counts, first_index, origin, shift, False, *out))
        lines.append(f"  bs_pc_voxel_finish                           {show(ms, 1e3, 'us')}")
        assert int(status) == 0 and torch.equal(out[0], r.points) and torch.equal(counts, r.counts)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
