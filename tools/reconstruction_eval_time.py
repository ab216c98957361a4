"""Times the reconstruction evaluation's pieces on the extract_pcd cloud of the 256-frame 640x480 map that tools/map_correction_time.py
builds (the reference's TSDF parameters): the index build (bounds, counts, scan, scatter: NearestNeighbours), the grid query of that cloud
against a copy moved by one voxel, the brute-force kernel on every 64th point of it, and the statistics of the distance array.  HIP
events, one warm-up run, then the median of five (brute force: of three).  Also swept, because the default cell size and the shell cap
are unmeasured choices: the query at half and at twice the default cell edge.  Reported, not asserted: there is no earlier
implementation and no target; the grid-against-brute ratio (per source point) and the points per second are what to read.

    python tools/reconstruction_eval_time.py [--out profiles/reconstruction_eval_time.txt]
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
from bodyslam_amd import _lib  # noqa: E402
from bodyslam_amd import pointcloud as PC  # noqa: E402
from bodyslam_amd.evaluation import distance_stats_record  # noqa: E402
from bodyslam_amd.tsdf import BATCH_MAX, TSDF, PinholeCameraIntrinsic  # noqa: E402


def timed(fn, reps=5, warm=1):
    ms = []
    for r in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if r >= warm:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reconstruction_eval_time.txt"))
    a = ap.parse_args()
    _lib.init(0)
    dev = torch.device("cuda", 0)
    intr = PinholeCameraIntrinsic(M.W, M.H, *M.K)
    rgbds, poses = M.sequence(dev)
    tsdf = TSDF()
    for j0 in range(0, M.N, BATCH_MAX):
        tsdf.build_3D_map_batch(rgbds[j0:j0 + BATCH_MAX], intr, poses[j0:j0 + BATCH_MAX])
    tsdf.sync()
    cloud = tsdf.extract_pcd(host=False).points
    n = int(cloud.shape[0])
    del rgbds
    moved = (cloud + torch.tensor([tsdf.voxel_length, 0.0, 0.0], device=dev)).contiguous()
    state = {}

    def build(cell=None):
        state["nn"] = PC.NearestNeighbours(moved, cell_size=cell)

    build_ms = timed(build)
    nn = state["nn"]
    h0 = nn.cell_size
    lines = [f"Reconstruction evaluation on {torch.cuda.get_device_name(0)}: the extract_pcd cloud of {M.N} frames of {M.W}x{M.H} (TSDF 1 mm / 0.1 m / "
             f"32^3 / stride 8), {n} points, against a copy moved by one voxel; HIP events, median of 5 after a warm-up",
             f"index build       {build_ms:9.2f} ms  ({n / build_ms / 1e3:8.1f} M points/s; default cell edge {h0:.6g} m, grid {nn.dims[0]} x {nn.dims[1]} x "
             f"{nn.dims[2]} = {PC.n_cells(nn.dims)} cells, shell cap {PC.SHELL_CAP})"]

    def query():
        state["d"], state["i"] = state["nn"].query(cloud)

    grid_ms = timed(query)
    dist = state["d"]
    lines.append(f"grid query        {grid_ms:9.2f} ms  ({n / grid_ms / 1e3:8.1f} M source points/s; {nn.last_fallback} sources went to the brute-force kernel)")
    sub = cloud[::64].contiguous()
    ns = int(sub.shape[0])

    def brute():
        state["bd"], state["bi"] = nn.query(sub, method="brute")

    brute_ms = timed(brute, reps=3)
    same = torch.equal(state["bd"].view(torch.int32), dist[::64].view(torch.int32)) and torch.equal(state["bi"], state["i"][::64])
    per_grid, per_brute = grid_ms / n, brute_ms / ns
    lines.append(f"brute force       {brute_ms:9.2f} ms  for every 64th source point ({ns} points, {ns * float(nn.n_finite) / brute_ms / 1e9:8.2f} T pairs/s); per "
                 f"source point grid {per_grid * 1e6:.3f} ns, brute {per_brute * 1e6:.1f} ns = {per_brute / per_grid:.0f} x; results bit-equal: {same}")
    stats_ms = timed(lambda: distance_stats_record(dist, (0.001, 0.002, 0.005)))
    rec = distance_stats_record(dist, (0.001, 0.002, 0.005))
    lines.append(f"statistics        {stats_ms:9.2f} ms  ({n / stats_ms / 1e3:8.1f} M distances/s, with the record's read-back; mean {rec[4] / rec[1]:.6e} m, median "
                 f"{rec[7]:.6e} m, max {rec[6]:.6e} m)")
    for factor in (0.5, 2.0):
        build(h0 * factor)
        ms = timed(query)
        eq = torch.equal(state["d"].view(torch.int32), dist.view(torch.int32))
        lines.append(f"grid query, cell edge x {factor}: {ms:9.2f} ms  ({PC.n_cells(state['nn'].dims)} cells; results bit-equal: {eq})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
