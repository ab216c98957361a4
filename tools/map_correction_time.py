"""Times the map step after a pose-graph update that moved poses: the rebuild (a fresh volume, every frame integrated again: the
reference's update_map_after_pg and run_slam_loop's default) against the in-place correction (plan_map_correction + TSDF.apply_batch:
the moved frames taken out and put back), on a map of 256 synthetic 640x480 frames with the reference's TSDF parameters (1 mm voxels,
0.1 m truncation, 32^3 units, stride 8) and 8 / 32 / 128 of the frames moved by about 2 mm / 2 mrad.  HIP events around the map step
only (for the rebuild that includes making the fresh volume, as in the loop), two warm-up runs, then the median of seven; the
correction alternates between the two pose sets so that every run moves the same frames.  Reported, not asserted: the comparison is
with the rebuild path of the same commit on the same machine; there is no target.

    python tools/map_correction_time.py [--out profiles/map_correction_time.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bodyslam_amd import _lib  # noqa: E402
from bodyslam_amd.map_correction import plan_map_correction  # noqa: E402
from bodyslam_amd.tsdf import BATCH_MAX, TSDF, PinholeCameraIntrinsic, RGBDImage  # noqa: E402

H, W = 480, 640
K = (383.1901395, 383.1901395, 276.4727783203125, 124.3335933685303)          # slam.py:25-28
N = 256
MOVED = (8, 32, 128)


def sequence(dev):
    """an endoscopic working distance, the camera drifting 2 mm sideways and 1 mm forward per frame (tools/probes/tsdf_full_size.py)"""
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rng = np.random.default_rng(0)
    color = torch.from_numpy(rng.integers(0, 256, size=(8, H, W, 3)).astype(np.uint8)).to(dev)
    depth = torch.from_numpy(np.stack([(0.12 + 0.03 * np.sin(u / 90.0 + 0.3 * f) * np.cos(v / 70.0)).astype(np.float32) for f in range(N)])).to(dev)
    poses = []
    for f in range(N):
        pose = np.eye(4)
        pose[:3, 3] = (0.002 * f, 0.0, 0.001 * f)
        poses.append(np.linalg.inv(pose))
    return [RGBDImage(color[f % 8], depth[f]) for f in range(N)], poses


def moved_poses(poses, k, seed=1):
    """every (N / k)-th frame moved by a small rigid motion: ~2 mrad about a random axis, ~2 mm"""
    rng = np.random.default_rng(seed)
    out = [p.copy() for p in poses]
    for j in range(0, N, N // k):
        w = rng.normal(size=3) * 2e-3
        Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        D = np.eye(4)
        D[:3, :3] = np.eye(3) + Kx + 0.5 * Kx @ Kx
        D[:3, 3] = rng.normal(size=3) * 2e-3
        out[j] = D @ poses[j]
    return out


def timed(fn, reps=7, warm=2):
    ms = []
    for r in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(r)
        e1.record()
        e1.synchronize()
        if r >= warm:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_correction_time.txt"))
    a = ap.parse_args()
    _lib.init(0)
    dev = torch.device("cuda", 0)
    intr = PinholeCameraIntrinsic(W, H, *K)
    rgbds, poses = sequence(dev)

    def build(extr, like=None):
        t = TSDF()
        if like is not None:
            t.reserve(like.n_units_known())
        for j0 in range(0, N, BATCH_MAX):
            t.build_3D_map_batch(rgbds[j0:j0 + BATCH_MAX], intr, extr[j0:j0 + BATCH_MAX])
        t.sync()
        return t

    tsdf = build(poses)
    lines = [f"The map step after a pose-graph update on {torch.cuda.get_device_name(0)}: {N} frames of {W}x{H}, TSDF 1 mm / 0.1 m / 32^3 / stride 8, "
             f"{tsdf.n_units} units ({tsdf.n_units * tsdf.unit_floats * 4 / 1e9:.1f} GB of voxels); HIP events around the map step, median of 7, warmed"]
    ledger = [p.copy() for p in poses]                              # the extrinsic every frame is in `tsdf` with

    def correct_to(new):
        plan = plan_map_correction(ledger, new, N - 1, mode="incremental")
        assert plan.decision == "correct" and not plan.added
        for (r0, r1) in plan.groups:
            recs = plan.records[r0:r1]
            tsdf.apply_batch([rgbds[j] for j, _, _ in recs], intr, [E for _, E, _ in recs], [rm for _, _, rm in recs])
        tsdf.sync()
        for j in plan.moved:
            ledger[j] = new[j]
        return plan

    for k in MOVED:
        sets = (poses, moved_poses(poses, k))
        state = {"fresh": None, "records": 0}

        def rebuild(r):
            state["fresh"] = None                                   # (the loop drops the old volume when the rebuild replaces it)
            state["fresh"] = build(sets[1], like=tsdf)

        def correct(r):
            plan = correct_to(sets[(r + 1) % 2])                    # there and back again: every run moves the same k frames
            assert len(plan.moved) == k
            state["records"] = len(plan.records)

        rebuild_ms = timed(rebuild)
        state["fresh"] = None
        correct_ms = timed(correct)
        correct_to(poses)                                           # the map as it was, for the next size
        lines.append(f"{k:3d} of {N} frames moved: rebuild {rebuild_ms:9.2f} ms ({N} integrations), correct {correct_ms:9.2f} ms "
                     f"({state['records']} records) = {rebuild_ms / correct_ms:6.2f} x")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
