"""Times the sparse-feature scale path on the device: SparseScale.displacements_block over 64 frames of 640 x 480 (63 pairs, every
stage one launch over the block, one readback) and the pair call, per-pair microseconds beside RGBDOdometry.track_block's for the same
frames.  HIP events, median of 10 after warm-up.  Reported, not asserted.

    python tools/sparse_scale_time.py [--out profiles/sparse_scale_time.txt]

The frames are tests/_corner_scene.py's tiles rendered at 640 x 480 on _render.g's height field along a straight camera path.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _corner_scene as S  # noqa: E402
from bodyslam_amd.rgbd_odometry import RGBDOdometry  # noqa: E402
from bodyslam_amd.scaling_system import SparseScale  # noqa: E402

H, W, N = 480, 640, 64
K = (640.0, 640.0, 320.0, 240.0)


def gpu_median_ms(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_scale_time.txt"))
    a = ap.parse_args()
    frames = [S.render(S.translation_pose(np.array([0.0004, -0.0002, 0.0001]) * i), "field", K, H, W) for i in range(N)]
    dev = torch.device("cuda:0")
    colors = torch.from_numpy(np.stack([f[0] for f in frames])).to(dev)
    depths = torch.from_numpy(np.stack([f[1] for f in frames])).to(dev)
    lines = [f"sparse-feature scale path timing on {torch.cuda.get_device_name(0)} ({N} frames of {W} x {H}; HIP events, median of 10, warmed)"]
    for association in ("reference", "matched"):
        eng = SparseScale(K, association=association)
        ms = gpu_median_ms(lambda: eng.displacements_block(colors, depths))
        c = eng.last_counts
        lines.append(f"displacements_block {association:9s}: {ms:8.3f} ms for {N - 1} pairs = {1e3 * ms / (N - 1):8.1f} us per pair "
                     f"(keypoints {c[:, 0].mean():.0f}, matches {c[:, 2].mean():.0f}, pairs used {c[:, 5].mean():.0f} per pair)")
        prev, curr = (types.SimpleNamespace(color=colors[i], depth=depths[i]) for i in (0, 1))
        ms = gpu_median_ms(lambda: eng(curr, prev))
        lines.append(f"pair call           {association:9s}: {1e3 * ms:8.1f} us per pair")
    odo = RGBDOdometry(K)

    def block():
        odo.reset()
        return odo.track_block(colors, depths)

    ms = gpu_median_ms(block)
    lines.append(f"RGBDOdometry.track_block          : {ms:8.3f} ms for {N - 1} pairs = {1e3 * ms / (N - 1):8.1f} us per pair")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
