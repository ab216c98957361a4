"""Times loop-closure detection on the device: one LoopCloser.detect of a 640 x 480 frame against 16, 128 and 1024 stored keyframes --
feature extraction of the frame, ONE bs_orb_match_pairs and ONE bs_loop_register over all keyframes, one readback of the per-pair records
-- and add_keyframe.  HIP events around the call (the readback ends it), median of 10 after warm-up.  Reported, not asserted; there is
no earlier implementation to compare with.

    python tools/loop_closure_time.py [--out profiles/loop_closure_time.txt]

The frames are tests/_corner_scene.py's tiles rendered at 640 x 480 on _render.g's height field from eight nearby poses; the store is
filled with them in turn, so every keyframe is a revisit candidate and every pair runs its full RANSAC (the expensive case: a pair
below min_matches returns at once).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _corner_scene as S  # noqa: E402
from bodyslam_amd.loop_closure import LoopCloser  # noqa: E402

H, W = 480, 640
K = (640.0, 640.0, 320.0, 240.0)
SIZES = (16, 128, 1024)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_closure_time.txt"))
    a = ap.parse_args()
    frames = [S.render(S.translation_pose(np.array([0.0004, -0.0002, 0.0001]) * i), "field", K, H, W) for i in range(9)]
    dev = torch.device("cuda:0")
    colors = torch.from_numpy(np.stack([f[0] for f in frames])).to(dev)
    depths = torch.from_numpy(np.stack([f[1] for f in frames])).to(dev)
    lines = [f"loop-closure detection timing on {torch.cuda.get_device_name(0)} (a {W} x {H} frame; HIP events, median of 10, warmed)"]
    closer = LoopCloser(K, min_gap=1)
    tmp = LoopCloser(K)
    ms = gpu_median_ms(lambda: tmp.add_keyframe(tmp.n, colors[0], depths[0]))
    lines.append(f"add_keyframe (features + lift)    : {ms:8.3f} ms")
    n = 0
    for size in SIZES:
        while n < size:
            closer.add_keyframe(n, colors[n % 8], depths[n % 8])
            n += 1
        edges = []
        ms = gpu_median_ms(lambda: edges.append(closer.detect(100000, colors[8], depths[8])))
        r = closer.last_records
        lines.append(f"detect against {size:5d} keyframes: {ms:8.3f} ms = {1e3 * ms / size:8.1f} us per keyframe "
                     f"(matches {r['matches'].mean():.0f}, correspondences {r['correspondences'].mean():.0f}, inliers {r['inliers'].mean():.0f} per pair; "
                     f"{int((r['status'] == 1).sum())} pairs registered, {len(edges[-1])} edge returned)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
