"""Build-machine only: tests/golden/sparse_scale.npz -- inputs and the reference's own outputs for what follows the match in its
sparse-feature path (like tools/make_trajectory_eval_golden.py; nothing on the GPU machine reads the reference).

    python tools/make_sparse_scale_golden.py --ref <reference checkout> [--out PATH] [--check]

What runs is the reference's code, BodySLAM_not_refactored/3DM/scaling_system.py: associate_depth twice with the arguments exactly as
compute_scaling_factor passes them (:129-130, the keypoint lists swapped in the second call, the matches not), calculate_displacements
(:133) and np.mean (:135).  The module imports cv2 at its top; an EMPTY stand-in module named cv2 is placed in sys.modules, which these
functions never touch -- they need from cv2 only objects with .pt, .queryIdx and .trainIdx, which are plain namespaces here.  Keypoints,
matches and depth maps are synthetic; depth maps are float64 so that the reference's arithmetic is fp64 under every numpy version.  Only
arrays go into the file.  --check compares a fresh run with the committed file instead of writing.

Cases:
  valid            depth valid everywhere
  misaligned       zeros in both depth maps that drop entries from one list only: the zip misaligns
  outside          keypoints whose int() position lies outside the depth image (and one at -0.5, which int() takes to 0: inside)
  more_prev        more keypoints in the previous frame than in the current one: the swapped index runs past the list and the bounds
                   check of associate_depth skips the match
  more_curr        the other way round
"""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "sparse_scale.npz")
H, W = 12, 16
K = (15.0, 15.5, 7.75, 5.625)


def load_reference(ref):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, os.path.join(ref, "BodySLAM_not_refactored", "3DM"))
    import scaling_system
    return scaling_system


def make_case(name, rng):
    n1, n2 = {"more_prev": (40, 25), "more_curr": (25, 40)}.get(name, (30, 30))
    pts1 = (rng.uniform(0, 1, (n1, 2)) * (W - 1, H - 1)).astype(np.float32)
    pts2 = (rng.uniform(0, 1, (n2, 2)) * (W - 1, H - 1)).astype(np.float32)
    m = min(n1, n2) - 3
    q, t = rng.permutation(n1)[:m], rng.permutation(n2)[:m]
    if name == "more_prev":
        q[:6] = np.arange(n2, n2 + 6)                # query indices past the current frame's list: skipped by the second call only
    if name == "more_curr":
        t[:6] = np.arange(n1, n1 + 6)                # train indices past the previous frame's list: skipped by the second call only
    matches = np.stack([q, t, np.sort(rng.integers(0, 80, m))], 1).astype(np.int64)
    d1 = rng.uniform(0.2, 0.6, (H, W))
    d2 = rng.uniform(0.2, 0.6, (H, W))
    if name == "misaligned":
        for k in (2, 9):                             # the previous frame's list loses entries 2 and 9
            x, y = pts1[matches[k, 0]]
            d1[int(y), int(x)] = 0.0
        x, y = pts2[matches[5, 0]]                   # the current frame's list loses entry 5 (looked up at keypoints2[queryIdx], sic)
        d2[int(y), int(x)] = 0.0
    if name == "outside":
        pts1[matches[1, 0]] = (W + 0.25, 3.0)
        pts1[matches[4, 0]] = (5.0, -1.5)
        pts1[matches[6, 0]] = (-0.5, 2.0)
        pts2[matches[3, 0]] = (2.0, H + 7.0)
    return pts1, pts2, matches, d1, d2


def run_reference(ss, pts1, pts2, matches, d1, d2):
    kp = lambda p: [types.SimpleNamespace(pt=(float(x), float(y))) for (x, y) in p]
    k1, k2 = kp(pts1), kp(pts2)
    ms = [types.SimpleNamespace(queryIdx=int(q), trainIdx=int(t), distance=float(d)) for (q, t, d) in matches]
    a_prev = ss.associate_depth(k1, k2, ms, d1)
    a_curr = ss.associate_depth(k2, k1, ms, d2)
    disp = ss.calculate_displacements(k1, k2, a_prev, a_curr, *K)
    return dict(assoc_prev=np.array([ms.index(m) for m, _ in a_prev], dtype=np.int64), assoc_curr=np.array([ms.index(m) for m, _ in a_curr], dtype=np.int64),
                displacements=np.array(disp, dtype=np.float64).reshape(-1, 3), mean=np.mean(disp, axis=0))


def build(ref):
    ss = load_reference(ref)
    out = {"K": np.array(K), "cases": np.array(["valid", "misaligned", "outside", "more_prev", "more_curr"])}
    for i, name in enumerate(out["cases"]):
        pts1, pts2, matches, d1, d2 = make_case(str(name), np.random.default_rng(100 + i))
        out.update({f"{name}/pts_prev": pts1, f"{name}/pts_curr": pts2, f"{name}/matches": matches, f"{name}/depth_prev": d1, f"{name}/depth_curr": d2})
        out.update({f"{name}/{k}": v for k, v in run_reference(ss, pts1, pts2, matches, d1, d2).items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    out = build(a.ref)
    if a.check:
        old = np.load(a.out)
        bad = [k for k in out if not np.array_equal(old[k], out[k])]
        print("differs:" if bad else "identical", bad)
        sys.exit(1 if bad else 0)
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")
    for name in out["cases"]:
        print(name, len(out[f"{name}/assoc_prev"]), len(out[f"{name}/assoc_curr"]), len(out[f"{name}/displacements"]), out[f"{name}/mean"])


if __name__ == "__main__":
    main()
