"""Build-machine only: tests/golden/trajectory_eval.npz -- inputs and the reference's own outputs for its similarity fit and its
training-time trajectory metrics (like tools/make_depth_eval_golden.py for the depth metrics; nothing on the GPU machine reads the
reference).

    python tools/make_trajectory_eval_golden.py --ref <reference checkout> [--out PATH] [--check]

What runs is the reference's code: estimate_similarity_transformation of BodySLAM_not_refactored/3DM/slam_utils.py:138-169 and
TrainingLoss.compute_scale_factor / compute_ARE_and_ATE / compute_RRE_and_RTE of MPEM/training_utils.py:473-585, imported with the
stubs SURVEY.md Appendix A lists (open3d, cv2, filterpy, torchvision) plus wandb, evo, lpips and kornia as mocks -- none of them is
touched by these functions.  The evo-based MPEM_Metrics.compute_pose_metrics cannot run here (evo is not installed); the "evo" protocol
is restated in tests/_trajectory_eval_ref.py instead.  Only arrays go into the file.  --check compares a fresh run with the committed
file instead of writing.
"""
import argparse
import os
import sys
from unittest import mock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "trajectory_eval.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _trajectory_eval_ref as TR  # noqa: E402  (only its trajectory generators: rot, random_walk, perturbed)

SIM_CASES = (("n3", 3, False), ("n50", 50, False), ("n50_reflection", 50, True), ("n5000", 5000, False))
TRAJ_CASES = (("len3", 3), ("kitti24", 24), ("len1000", 1000))
DELTAS = (1, 5)


def load_reference(ref):
    stubs = ["open3d", "open3d.core", "open3d.visualization", "cv2", "filterpy", "filterpy.kalman", "torchvision", "torchvision.transforms",
             "wandb", "evo", "evo.core", "evo.core.metrics", "evo.tools", "evo.tools.file_interface", "lpips", "kornia", "tsdf"]
    for m in stubs:
        sys.modules.setdefault(m, mock.MagicMock())
    root = os.path.join(ref, "BodySLAM_not_refactored")
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "3DM"))
    import slam_utils
    from MPEM.training_utils import TrainingLoss
    try:
        loss = TrainingLoss()
    except TypeError:
        loss = TrainingLoss.__new__(TrainingLoss)          # the three functions read nothing of self
    return slam_utils.estimate_similarity_transformation, loss


def read_kitti(path):
    rows = np.loadtxt(path, dtype=np.float64).reshape(-1, 3, 4)
    T = np.tile(np.eye(4), (len(rows), 1, 1))
    T[:, :3, :] = rows
    return T


def sim_inputs():
    """(name, source [n, 3], target [n, 3]): target = a similarity of source plus noise; the reflection case mirrors the target so that
    det(Sxy) < 0"""
    rng = np.random.default_rng(20261)
    out = []
    for name, n, reflect in SIM_CASES:
        x = rng.normal(size=(n, 3)) * [1.0, 0.6, 0.3] + [0.5, -2.0, 4.0]
        R = TR.rot(rng.normal(size=3), 0.9)
        y = 1.7 * x @ R.T + [0.2, 3.0, -1.0] + 1e-3 * rng.normal(size=(n, 3))
        if reflect:
            y = y * [1.0, 1.0, -1.0]
        # the file stores the points as float16 (size); the reference is given exactly the stored values
        out.append((name, x.astype(np.float16).astype(np.float64), y.astype(np.float16).astype(np.float64)))
    return out


def traj_inputs():
    rng = np.random.default_rng(20262)
    kitti = read_kitti(os.path.join(ROOT, "tests", "golden", "kitti_poses_24.txt"))
    out = []
    for name, n in TRAJ_CASES:
        gt = kitti if name == "kitti24" else TR.random_walk(rng, n)
        pred = TR.perturbed(rng, gt)
        if n > 100:     # stored as float32 (size); the reference is given exactly the stored values
            gt, pred = gt.astype(np.float32).astype(np.float64), pred.astype(np.float32).astype(np.float64)
        out.append((name, gt, pred))
    return out


def make(ref):
    est, loss = load_reference(ref)
    d = {"sim_names": np.array([c[0] for c in SIM_CASES]), "traj_names": np.array([c[0] for c in TRAJ_CASES]), "deltas": np.array(DELTAS)}
    for name, x, y in sim_inputs():
        R, s, t = est(x.T.copy(), y.T.copy())                # the reference takes [3, n]
        d[f"sim_{name}_source"], d[f"sim_{name}_target"] = x.astype(np.float16), y.astype(np.float16)
        d[f"sim_{name}_R"], d[f"sim_{name}_s"], d[f"sim_{name}_t"] = np.asarray(R), np.float64(s), np.asarray(t)
        d[f"sim_{name}_detSxy"] = np.float64(np.linalg.det((y - y.mean(0)).T @ (x - x.mean(0)) / len(x)))
    for name, gt, pred in traj_inputs():
        st = np.float32 if len(gt) > 100 else np.float64
        d[f"traj_{name}_gt"], d[f"traj_{name}_pred"] = gt[:, :3, :].astype(st), pred[:, :3, :].astype(st)     # the top three rows
        lists = lambda: ([g.copy() for g in gt], [p.copy() for p in pred])     # compute_ARE_and_ATE scales its predictions in place
        g, p = lists()
        d[f"traj_{name}_scale"] = np.float64(loss.compute_scale_factor(g, p))
        g, p = lists()
        ate, are = loss.compute_ARE_and_ATE(g, p)
        d[f"traj_{name}_ate"], d[f"traj_{name}_are"] = np.float64(ate), np.float64(are)
        for delta in DELTAS:
            if len(gt) <= delta:
                continue                                        # (count = 0: the reference divides by zero)
            g, p = lists()
            rre, rte = loss.compute_RRE_and_RTE(g, p, delta=delta)
            d[f"traj_{name}_rre_d{delta}"], d[f"traj_{name}_rte_d{delta}"] = np.float64(rre), np.float64(rte)
    return d


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ref", required=True, help="checkout of the reference (GuidoManni/BodySLAM)")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--check", action="store_true", help="compare with the committed file instead of writing")
    a = ap.parse_args()
    d = make(a.ref)
    if a.check:
        old = np.load(OUT)
        bad = [k for k in d if not (np.allclose(d[k], old[k], rtol=1e-12, atol=1e-15) if d[k].dtype.kind == "f" else np.array_equal(d[k], old[k]))]
        print("trajectory_eval golden:", "reproduced" if not bad else f"DIFFERS in {bad}")
        sys.exit(1 if bad else 0)
    np.savez_compressed(a.out, **d)
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes)")
    for name, _, _ in SIM_CASES:
        print(f"  sim {name:16s} s {d[f'sim_{name}_s']:.12g}  det R {np.linalg.det(d[f'sim_{name}_R']):+.6f}  det Sxy {d[f'sim_{name}_detSxy']:+.3e}")
    for name, _ in TRAJ_CASES:
        print(f"  traj {name:10s} scale {d[f'traj_{name}_scale']:.12g}  ATE {d[f'traj_{name}_ate']:.6g}  ARE {d[f'traj_{name}_are']:.6g}  " +
              "  ".join(f"d{dl}: RRE {d[f'traj_{name}_rre_d{dl}']:.6g} RTE {d[f'traj_{name}_rte_d{dl}']:.6g}"
                        for dl in DELTAS if f"traj_{name}_rre_d{dl}" in d))


if __name__ == "__main__":
    main()
