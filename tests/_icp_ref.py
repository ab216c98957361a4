"""Numpy statement of the rigid ICP registration (csrc/icp.hip, bodyslam_amd/registration.py) -- TEST INFRASTRUCTURE ONLY,
independent of the product code.

The role is Open3D's ``registration_icp(source, target, max_correspondence_distance, init, TransformationEstimationPointToPlane() /
TransformationEstimationPointToPoint(), ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration))`` and
``evaluate_registration``.  Open3D is not available: **parity unpinned**; the defaults restate its published interface, the algorithm is
the statement below.  Correspondences are `_pointcloud_ref.nn_brute`, the float32 contract of the cloud-to-cloud distances, with a
radius; everything after that is float64.

One iteration at T (4 x 4 float64, source -> target):
  point           p = float32(((a0 s0 + a1 s1) + a2 s2) + t) per row, in float64, rounded once (`_pointcloud_ref.apply_transform`)
  correspondence  the exact nearest target point of p (ties to the lower index), valid when the float32 distance d <= the radius; a
                  non-finite row has none.  count = the valid pairs, fitness = count / m over all m source rows,
                  inlier_rmse = sqrt(sum d^2 / count) with d widened to float64 (0 without a pair)
  coordinates     every sum uses coordinates relative to c = (lo + hi) / 2 in float64, the midpoint of the box of the finite target points
  point_to_plane  target normals n float32 [n, 3]; a pair whose normal is non-finite or zero is left out of the sums (it still counts for
                  fitness and rmse); r = (p - q) . n, J = [(p - c) x n, n], A = sum J J^T unweighted, b = sum J r; delta = -A^-1 b by
                  Cholesky; T <- C exp(delta) C^-1 T, C the translation by c, exp the SE(3) exponential of the left twist (omega, nu) of
                  oracle/rgbd_odometry_ref.se3_exp.  Fewer than 6 usable pairs or a non-positive pivot: "degenerate", T as it was
  point_to_point  sum (p - c), sum (q - c), sum (p - c)(q - c)^T, centred; R = V diag(1, 1, det(V U^T)) U^T from the SVD of the covariance
                  (singular values descending: the sign goes to the smallest), t = mean q - R mean p, T <- [R | t] T.  Fewer than 3 pairs
                  or a second singular value that is not positive: "degenerate".  No scale
  stopping        iteration k = 0, 1, ... logs (fitness_k, rmse_k, count_k) at the current T; for k >= 1, |fitness_k - fitness_(k-1)| <
                  relative_fitness and |rmse_k - rmse_(k-1)| < relative_rmse stop with "converged" before any update; otherwise T is
                  updated, and after max_iteration updates the run stops with "max_iteration"
  result          the fitness and rmse of the RETURNED transform, from one more correspondence pass without an update

Also here, shared by tests/test_icp_cpu.py and tests/test_icp_gpu.py: the bumpy pair and its poses.  (The height field of _render.g, the base
pair of _pointcloud_ref.py, is ill-posed for ICP -- its in-plane directions slide -- and no test may use it to assert convergence.)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pointcloud_ref as P  # noqa: E402
from _render import small_pose  # noqa: E402
from oracle.rgbd_odometry_ref import se3_exp  # noqa: E402

f32, f64 = np.float32, np.float64
N_PLANE, N_POINT = 27, 15


def centre(tgt):
    lo, hi = P.bounds(tgt)
    return (lo.astype(f64) + hi.astype(f64)) / 2.0


def correspondences(src, tgt, T, radius):
    """-> (p float32 [m, 3], index [m] (-1: none), distance float32 [m])"""
    with np.errstate(invalid="ignore"):                                    # (a non-finite row stays non-finite and gets no neighbour)
        p = P.apply_transform(src, T)
    idx, _, d = P.nn_brute(p, tgt, radius)
    return p, idx, d


def iteration(src, tgt, T, radius, estimation, normals=None):
    """One pass at T -> dict: count, usable, sum_d2, fitness, rmse, sums (27: the upper entries of A then b; or 15: sum (p - c), sum (q - c),
    sum (p - c)(q - c)^T row-major) and abs_sums, the sums of the absolute terms (what a tolerance on a reordered sum is relative to)"""
    tgt = np.asarray(tgt).astype(f32)
    p, idx, d = correspondences(src, tgt, T, radius)
    ok = idx >= 0
    count = int(ok.sum())
    d64 = d[ok].astype(f64)
    sum_d2 = float(np.sum(d64 * d64))
    c = centre(tgt)
    pp, q = p[ok].astype(f64), tgt[idx[ok]].astype(f64)
    if estimation == "point_to_plane":
        n = np.asarray(normals).astype(f32)[idx[ok]]
        use = np.isfinite(n).all(1) & (n != 0).any(1)
        pp, q, n = pp[use], q[use], n[use].astype(f64)
        r = ((pp[:, 0] - q[:, 0]) * n[:, 0] + (pp[:, 1] - q[:, 1]) * n[:, 1]) + (pp[:, 2] - q[:, 2]) * n[:, 2]
        J = np.concatenate([np.cross(pp - c, n), n], 1)
        terms = np.stack([J[:, a] * J[:, b] for a in range(6) for b in range(a, 6)] + [J[:, a] * r for a in range(6)], 1)
        usable = int(use.sum())
    else:
        a, b = pp - c, q - c
        terms = np.concatenate([a, b, (a[:, :, None] * b[:, None, :]).reshape(-1, 9)], 1)
        usable = count
    return dict(count=count, usable=usable, sum_d2=sum_d2, fitness=count / len(p), rmse=float(np.sqrt(sum_d2 / count)) if count else 0.0,
                sums=terms.sum(0), abs_sums=np.abs(terms).sum(0), sum_d2_abs=sum_d2, c=c)


def normal_matrix(sums):
    A = np.zeros((6, 6))
    k = 0
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = sums[k]
            k += 1
    return A, np.asarray(sums[21:27])


def update(it, estimation):
    """The 4 x 4 that the pass `it` multiplies T by from the left, or None (degenerate)"""
    c, s = it["c"], it["sums"]
    C, Ci = np.eye(4), np.eye(4)
    C[:3, 3], Ci[:3, 3] = c, -c
    M = np.eye(4)
    if estimation == "point_to_plane":
        if it["usable"] < 6:
            return None
        A, b = normal_matrix(s)
        try:
            Lc = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            return None
        delta = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, b))
        if not np.isfinite(delta).all():
            return None
        M = se3_exp(delta)
    else:
        n = it["count"]
        if n < 3:
            return None
        mp, mq = s[0:3] / n, s[3:6] / n
        H = s[6:15].reshape(3, 3) - n * np.outer(mp, mq)                  # sum (p - mean p)(q - mean q)^T
        U, sv, Vt = np.linalg.svd(H)
        if not (sv[1] > 0 and np.isfinite(sv).all()):
            return None
        V = Vt.T
        Rm = V @ np.diag([1.0, 1.0, np.sign(np.linalg.det(V @ U.T))]) @ U.T
        M[:3, :3], M[:3, 3] = Rm, mq - Rm @ mp
    return C @ M @ Ci


def evaluate(src, tgt, radius, T=None):
    """(fitness, rmse, count) at T: evaluate_registration"""
    it = iteration(src, tgt, np.eye(4) if T is None else T, radius, "point_to_point")
    return it["fitness"], it["rmse"], it["count"]


def icp(src, tgt, radius, init=None, estimation="point_to_plane", normals=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """-> dict: T, fitness, rmse, iterations, status, log [(fitness, rmse, count)]"""
    T = np.eye(4) if init is None else np.array(init, dtype=f64)
    log, status = [], "max_iteration"
    for k in range(max_iteration):
        it = iteration(src, tgt, T, radius, estimation, normals)
        log.append((it["fitness"], it["rmse"], it["count"]))
        if k >= 1 and abs(log[k][0] - log[k - 1][0]) < relative_fitness and abs(log[k][1] - log[k - 1][1]) < relative_rmse:
            status = "converged"
            break
        M = update(it, estimation)
        if M is None:
            status = "degenerate"
            break
        T = M @ T
    fitness, rmse, _ = evaluate(src, tgt, radius, T)
    return dict(T=T, fitness=fitness, rmse=rmse, iterations=len(log), status=status, log=log)


# ---- the bumpy pair ------------------------------------------------------------------------------------------------------------------------
PITCH, RADIUS = 0.002, 0.005
N_TARGET, N_SOURCE = 61 * 46, 1937
SMALL = (0.01, -0.008, 0.012, 0.002, -0.0015, 0.001)
MEDIUM = (0.03, -0.02, 0.025, 0.004, -0.003, 0.002)
LATTICE_MOTION = (2e-4, -1.5e-4, 3e-4, 1e-4, -8e-5, 5e-5)          # moves every lattice point by less than 0.3 of the smallest spacing


def bumpy(x, y):
    return 0.30 + 0.012 * np.sin(60.0 * x) * np.cos(50.0 * y) + 0.010 * np.cos(35.0 * x + 45.0 * y)


def bumpy_normal(x, y):
    """analytic unit normals (-dz/dx, -dz/dy, 1) / |.|"""
    zx = 0.012 * 60.0 * np.cos(60.0 * x) * np.cos(50.0 * y) - 0.010 * 35.0 * np.sin(35.0 * x + 45.0 * y)
    zy = -0.012 * 50.0 * np.sin(60.0 * x) * np.sin(50.0 * y) - 0.010 * 45.0 * np.sin(35.0 * x + 45.0 * y)
    n = np.stack([-zx, -zy, np.ones_like(zx)], 1)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def bumpy_target():
    """(points float32 [2806, 3], unit normals float32 [2806, 3]): a 61 x 46 lattice of 2 mm pitch, jittered by +-0.2 pitch in x and y only,
    z on the surface"""
    rng = np.random.default_rng(17)
    x, y = np.meshgrid((np.arange(61) - 30) * PITCH, (np.arange(46) - 22.5) * PITCH, indexing="ij")
    x = x.ravel() + rng.uniform(-0.2 * PITCH, 0.2 * PITCH, N_TARGET)
    y = y.ravel() + rng.uniform(-0.2 * PITCH, 0.2 * PITCH, N_TARGET)
    return np.stack([x, y, bumpy(x, y)], 1).astype(f32), bumpy_normal(x, y).astype(f32)


def bumpy_source_true():
    """1937 uniform samples of the surface over +-0.05 x +-0.035 m, float64: where the registered source points belong"""
    rng = np.random.default_rng(18)
    x = rng.uniform(-0.05, 0.05, N_SOURCE)
    y = rng.uniform(-0.035, 0.035, N_SOURCE)
    return np.stack([x, y, bumpy(x, y)], 1)


def displaced(points, motion):
    """the points moved by the inverse of small_pose(*motion), float32: registering them finds small_pose(*motion)"""
    Ti = np.linalg.inv(small_pose(*motion))
    return (np.asarray(points, f64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(f32)


def moved(points, T):
    """T applied in float64 (for measuring, not part of the contract)"""
    return np.asarray(points).astype(f64) @ T[:3, :3].T + T[:3, 3]
