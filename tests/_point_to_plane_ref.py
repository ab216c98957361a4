"""Numpy restatement of the frame-to-model tracking step (bodyslam_amd.rgbd_odometry.PointToPlaneOdometry,
MAP.track_frame_to_model) -- TEST INFRASTRUCTURE ONLY, independent of the product code.

The role is Open3D's ``Model.track_frame_to_model(input_frame, raycast_frame, depth_scale=1000, depth_max=3.0, depth_diff=0.07)``
(point-to-plane, criteria 6 / 3 / 1), which the reference's MAP wraps (BodySLAM_not_refactored/3DM/tsdf.py:56-107).  Open3D is not
available: **parity unpinned**; the defaults restate its published interface, the algorithm is the statement below.

  inputs:     source depth = the input frame in metres, <= 0 or > depth_max -> NaN; target depth = the model's ray-cast depth,
              0 (no surface) -> NaN
  pyramid:    both get the 3-level depth pyramid of oracle/rgbd_odometry_ref.py (threshold 2 * depth_diff), intrinsics halved
  target:     per level, vertex V(u, v) = ((u - cx) z / fx, (v - cy) z / fy, z) and the forward-difference normal
              n = normalise((V(u+1, v) - V(u, v)) x (V(u, v+1) - V(u, v))): NaN on the last row and column, where one of the
              three vertices is invalid, or where the cross product has zero length
  one step:   for every valid source pixel: p = T v_s (skip p.z <= 0); the NEAREST target pixel of p's projection (round half
              away from zero; skip outside the image); q, n there (skip if invalid); r = (p - q) . n (skip |r| > depth_diff);
              J = [p x n, n] for the left twist (omega, nu)
  sums:       A = sum J J^T unweighted, b = sum J clip(r, +-huber), cost = sum huber(r), huber = 0.05; the inlier count
  update:     delta = -(A + 1e-12 I)^-1 b, T <- exp(delta) T; fewer than 6 inliers leave T alone
  schedule:   coarse to fine, (6, 3, 1) iterations, all of them run
"""
import numpy as np

from oracle import rgbd_odometry_ref as R

DEPTH_DIFF, DEPTH_HUBER = 0.07, 0.05
ITERATIONS = (6, 3, 1)

# the cases of the tests: intrinsics and rendered motions (rx, ry, rz, tx, ty, tz) of tests/test_rgbd_odometry_gpu.py
K_SMALL = (150.0, 150.0, 80.0, 60.0)                                                   # 120 x 160
K_FULL = (383.1901395, 383.1901395, 276.4727783203125, 124.3335933685303)             # 480 x 640, the reference's
SMALL, MEDIUM = (0.004, -0.006, 0.003, 0.002, -0.0015, 0.001), (0.01, -0.015, 0.008, 0.012, -0.009, 0.006)
FULL = (0.002, -0.003, 0.001, 0.0015, -0.001, 0.0008)


def pair(motion, K, H, W, holes=False):
    """(true source -> target motion, source depth, target depth) of two renderings; holes: 5 % of the source pixels and a 10 x 20
    target patch invalid"""
    from _render import render, small_pose
    pose_s = small_pose(*motion)
    _, dt = render(np.eye(4), K, H, W)
    _, ds = render(pose_s, K, H, W)
    if holes:
        rng = np.random.default_rng(3)
        ds[rng.random((H, W)) < 0.05] = 0.0
        dt[40:50, 70:90] = 0.0
    return pose_s, ds, dt


def prepare_source(depth_m, depth_max):
    d = np.asarray(depth_m, dtype=np.float64).copy()
    d[~((d > 0) & (d <= depth_max))] = np.nan
    return d


def prepare_target(depth_m):
    d = np.asarray(depth_m, dtype=np.float64).copy()
    d[~(d > 0)] = np.nan
    return d


def depth_pyramid(d, K, depth_diff=DEPTH_DIFF, levels=3):
    out = [(d, tuple(K))]
    for _ in range(levels - 1):
        d, k = out[-1]
        out.append((R.pyr_down_depth(d, 2 * depth_diff), tuple(v / 2 for v in k)))
    return out


def vertex_map(d, K):
    fx, fy, cx, cy = K
    H, W = d.shape
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.stack([(u - cx) * d / fx, (v - cy) * d / fy, d], -1)


def normal_map(V):
    n = np.full(V.shape, np.nan)
    c = np.cross(V[:-1, 1:] - V[:-1, :-1], V[1:, :-1] - V[:-1, :-1])
    length = np.sqrt((c * c).sum(-1))
    with np.errstate(invalid="ignore", divide="ignore"):
        n[:-1, :-1] = np.where((length > 0)[..., None], c / length[..., None], np.nan)
    return n


def accumulate(Ds, Vt, Nt, K, T, depth_diff=DEPTH_DIFF, huber=DEPTH_HUBER):
    """(A [6, 6], b [6], cost, inliers) of one step at pose T (source -> target)"""
    fx, fy, cx, cy = K
    H, W = Ds.shape
    ok = ~np.isnan(Ds)
    Vs = vertex_map(np.where(ok, Ds, 1.0), K)
    p = Vs @ T[:3, :3].T + T[:3, 3]
    ok &= p[..., 2] > 0
    pz = np.where(ok, p[..., 2], 1.0)
    uf, vf = fx * p[..., 0] / pz + cx, fy * p[..., 1] / pz + cy
    rnd = lambda a: np.sign(a) * np.floor(np.abs(a) + 0.5)
    ur, vr = rnd(np.where(ok, uf, 0.0)), rnd(np.where(ok, vf, 0.0))
    ok &= (ur >= 0) & (ur <= W - 1) & (vr >= 0) & (vr <= H - 1)
    ui, vi = np.where(ok, ur, 0).astype(int), np.where(ok, vr, 0).astype(int)
    q, n = Vt[vi, ui], Nt[vi, ui]
    ok &= ~np.isnan(q).any(-1) & ~np.isnan(n).any(-1)
    r = ((p - q) * n).sum(-1)
    ok &= np.abs(np.where(np.isnan(r), 1e9, r)) <= depth_diff
    m = ok.ravel()
    p, n, r = p.reshape(-1, 3)[m], n.reshape(-1, 3)[m], r.ravel()[m]
    J = np.concatenate([np.cross(p, n), n], 1)
    clipped = np.where(np.abs(r) < huber, r, np.sign(r) * huber)
    cost = np.where(np.abs(r) < huber, 0.5 * r * r, huber * (np.abs(r) - 0.5 * huber)).sum()
    return J.T @ J, J.T @ clipped, float(cost), int(m.sum())


def point_to_plane(src_depth, tgt_depth, K, depth_max=3.0, init=None, iterations=ITERATIONS, depth_diff=DEPTH_DIFF, huber=DEPTH_HUBER,
                   trace=None):
    """T (4x4): source points -> target frame"""
    ps = depth_pyramid(prepare_source(src_depth, depth_max), K, depth_diff, len(iterations))
    pt = depth_pyramid(prepare_target(tgt_depth), K, depth_diff, len(iterations))
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    for level, iters in zip(range(len(ps) - 1, -1, -1), iterations):
        Ds, k = ps[level]
        Vt = vertex_map(pt[level][0], k)
        Nt = normal_map(Vt)
        for _ in range(iters):
            A, b, cost, n = accumulate(Ds, Vt, Nt, k, T, depth_diff, huber)
            if trace is not None:
                trace.append((level, A.copy(), b.copy(), cost, n))
            if n < 6:
                continue
            T = R.se3_exp(np.linalg.solve(A + 1e-12 * np.eye(6), -b)) @ T
    return T
