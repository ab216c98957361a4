"""Numpy restatement of the TSDF ray cast (csrc/tsdf.hip, tsdf_raycast_kernel) -- TEST INFRASTRUCTURE ONLY.

Works on any object with ``units`` (a mapping (ix, iy, iz) -> fp32 [res, res, res, 5] with ``get``), ``vl``, ``trunc``, ``res``,
``L``, ``tsdf_at`` and ``normal_at``: oracle.tsdf_ref.TSDFRef as it stands.  Positions are Python floats (IEEE fp64, no fused
multiply-add) and every expression is written in the order the kernel evaluates it, so the two agree to the last bit except
where a library call (numpy's products inside ``tsdf_at``) rounds differently.

Per pixel (u, v) of a view with camera -> world pose (R, o):  d_cam = ((u - cx) / fx, (v - cy) / fy, 1),  d = R d_cam,
n = |d_cam|;  t = depth_min, f_prev = -1;  while t < depth_max:  p = o + t d;  unit = floor(p / L);
  unit absent:  t += max(exit of the unit's box, 0) + 0.5 vl / n,  f_prev = -1;
  else (f, w) = nearest voxel;  near band (w > 0 and |f| trunc < 2 vl): f = tsdf_at(p);
       hit when w > 0, f_prev > 0 and f <= 0:  t* = t_prev + (t - t_prev) f_prev / (f_prev - f);
       otherwise t_prev = t, f_prev = (w > 0 ? f : -1), t += max(w > 0 ? f trunc : 0, vl) / n.
The depth of a hit is t* (the camera-frame z of the point, as tests/_render.py and the integration define depth)."""
import math

import numpy as np

MAX_STEPS = 1 << 16           # the kernel's cap on steps per ray (never binds on these maps)


def _ray(pose, K, u, v):
    fx, fy, cx, cy = (float(x) for x in K)
    dc0, dc1 = (float(u) - cx) / fx, (float(v) - cy) / fy
    R = [[float(pose[a, b]) for b in range(3)] for a in range(3)]
    d = [R[a][0] * dc0 + R[a][1] * dc1 + R[a][2] for a in range(3)]
    n = math.sqrt(dc0 * dc0 + dc1 * dc1 + 1.0)
    return d, n


def cast_ray(ref, o, d, n, depth_min, depth_max):
    """-> (t* or 0.0, steps)"""
    vl, trunc, res, L = ref.vl, ref.trunc, ref.res, ref.L
    half_step = 0.5 * vl / n
    t, tp, fp, steps = float(depth_min), float(depth_min), -1.0, 0
    while t < depth_max and steps < MAX_STEPS:
        steps += 1
        p = [o[a] + t * d[a] for a in range(3)]
        ui = [math.floor(p[a] / L) for a in range(3)]
        vox = ref.units.get((ui[0], ui[1], ui[2]))
        if vox is None:
            te = math.inf
            for a in range(3):
                if d[a] > 0.0:
                    te = min(te, ((ui[a] + 1) * L - p[a]) / d[a])
                elif d[a] < 0.0:
                    te = min(te, (ui[a] * L - p[a]) / d[a])
            tp, fp = t, -1.0
            t = t + (max(te, 0.0) + half_step)
            continue
        idx = [min(max(math.floor((p[a] - ui[a] * L) / vl), 0), res - 1) for a in range(3)]
        cell = vox[idx[0], idx[1], idx[2]]
        f, w = float(cell[0]), float(cell[1])
        if w > 0.0 and abs(f) * trunc < 2.0 * vl:
            f = float(ref.tsdf_at(p))
        if w > 0.0 and fp > 0.0 and f <= 0.0:
            return tp + (t - tp) * fp / (fp - f), steps
        tp, fp = t, (f if w > 0.0 else -1.0)
        t = t + max(f * trunc if w > 0.0 else 0.0, vl) / n
    return 0.0, steps


def color_at(ref, p):
    """trilinear mean of r, g, b over the eight voxel centres around p, over the corners with weight > 0 only, renormalised and
    rounded to nearest (u8); zeros when no corner carries weight"""
    vl, res, L = ref.vl, ref.res, ref.L
    index0, idx0, rr = [0] * 3, [0] * 3, [0.0] * 3
    for a in range(3):
        pl = p[a] - 0.5 * vl
        index0[a] = math.floor(pl / L)
        pg = (pl - index0[a] * L) / vl
        idx0[a] = min(max(math.floor(pg), 0), res - 1)
        rr[a] = pg - idx0[a]
    acc, wsum = [0.0, 0.0, 0.0], 0.0
    for c in range(8):
        w, idx1, index1 = 1.0, [0] * 3, [0] * 3
        for a in range(3):
            sh = (c >> (2 - a)) & 1
            w *= rr[a] if sh else 1.0 - rr[a]
            idx1[a], index1[a] = idx0[a] + sh, index0[a]
            if idx1[a] >= res:
                idx1[a] -= res
                index1[a] += 1
        vox = ref.units.get((index1[0], index1[1], index1[2]))
        if vox is None:
            continue
        cell = vox[idx1[0], idx1[1], idx1[2]]
        if float(cell[1]) > 0.0:
            wsum += w
            for k in range(3):
                acc[k] += w * float(cell[2 + k])
    if not wsum > 0.0:
        return np.zeros(3, np.uint8)
    return np.array([min(max(math.floor(acc[k] / wsum + 0.5), 0), 255) for k in range(3)], dtype=np.uint8)


def raycast(ref, K, extrinsic, H, W, depth_min, depth_max, pixels=None, normal=False, color=False, steps=False):
    """Cast the rays of one view (extrinsic = world -> camera 4x4).  pixels: None = the whole image (outputs [H, W, ...]), or an
    int array [M, 2] of (v, u) pairs (outputs [M, ...]).  Returns a dict: depth fp64, vertex fp64 x 3, and on request normal
    fp64 x 3 (``ref.normal_at`` of the hit point), color u8 x 3, steps int."""
    pose = np.linalg.inv(np.asarray(extrinsic, dtype=np.float64))
    o = [float(pose[a, 3]) for a in range(3)]
    if pixels is None:
        vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        pix, shape = np.stack([vv.reshape(-1), uu.reshape(-1)], 1), (H, W)
    else:
        pix = np.asarray(pixels, dtype=np.int64).reshape(-1, 2)
        shape = (pix.shape[0],)
    M = pix.shape[0]
    out = {"depth": np.zeros(M), "vertex": np.zeros((M, 3))}
    if normal:
        out["normal"] = np.zeros((M, 3))
    if color:
        out["color"] = np.zeros((M, 3), np.uint8)
    if steps:
        out["steps"] = np.zeros(M, np.int64)
    for m in range(M):
        d, n = _ray(pose, K, pix[m, 1], pix[m, 0])
        t, k = cast_ray(ref, o, d, n, depth_min, depth_max)
        if steps:
            out["steps"][m] = k
        if not t > 0.0:
            continue
        p = [o[a] + t * d[a] for a in range(3)]
        out["depth"][m] = t
        out["vertex"][m] = p
        if normal:
            out["normal"][m] = ref.normal_at(np.array(p))
        if color:
            out["color"][m] = color_at(ref, p)
    return {k: v.reshape(shape + v.shape[1:]) for k, v in out.items()}


# ---- the toy scene of the ray-cast tests: tests/_render.py's height field, four integrated poses, three views ------------------------
TOY_HW = (48, 64)
TOY_K = (60.0, 60.0, 32.0, 24.0)
TOY_MAPS = ((0.01, 0.04), (0.004, 0.02))           # (voxel_length, sdf_trunc); res 8, stride 4
DEPTH_MIN, DEPTH_MAX = 0.05, 1.0


def toy_poses():
    """camera -> world of the four integrated frames"""
    import _render as R
    return [R.small_pose(0.02 * i, -0.03 * i, 0.01 * i, 0.01 * i, -0.008 * i, 0.005 * i) for i in range(4)]


def toy_views():
    """camera -> world of the three views that are cast: two integrated poses and one the map has never seen"""
    import _render as R
    P = toy_poses()
    return [P[0], P[3], R.small_pose(0.03, 0.04, -0.02, -0.012, 0.01, 0.004)]


def analytic_normal(X, Y):
    """unit normal line of the height field Z = g(X, Y) at (X, Y), pointing towards -z (the side the cameras are on)"""
    import _render as R
    eps = 1e-6
    gx = (R.g(X + eps, Y) - R.g(X - eps, Y)) / (2 * eps)
    gy = (R.g(X, Y + eps) - R.g(X, Y - eps)) / (2 * eps)
    n = np.stack([gx, gy, -np.ones_like(gx)], -1)
    return n / np.linalg.norm(n, axis=-1, keepdims=True)
