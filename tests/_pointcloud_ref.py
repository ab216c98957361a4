"""Numpy statement of the cloud-to-cloud distances (csrc/pointcloud.hip) -- TEST INFRASTRUCTURE ONLY.

The contract, in float32 throughout: for a source s and a target t, dx = s.x - t.x, dy and dz alike, d2 = (dx * dx + dy * dy) + dz * dz
(numpy does not contract); the nearest neighbour is the lexicographic minimum of (d2, index in the target as given); the distance is
np.sqrt(d2) in float32 (correctly rounded).  Non-finite target points are left out (indices still count them); a source point with a
non-finite coordinate gets (NaN, -1); no finite target point gives (+inf, -1); with max_distance a source whose distance is > max_distance,
compared in float32, gets (+inf, -1).  Restated from the documented meaning of Open3D's PointCloud.compute_point_cloud_distance; nothing
here comes from Open3D's code or from the reference, which only calls that function (3DM/mapping_module.py:45,48,62).

nn_brute is the contract as written.  nn_grid is the grid algorithm of the device -- the same cell function, Chebyshev shells, the
same conservative stop test -- and must equal nn_brute bit for bit for every cell size (tests/test_pointcloud_cpu.py).  stats and
metrics state the statistics record and evaluation.evaluate_reconstruction.

Also here, shared by tests/test_pointcloud_cpu.py and tests/test_pointcloud_gpu.py: the base clouds and the small map experiment.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render as R  # noqa: E402

f32 = np.float32
CHUNK = 512


def _finite_rows(a):
    return np.isfinite(a).all(1)


def nn_brute(src, tgt, max_distance=None):
    """-> (index int32 [n], d2 float32 [n], distance float32 [n]).  d2 of an unmatched or non-finite source is +inf / NaN like its distance."""
    src = np.asarray(src).astype(f32)
    tgt = np.asarray(tgt).astype(f32)
    keep = np.nonzero(_finite_rows(tgt))[0]                       # ascending: the first minimum among the kept is the lowest original index
    t = tgt[keep]
    n = len(src)
    idx = np.full(n, -1, np.int64)
    d2o = np.full(n, np.inf, f32)
    if len(t):
        with np.errstate(invalid="ignore", over="ignore"):
            for a in range(0, n, CHUNK):
                s = src[a:a + CHUNK]
                dx = s[:, None, 0] - t[None, :, 0]
                dy = s[:, None, 1] - t[None, :, 1]
                dz = s[:, None, 2] - t[None, :, 2]
                d2 = (dx * dx + dy * dy) + dz * dz
                i = np.argmin(d2, 1)                              # first minimum = lowest index
                idx[a:a + CHUNK] = keep[i]
                d2o[a:a + CHUNK] = d2[np.arange(len(s)), i]
    return _finish(src, idx, d2o, max_distance)


def _finish(src, idx, d2o, max_distance):
    with np.errstate(invalid="ignore"):
        d = np.sqrt(d2o)
    if max_distance is not None:
        miss = d > f32(max_distance)
        idx[miss], d2o[miss], d[miss] = -1, np.inf, np.inf
    bad = ~_finite_rows(src)
    idx[bad], d2o[bad], d[bad] = -1, np.nan, np.nan
    return idx.astype(np.int32), d2o, d


# ---- the grid ------------------------------------------------------------------------------------------------------------------------------
def bounds(tgt):
    """(lo, hi) float32 [3] over the finite rows; zeros without one"""
    t = np.asarray(tgt).astype(f32)
    t = t[_finite_rows(t)]
    if not len(t):
        return np.zeros(3, f32), np.zeros(3, f32)
    return t.min(0), t.max(0)


def dims_for(lo, hi, h):
    with np.errstate(over="ignore"):
        return np.minimum(np.floor((hi - lo) / f32(h)), f32(2.0 ** 30)).astype(np.int64) + 1


def default_cell_size(lo, hi, n):
    """the device's default: (product of the positive extents / n)^(1 / their number) as float32, grown by 1.25 until <= 2^24 cells"""
    ext = (hi - lo).astype(np.float64)
    pos = ext[(ext > 0) & np.isfinite(ext)]
    if pos.size == 0 or n < 1:
        return 1.0
    h = float(f32(np.exp((np.sum(np.log(pos)) - np.log(n)) / pos.size)))
    h = max(h, float(np.finfo(f32).tiny))
    while int(np.prod(dims_for(lo, hi, h).astype(object))) > 2 ** 24:
        h = float(f32(h * 1.25))
    return h


def cells_of(p, lo, h, dims):
    """cell coordinates [n, 3] of float32 points: min(max(floor((x - lo) / h), 0), n - 1) in float32"""
    with np.errstate(over="ignore"):
        t = np.floor((p - lo[None, :]) / f32(h))
    t = np.minimum(np.maximum(t, f32(0.0)), (dims - 1).astype(f32)[None, :])
    return t.astype(np.int64)


def nn_grid(src, tgt, h=None, max_distance=None, shell_cap=None, stats_out=None):
    """the grid algorithm.  shell_cap: a source still searching after that shell is finished by nn_brute (None: never).  stats_out: a dict
    that receives 'fallback' (the number of such sources) and 'shells' (the last shell of each source)."""
    src = np.asarray(src).astype(f32)
    tgt = np.asarray(tgt).astype(f32)
    keep = np.nonzero(_finite_rows(tgt))[0]
    t = tgt[keep]
    lo, hi = bounds(tgt)
    if h is None:
        h = default_cell_size(lo, hi, len(t))
    h = f32(h)
    dims = dims_for(lo, hi, h)
    nx, ny, nz = (int(v) for v in dims)
    tc = cells_of(t, lo, h, dims) if len(t) else np.zeros((0, 3), np.int64)
    cell = (tc[:, 2] * ny + tc[:, 1]) * nx + tc[:, 0]
    order = np.argsort(cell, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=nx * ny * nz))])
    tx, ty, tz, tid = t[order, 0], t[order, 1], t[order, 2], keep[order]
    n = len(src)
    idx = np.full(n, -1, np.int64)
    d2o = np.full(n, np.inf, f32)
    shells = np.zeros(n, np.int64)
    fallback = []
    md = f32(np.inf) if max_distance is None else f32(max_distance)
    ok = _finite_rows(src)
    sc = cells_of(np.where(ok[:, None], src, f32(0.0)), lo, h, dims)
    ext = hi - lo
    for i in range(n):
        if not ok[i]:
            continue
        s = src[i]
        cx, cy, cz = (int(v) for v in sc[i])
        slack = f32(np.max(ext + np.abs(s - lo))) * f32(2.0 ** -21)
        r_all = max(cx, nx - 1 - cx, cy, ny - 1 - cy, cz, nz - 1 - cz)
        best, bi = f32(np.inf), 2 ** 31 - 1
        r = 0
        while True:
            runs = []
            x0, x1 = max(cx - r, 0), min(cx + r, nx - 1)
            for z in range(max(cz - r, 0), min(cz + r, nz - 1) + 1):
                for y in range(max(cy - r, 0), min(cy + r, ny - 1) + 1):
                    row = (z * ny + y) * nx
                    if abs(z - cz) == r or abs(y - cy) == r:
                        runs.append((start[row + x0], start[row + x1 + 1]))
                    else:
                        if cx - r >= 0:
                            runs.append((start[row + cx - r], start[row + cx - r + 1]))
                        if cx + r <= nx - 1:
                            runs.append((start[row + cx + r], start[row + cx + r + 1]))
            k = np.concatenate([np.arange(a, b) for a, b in runs]) if runs else np.zeros(0, np.int64)
            if len(k):
                with np.errstate(over="ignore"):
                    dx, dy, dz = s[0] - tx[k], s[1] - ty[k], s[2] - tz[k]
                    d2 = (dx * dx + dy * dy) + dz * dz
                m = d2.min()
                j = int(tid[k][d2 == m].min())
                if m < best or (m == best and j < bi):
                    best, bi = m, j
            shells[i] = r
            if r >= r_all:
                break
            lb = (f32(r) * h - slack) * f32(0.99999)
            if lb > 0 and best < lb * lb:
                break
            if lb * f32(0.9999) > md:
                break
            if shell_cap is not None and r >= shell_cap:
                fallback.append(i)
                bi = -2
                break
            r += 1
        if bi == -2:
            continue
        if bi != 2 ** 31 - 1:
            idx[i], d2o[i] = bi, best
    if fallback:
        fi, fd2, _ = nn_brute(src[fallback], tgt)
        idx[fallback], d2o[fallback] = fi, fd2
    if stats_out is not None:
        stats_out["fallback"], stats_out["shells"] = len(fallback), shells
    return _finish(src, idx, d2o, max_distance)


# ---- statistics and the evaluation -------------------------------------------------------------------------------------------------------
def stats(d, taus=()):
    """the record of bs_pc_stats over float32 distances: n, finite, infinite, NaN entries; over the finite ones sum, sum of squares (float64),
    max, exact median (np.median of the float64 values: the mean of the two middle ones for an even count); the count of d < tau per tau,
    compared in float32"""
    d = np.asarray(d, dtype=f32)
    fin = d[np.isfinite(d)]
    d64 = fin.astype(np.float64)
    return dict(n=len(d), n_finite=len(fin), n_unmatched=int(np.isinf(d).sum()), n_nan=int(np.isnan(d).sum()), sum=float(np.sum(d64)),
                sumsq=float(np.sum(d64 * d64)), max=float(fin.max()) if len(fin) else np.nan, median=float(np.median(d64)) if len(fin) else np.nan,
                counts=[int((fin < f32(t)).sum()) for t in taus])


def affine_rows(transform):
    """[s R | t] float64 [3, 4] of a 4 x 4 or of (R, s, t)"""
    if isinstance(transform, (tuple, list)) and len(transform) == 3:
        Rm, s, t = transform
        return np.concatenate([float(s) * np.asarray(Rm, np.float64), np.asarray(t, np.float64).reshape(3, 1)], 1)
    return np.asarray(transform, np.float64)[:3].copy()


def apply_transform(p, transform):
    """((a0 p0 + a1 p1) + a2 p2) + t per row in float64, rounded once to float32"""
    A = affine_rows(transform)
    p = np.asarray(p).astype(np.float64)
    return np.stack([((A[r, 0] * p[:, 0] + A[r, 1] * p[:, 1]) + A[r, 2] * p[:, 2]) + A[r, 3] for r in range(3)], 1).astype(f32)


def metrics(pred, gt, taus=(0.001, 0.002, 0.005), transform=None, max_distance=None):
    """evaluate_reconstruction as a dict: accuracy / completeness (mean, median, rmse, max), chamfer, precision / recall / fscore per tau,
    the counts, and the two statistics records ('rec_accuracy', 'rec_completeness') and distance arrays"""
    pred = np.asarray(pred)
    p = apply_transform(pred, transform) if transform is not None else pred.astype(f32)
    g = np.asarray(gt).astype(f32)
    d_pg = nn_brute(p, g, max_distance)[2]
    d_gp = nn_brute(g, p, max_distance)[2]
    ra, rc = stats(d_pg, taus), stats(d_gp, taus)

    def side(r):
        n = r["n_finite"]
        if n == 0:
            return dict(mean=np.nan, median=np.nan, rmse=np.nan, max=np.nan)
        return dict(mean=r["sum"] / n, median=r["median"], rmse=float(np.sqrt(r["sumsq"] / n)), max=r["max"])
    acc, comp = side(ra), side(rc)
    with np.errstate(invalid="ignore", divide="ignore"):
        prec = np.array(ra["counts"], np.float64) / (ra["n_finite"] + ra["n_unmatched"])
        rec = np.array(rc["counts"], np.float64) / (rc["n_finite"] + rc["n_unmatched"])
        f = np.where(prec + rec > 0, 2 * prec * rec / (prec + rec), 0.0)
    return dict(accuracy=acc, completeness=comp, chamfer=(acc["mean"] + comp["mean"]) / 2, precision=prec, recall=rec, fscore=f,
                n_pred=ra["n"], n_gt=rc["n"], n_unmatched_pred=ra["n_unmatched"], n_unmatched_gt=rc["n_unmatched"], rec_accuracy=ra,
                rec_completeness=rc, d_pred_gt=d_pg, d_gt_pred=d_gp)


# ---- the base clouds -------------------------------------------------------------------------------------------------------------------
PITCH, JITTER = 0.002, 0.0004
N_TARGET, N_SOURCE = 61 * 46, 1937


def base_target():
    """the height field _render.g on a 61 x 46 lattice of 2 mm pitch around the origin, jittered by +-0.4 mm per axis: float32 [2806, 3]"""
    rng = np.random.default_rng(7)
    x, y = np.meshgrid((np.arange(61) - 30) * PITCH, (np.arange(46) - 22.5) * PITCH, indexing="ij")
    p = np.stack([x.ravel(), y.ravel(), R.g(x.ravel(), y.ravel())], 1)
    return (p + rng.uniform(-JITTER, JITTER, size=p.shape)).astype(f32)


def base_source():
    """1937 uniform samples of the same surface over the lattice's footprint: float32 [1937, 3]"""
    rng = np.random.default_rng(8)
    x = rng.uniform(-30 * PITCH, 30 * PITCH, N_SOURCE)
    y = rng.uniform(-22.5 * PITCH, 22.5 * PITCH, N_SOURCE)
    return np.stack([x, y, R.g(x, y)], 1).astype(f32)


# ---- the small map experiment (tests/test_pointcloud_gpu.py case 9) ---------------------------------------------------------------------
MAP_H, MAP_W, MAP_K = 48, 64, (60.0, 60.0, 32.0, 24.0)         # tests/_tsdf_correct_ref.py's camera
MAP_VL, MAP_TRUNC, MAP_RES, MAP_STRIDE, MAP_FRAMES = 0.002, 0.008, 8, 4, 8
MAP_DRIFT_VOXELS = 3.0                                          # per frame, along x


def map_frames():
    """eight renderings of the height field along a short known trajectory: [(colour u8, depth fp32, camera -> world 4x4)]"""
    out = []
    for i in range(MAP_FRAMES):
        pose = R.small_pose(0.01 * i, -0.008 * i, 0.005 * i, 0.004 * i - 0.014, 0.003 * i - 0.01, 0.002 * i)
        col, dep = R.render(pose, MAP_K, MAP_H, MAP_W)
        out.append((col, dep, pose))
    return out


def map_extrinsics(frames, drift):
    """world -> camera per frame; drift: frame i's camera is placed MAP_DRIFT_VOXELS * i voxels along x from where it was"""
    Es = []
    for i, (_, _, pose) in enumerate(frames):
        q = pose.copy()
        if drift:
            q[0, 3] += MAP_DRIFT_VOXELS * MAP_VL * i
        Es.append(np.linalg.inv(q))
    return Es


def map_gt_samples(n=6000):
    """samples of the true surface over the region the eight cameras see (a 0.30 x 0.24 m footprint under the trajectory)"""
    rng = np.random.default_rng(9)
    x = rng.uniform(-0.16, 0.16, n)
    y = rng.uniform(-0.13, 0.13, n)
    return np.stack([x, y, R.g(x, y)], 1).astype(f32)
