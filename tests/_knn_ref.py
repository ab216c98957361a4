"""Numpy statement of the k nearest neighbours, the normal estimation and the statistical outlier removal (csrc/knn.hip,
bodyslam_amd/pointcloud.py) -- TEST INFRASTRUCTURE ONLY, independent of the product code.

The roles are Open3D's ``KDTreeFlann.search_knn_vector_3d`` / ``search_hybrid_vector_3d``, ``PointCloud.estimate_normals`` (which the
reference calls at 3DM/mapping_module.py:184; Open3D's default search there is k-NN with k = 30) and ``PointCloud.remove_statistical_outlier``
(mapping_module.py:87, nb_neighbors=20, std_ratio=2.0).  Open3D is not available: **parity unpinned**; the text below restates the
documented meaning and is the contract.

k-NN      the arithmetic of `_pointcloud_ref.nn_brute`, float32 without contraction: d2 = (dx * dx + dy * dy) + dz * dz.  The neighbours of a
          source are the k lexicographically smallest (d2, index in the target as given) among the finite target points, ascending.  With
          a radius (hybrid search) a candidate counts only when np.sqrt(d2) <= radius in float32 (a target at exactly the radius is in).
          Per source: index int32 [m, k] padded with -1, d2 float32 [m, k] padded with +inf, count int32 [m].  A source with a non-finite
          coordinate gets count 0, indices -1 and d2 NaN.  Non-finite targets are left out and indices still count them.  A source that
          is a point of the target finds itself first (d2 = 0).  1 <= k <= KNN_MAX = 32.  For k = 1 the result is nn_brute's.
normals   from a k-NN result of a cloud on itself, float64, neighbours j = 0 .. count - 1 in list order: q_j = t[idx_j] - p (exact);
          S = sum q_j and M = sum q_j q_j^T added sequentially, one product and one add each; C = M / count - (S / count)(S / count)^T; the
          one-sided Jacobi SVD of C that csrc/svd3.h runs (C is symmetric PSD: the singular triplets are the eigenpairs); the normal is
          the normalised column of V with the smallest singular value (ties: the lowest column), rounded to float32 once at the end.
          Zero when count < 3 or the largest eigenvalue is not positive and finite.  For exactly collinear neighbours the direction is
          unspecified (finite; unit or zero).  Sign: direction=v flips when n . v < 0; camera_location=c flips when n . (c - p) < 0, in
          float64; with neither, the component of largest magnitude is made positive (the first such on ties).  Eigenvalues ascending,
          float64 [n, 3] (zeros for an empty list).
outliers  avg_i = float32((sum_j float64(np.sqrt(d2_ij))) / count_i) over the point's nb_neighbors nearest, itself included, added in list
          order (NaN for a non-finite point); over the finite avg: n, sum, sumsq in float64 (`_pointcloud_ref.stats`);
          mean = sum / n, std = sqrt(max(sumsq - n mean^2, 0) / (n - 1)) (0 for n < 2); threshold = mean + std_ratio std; a point is kept
          when float64(avg_i) < threshold (NaN is never kept).  The result: the ascending kept indices and a boolean mask.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pointcloud_ref as P  # noqa: E402

f32, f64 = np.float32, np.float64
KNN_MAX = 32
CHUNK = 256


def knn_brute(src, tgt, k, radius=None):
    """-> (index int32 [m, k], d2 float32 [m, k], count int32 [m])"""
    if not 1 <= k <= KNN_MAX:
        raise ValueError(f"k = {k}")
    src = np.asarray(src).astype(f32)
    tgt = np.asarray(tgt).astype(f32)
    keep = np.nonzero(np.isfinite(tgt).all(1))[0]                 # ascending: a stable sort breaks ties of d2 by the original index
    t = tgt[keep]
    m = len(src)
    idx = np.full((m, k), -1, np.int32)
    d2o = np.full((m, k), np.inf, f32)
    cnt = np.zeros(m, np.int32)
    ok = np.isfinite(src).all(1)
    if len(t):
        with np.errstate(invalid="ignore", over="ignore"):
            for a in range(0, m, CHUNK):
                s = src[a:a + CHUNK]
                dx = s[:, None, 0] - t[None, :, 0]
                dy = s[:, None, 1] - t[None, :, 1]
                dz = s[:, None, 2] - t[None, :, 2]
                d2 = (dx * dx + dy * dy) + dz * dz
                valid = np.ones(d2.shape, bool) if radius is None else np.sqrt(d2) <= f32(radius)
                key = np.where(valid, d2, f32(np.inf))                    # (with a finite radius every valid d2 is finite: the invalid sort last)
                order = np.argsort(key, axis=1, kind="stable")[:, :k]
                rows = np.arange(len(s))[:, None]
                n_valid = np.minimum(valid.sum(1), k)
                got = np.arange(order.shape[1])[None, :] < n_valid[:, None]
                kk = order.shape[1]
                idx[a:a + CHUNK, :kk] = np.where(got, keep[order], -1)
                d2o[a:a + CHUNK, :kk] = np.where(got, d2[rows, order], f32(np.inf))
                cnt[a:a + CHUNK] = n_valid
    idx[~ok], d2o[~ok], cnt[~ok] = -1, np.nan, 0
    return idx, d2o, cnt


def d2_cutoff(radius):
    """the largest float32 d2 with np.sqrt(d2) <= radius: the device's form of the radius test (the same predicate, sqrt is monotone)"""
    r = f32(radius)
    if not np.isfinite(r):
        return f32(np.inf)
    with np.errstate(over="ignore"):
        c = r * r
    if not np.isfinite(c):
        c = np.finfo(f32).max
    while c > 0 and np.sqrt(c) > r:
        c = np.nextafter(c, f32(0.0))
    while True:
        up = np.nextafter(c, f32(np.inf))
        if not np.isfinite(up) or np.sqrt(up) > r:
            return c
        c = up


# ---- normals -----------------------------------------------------------------------------------------------------------------------------
def svd3_jacobi(M):
    """csrc/svd3.h's one-sided Jacobi over a batch, operation for operation: M float64 [n, 3, 3] -> (s [n, 3] in no particular order,
    V [n, 3, 3]); a matrix leaves the sweeps when its largest |cos| between two columns is below 1e-17, after 40 sweeps at the latest"""
    A = np.array(M, dtype=f64)
    n = len(A)
    V = np.broadcast_to(np.eye(3), (n, 3, 3)).copy()
    active = np.ones(n, bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for _ in range(40):
            off = np.zeros(n)
            for p, q in ((0, 1), (0, 2), (1, 2)):
                alpha = (A[:, 0, p] * A[:, 0, p] + A[:, 1, p] * A[:, 1, p]) + A[:, 2, p] * A[:, 2, p]
                beta = (A[:, 0, q] * A[:, 0, q] + A[:, 1, q] * A[:, 1, q]) + A[:, 2, q] * A[:, 2, q]
                gamma = (A[:, 0, p] * A[:, 0, q] + A[:, 1, p] * A[:, 1, q]) + A[:, 2, p] * A[:, 2, q]
                off = np.maximum(off, np.abs(gamma) / np.sqrt(alpha * beta + 1e-300))
                rot = active & (np.abs(gamma) > 1e-300)
                zeta = (beta - alpha) / (2.0 * gamma)
                t = np.where(zeta >= 0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                cs = 1.0 / np.sqrt(1.0 + t * t)
                sn = cs * t
                for X in (A, V):
                    for i in range(3):
                        xp, xq = X[:, i, p].copy(), X[:, i, q].copy()
                        X[:, i, p] = np.where(rot, cs * xp - sn * xq, xp)
                        X[:, i, q] = np.where(rot, sn * xp + cs * xq, xq)
            active &= ~(off < 1e-17)
            if not active.any():
                break
    s = np.sqrt((A[:, 0, :] * A[:, 0, :] + A[:, 1, :] * A[:, 1, :]) + A[:, 2, :] * A[:, 2, :])
    return s, V


def covariances(points, idx, cnt):
    """C float64 [n, 3, 3] per the statement (zeros for an empty list)"""
    pts = np.asarray(points).astype(f32)
    n, k = idx.shape
    with np.errstate(invalid="ignore"):
        p = pts.astype(f64)
        S = np.zeros((n, 3))
        M = np.zeros((n, 3, 3))
        for j in range(k):
            use = j < cnt
            q = np.where(use[:, None], p[np.where(use, idx[:, j], 0)] - p, 0.0)
            S = S + q                                                      # (+ 0.0 leaves a finished row's sums as they are)
            M = M + q[:, :, None] * q[:, None, :]
        c = np.maximum(cnt, 1).astype(f64)
        mean = S / c[:, None]
        C = M / c[:, None, None] - mean[:, :, None] * mean[:, None, :]
    C[cnt == 0] = 0.0
    return C


def normals_from_knn(points, idx, cnt, direction=None, camera_location=None):
    """-> (normals float32 [n, 3], eigenvalues float64 [n, 3] ascending)"""
    if direction is not None and camera_location is not None:
        raise ValueError("direction and camera_location are mutually exclusive")
    pts = np.asarray(points).astype(f32)
    s, V = svd3_jacobi(covariances(pts, idx, cnt))
    n = len(pts)
    lo = np.argmin(s, 1)                                                   # the first minimum: ties to the lowest column
    ev = np.sort(s, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = V[np.arange(n), :, lo]
        v = v / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])[:, None]
        if direction is not None:
            d = np.asarray(direction, f64)
            dot = (v[:, 0] * d[0] + v[:, 1] * d[1]) + v[:, 2] * d[2]
        elif camera_location is not None:
            w = np.asarray(camera_location, f64)[None, :] - pts.astype(f64)
            dot = (v[:, 0] * w[:, 0] + v[:, 1] * w[:, 1]) + v[:, 2] * w[:, 2]
        else:
            dot = v[np.arange(n), np.argmax(np.abs(v), 1)]                 # the first maximum
        v = np.where((dot < 0)[:, None], -v, v)
    ok = (cnt >= 3) & (ev[:, 2] > 0) & np.isfinite(ev[:, 2]) & np.isfinite(v).all(1)
    v[~ok] = 0.0
    ev[cnt == 0] = 0.0
    return v.astype(f32), ev


def estimate_normals(points, k=30, radius=None, direction=None, camera_location=None):
    idx, _, cnt = knn_brute(points, points, k, radius)
    return normals_from_knn(points, idx, cnt, direction, camera_location)


# ---- statistical outlier removal ---------------------------------------------------------------------------------------------------------
def knn_mean_distance(d2, cnt):
    """avg float32 [m]"""
    m, k = d2.shape
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.zeros(m)
        for j in range(k):
            s = s + np.where(j < cnt, np.sqrt(d2[:, j]).astype(f64), 0.0)
        return (s / cnt.astype(f64)).astype(f32)


def outlier_threshold(avg, std_ratio):
    """(mean, std, threshold) in float64 from the statistics record of the finite entries"""
    r = P.stats(avg)
    n = r["n_finite"]
    if n == 0:
        return np.nan, 0.0, np.nan
    mean = r["sum"] / n
    std = float(np.sqrt(max(r["sumsq"] - n * mean * mean, 0.0) / (n - 1))) if n >= 2 else 0.0
    return mean, std, mean + float(std_ratio) * std


def remove_statistical_outlier(points, nb_neighbors=20, std_ratio=2.0):
    """-> (kept indices int64 ascending, mask bool [n], avg float32 [n], threshold)"""
    _, d2, cnt = knn_brute(points, points, nb_neighbors)
    avg = knn_mean_distance(d2, cnt)
    thr = outlier_threshold(avg, std_ratio)[2]
    with np.errstate(invalid="ignore"):
        mask = avg.astype(f64) < thr
    return np.nonzero(mask)[0].astype(np.int64), mask, avg, thr


# ---- the test clouds -------------------------------------------------------------------------------------------------------------------
def tie_lattice():
    """the 9 x 7 x 3 integer lattice scaled by 2^-8: float32 [189, 3], x fastest; every d2 is exact, and ties are everywhere"""
    z, y, x = np.meshgrid(np.arange(3), np.arange(7), np.arange(9), indexing="ij")
    return (np.stack([x.ravel(), y.ravel(), z.ravel()], 1) * 2.0 ** -8).astype(f32)


def planted_cloud():
    """(the bumpy target with 12 rows moved 0.01 - 0.03 m along +- their analytic normals float32 [2806, 3], those rows ascending)"""
    import _icp_ref as I
    tgt, nrm = I.bumpy_target()
    rng = np.random.default_rng(23)
    rows = np.sort(rng.choice(len(tgt), 12, replace=False))
    step = rng.uniform(0.01, 0.03, 12) * rng.choice([-1.0, 1.0], 12)
    out = tgt.astype(f64)
    out[rows] += step[:, None] * nrm[rows].astype(f64)
    return out.astype(f32), rows
