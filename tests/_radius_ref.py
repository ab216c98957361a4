"""Numpy statement of the radius search, the radius outlier removal and the DBSCAN clustering (csrc/radius.hip, bodyslam_amd/pointcloud.py,
DESIGN section 3.22) -- TEST INFRASTRUCTURE ONLY, independent of the product code.

The roles are Open3D's ``KDTreeFlann.search_radius_vector_3d``, ``PointCloud.remove_radius_outlier`` and ``PointCloud.cluster_dbscan``.
Open3D is not available: **parity unpinned**; the text below restates the documented meaning and is the contract.

radius    the arithmetic of `_knn_ref.knn_brute`, float32 without contraction: d2 = (dx * dx + dy * dy) + dz * dz.  A finite target point is
          a neighbour of a finite source when np.sqrt(d2) <= radius in float32 -- a target at exactly the radius is in --, which is
          d2 <= `_knn_ref.d2_cutoff(radius)` (sqrt is monotone).  A source with a non-finite coordinate has no neighbours; non-finite
          targets are left out and indices still count them.  Rows are CSR: row_start int64 [m + 1], index int32 [total], d2 float32
          [total], every row ascending in (d2, index) -- `knn_brute`'s order.  A source that is a point of the target finds itself first.
outliers  a point is kept when the number of points of the cloud within `radius` of it, itself included, is > nb_points (Open3D's rule as
          its source has it, restated from memory); a non-finite point is never kept.  The ascending kept indices and a boolean mask.
dbscan    with count = the radius count of the cloud on itself at eps:
          core     a finite point with count >= min_points (itself included);
          cluster  the connected components of the graph on the core points with an edge where d2 <= cutoff, numbered 0, 1, ... in ascending
                   order of each component's smallest core index;
          border   a finite non-core point with at least one core point within eps: it takes the SMALLEST CLUSTER NUMBER among those core
                   points (not the nearest one's, not the lowest-indexed one's);
          noise    everything else and every non-finite point: label -1.
          This is what the textbook sequential scan gives when it visits the points in ascending index order.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_ref as K  # noqa: E402

f32 = np.float32
CHUNK = 256


def radius_brute(src, tgt, radius):
    """-> (row_start int64 [m + 1], index int32 [total], d2 float32 [total])"""
    src = np.asarray(src).astype(f32)
    tgt = np.asarray(tgt).astype(f32)
    cut = K.d2_cutoff(radius)
    keep = np.nonzero(np.isfinite(tgt).all(1))[0]
    t = tgt[keep]
    m = len(src)
    ok = np.isfinite(src).all(1)
    counts = np.zeros(m, np.int64)
    idx_parts, d2_parts = [], []
    if len(t):
        with np.errstate(invalid="ignore", over="ignore"):
            for a in range(0, m, CHUNK):
                s = src[a:a + CHUNK]
                dx = s[:, None, 0] - t[None, :, 0]
                dy = s[:, None, 1] - t[None, :, 1]
                dz = s[:, None, 2] - t[None, :, 2]
                d2 = (dx * dx + dy * dy) + dz * dz
                valid = (d2 <= cut) & ok[a:a + CHUNK, None]
                rows, cols = np.nonzero(valid)
                dv = d2[rows, cols]
                order = np.lexsort((keep[cols], dv, rows))                 # by row, then d2, then the original index
                idx_parts.append(keep[cols][order].astype(np.int32))
                d2_parts.append(dv[order])
                counts[a:a + CHUNK] = valid.sum(1)
    row_start = np.zeros(m + 1, np.int64)
    row_start[1:] = np.cumsum(counts)
    index = np.concatenate(idx_parts) if idx_parts else np.zeros(0, np.int32)
    d2o = np.concatenate(d2_parts).astype(f32) if d2_parts else np.zeros(0, f32)
    return row_start, index.astype(np.int32), d2o


def radius_count(src, tgt, radius):
    """-> count int32 [m]"""
    return np.diff(radius_brute(src, tgt, radius)[0]).astype(np.int32)


def first_of_rows(row_start, index, d2, max_nn):
    """the first max_nn entries of every row -> (row_start, index, d2)"""
    cnt = np.minimum(np.diff(row_start), max_nn)
    start = np.zeros(len(row_start), np.int64)
    start[1:] = np.cumsum(cnt)
    pos = np.concatenate([np.arange(b, b + c) for b, c in zip(row_start[:-1], cnt)]) if cnt.sum() else np.zeros(0, np.int64)
    return start, index[pos], d2[pos]


def remove_radius_outlier(points, nb_points, radius):
    """-> (kept indices int64 ascending, mask bool [n], count int32 [n])"""
    cnt = radius_count(points, points, radius)
    mask = cnt > nb_points
    return np.nonzero(mask)[0].astype(np.int64), mask, cnt


def cluster_dbscan(points, eps, min_points, details=False):
    """-> labels int32 [n]; with details also (core bool [n], clusters, border bool [n])"""
    pts = np.asarray(points).astype(f32)
    n = len(pts)
    row_start, index, _ = radius_brute(pts, pts, eps)
    cnt = np.diff(row_start)
    core = np.isfinite(pts).all(1) & (cnt >= min_points)
    labels = np.full(n, -1, np.int32)
    clusters = 0
    for i in range(n):                                                     # ascending: a component is met at its smallest core index
        if not core[i] or labels[i] >= 0:
            continue
        labels[i] = clusters
        stack = [i]
        while stack:
            a = stack.pop()
            for j in index[row_start[a]:row_start[a + 1]]:
                if core[j] and labels[j] < 0:
                    labels[j] = clusters
                    stack.append(int(j))
        clusters += 1
    border = np.zeros(n, bool)
    for i in np.nonzero(~core & np.isfinite(pts).all(1))[0]:
        nb = index[row_start[i]:row_start[i + 1]]
        nb = nb[core[nb]]
        if len(nb):
            labels[i] = labels[nb].min()
            border[i] = True
    return (labels, core, clusters, border) if details else labels


# ---- the constructed clouds --------------------------------------------------------------------------------------------------------------
PLATES_EPS, PLATES_MIN_POINTS = f32(2.0 ** -8), 4
CHAIN_EPS, CHAIN_N = f32(2.0 ** -8), 600


def two_plates():
    """Two 3 x 3 lattice plates of spacing 2^-8 in the plane z = 0, two spacings apart, and one point B between them at exactly eps = 2^-8
    from the middle of the facing edge of each -> (float32 [19, 3], the row of B, the row of plate 0's contact, the row of plate 1's
    contact).  With min_points = 4 a plate's corners (3 within eps) are borders, its edge middles (4, the contacts 5) and its centre (5)
    are core, and B (the two contacts and itself: 3) is not.  Row 0 is the centre of the plate at x = 0 .. 2: cluster 0.  Row 1 is the
    contact of the OTHER plate (cluster 1); the contact of plate 0 is the LAST row.  So B's core neighbours are row 1 (cluster 1) and
    row 18 (cluster 0), both at exactly eps: the statement gives B the label 0, while "the nearest core point" (ties by index) and
    "the lowest-indexed core point" both give 1."""
    plate0 = [(x, y) for y in range(3) for x in range(3)]
    plate1 = [(x + 4, y) for y in range(3) for x in range(3)]
    contact0, contact1, centre0, b = (2, 1), (4, 1), (1, 1), (3, 1)
    rest0 = [q for q in plate0 if q not in (contact0, centre0)]
    rest1 = [q for q in plate1 if q != contact1]
    rows = [centre0, contact1] + rest0 + rest1 + [b, contact0]
    pts = np.array([(x, y, 0) for x, y in rows], np.float64) * 2.0 ** -8
    return pts.astype(f32), len(rows) - 2, len(rows) - 1, 1


def chain(seed=5):
    """600 lattice points on a line, spacing 2^-8 (every coordinate and every d2 exact), rows shuffled by a fixed seed -> float32 [600, 3].
    With eps = 2^-8: an inner point has 3 within eps, an end point 2."""
    x = np.arange(CHAIN_N, dtype=np.float64) * 2.0 ** -8
    pts = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1).astype(f32)
    return pts[np.random.default_rng(seed).permutation(CHAIN_N)]
