"""Cloud-to-cloud distances on the device: the exact nearest neighbour of every point of one cloud in another.

The primitive is Open3D's ``PointCloud.compute_point_cloud_distance``, which the reference calls at
BodySLAM_not_refactored/3DM/mapping_module.py:45,48,62.  Open3D is not vendored: the meaning is restated from its documentation and
parity with Open3D is unpinned.  The arithmetic is fixed (include/bodyslam_hip.h, tests/_pointcloud_ref.py): in fp32 without contraction
d2 = (dx dx + dy dy) + dz dz, the neighbour is the lexicographic minimum of (d2, index in the target as given), the distance sqrtf(d2).
So the answer does not depend on the spatial index at all -- not on the cell size, not on the order points land in a cell -- and
``method="grid"`` and ``method="brute"`` return the same bits.

``NearestNeighbours`` builds a uniform grid over the finite target points once (csrc/pointcloud.hip: bounds, counts per cell, a scan,
a scatter into 16-byte records); ``query`` walks the shells of cells around every source point and hands the few points that are far
from everything to the brute-force kernel.  There is no CPU fallback: without a GPU the calls raise BodySlamHipError.

``query_knn`` extends the same walk from the minimum to the k smallest under the same total order (csrc/knn.hip; Open3D's
search_knn_vector_3d / search_hybrid_vector_3d), and two things stand on it: ``estimate_normals`` (PointCloud.estimate_normals) and
``remove_statistical_outlier`` (PointCloud.remove_statistical_outlier).  Restated, parity with Open3D unpinned; the statement is
tests/_knn_ref.py.

``voxel_down_sample`` (PointCloud.voxel_down_sample, PointCloud.voxel_down_sample_and_trace) thins a cloud to one point per occupied cube
(csrc/voxel.hip: a hash table of voxel keys, integer sums, rows in order of first appearance; Open3D's PointCloud.voxel_down_sample,
mapping_module.py:72,156,187).  Restated, parity with Open3D unpinned; the statement is tests/_voxel_ref.py.

``sample_mesh`` (TriangleMesh.sample_points_uniformly, mapping_module.py:289) draws points of a triangle mesh uniformly by area
(csrc/mesh_scene.hip: integer weights, an integer scan, a counter-based hash -- a sample depends on (seed, its number) alone).  Restated,
parity with Open3D unpinned; the statement is tests/_mesh_scene_ref.py.  Distances to the surface itself: bodyslam_amd/raycasting.py.

``query_radius`` / ``count_radius`` drop the cap on the list: every target point within a radius, however many (csrc/radius.hip; Open3D's
search_radius_vector_3d), and on them stand ``remove_radius_outlier`` (PointCloud.remove_radius_outlier) and ``cluster_dbscan``
(PointCloud.cluster_dbscan, made deterministic).  Restated, parity with Open3D unpinned; the statement is tests/_radius_ref.py.

``orient_normals_consistent_tangent_plane`` gives the normals of a cloud one sign per surface: the signs are propagated along the minimum
spanning tree of the k-NN graph (csrc/orient.hip: Boruvka's rounds by 64-bit integer atomics over a union-find with a parity bit,
csrc/union_parity.h; Open3D's PointCloud.orient_normals_consistent_tangent_plane without its Delaunay edges).  Restated, parity with Open3D
unpinned; the statement is tests/_orient_ref.py.

Not built: k > 32, Open3D's cubic-id trace format, Poisson-disk sampling of a mesh.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _args as AR
from . import _lib as L

SHELL_CAP = 8               # a source still searching after this shell goes to the brute-force kernel (a starting point, not tuned)
METHODS = ("grid", "brute")


as_points = AR.points


def _check_cell_size(cell_size) -> Optional[float]:
    if cell_size is None:
        return None
    return AR.number(cell_size, "cell_size", "None or a positive number (finite and non-zero in fp32)", AR.positive, fp32=True)


def _check_max_distance(max_distance) -> float:
    if max_distance is None:
        return math.inf
    return AR.number(max_distance, "max_distance", "None or a number >= 0", lambda v: v >= 0.0, fp32=True)


def _check_k(k, what: str = "k") -> int:
    return AR.integer(k, what, 1, L.PC_KNN_MAX)


def _check_radius(radius) -> float:
    """None -> inf (no radius); otherwise a positive number, finite and non-zero in fp32"""
    if radius is None:
        return math.inf
    return AR.number(radius, "radius", "None or a positive number (finite and non-zero in fp32)", AR.positive, fp32=True)


def _check_search_radius(radius, what: str = "radius") -> float:
    """a radius search needs its radius: a positive number, finite and non-zero in fp32"""
    return AR.number(radius, what, "a positive number (finite and non-zero in fp32)", AR.positive, fp32=True)


def _check_orientation(direction, camera_location) -> Tuple[int, Optional[np.ndarray]]:
    if direction is not None and camera_location is not None:
        raise ValueError("direction and camera_location are mutually exclusive")
    for name, v, mode in (("direction", direction, L.PC_ORIENT_DIRECTION), ("camera_location", camera_location, L.PC_ORIENT_CAMERA)):
        if v is None:
            continue
        try:
            a = np.asarray(_np(v), dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError(f"{name}: expected three finite numbers") from None
        if a.shape != (3,) or not np.isfinite(a).all():
            raise ValueError(f"{name}: expected three finite numbers")
        return mode, a
    return L.PC_ORIENT_AXIS, None


def grid_dims(lo: np.ndarray, hi: np.ndarray, h: float) -> np.ndarray:
    """cells per axis of the grid over [lo, hi] (fp32 [3] each) with edge h, in the kernels' fp32 arithmetic: floor((hi - lo) / h) + 1"""
    f32 = np.float32
    with np.errstate(over="ignore"):
        q = np.floor((hi.astype(f32) - lo.astype(f32)) / f32(h))
    return np.minimum(q, f32(2.0 ** 30)).astype(np.int64) + 1


def n_cells(dims) -> int:
    return int(dims[0]) * int(dims[1]) * int(dims[2])


def default_cell_size(lo: np.ndarray, hi: np.ndarray, n: int) -> float:
    """The default edge: over the k axes of positive extent, h = (the product of those extents / n)^(1 / k) -- about as many cells as
    points -- rounded to fp32, then grown by factors of 1.25 until the grid holds at most 2^24 cells.  No positive extent (one
    point, or all points equal): 1.0, a single cell."""
    ext = (hi.astype(np.float32) - lo.astype(np.float32)).astype(np.float64)
    pos = ext[(ext > 0.0) & np.isfinite(ext)]
    if pos.size == 0 or n < 1:
        return 1.0
    h = float(np.float32(np.exp((np.sum(np.log(pos)) - np.log(n)) / pos.size)))
    h = max(h, float(np.finfo(np.float32).tiny))
    while n_cells(grid_dims(lo, hi, h)) > L.PC_MAX_CELLS:
        h = float(np.float32(h * 1.25))
    return h


def radius_cell_size(lo: np.ndarray, hi: np.ndarray, radius: float) -> float:
    """The default edge of an index that is searched with one radius: the radius itself (one shell of cells then covers the search), rounded
    to fp32, then grown by factors of 1.25 until the grid holds at most 2^24 cells."""
    h = float(np.float32(radius))
    while n_cells(grid_dims(lo, hi, h)) > L.PC_MAX_CELLS:
        h = float(np.float32(h * 1.25))
    return h


def _decode_bounds(raw: np.ndarray) -> Tuple[np.ndarray, np.ndarray, int]:
    """bs_pc_bounds' 8 words -> (lo fp32 [3], hi fp32 [3], finite points)"""
    o = raw.astype(np.uint32).copy()
    o[3:6] = ~o[3:6]
    b = np.where((o[:6] & np.uint32(0x80000000)) != 0, o[:6] & np.uint32(0x7fffffff), ~o[:6]).astype(np.uint32)
    v = b.view(np.float32)
    return v[:3].copy(), v[3:6].copy(), int(o[6])


class NearestNeighbours:
    """The index over `target`, built once; ``query`` may be called any number of times.

    target: numpy array or torch tensor [n, 3], fp32 or fp64 (fp64 is rounded to fp32 once, before anything else: the neighbours are
    those of the rounded points), host or device; a tsdf.PointCloud; a tsdf.TriangleMesh (its vertices).  Non-finite target points are
    left out; indices always refer to `target` as given.  cell_size: the grid's edge, None = default_cell_size; a ValueError if the grid
    would exceed 2^24 cells.  The cell size changes the time, never the result.  ``for_radius`` builds the index with the default cell of a
    radius search."""

    def __init__(self, target, cell_size: Optional[float] = None, device: int = 0):
        self._build(target, cell_size, device, None)

    @classmethod
    def for_radius(cls, target, radius: float, cell_size: Optional[float] = None, device: int = 0) -> "NearestNeighbours":
        """The index for searches with one radius: as the constructor, but cell_size None means radius_cell_size -- the radius itself, as far
        as the grid allows, so that one shell of cells covers a search -- instead of default_cell_size."""
        nn = object.__new__(cls)
        nn._build(target, cell_size, device, _check_search_radius(radius))
        return nn

    def _build(self, target, cell_size, device, r):
        t = as_points(target, "target")
        h = _check_cell_size(cell_size)
        self.dev = AR.device_for(t, device=device)
        with torch.cuda.device(self.dev):
            self.target = t.to(self.dev).to(torch.float32).contiguous()
            raw = torch.empty(8, dtype=torch.int32, device=self.dev)
            L.pc_bounds(self.target, raw)
            lo, hi, n_finite = _decode_bounds(raw.cpu().numpy().view(np.uint32))
            if n_finite == 0:
                lo, hi = np.zeros(3, np.float32), np.zeros(3, np.float32)
            self.lo, self.hi, self.n_finite = lo, hi, n_finite
            self.cell_size = h if h is not None else default_cell_size(lo, hi, n_finite) if r is None else radius_cell_size(lo, hi, r)
            dims = grid_dims(lo, hi, self.cell_size)
            if n_cells(dims) > L.PC_MAX_CELLS:
                raise ValueError(f"cell_size {self.cell_size}: a grid of {dims[0]} x {dims[1]} x {dims[2]} cells, at most 2^24")
            self.dims = dims.astype(np.int32)
            cells = n_cells(dims)
            counts = torch.zeros(cells, dtype=torch.int32, device=self.dev)
            self.records = torch.empty(max(n_finite, 1), 4, dtype=torch.float32, device=self.dev)       # rows 0 .. n_finite - 1
            self.cell_start = torch.zeros(cells + 1, dtype=torch.int32, device=self.dev)
            if n_finite:
                L.pc_grid_count(self.target, lo, hi, self.cell_size, self.dims, counts)
                self.cell_start[1:] = torch.cumsum(counts, 0).to(torch.int32)                  # the scan is plumbing: integer, exact
                cursor = self.cell_start[:-1].clone()
                L.pc_grid_scatter(self.target, lo, hi, self.cell_size, self.dims, cursor, self.records, n_finite)

    def __len__(self) -> int:
        return int(self.target.shape[0])

    def query(self, source, max_distance: Optional[float] = None, method: str = "grid") -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (distance fp32 [n], index int32 [n]), device tensors: for every source point its nearest target point.

        source: as `target` (fp64 is rounded to fp32 once).  A source point with a non-finite coordinate gets (NaN, -1); without a finite
        target point every finite source gets (+inf, -1).  max_distance: a source whose distance is > max_distance (compared in fp32)
        gets (+inf, -1).  method: "grid" (the index; sources far from every target are finished by brute force) or "brute" (brute force
        for all: the path for small targets and the cross-check) -- the same bits either way."""
        if method not in METHODS:
            raise ValueError(f"unknown method {method!r}: one of {METHODS}")
        md = _check_max_distance(max_distance)
        s = as_points(source, "source")
        with torch.cuda.device(self.dev):
            s = s.to(self.dev).to(torch.float32).contiguous()
            m = int(s.shape[0])
            dist = torch.empty(m, dtype=torch.float32, device=self.dev)
            index = torch.empty(m, dtype=torch.int32, device=self.dev)
            if method == "grid":
                fb_list = torch.empty(m, dtype=torch.int32, device=self.dev)
                fb_count = torch.empty(1, dtype=torch.int32, device=self.dev)
                L.pc_query_grid(self.records, self.n_finite, self.cell_start, self.lo, self.hi, self.cell_size, self.dims, s, md, SHELL_CAP, dist, index, fb_list,
                                fb_count)
                n_fb = int(fb_count.cpu())
                if n_fb:
                    keys = torch.empty(n_fb, dtype=torch.int64, device=self.dev)
                    L.pc_query_brute(self.records, self.n_finite, s, fb_list, n_fb, md, keys, dist, index)
                self.last_fallback = n_fb
            else:
                keys = torch.empty(m, dtype=torch.int64, device=self.dev)
                L.pc_query_brute(self.records, self.n_finite, s, None, m, md, keys, dist, index)
        return dist, index


    def query_knn(self, source, k: int, radius: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """-> (index int32 [m, k], d2 fp32 [m, k], count int32 [m]), device tensors: for every source point its k nearest target points --
        Open3D's KDTreeFlann.search_knn_vector_3d, and with `radius` search_hybrid_vector_3d (restated, parity unpinned).

        The neighbours are the k lexicographically smallest (d2, index in the target as given) among the finite target points, ascending,
        d2 in ``query``'s fp32 arithmetic; with a radius a candidate counts only when sqrtf(d2) <= radius in fp32 (a target at exactly
        the radius is in).  Rows are padded with index -1 and d2 +inf; a source point with a non-finite coordinate gets count 0, index
        -1 and d2 NaN.  A source that is a point of the target finds itself first (d2 = 0).  1 <= k <= 32; for k = 1 the result is
        ``query``'s.  The walk has no shell cap and no brute-force fallback: a source far from every target, or a k above the number of
        targets in reach, costs time and never changes the result.  Every neighbour within a radius, however many: ``query_radius``."""
        k = _check_k(k)
        r = _check_radius(radius)
        s = as_points(source, "source")
        with torch.cuda.device(self.dev):
            s = s.to(self.dev).to(torch.float32).contiguous()
            m = int(s.shape[0])
            index = torch.empty(m, k, dtype=torch.int32, device=self.dev)
            d2 = torch.empty(m, k, dtype=torch.float32, device=self.dev)
            count = torch.empty(m, dtype=torch.int32, device=self.dev)
            L.pc_query_knn(self.records, self.n_finite, self.cell_start, self.lo, self.hi, self.cell_size, self.dims, s, k, r, index, d2, count)
        return index, d2, count

    def _index(self):
        return self.records, self.n_finite, self.cell_start, self.lo, self.hi, self.cell_size, self.dims

    def count_radius(self, source, radius: float) -> torch.Tensor:
        """-> count int32 [m], a device tensor: for every source point the number of finite target points within `radius` -- sqrtf(d2) <=
        radius in ``query``'s fp32 arithmetic, a target at exactly the radius is in; 0 for a source with a non-finite coordinate.  One
        launch (csrc/radius.hip, bs_pc_radius_count); the walk ends when its shells cover the radius."""
        r = _check_search_radius(radius)
        s = as_points(source, "source")
        with torch.cuda.device(self.dev):
            s = s.to(self.dev).to(torch.float32).contiguous()
            count = torch.empty(int(s.shape[0]), dtype=torch.int32, device=self.dev)
            L.pc_radius_count(self._index(), s, r, count)
        return count

    def query_radius(self, source, radius: float, max_nn: Optional[int] = None, sort: bool = True) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """-> (row_start int64 [m + 1], index int32 [total], d2 fp32 [total]), device tensors: for every source point ALL the target points
        within `radius`, however many -- Open3D's KDTreeFlann.search_radius_vector_3d (restated, parity unpinned; the statement is
        tests/_radius_ref.py).  Source i owns the entries row_start[i] .. row_start[i + 1] - 1.

        The rule is ``count_radius``'s; indices refer to the target as given.  Rows are in ascending (d2, index) order, ``query_knn``'s
        order: a source that is a point of the target finds itself first (d2 = 0).  sort=False skips the sort: the rows are then the same
        sets in an unspecified order.  max_nn keeps the first max_nn of every sorted row (it implies the sort).  A count launch, a scan,
        a fill launch, the sort and an unpack launch; total must stay below 2^31 (ValueError naming it, before anything is filled)."""
        r = _check_search_radius(radius)
        k = None if max_nn is None else AR.integer(max_nn, "max_nn", 1)
        s = as_points(source, "source")
        with torch.cuda.device(self.dev):
            s = s.to(self.dev).to(torch.float32).contiguous()
            m = int(s.shape[0])
            count = torch.empty(m, dtype=torch.int32, device=self.dev)
            L.pc_radius_count(self._index(), s, r, count)
            row_start = torch.zeros(m + 1, dtype=torch.int64, device=self.dev)
            row_start[1:] = torch.cumsum(count, 0, dtype=torch.int64)                          # the scan is plumbing: integer, exact
            total = int(row_start[-1].cpu())
            if total >= 2 ** 31:
                raise ValueError(f"radius {radius!r}: {total} neighbours in all, the lists hold fewer than 2^31; query fewer sources at a time")
            index = torch.empty(total, dtype=torch.int32, device=self.dev)
            d2 = torch.empty(total, dtype=torch.float32, device=self.dev)
            if total == 0:
                return row_start, index, d2
            keys = torch.empty(total, dtype=torch.int64, device=self.dev)
            status = torch.zeros(1, dtype=torch.int32, device=self.dev)
            L.pc_radius_fill(self._index(), s, r, row_start, total, keys, status)
            if sort or k is not None:
                ordered = torch.empty_like(keys)
                L.pc_radius_sort(keys, row_start, ordered)
                keys = ordered
            if int(status.cpu()):
                raise L.BodySlamHipError(f"query_radius: a row found more neighbours than were counted (status {int(status.cpu())})")
            if k is not None:                                                                   # a second scan and a gather: plumbing
                kept = count.clamp(max=k).to(torch.int64)
                start = torch.zeros(m + 1, dtype=torch.int64, device=self.dev)
                start[1:] = torch.cumsum(kept, 0)
                rows = torch.repeat_interleave(torch.arange(m, device=self.dev), kept)
                keys = keys[torch.arange(rows.numel(), device=self.dev) - start[rows] + row_start[rows]].contiguous()
                row_start = start
                index, d2 = index[:keys.numel()].contiguous(), d2[:keys.numel()].contiguous()
            L.pc_radius_unpack(keys, index, d2)
        return row_start, index, d2


last_rounds = 0                 # cluster_dbscan: the (hook, compress) rounds of the last call, the confirming one included; after
                                # orient_normals_consistent_tangent_plane: its Boruvka rounds, the one that found no edge included
last_clusters = 0               # cluster_dbscan: the clusters of the last call


def remove_radius_outlier(points, nb_points: int, radius: float, cell_size: Optional[float] = None,
                          device: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (the kept indices int64 ascending, the mask bool [n]), device tensors: Open3D's PointCloud.remove_radius_outlier (restated, parity
    unpinned; tests/_radius_ref.py).  A point is kept when the number of points of the cloud within `radius` of it, itself included
    (``count_radius`` of the cloud on itself), is > nb_points; a non-finite point is never kept.  nb_points >= 0, with no upper limit.
    cell_size None: radius_cell_size.  One count launch.  Raises ValueError on bad arguments before the GPU is touched."""
    nb = AR.integer(nb_points, "nb_points", 0)
    r = _check_search_radius(radius)
    _check_cell_size(cell_size)
    as_points(points, "points")
    nn = NearestNeighbours.for_radius(points, r, cell_size=cell_size, device=device)
    with torch.cuda.device(nn.dev):
        mask = nn.count_radius(nn.target, r) > nb                         # (the compaction is plumbing: a comparison and torch.nonzero)
        return torch.nonzero(mask).reshape(-1), mask


def cluster_dbscan(points, eps: float, min_points: int, cell_size: Optional[float] = None, device: int = 0) -> torch.Tensor:
    """-> labels int32 [n], a device tensor, -1 for noise: Open3D's PointCloud.cluster_dbscan, made deterministic (restated, parity
    unpinned; tests/_radius_ref.py).  ``last_clusters`` and ``last_rounds`` hold the number of clusters and the rounds the labelling took.

    With ``count_radius``'s rule for "within eps": a finite point is CORE when it has at least min_points points within eps, itself
    included.  The clusters are the connected components of the core points under "within eps", numbered 0, 1, ... in ascending order of
    their smallest core index.  A finite non-core point with a core point within eps is a BORDER: it takes the smallest cluster number
    among those core points (not the nearest one's).  Everything else, and every non-finite point, is noise.  This is what the textbook
    scan gives when it visits the points in ascending index order; the result does not depend on any schedule.

    csrc/radius.hip: a count launch, then rounds of (hook the core neighbours by minimum, compress) until nothing changes -- the
    neighbourhood is walked again every round, memory stays O(n) -- then the roots, a scan and the labels.  cell_size None:
    radius_cell_size.  Raises ValueError on bad arguments before the GPU is touched."""
    global last_rounds, last_clusters
    r = _check_search_radius(eps, "eps")
    mp = AR.integer(min_points, "min_points", 1, 2 ** 31 - 1)
    _check_cell_size(cell_size)
    as_points(points, "points")
    nn = NearestNeighbours.for_radius(points, r, cell_size=cell_size, device=device)
    n, idx = len(nn), nn._index()
    with torch.cuda.device(nn.dev):
        i32 = dict(dtype=torch.int32, device=nn.dev)
        count = nn.count_radius(nn.target, r)
        parent = torch.arange(n, **i32)
        changed = torch.zeros(1, **i32)
        rounds = 0
        for _ in range(n + 1):                       # every round that reports a change removes a root for good: at most n do
            changed.zero_()
            L.pc_dbscan_hook(idx, nn.target, r, count, mp, parent, changed)
            L.pc_dbscan_compress(parent)
            rounds += 1
            if int(changed.cpu()) == 0:
                break
        else:
            raise L.BodySlamHipError(f"cluster_dbscan: no fixed point after {n + 1} rounds")
        is_root = torch.empty(n, **i32)
        L.pc_dbscan_roots(parent, count, mp, is_root)
        rank = torch.cumsum(is_root, 0).to(torch.int32)                   # the scan is plumbing: integer, exact
        clusters = int(rank[-1].cpu())
        labels = torch.empty(n, **i32)
        L.pc_dbscan_labels(idx, nn.target, r, count, mp, parent, rank, clusters, labels)
    last_rounds, last_clusters = rounds, clusters
    return labels


def estimate_normals(points, k: int = 30, radius: Optional[float] = None, direction=None, camera_location=None,
                     cell_size: Optional[float] = None, device: int = 0, return_eigenvalues: bool = False):
    """Normals of a cloud that has none -> fp32 [n, 3] device tensor (and, with return_eigenvalues, the eigenvalues fp64 [n, 3] ascending):
    Open3D's PointCloud.estimate_normals with KDTreeSearchParamKNN(k) or, with `radius`, KDTreeSearchParamHybrid(radius, k).  Open3D is
    not vendored: the meaning is restated from its documentation and parity with Open3D is unpinned; the statement is tests/_knn_ref.py.

    Per point, over its neighbours in ``query_knn``'s order (itself included), in fp64: the covariance C of the neighbours, the Jacobi
    eigen-decomposition of csrc/svd3.h, the unit eigenvector of the smallest eigenvalue, rounded to fp32 once.  The normal is zero when
    there are fewer than 3 neighbours or the largest eigenvalue is not positive and finite -- the convention of PointCloud.normals and of
    registration_icp: a zero normal leaves its pairs out; for exactly collinear neighbours the direction is unspecified.  Sign:
    direction=v flips when n . v < 0, camera_location=c when n . (c - p) < 0 (the two exclude each other); with neither, the component
    of largest magnitude is made positive, so that the result is deterministic -- not one sign per surface: on a tube both signs appear.
``orient_normals_consistent_tangent_plane`` propagates one sign along a spanning tree.
    The cell size changes the time, never the bits.  Raises ValueError on bad arguments before the GPU is touched."""
    k = _check_k(k)
    _check_radius(radius)
    mode, vec = _check_orientation(direction, camera_location)
    _check_cell_size(cell_size)
    as_points(points, "points")
    nn = NearestNeighbours(points, cell_size=cell_size, device=device)
    with torch.cuda.device(nn.dev):
        index, _, count = nn.query_knn(nn.target, k, radius)
        n = len(nn)
        normals = torch.empty(n, 3, dtype=torch.float32, device=nn.dev)
        eig = torch.empty(n, 3, dtype=torch.float64, device=nn.dev) if return_eigenvalues else None
        L.pc_normals(nn.target, index, count, k, mode, vec, normals, eig)
    return (normals, eig) if return_eigenvalues else normals


last_components = 0             # orient_normals_consistent_tangent_plane: the trees of the last call (one per component of the valid points)


def _check_items(n: int, what: str) -> int:
    """union_parity.h packs parent << 1 | parity into 32 bits"""
    if n > L.ORIENT_MAX_ITEMS:
        raise ValueError(f"{what}: {n} rows, at most 2^30 can be oriented")
    return n


def orient_normals_consistent_tangent_plane(points, normals, k: int, direction=(0.0, 0.0, 1.0), cell_size: Optional[float] = None,
                                            device: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """One sign per surface -> (normals fp32 [n, 3], flipped bool [n]), device tensors: the role of Open3D's
    PointCloud.orient_normals_consistent_tangent_plane(k) (Hoppe et al. 1992).  Open3D is not vendored: the meaning is restated from its
    documentation and parity with Open3D is unpinned; the statement is tests/_orient_ref.py and the result is bit-equal to it, the same bits
    in every run.  ``last_components`` and ``last_rounds`` hold the number of trees and the rounds the last call took.

    A point is VALID when its coordinates are finite and its normal is finite and not all zero.  The graph: the undirected edge {i, j},
    i != j, exists when j is in row i of ``query_knn(cloud, cloud, k)`` or i in row j, and both ends are valid; k counts the point itself,
    as in ``estimate_normals``, 2 <= k <= 32.  In fp64 without contraction, on the fp32 normals: d = (ax bx + ay by) + az bz, the weight
    w = fl32(max(1 - |d|, 0)), the sign link s = (d < 0).  Edges are ordered by (the bits of w, min(i, j), max(i, j)); under that total
    order the minimum spanning forest is unique (on a plane every weight is exactly 0: the indices decide).  Per tree the seed is the valid
    point of largest fp32 z, ties to the lowest index; it is flipped when n . direction < 0 (the same fp64 expression; 0 does not flip), and
    flip(x) = the seed's flip xor the parity of the signs s along the tree path from x to the seed.  A flipped normal has its three sign
    bits toggled; invalid rows come back bit for bit and are never traversed.

    Departure from Open3D: no Delaunay edges are added to the k-NN graph, so a disconnected graph gives several trees and each is oriented
    on its own (``last_components`` tells); Open3D's lambda / cos_alpha_tol penalties are not built.

    csrc/orient.hip: Boruvka's rounds on the k-NN lists as they lie -- clear, select the (w, low index) minimum per root by 64-bit integer
    atomics, select the high index, hook with a parity bit (csrc/union_parity.h), compress -- until a round finds no edge between two
    trees, then the seeds and the flips.  The cell size changes the time, never the bits.  Raises ValueError on bad arguments before the GPU
    is touched; there is no CPU fallback."""
    global last_components, last_rounds
    k = AR.integer(k, "k", 2, L.PC_KNN_MAX)
    _, vec = _check_orientation(direction, None)
    if vec is None:
        raise ValueError("direction: expected three finite numbers")
    _check_cell_size(cell_size)
    pts = as_points(points, "points")
    n = _check_items(int(pts.shape[0]), "points")
    nrm = _as_attribute(normals, "normals", n)
    if nrm is None:
        raise ValueError(f"normals: expected a float32 or float64 array or tensor of shape [{n}, 3]")
    nn = NearestNeighbours(pts, cell_size=cell_size, device=device)
    dev = nn.dev
    with torch.cuda.device(dev):
        nrm = nrm.to(dev).to(torch.float32).contiguous()
        index, _, count = nn.query_knn(nn.target, k)
        i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
        keys, valid = torch.empty(n * k, **i64), torch.empty(n, **i32)
        L.pc_orient_edges(nn.target, nrm, index, count, keys, valid)
        word = torch.arange(n, **i32) * 2                                    # parent << 1 | parity: every point its own root
        best, best_hi = torch.empty(n, **i64), torch.empty(n, **i32)
        crossing = torch.zeros(1, **i32)
        rounds = 0
        for _ in range(n + 1):                       # every round that finds a crossing edge hooks one for good: at most n - 1 do
            crossing.zero_()
            L.pc_orient_clear(best, best_hi)
            L.pc_orient_select(keys, index, word, best, crossing)
            rounds += 1
            if int(crossing.cpu()) == 0:
                break
            L.pc_orient_select_hi(keys, index, word, best, best_hi)
            L.pc_orient_hook(nrm, word, best, best_hi)
            L.pc_orient_compress(word)
        else:
            raise L.BodySlamHipError(f"orient_normals_consistent_tangent_plane: still an edge between two trees after {n + 1} rounds")
        L.pc_orient_clear(best)                                               # (best now holds the seeds)
        L.pc_orient_seed(nn.target, valid, word, best)
        out, flipped = torch.empty(n, 3, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
        L.pc_orient_flip(nrm, valid, word, best, vec, out, flipped)
        last_components, last_rounds = int((best != L.ORIENT_NO_KEY).sum().cpu()), rounds
    return out, flipped.to(torch.bool)


def knn_mean_distance(points, nb_neighbors: int = 20, cell_size: Optional[float] = None, device: int = 0) -> torch.Tensor:
    """fp32 [n] device tensor: for every point the mean distance to its nb_neighbors nearest points of the same cloud, itself included --
    fl32((sum_j (double) sqrtf(d2_j)) / count) in ``query_knn``'s order; NaN for a non-finite point."""
    k = _check_k(nb_neighbors, "nb_neighbors")
    _check_cell_size(cell_size)
    as_points(points, "points")
    nn = NearestNeighbours(points, cell_size=cell_size, device=device)
    with torch.cuda.device(nn.dev):
        _, d2, count = nn.query_knn(nn.target, k)
        avg = torch.empty(len(nn), dtype=torch.float32, device=nn.dev)
        L.pc_knn_mean_distance(d2, count, k, avg)
    return avg


def remove_statistical_outlier(points, nb_neighbors: int = 20, std_ratio: float = 2.0, cell_size: Optional[float] = None,
                               device: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (the kept indices int64 ascending, the mask bool [n]), device tensors: Open3D's PointCloud.remove_statistical_outlier, which the
    reference runs on its scene cloud with (20, 2.0) (restated, parity unpinned; tests/_knn_ref.py).

    avg = ``knn_mean_distance``; over its finite entries bs_pc_stats gives n, sum and sum of squares in its fixed order; in fp64
    mean = sum / n, std = sqrt(max(sumsq - n mean^2, 0) / (n - 1)) (0 for n < 2); a point is kept when (double) avg < mean + std_ratio std.
    A non-finite point is never kept.  1 <= nb_neighbors <= 32.  Raises ValueError on bad arguments before the GPU is touched."""
    AR.number(std_ratio, "std_ratio", "a finite number")
    avg = knn_mean_distance(points, nb_neighbors, cell_size=cell_size, device=device)
    with torch.cuda.device(avg.device):
        ws = torch.empty(L.PC_STATS_WORKSPACE_BYTES, dtype=torch.uint8, device=avg.device)
        out = torch.empty(L.PC_STATS_FIELDS, dtype=torch.float64, device=avg.device)
        L.pc_stats(avg, (), ws, out)
        rec = out.cpu().numpy()
        n, total, sumsq = rec[1], rec[4], rec[5]
        if n == 0:
            threshold = math.nan
        else:
            mean = total / n
            std = math.sqrt(max(sumsq - n * mean * mean, 0.0) / (n - 1)) if n >= 2 else 0.0
            threshold = mean + float(std_ratio) * std
        mask = avg.to(torch.float64) < threshold                     # (the compaction is plumbing: a comparison and torch.nonzero)
        return torch.nonzero(mask).reshape(-1), mask


@dataclass
class VoxelDownSample:
    """voxel_down_sample's result, device tensors; m voxels in order of first appearance"""
    points: torch.Tensor                    # fp32 [m, 3]
    colors: Optional[torch.Tensor]          # fp32 [m, 3], None when no colours were given
    normals: Optional[torch.Tensor]         # fp32 [m, 3], None when no normals were given
    counts: torch.Tensor                    # int32 [m]: the points in the voxel
    first_index: torch.Tensor               # int32 [m]: the voxel's lowest point index
    row_of_point: torch.Tensor              # int32 [n]: the row every input point went to, -1 for a non-finite point


def _check_voxel_size(voxel_size) -> float:
    return AR.number(voxel_size, "voxel_size", "a positive finite number", AR.positive)


def _as_attribute(a, what: str, n: int) -> Optional[torch.Tensor]:
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a)) if a.dtype in (np.float32, np.float64) else a
    if not isinstance(a, torch.Tensor) or a.dtype not in (torch.float32, torch.float64) or tuple(a.shape) != (n, 3):
        raise ValueError(f"{what}: expected a float32 or float64 array or tensor of shape [{n}, 3]")
    return a.detach()


def voxel_geometry(lo: np.ndarray, hi: np.ndarray, h: float) -> Tuple[np.ndarray, int]:
    """-> (the origin o = (double) lo - 0.5 h as float64 [3], the shift s = 32 - e with max((double) hi - o) = f 2^e, 0.5 <= f < 1) of the voxel
    grid over the fp32 bounds lo, hi; ValueError when an axis would need 2^21 voxels or more"""
    o = lo.astype(np.float64) - 0.5 * h
    ext = hi.astype(np.float64) - o
    with np.errstate(over="ignore", invalid="ignore"):
        top = np.floor(ext / h)
    if not bool((top < 2.0 ** L.PC_VOXEL_AXIS_BITS).all()):
        raise ValueError(f"voxel_size {h!r} too small: {float(top.max()):.0f} voxels along an axis, at most 2^{L.PC_VOXEL_AXIS_BITS}")
    return o, 32 - int(math.frexp(float(ext.max()))[1])


def voxel_table_slots(n: int) -> int:
    """the default table: the smallest power of two that is at least 2 n (the kernels need a power of two above n)"""
    return 1 << max(int(2 * n - 1).bit_length(), 1)


def voxel_down_sample(points, voxel_size, colors=None, normals=None, unit_normals=False, device: int = 0) -> VoxelDownSample:
    """One point per occupied cube of edge voxel_size: Open3D's PointCloud.voxel_down_sample, which the reference runs on its clouds with
    0.005, 0.009 and 0.05 m (3DM/mapping_module.py:72,156,187) -> VoxelDownSample, device tensors.  Open3D is not vendored: the meaning is
    restated from its documentation and parity with Open3D is unpinned; the statement is tests/_voxel_ref.py, and the result is bit-equal
    to it: the same bits in every run, for every order the atomics arrive in.

    points: as ``as_points`` takes them (fp64 is rounded to fp32 once); a point with a non-finite coordinate belongs to no voxel.  With
    lo, hi the fp32 bounds of the finite points and h = voxel_size as a double: the grid's origin is o = (double) lo - 0.5 h; a point's
    voxel floor(((double) p - o) / h) per axis in fp64, each component below 2^21 (else ValueError, decided from the bounds before any
    voxel kernel runs).  Rows come in order of first appearance.  A voxel's position is the mean of its points in exact integer
    arithmetic -- Q = rint(((double) p - o) 2^s) with s chosen so that the extent fills 32 bits, S = sum Q, fl32(o + S / count / 2^s): off
    the fp64 mean by less than extent 2^-32 plus half an fp32 ulp -- and a voxel of exactly one point returns that point's bits, its
    colour's and normal's too.  colors, normals: [n, 3] fp32 or fp64, every component of a point in a voxel finite with |a| <= 2 (else
    ValueError after the call's read-back), averaged alike with 30 fractional bits: the plain mean, as Open3D documents.  unit_normals
    scales every averaged normal to unit length in fp64 before the rounding (zero when its length is not positive): what
    registration_icp wants from a thinned cloud.  counts, first_index and row_of_point play the role of voxel_down_sample_and_trace in
    tensor form; Open3D's own trace format (the cubic-id matrix) is not built.  Without a finite point every output is empty.  Raises
    ValueError on bad arguments before the GPU is touched; there is no CPU fallback."""
    h = _check_voxel_size(voxel_size)
    t = as_points(points, "points")
    n = int(t.shape[0])
    c, nr = _as_attribute(colors, "colors", n), _as_attribute(normals, "normals", n)
    dev = AR.device_for(t, device=device)
    with torch.cuda.device(dev):
        pts = t.to(dev).to(torch.float32).contiguous()
        c, nr = (None if a is None else a.to(dev).to(torch.float32).contiguous() for a in (c, nr))
        raw = torch.empty(8, dtype=torch.int32, device=dev)
        L.pc_bounds(pts, raw)
        lo, hi, n_finite = _decode_bounds(raw.cpu().numpy().view(np.uint32))
        if n_finite == 0:
            def empty(given=True):
                return torch.empty(0, 3, dtype=torch.float32, device=dev) if given else None
            none = torch.empty(0, dtype=torch.int32, device=dev)
            return VoxelDownSample(empty(), empty(c is not None), empty(nr is not None), none, none.clone(),
                                   torch.full((n,), -1, dtype=torch.int32, device=dev))
        origin, shift = voxel_geometry(lo, hi, h)
        return _voxel_rows(pts, c, nr, origin, h, shift, bool(unit_normals), voxel_table_slots(n))


def _voxel_rows(pts, colors, normals, origin, h, shift, unit_normals, slots) -> VoxelDownSample:
    """the four launches over fp32 device tensors, with the table size as an argument (the result does not depend on it)"""
    dev, n = pts.device, int(pts.shape[0])
    i32 = dict(dtype=torch.int32, device=dev)
    keys = torch.full((slots,), L.PC_VOXEL_EMPTY_KEY, dtype=torch.int64, device=dev)           # (the fills and the scan are plumbing)
    first = torch.full((slots,), L.PC_VOXEL_NO_POINT, **i32)
    slot_of_point, row_of_point = torch.empty(n, **i32), torch.empty(n, **i32)
    status = torch.zeros(1, **i32)
    L.pc_voxel_assign(pts, origin, h, keys, first, slot_of_point, status)
    leader, rank, (m,) = AR.first_ranks(L.pc_voxel_flags, slot_of_point, first)
    if m == 0:                                                                                   # (only with a status bit set)
        _voxel_status(int(status.cpu()), h)
        raise L.BodySlamHipError("voxel_down_sample: no voxel for the finite points")
    terms = 3 + 3 * (colors is not None) + 3 * (normals is not None)
    sums = torch.zeros(m, terms, dtype=torch.int64, device=dev)
    counts = torch.zeros(m, **i32)
    first_index = torch.empty(m, **i32)
    L.pc_voxel_accumulate(pts, colors, normals, origin, shift, leader, rank, sums, counts, first_index, row_of_point, status)
    out = [None if a is None else torch.empty(m, 3, dtype=torch.float32, device=dev) for a in (pts, colors, normals)]
    L.pc_voxel_finish(pts, colors, normals, sums, counts, first_index, origin, shift, unit_normals, *out)
    _voxel_status(int(status.cpu()), h)
    return VoxelDownSample(out[0], out[1], out[2], counts, first_index, row_of_point)


def _voxel_status(word: int, h: float) -> None:
    if word & L.PC_VOXEL_TABLE_FULL:
        raise L.BodySlamHipError("voxel_down_sample: the voxel table is full")
    if word & L.PC_VOXEL_OUT_OF_RANGE:
        raise ValueError(f"voxel_size {h!r} too small: a voxel coordinate outside [0, 2^{L.PC_VOXEL_AXIS_BITS})")
    if word & L.PC_VOXEL_BAD_ATTRIBUTE:
        raise ValueError("colors / normals: every component must be finite with |a| <= 2")
    if word:
        raise L.BodySlamHipError(f"voxel_down_sample: status {word}")


def _check_count(n, what: str, lo: int, hi: int) -> int:
    return AR.integer(n, what, lo, hi - 1)


def sample_mesh(vertices, triangles, number_of_points, vertex_colors=None, seed: int = 0, first: int = 0, device: int = 0):
    """Points drawn uniformly by area from a triangle mesh: Open3D's TriangleMesh.sample_points_uniformly, which the reference runs on its
    mesh at 3DM/mapping_module.py:289 -> (points fp32 [n, 3], colors fp32 [n, 3] or None, normals fp32 [n, 3], triangle int32 [n]), device
    tensors.  Open3D is not vendored: the meaning is restated from its documentation and parity with Open3D is unpinned; the statement is
    tests/_mesh_scene_ref.py, and the result is bit-equal to it.

    vertices [V, 3] fp32 or fp64 (rounded to fp32 once), triangles [T, 3] integers, T <= 2^22, numpy or torch, host or device; an index
    outside [0, V) is a ValueError.  A triangle with a non-finite vertex or a zero fp32 cross product has weight 0.  Weights are integers,
    w = floor(area / max area 2^40) with fp64 areas, scanned exactly; sample i (numbered from `first`: a cloud may be drawn in batches,
    each sample depends on (seed, i) alone) takes three values of a counter-based hash of (seed, i): the first picks the triangle by
    multiply-high against the total and a bisection of the scan, the others give r1, r2 = (k + 0.5) 2^-24 and the point
    (1 - s) A + s (1 - r2) B + s r2 C with s = sqrt(r1), in one fixed fp32 expression.  colors: the same weights on vertex_colors [V, 3];
    normals: the unit (v1 - v0) x (v2 - v0) of the sample's triangle.  A mesh without a triangle of positive weight returns empty tensors.
    Raises ValueError on bad arguments before any kernel runs; there is no CPU fallback."""
    from .raycasting import as_triangles, check_indices
    n = _check_count(number_of_points, "number_of_points", 1, 2 ** 31)
    seed, first = _check_count(seed, "seed", 0, 2 ** 64), _check_count(first, "first", 0, 2 ** 63)
    v, t = as_triangles(vertices, triangles)
    if t.shape[0] > L.MESH_MAX_SAMPLED_TRIANGLES:
        raise ValueError(f"triangles: {t.shape[0]} rows, at most 2^22 can be sampled")
    c = _as_attribute(vertex_colors, "vertex_colors", int(v.shape[0]))
    dev = AR.device_for(v, device=device)
    with torch.cuda.device(dev):
        v, t = v.to(dev), t.to(dev)
        check_indices(t, int(v.shape[0]))
        v, t = v.to(torch.float32).contiguous(), t.to(torch.int32).contiguous()
        c = None if c is None else c.to(dev).to(torch.float32).contiguous()
        T = int(t.shape[0])
        f = dict(dtype=torch.float32, device=dev)

        def empty():
            return (torch.empty(0, 3, **f), None if c is None else torch.empty(0, 3, **f), torch.empty(0, 3, **f),
                    torch.empty(0, dtype=torch.int32, device=dev))
        if T == 0:
            return empty()
        records = torch.empty(T, 3, 4, **f)
        kept = torch.empty(1, dtype=torch.int32, device=dev)
        L.mesh_records(v, t, records, kept)
        weights = torch.empty(T, dtype=torch.int64, device=dev)
        L.mesh_sample_weights(records, torch.empty(T, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.int64, device=dev), weights)
        cum = torch.cumsum(weights, 0)                                       # the scan is plumbing: int64, exact (T 2^40 <= 2^62)
        if int(cum[-1].cpu()) == 0:
            return empty()
        points, normals = torch.empty(n, 3, **f), torch.empty(n, 3, **f)
        colors = None if c is None else torch.empty(n, 3, **f)
        index = torch.empty(n, dtype=torch.int32, device=dev)
        L.mesh_sample(records, cum, t if c is not None else None, c, seed, first, points, colors, normals, index)
    return points, colors, normals, index


def point_cloud_distance(source, target, cell_size: Optional[float] = None, device: int = 0, max_distance: Optional[float] = None,
                         method: str = "grid") -> Tuple[torch.Tensor, torch.Tensor]:
    """NearestNeighbours(target, cell_size, device).query(source, max_distance, method) in one call."""
    if method not in METHODS:
        raise ValueError(f"unknown method {method!r}: one of {METHODS}")
    _check_max_distance(max_distance)
    as_points(source, "source")
    return NearestNeighbours(target, cell_size=cell_size, device=device).query(source, max_distance=max_distance, method=method)


def transform_points(points, transform) -> torch.Tensor:
    """s R p + t on the device in fp64, rounded once to fp32 -> fp32 [n, 3] device tensor.  transform: a 4 x 4 (its top three rows are
    applied) or (R [3, 3], s, t [3]) as evaluation.similarity_transform returns it."""
    A = affine_rows(transform)
    p = as_points(points, "points")
    dev = AR.device_for(p)
    with torch.cuda.device(dev):
        p = p.to(dev).contiguous()
        out = torch.empty(p.shape[0], 3, dtype=torch.float32, device=dev)
        L.pc_transform(p, A, out)
    return out


def affine_rows(transform) -> np.ndarray:
    """-> float64 [3, 4] = [s R | t]; ValueError on anything that is neither a 4 x 4 nor (R, s, t)"""
    if isinstance(transform, (tuple, list)) and len(transform) == 3:
        R, s, t = transform
        R, t = np.asarray(_np(R), dtype=np.float64), np.asarray(_np(t), dtype=np.float64).reshape(-1)
        if R.shape != (3, 3) or t.shape != (3,):
            raise ValueError(f"transform (R, s, t): R {R.shape}, t {t.shape}; expected [3, 3] and [3]")
        try:
            s = float(s)
        except (TypeError, ValueError):
            raise ValueError(f"transform (R, s, t): s {s!r} is not a number") from None
        return np.concatenate([s * R, t[:, None]], 1)
    try:
        T = np.asarray(_np(transform), dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("transform: expected a 4 x 4 or (R, s, t)") from None
    if T.shape != (4, 4):
        raise ValueError(f"transform: shape {T.shape}, expected a 4 x 4 or (R, s, t)")
    return T[:3].copy()


def _np(m):
    return m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else m
