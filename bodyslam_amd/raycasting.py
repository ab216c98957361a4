"""A scene of triangle meshes on the device: the nearest hit of a ray and the closest surface point of a query point.

The surface is Open3D's ``t.geometry.RaycastingScene`` (add_triangles, create_rays_pinhole, cast_rays, compute_closest_points,
compute_distance), which the reference uses to render synthetic depth from a mesh (BodySLAM_not_refactored/3DM/mapping_module.py:204-237,
3DM/synthetic_depth_generator.py:24-97).  Open3D and Embree are not vendored: the meaning is restated from Open3D's documented interface
and parity with Open3D / Embree is UNPINNED.  The arithmetic is fixed instead (csrc/mesh_scene.hip, tests/_mesh_scene_ref.py): fp32
without contraction, a watertight two-sided ray / triangle test (Woop, Benthin, Wald 2013) whose edge functions are exactly negated across
a shared edge, Ericson's closest point on a triangle, and the answer of a query is the minimum of (t or d2, global triangle index) -- a
total order, so no result depends on how the work is spread, and every output is bit-equal to the numpy statement.

The index is a uniform grid over the scene's box, built on the device (count, an integer scan, scatter, as NearestNeighbours): a triangle
is referenced from every cell its padded box overlaps.  ``method="grid"`` walks it -- a 3-D DDA for rays, pointcloud's Chebyshev shells for
distances -- and hands what the walk does not cover (rays from far outside the box, points far from every triangle) to the brute-force
kernels (rays across lanes, triangles streamed through LDS tiles); ``method="brute"`` is those kernels for everything, the cross-check.
The cell size changes the time, never the result: both methods return the same bits (the bound: top of csrc/mesh_scene.hip).  There is no
CPU fallback: without a GPU the calls raise BodySlamHipError.

Every hit of a ray, not the nearest (count_intersections, list_intersections, test_occlusions; compute_occupancy and
compute_signed_distance are composed from the counts): the same walk without its early stop, every triangle tested in the first visited
cell of its cell range, and -- for counts and lists -- a COUNTING predicate: cast_rays' arithmetic, except that an edge value of exactly 0
takes the sign it would have with the ray moved by (eps, eps^2) in the sheared plane, so that exactly one of the triangles at a shared edge
or vertex claims the ray and the parity of a count is right for a closed mesh (tests/_mesh_hits_ref.py; parity with Open3D unpinned).

Not built: BVHs, a fused pinhole kernel that never materialises rays.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _args as AR
from . import _lib as L
from . import pointcloud as PC

# sample j of an occupancy query casts along row j: exactly representable directions
OCCUPANCY_DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, 0, 0), (0, -1, 0), (0, 0, -1), (-1, -1, -1),
                        (1, -1, -1), (-1, 1, -1), (-1, -1, 1), (1, 2, 3))
INVALID_ID = 0xFFFFFFFF             # geometry_ids / primitive_ids of a miss: the bit pattern of -1 in the int32 tensors returned
METHODS = ("grid", "brute")
SHELL_CAP = PC.SHELL_CAP


def max_references(n_triangles: int) -> int:
    """the reference table's limit: max(8 T, 2^16) (and what an int32 scan holds)"""
    return min(max(8 * int(n_triangles), 1 << 16), (1 << 31) - 1)


def grid_padding(lo: np.ndarray, hi: np.ndarray):
    """-> (pad, origin limit) in fp32: M = max |lo|, |hi| + the largest extent; pad = 2^-9 largest extent + 2^-14 M is what every triangle's
    box is grown by; a ray whose origin has a coordinate beyond 8 M in magnitude is not walked (csrc/mesh_scene.hip derives both)"""
    f32 = np.float32
    ext = (hi.astype(f32) - lo.astype(f32)).max()
    M = f32(max(np.abs(lo).max(), np.abs(hi).max())) + ext
    return float(ext * f32(2.0 ** -9) + M * f32(2.0 ** -14)), float(f32(8) * M)


def as_triangles(vertices, triangles=None):
    """-> (vertices fp32 or fp64 torch [V, 3], triangles torch integer [T, 3]) where they lie.  (vertices, triangles): numpy arrays or torch
    tensors, or a tsdf.TriangleMesh alone.  ValueError on anything else; the index range is checked where the data is (check_indices)."""
    return AR.triangles(vertices, triangles)


def check_indices(t: torch.Tensor, n_vertices: int) -> None:
    """ValueError when an index lies outside [0, V): decided where the triangles are, with one read-back, before any kernel follows one"""
    if t.numel() and bool(((t < 0) | (t >= n_vertices)).any()):
        raise ValueError(f"triangles: an index outside [0, {n_vertices})")


def _as_rows(x, width: int, what: str) -> torch.Tensor:
    x = AR.floating(x, what)
    if x.dim() < 1 or x.shape[-1] != width:
        raise ValueError(f"{what}: shape {tuple(x.shape)}, expected [..., {width}]")
    if x.numel() // width >= 2 ** 31:
        raise ValueError(f"{what}: {x.numel() // width} rows, at most 2^31 - 1")
    return x


def _check_method(method) -> None:
    if method not in METHODS:
        raise ValueError(f"unknown method {method!r}: one of {METHODS}")


def _check_range(tnear, tfar):
    """-> (tnear, tfar) as the fp32 values the kernels compare with; ValueError for anything but two numbers that are not NaN"""
    out = []
    for name, v in (("tnear", tnear), ("tfar", tfar)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or v != v:
            raise ValueError(f"{name} {v!r}: expected a number")
        out.append(float(np.float32(v)))
    return tuple(out)


def _check_nsamples(nsamples) -> int:
    n = AR.integer(nsamples, "nsamples", 1, len(OCCUPANCY_DIRECTIONS), "an odd integer in 1 .. 15")
    if n % 2 == 0:
        raise ValueError(f"nsamples {nsamples!r}: expected an odd integer in 1 .. 15")
    return n


class RaycastingScene:
    """Triangle meshes to cast rays at and to measure distances to; geometries are added with ``add_triangles`` and the device arrays are
    rebuilt lazily by the first query after an add.  device: the GPU's index.  cell_size: the grid's edge; None: pointcloud.default_cell_size
    over the scene's box and its kept triangles, grown by factors of 1.25 until the grid has at most 2^24 cells and the table at most
    max(8 T, 2^16) references; an explicit one that breaks either limit raises ValueError at the first query.  The cell size changes the
    time, never the result.  last_fallback: how many rays or points of the last grid query were finished by brute force."""

    def __init__(self, device: int = 0, cell_size: Optional[float] = None):
        self._cell_size = PC._check_cell_size(cell_size)
        self.last_fallback = 0
        self.dev = AR.device_for(device=AR.integer(device, "device", 0, None, "a GPU index"))
        self._geometries = []                      # (vertices fp32 [V, 3], triangles int32 [T, 3]) on the device
        self._dirty = True
        self.n_triangles = self.n_kept = 0
        self.records = self.geom_start = None

    def add_triangles(self, vertices, triangles=None) -> int:
        """(vertices [V, 3] fp32 or fp64 -- rounded to fp32 once --, triangles [T, 3] integers), numpy or torch, host or device, or a
        tsdf.TriangleMesh -> the geometry's id 0, 1, ...  ValueError for an index outside [0, V).  A triangle with a non-finite vertex, or
        whose fp32 cross product (v1 - v0) x (v2 - v0) is exactly zero or not finite, is in no result; primitive ids still count it."""
        v, t = as_triangles(vertices, triangles)
        with torch.cuda.device(AR.device_for(device=self.dev.index)):
            v, t = v.to(self.dev), t.to(self.dev)
            check_indices(t, int(v.shape[0]))
            total = sum(int(g[1].shape[0]) for g in self._geometries) + int(t.shape[0])
            if total > L.MESH_MAX_TRIANGLES:
                raise ValueError(f"{total} triangles in the scene, at most 2^29")
            self._geometries.append((v.to(torch.float32).contiguous(), t.to(torch.int32).contiguous()))
        self._dirty = True
        return len(self._geometries) - 1

    def _build(self) -> None:
        if not self._dirty:
            return
        with torch.cuda.device(self.dev):
            starts, base, tris = [0], 0, []
            for v, t in self._geometries:
                tris.append(t + base)                                       # (concatenation and offsets are plumbing: integers)
                base += int(v.shape[0])
                starts.append(starts[-1] + int(t.shape[0]))
            self.n_triangles = starts[-1]
            self.geom_start = torch.tensor(starts, dtype=torch.int32, device=self.dev)
            self.records = torch.empty(max(self.n_triangles, 1), 3, 4, dtype=torch.float32, device=self.dev)
            self.n_kept = 0
            if self.n_triangles:
                kept = torch.empty(1, dtype=torch.int32, device=self.dev)
                L.mesh_records(torch.cat([v for v, _ in self._geometries]), torch.cat(tris).contiguous(), self.records, kept)
                self.n_kept = int(kept.cpu())
            self.grid = None
            if self.n_kept:
                self._build_grid()
        self._dirty = False

    def _build_grid(self) -> None:
        """bounds of the kept triangles' vertices (reductions and a read-back: plumbing), then count, scan, scatter on the device"""
        rec = self.records[:self.n_triangles]
        pts = rec[rec[:, 0, 3].contiguous().view(torch.int32) >= 0][:, :, :3].reshape(-1, 3)
        lo, hi = pts.amin(0).cpu().numpy(), pts.amax(0).cpu().numpy()
        pad, limit = grid_padding(lo, hi)
        h = PC.default_cell_size(lo, hi, self.n_kept) if self._cell_size is None else self._cell_size
        cap = max_references(self.n_triangles)
        while True:
            dims = PC.grid_dims(lo, hi, h)
            cells, n_refs = PC.n_cells(dims), None
            if cells <= L.PC_MAX_CELLS:
                grid = (lo, hi, h, dims.astype(np.int32), pad)
                counts = torch.zeros(cells, dtype=torch.int32, device=self.dev)
                L.mesh_grid_count(self.records, self.n_triangles, grid, counts)
                n_refs = int(counts.sum(dtype=torch.int64).cpu())
                if n_refs <= cap:
                    break
            if self._cell_size is not None:
                what = f"{cells} cells, at most 2^24" if n_refs is None else f"{n_refs} references, at most {cap}"
                raise ValueError(f"cell_size {h}: a grid of {dims[0]} x {dims[1]} x {dims[2]} with {what}")
            h = float(np.float32(h * 1.25))
        self.cell_start = torch.zeros(cells + 1, dtype=torch.int32, device=self.dev)
        self.cell_start[1:] = torch.cumsum(counts, 0).to(torch.int32)                        # the scan is plumbing: integer, exact
        self.refs = torch.empty(max(n_refs, 1), dtype=torch.int32, device=self.dev)
        L.mesh_grid_scatter(self.records, self.n_triangles, grid, self.cell_start[:-1].clone(), self.refs)
        self.grid, self.origin_limit, self.cell_size, self.dims, self.n_references = grid, limit, h, grid[3], n_refs

    @staticmethod
    def create_rays_pinhole(intrinsic_matrix, extrinsic_matrix, width_px: int, height_px: int, pixel_center: float = 0.5) -> torch.Tensor:
        """-> fp32 host tensor [height_px, width_px, 6] of (origin, direction) for ``cast_rays``.  intrinsic_matrix 3 x 3, extrinsic_matrix
        4 x 4 world -> camera [R | t].  The origin is the camera centre -R^T t; the direction is R^T ((u + pixel_center - cx) / fx,
        (v + pixel_center - cy) / fy, 1): its camera-frame z is 1, so t_hit IS the z-depth.  pixel_center 0.5 is Open3D's documented
        convention, 0.0 that of TSDF.raycast.  Computed in fp64 on the host with the sums in a fixed order and rounded once."""
        K, E = np.asarray(PC._np(intrinsic_matrix), dtype=np.float64), np.asarray(PC._np(extrinsic_matrix), dtype=np.float64)
        if K.shape != (3, 3) or E.shape != (4, 4) or not (np.isfinite(K).all() and np.isfinite(E).all()):
            raise ValueError(f"create_rays_pinhole: a finite 3 x 3 intrinsic and 4 x 4 extrinsic matrix, got {K.shape} and {E.shape}")
        for name, n in (("width_px", width_px), ("height_px", height_px)):
            AR.integer(n, f"create_rays_pinhole: {name}", 1, None, "a positive integer")
        if K[0, 0] == 0.0 or K[1, 1] == 0.0:
            raise ValueError("create_rays_pinhole: a zero focal length")
        AR.number(pixel_center, "create_rays_pinhole: pixel_center", "a finite number")
        R, t = E[:3, :3], E[:3, 3]
        v, u = np.meshgrid(np.arange(int(height_px), dtype=np.float64), np.arange(int(width_px), dtype=np.float64), indexing="ij")
        x = ((u + np.float64(pixel_center)) - K[0, 2]) / K[0, 0]
        y = ((v + np.float64(pixel_center)) - K[1, 2]) / K[1, 1]
        out = np.empty((int(height_px), int(width_px), 6), np.float64)
        for k in range(3):
            out[..., k] = -((R[0, k] * t[0] + R[1, k] * t[1]) + R[2, k] * t[2])
            out[..., 3 + k] = (R[0, k] * x + R[1, k] * y) + R[2, k]
        return torch.from_numpy(out.astype(np.float32))

    def cast_rays(self, rays, method: str = "grid") -> Dict[str, torch.Tensor]:
        """rays [..., 6] (origin, direction; fp64 is rounded to fp32 once; the direction is not normalised) -> a dict of device tensors:
        t_hit fp32 [...] in units of |d| (+inf: a miss); geometry_ids, primitive_ids int32 [...] (INVALID_ID's bit pattern, -1: a miss;
        primitive ids are local to their geometry); primitive_uvs fp32 [..., 2] with p = (1 - u - v) v0 + u v1 + v v2; primitive_normals
        fp32 [..., 3], the unit (v1 - v0) x (v2 - v0), not turned towards the ray, zero for a miss.  The test is two-sided and watertight
        across shared edges and vertices; among equal t the earlier geometry and then the lower row wins.  A ray with a non-finite
        component or a zero direction is a miss."""
        _check_method(method)
        r = _as_rows(rays, 6, "rays")
        shape = tuple(r.shape[:-1])
        self._build()
        with torch.cuda.device(self.dev):
            r = r.to(self.dev).to(torch.float32).reshape(-1, 6).contiguous()
            m = int(r.shape[0])
            f = dict(dtype=torch.float32, device=self.dev)
            out = dict(t_hit=torch.empty(m, **f), geometry_ids=torch.empty(m, dtype=torch.int32, device=self.dev),
                       primitive_ids=torch.empty(m, dtype=torch.int32, device=self.dev), primitive_uvs=torch.empty(m, 2, **f),
                       primitive_normals=torch.empty(m, 3, **f))
            o = (out["t_hit"], out["geometry_ids"], out["primitive_ids"], out["primitive_uvs"], out["primitive_normals"])
            if m and method == "grid" and self.grid is not None:
                fb_list = torch.empty(m, dtype=torch.int32, device=self.dev)
                fb_count = torch.empty(1, dtype=torch.int32, device=self.dev)
                L.mesh_cast_grid(self.records, self.n_triangles, self.refs, self.cell_start, self.grid, self.origin_limit, r, self.geom_start, *o,
                                 fb_list, fb_count)
                n_fb = int(fb_count.cpu())
                if n_fb:
                    keys = torch.empty(n_fb, dtype=torch.int64, device=self.dev)
                    L.mesh_cast_brute(self.records, self.n_triangles, r, fb_list, n_fb, keys, self.geom_start, *o)
                self.last_fallback = n_fb
            elif m:
                keys = torch.empty(m, dtype=torch.int64, device=self.dev)
                L.mesh_cast_brute(self.records, self.n_triangles, r, None, m, keys, self.geom_start, *o)
        return {k: v.reshape(shape + tuple(v.shape[1:])) for k, v in out.items()}

    def compute_closest_points(self, query, max_distance: Optional[float] = None, method: str = "grid") -> Dict[str, torch.Tensor]:
        """query [..., 3] (fp64 is rounded to fp32 once) -> a dict of device tensors: points fp32 [..., 3], the closest point of the surface;
        distance fp32 [...] = sqrt(d2); geometry_ids, primitive_ids, primitive_uvs as ``cast_rays`` returns them.  Among equal d2 the
        earlier geometry and then the lower row wins.  A query with a non-finite coordinate gets NaN points and distance and invalid
        ids; a scene without a kept triangle, or -- with max_distance, compared in fp32 as NearestNeighbours.query does -- nothing within
        max_distance: NaN points, distance +inf, invalid ids."""
        _check_method(method)
        md = PC._check_max_distance(max_distance)
        q = _as_rows(query, 3, "query")
        shape = tuple(q.shape[:-1])
        self._build()
        with torch.cuda.device(self.dev):
            q = q.to(self.dev).to(torch.float32).reshape(-1, 3).contiguous()
            m = int(q.shape[0])
            f = dict(dtype=torch.float32, device=self.dev)
            out = dict(points=torch.empty(m, 3, **f), distance=torch.empty(m, **f), geometry_ids=torch.empty(m, dtype=torch.int32, device=self.dev),
                       primitive_ids=torch.empty(m, dtype=torch.int32, device=self.dev), primitive_uvs=torch.empty(m, 2, **f))
            o = (out["points"], out["distance"], out["geometry_ids"], out["primitive_ids"], out["primitive_uvs"])
            if m and method == "grid" and self.grid is not None:
                fb_list = torch.empty(m, dtype=torch.int32, device=self.dev)
                fb_count = torch.empty(1, dtype=torch.int32, device=self.dev)
                L.mesh_closest_grid(self.records, self.n_triangles, self.refs, self.cell_start, self.grid, q, md, SHELL_CAP, self.geom_start, *o,
                                    fb_list, fb_count)
                n_fb = int(fb_count.cpu())
                if n_fb:
                    keys = torch.empty(n_fb, dtype=torch.int64, device=self.dev)
                    L.mesh_closest_brute(self.records, self.n_triangles, q, fb_list, n_fb, md, keys, self.geom_start, *o)
                self.last_fallback = n_fb
            elif m:
                keys = torch.empty(m, dtype=torch.int64, device=self.dev)
                L.mesh_closest_brute(self.records, self.n_triangles, q, None, m, md, keys, self.geom_start, *o)
        return {k: v.reshape(shape + tuple(v.shape[1:])) for k, v in out.items()}

    def compute_distance(self, query, max_distance: Optional[float] = None, method: str = "grid") -> torch.Tensor:
        """compute_closest_points(query)["distance"]: fp32 [...] device tensor, the unsigned distance to the surface"""
        return self.compute_closest_points(query, max_distance=max_distance, method=method)["distance"]

    # ---- every hit of a ray ----------------------------------------------------------------------------------------------------------------
    def _hits(self, r: torch.Tensor, mode: int, method: str, tnear: float = 0.0, tfar: float = float("inf"), out=None, row_start=None, keys=None):
        """one sink (L.MESH_HITS_*) over the rays r fp32 [m, 6] on the device, m >= 1: the walk and the brute force for its list, or the brute
        force alone"""
        m = int(r.shape[0])
        fill = mode == L.MESH_HITS_FILL
        if method == "grid" and self.grid is not None:
            fb_list = torch.empty(m, dtype=torch.int32, device=self.dev)
            fb_count = torch.empty(1, dtype=torch.int32, device=self.dev)
            L.mesh_hits_grid(self.records, self.n_triangles, self.refs, self.cell_start, self.grid, self.origin_limit, r, mode, tnear, tfar, out,
                             row_start, keys, fb_list, fb_count)
            n_fb = int(fb_count.cpu())
            if n_fb:
                cursor = torch.empty(n_fb, dtype=torch.int32, device=self.dev) if fill else None
                L.mesh_hits_brute(self.records, self.n_triangles, r, fb_list, n_fb, mode, tnear, tfar, out, row_start, keys, cursor)
            self.last_fallback = n_fb
        else:
            cursor = torch.empty(m, dtype=torch.int32, device=self.dev) if fill else None
            L.mesh_hits_brute(self.records, self.n_triangles, r, None, m, mode, tnear, tfar, out, row_start, keys, cursor)

    def _rays(self, rays):
        r = _as_rows(rays, 6, "rays")
        self._build()
        return tuple(r.shape[:-1]), r

    def count_intersections(self, rays, method: str = "grid") -> torch.Tensor:
        """rays [..., 6] as ``cast_rays`` takes them -> int32 [...] device tensor: how many kept triangles the ray hits with 0 <= t < inf
        under the counting predicate (the module's docstring): a ray through a shared edge or vertex counts one of the triangles there, so
        for a closed mesh the count's parity says on which side the origin lies.  A ray that passes a triangle seen edge-on (|det| below
        2^-12 of its products) does not count it: such a ray can be off by one.  A ray with a non-finite component or a zero direction: 0."""
        _check_method(method)
        shape, r = self._rays(rays)
        with torch.cuda.device(self.dev):
            r = r.to(self.dev).to(torch.float32).reshape(-1, 6).contiguous()
            out = torch.zeros(int(r.shape[0]), dtype=torch.int32, device=self.dev)
            if r.shape[0]:
                self._hits(r, L.MESH_HITS_COUNT, method, out=out)
        return out.reshape(shape)

    def test_occlusions(self, rays, tnear: float = 0.0, tfar: float = float("inf"), method: str = "grid") -> torch.Tensor:
        """rays [..., 6] -> bool [...] device tensor: whether the ray hits a kept triangle with tnear <= t <= tfar (compared in fp32) under
        ``cast_rays``' own closed predicate, found by a walk that stops at the first such hit: with the defaults it equals
        isfinite(cast_rays(rays)["t_hit"]) exactly.  A ray with a non-finite component or a zero direction: False."""
        _check_method(method)
        tn, tf = _check_range(tnear, tfar)
        shape, r = self._rays(rays)
        with torch.cuda.device(self.dev):
            r = r.to(self.dev).to(torch.float32).reshape(-1, 6).contiguous()
            out = torch.zeros(int(r.shape[0]), dtype=torch.int32, device=self.dev)
            if r.shape[0]:
                self._hits(r, L.MESH_HITS_ANY, method, tn, tf, out=out)
        return (out != 0).reshape(shape)

    def list_intersections(self, rays, method: str = "grid") -> Dict[str, torch.Tensor]:
        """rays [..., 6], m of them when flattened -> a dict of device tensors over all the hits ``count_intersections`` counts: ray_splits
        int64 [m + 1] (the rows of ray i are ray_splits[i] .. ray_splits[i + 1] - 1); ray_ids int64 [total]; t_hit fp32 [total];
        geometry_ids, primitive_ids int32 [total]; primitive_uvs fp32 [total, 2], as ``cast_rays`` defines them.  Rows are in ray order
        and, within a ray, ascending in (t, global triangle index).  ValueError when total exceeds 2^31 - 1.  For a ray with no edge value
        of exactly 0 the first row is ``cast_rays``' hit."""
        _check_method(method)
        _, r = self._rays(rays)
        with torch.cuda.device(self.dev):
            r = r.to(self.dev).to(torch.float32).reshape(-1, 6).contiguous()
            m = int(r.shape[0])
            counts = torch.zeros(m, dtype=torch.int32, device=self.dev)
            if m:
                self._hits(r, L.MESH_HITS_COUNT, method, out=counts)
            splits = torch.zeros(m + 1, dtype=torch.int64, device=self.dev)
            splits[1:] = torch.cumsum(counts, 0, dtype=torch.int64)                          # the scan is plumbing: integer, exact
            total = int(splits[-1].cpu())
            if total > 2 ** 31 - 1:
                raise ValueError(f"list_intersections: {total} hits, at most 2^31 - 1")
            f = dict(dtype=torch.float32, device=self.dev)
            out = dict(ray_splits=splits, ray_ids=torch.repeat_interleave(torch.arange(m, dtype=torch.int64, device=self.dev), counts.to(torch.int64)),
                       t_hit=torch.empty(total, **f), geometry_ids=torch.empty(total, dtype=torch.int32, device=self.dev),
                       primitive_ids=torch.empty(total, dtype=torch.int32, device=self.dev), primitive_uvs=torch.empty(total, 2, **f))
            if total:
                keys, ordered = torch.empty(total, dtype=torch.int64, device=self.dev), torch.empty(total, dtype=torch.int64, device=self.dev)
                self._hits(r, L.MESH_HITS_FILL, method, row_start=splits, keys=keys)
                L.pc_radius_sort(keys, splits, ordered)
                L.mesh_hits_unpack(self.records, self.n_triangles, r, ordered, out["ray_ids"].contiguous(), self.geom_start, out["t_hit"],
                                   out["geometry_ids"], out["primitive_ids"], out["primitive_uvs"])
        return out

    def compute_occupancy(self, query, nsamples: int = 1, method: str = "grid") -> torch.Tensor:
        """query [..., 3] -> fp32 [...] device tensor: 1.0 inside, 0.0 outside, NaN for a query with a non-finite coordinate.  Sample j casts
        from the query along OCCUPANCY_DIRECTIONS[j]; the point is inside when the majority of the nsamples (odd, 1 .. 15, else ValueError)
        ``count_intersections`` is odd (rays and vote are composed with torch: plumbing, integers).  The answer is meaningful only for a
        CLOSED mesh (tsdf.TriangleMesh.is_closed) and is undefined at distance ~ 0 from the surface.  A ray through a triangle seen
        edge-on (the 2^-12 rule of the arithmetic) misses it and flips that sample: nsamples > 1 exists for this case."""
        _check_method(method)
        n = _check_nsamples(nsamples)
        q = _as_rows(query, 3, "query")
        shape = tuple(q.shape[:-1])
        if q.numel() // 3 * n >= 2 ** 31:
            raise ValueError(f"query: {q.numel() // 3} points by {n} samples, at most 2^31 - 1 rays")
        self._build()
        with torch.cuda.device(self.dev):
            q = q.to(self.dev).to(torch.float32).reshape(-1, 3)
            m = int(q.shape[0])
            rays = torch.empty(n, m, 6, dtype=torch.float32, device=self.dev)
            rays[:, :, :3] = q[None]
            rays[:, :, 3:] = torch.tensor(OCCUPANCY_DIRECTIONS[:n], dtype=torch.float32, device=self.dev)[:, None, :]
            odd = (self.count_intersections(rays, method=method) & 1).sum(0)
            occ = (2 * odd > n).to(torch.float32)
            occ = torch.where(torch.isfinite(q).all(1), occ, torch.full_like(occ, float("nan")))
        return occ.reshape(shape)

    def compute_signed_distance(self, query, nsamples: int = 1, method: str = "grid") -> torch.Tensor:
        """query [..., 3] -> fp32 [...] device tensor: ``compute_distance``'s bits, negated where ``compute_occupancy(query, nsamples)`` is 1.
        NaN (a non-finite query) stays NaN; a scene without a kept triangle gives +inf.  The sign is meaningful only for a CLOSED mesh and
        undefined at distance ~ 0; an edge-on triangle on a sample's ray can flip that sample, which nsamples > 1 outvotes."""
        occ = self.compute_occupancy(query, nsamples=nsamples, method=method)
        d = self.compute_distance(query, method=method)
        return torch.where(occ == 1.0, -d, d)
