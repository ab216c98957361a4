"""Mesh topology and clean-up where the mesh lies (csrc/mesh_ops.hip): the edge table, edge-connected components,
triangle and vertex normals, surface area, removal of small components, Laplacian and Taubin smoothing.

These take the roles of Open3D's TriangleMesh.cluster_connected_triangles, remove_triangles_by_mask, remove_unreferenced_vertices,
get_non_manifold_edges, is_edge_manifold, compute_triangle_normals, compute_vertex_normals, get_surface_area, filter_smooth_laplacian and
filter_smooth_taubin.  Open3D is not vendored: the meaning is restated from its documentation and parity with Open3D is unpinned; the
statement is tests/_mesh_ops_ref.py and every result is bit-equal to it, the same bits in every run.

Every function takes (vertices [V, 3] fp32 or fp64, triangles [T, 3] integers) as numpy arrays or torch tensors, host or device, or a
tsdf.TriangleMesh alone, and returns device tensors; the methods of tsdf.TriangleMesh return the kind the mesh is made of.  fp64 vertices
are rounded to fp32 once.  A triangle is VALID when its three indices lie in [0, V) and are pairwise distinct; an invalid one takes part in
nothing (cluster -1, zero normal, zero area, no edge) and is counted in MeshEdges.n_invalid_triangles.  A valid triangle is KEPT when its
vertices are finite and its fp32 cross product finite and non-zero (the rule of the ray-casting scene); topology uses the valid triangles,
normals and areas the kept ones.  Argument errors are ValueErrors raised before any launch; an empty mesh gives empty results; there is no
CPU fallback.

``orient_triangles`` / ``is_orientable`` / ``orientable_components`` (Open3D's orient_triangles and is_orientable) repair the winding: a
union-find with one parity bit per link over the two-triangle edges (csrc/union_parity.h); the statement is
tests/_orient_ref.py.

Is the mesh a solid (csrc/mesh_solid.hip; the statement is tests/_mesh_solid_ref.py): ``get_non_manifold_vertices`` /
``is_vertex_manifold``, ``get_self_intersecting_triangles`` / ``is_self_intersecting``, ``get_intersecting_triangles`` / ``is_intersecting``,
``is_watertight``, ``component_volumes`` / ``get_volume``, ``orient_outward`` and ``check_solid`` -- Open3D's predicate family restated,
parity unpinned.  Every decision is a sign of a fixed-order fp64 expression or an exact comparison: the same result in every run, for
every grid and table size.

Not built: exact arithmetic beyond fp64 (a determinant below the bound of DESIGN 3.26 takes the sign the stated arithmetic gives it),
intersections of triangles that share a vertex, welding (merge_close_vertices), simplification, subdivision, hole filling or any other
repair, booleans."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _args as AR
from . import _lib as L

last_rounds = 0          # the (hook, compress) rounds of the latest cluster_connected_triangles, the final unchanged one included
last_orient_rounds = 0   # the (hook, compress) rounds of the latest orient_triangles / is_orientable / orientable_components, likewise
last_fan_rounds = 0      # the (hook, compress) rounds of the latest get_non_manifold_vertices / is_vertex_manifold, likewise
last_fallback = 0        # the query triangles of the latest grid search for intersecting pairs that were finished by brute force
PAIR_METHODS = ("auto", "grid", "brute")
PAIR_CELL_CAP = 512      # a query triangle whose cell box holds more cells than this is finished by brute force (a starting point, not tuned)
PAIR_AUTO_BRUTE = 1 << 16    # method="auto": brute force when (query triangles) x (triangles) is at most this, the grid otherwise


@dataclass
class MeshEdges:
    """edge_topology's result, device tensors; E unique undirected edges in the order of their first half-edge (half-edge 3 t + c runs from
    triangles[t][c] to triangles[t][(c + 1) % 3])"""
    edges: torch.Tensor                     # int32 [E, 2]: (min, max) vertex
    edge_count: torch.Tensor                # int32 [E]: the half-edges (triangle sides) on the edge
    edge_forward: torch.Tensor              # int32 [E]: those that run from the lower to the higher vertex
    edge_first_triangle: torch.Tensor       # int32 [E]: the triangle of the first half-edge
    edge_of_half: torch.Tensor              # int32 [3 T]: the edge of every half-edge, -1 for those of an invalid triangle
    n_invalid_triangles: int
    n_vertices: int

    def get_non_manifold_edges(self, allow_boundary_edges: bool = True) -> torch.Tensor:
        """int32 [n, 2]: the edges with more than two triangles; allow_boundary_edges=False: those without exactly two"""
        c = self.edge_count
        return self.edges[(c > 2) if allow_boundary_edges else (c != 2)]

    def get_boundary_edges(self) -> torch.Tensor:
        return self.edges[self.edge_count == 1]

    def is_edge_manifold(self, allow_boundary_edges: bool = True) -> bool:
        return int(self.get_non_manifold_edges(allow_boundary_edges).shape[0]) == 0

    def is_consistently_oriented(self) -> bool:
        """every edge of two triangles is run once in each direction"""
        return bool((self.edge_forward[self.edge_count == 2] == 1).all())

    def is_closed(self) -> bool:
        """every edge has exactly two triangles"""
        return bool((self.edge_count == 2).all())


# ---- arguments -----------------------------------------------------------------------------------------------------------------------------
def _as_mesh(vertices, triangles=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (vertices fp32 / fp64 torch [V, 3], triangles integer torch [T, 3]) where they lie; V and T may be 0, indices are not checked"""
    return AR.triangles(vertices, triangles, allow_empty_vertices=True)


def _device(v: torch.Tensor, t: torch.Tensor, device: int) -> torch.device:
    return AR.device_for(v, t, device=device)


def _on_device(v, t, dev) -> Tuple[torch.Tensor, torch.Tensor]:
    v = v.to(dev).to(torch.float32).contiguous()
    t = t.to(dev)
    if t.dtype != torch.int32:                 # an index that int32 cannot hold is outside [0, V): any invalid value will do
        t = torch.where((t >= 0) & (t < 2 ** 31), t, torch.full_like(t, -1)).to(torch.int32)
    return v, t.contiguous()


def _check_iterations(n) -> int:
    return AR.integer(n, "number_of_iterations", 0, 2 ** 31 - 1, "an integer >= 0")


def _check_factor(x, what: str) -> float:
    return AR.number(x, what, "a finite number")


def _check_slots(slots, n_half: int) -> int:
    if slots is None:
        return edge_table_slots(n_half // 3)
    n = AR.integer(slots, "slots", 1, 2 ** 31, "a power of two, at most 2^31")
    if n & (n - 1):
        raise ValueError(f"slots {slots!r}: expected a power of two, at most 2^31")
    return n


def edge_table_slots(n_triangles: int) -> int:
    """the default table: the smallest power of two above 3 T"""
    return 1 << int(3 * n_triangles).bit_length()


# ---- the edge table ------------------------------------------------------------------------------------------------------------------------
def edge_topology(vertices, triangles=None, slots: Optional[int] = None, device: int = 0) -> MeshEdges:
    """The unique undirected edges of the valid triangles and what lies on them -> MeshEdges.  slots: the size of the hash table, a power of
    two; None: the smallest above 3 T.  The result does not depend on it; a table too small for the edges raises BodySlamHipError."""
    v, t = _as_mesh(vertices, triangles)
    slots = _check_slots(slots, 3 * int(t.shape[0]))
    dev = _device(v, t, device)
    with torch.cuda.device(dev):
        v, t = _on_device(v, t, dev)
        return _edge_rows(t, int(v.shape[0]), slots)


def _edge_rows(t: torch.Tensor, n_vertices: int, slots: int) -> MeshEdges:
    """the three launches over int32 device triangles, with the table size as an argument"""
    dev, T = t.device, int(t.shape[0])
    i32 = dict(dtype=torch.int32, device=dev)
    if T == 0:
        e = torch.empty(0, **i32)
        return MeshEdges(torch.empty(0, 2, **i32), e, e.clone(), e.clone(), e.clone(), 0, n_vertices)
    keys = torch.full((slots,), L.MESH_EDGE_EMPTY_KEY, dtype=torch.int64, device=dev)            # (the fills and the scan are plumbing)
    first_half = torch.full((slots,), L.MESH_EDGE_NO_HALF, **i32)
    count, forward = torch.zeros(slots, **i32), torch.zeros(slots, **i32)
    slot_of_half, edge_of_half = torch.empty(3 * T, **i32), torch.empty(3 * T, **i32)
    status = torch.zeros(2, **i32)
    L.mesh_edge_insert(t, n_vertices, keys, first_half, count, forward, slot_of_half, status)
    leader, rank, (word, n_invalid, E) = AR.first_ranks(L.mesh_edge_flags, slot_of_half, first_half, status)
    if word & L.MESH_EDGE_TABLE_FULL:
        raise L.BodySlamHipError(f"edge_topology: the edge table of {slots} slots is full")
    if word:
        raise L.BodySlamHipError(f"edge_topology: status {word}")
    edges = torch.empty(E, 2, **i32)
    edge_count, edge_forward, edge_first = (torch.empty(E, **i32) for _ in range(3))
    L.mesh_edge_rows(t, slot_of_half, count, forward, leader, rank, edges, edge_count, edge_forward, edge_first, edge_of_half)
    return MeshEdges(edges, edge_count, edge_forward, edge_first, edge_of_half, n_invalid, n_vertices)


# ---- components ----------------------------------------------------------------------------------------------------------------------------
def _labels(me: MeshEdges, T: int) -> torch.Tensor:
    """parent int32 [T]: the smallest triangle index of every triangle's component.  A round that reports a change turns at least one root
    into a non-root for good (parent only decreases), so at most T rounds report one: the cap is T + 1 rounds."""
    global last_rounds
    dev = me.edge_of_half.device
    parent = torch.arange(T, dtype=torch.int32, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    last_rounds = 0
    for _ in range(T + 1):
        changed.zero_()
        L.mesh_cc_hook(me.edge_of_half, me.edge_first_triangle, parent, changed)
        L.mesh_cc_compress(parent)
        last_rounds += 1
        if int(changed.cpu()) == 0:
            return parent
    raise L.BodySlamHipError(f"cluster_connected_triangles: no fixed point after {T + 1} rounds")


def _segment_sums(values: torch.Tensor, start: torch.Tensor) -> torch.Tensor:
    out = torch.empty(start.numel() - 1, dtype=torch.float64, device=values.device)
    L.mesh_segment_sum(values, start, out)
    return out


def _clusters(v, t, slots, per_triangle=None):
    """per_triangle(me, parent) -> fp64 [T]: what to sum per cluster; None: the areas of the kept triangles"""
    dev, T = t.device, int(t.shape[0])
    i32 = dict(dtype=torch.int32, device=dev)
    if T == 0:
        return torch.empty(0, **i32), torch.empty(0, **i32), torch.empty(0, dtype=torch.float64, device=dev)
    me = _edge_rows(t, int(v.shape[0]), slots)
    parent = _labels(me, T)
    is_root = torch.empty(T, **i32)
    L.mesh_cc_roots(parent, me.edge_of_half, is_root)
    rank = torch.cumsum(is_root, 0).to(torch.int32)
    C = int(rank[-1].cpu())
    clusters, n_tri = torch.empty(T, **i32), torch.zeros(C, **i32)
    L.mesh_cc_clusters(parent, me.edge_of_half, rank, clusters, n_tri)
    c_area = torch.empty(0, dtype=torch.float64, device=dev)
    if C:
        if per_triangle is None:
            area = torch.empty(T, dtype=torch.float64, device=dev)
            L.mesh_triangle_geometry(_safe_vertices(v), t, area=area)
        else:
            area = per_triangle(me, parent)
        order = torch.sort(clusters, stable=True)[1]                                             # (the sort and the gather are plumbing)
        start = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(n_tri.to(torch.int64), 0)]) + (T - int(n_tri.sum().cpu()))
        c_area = _segment_sums(area[order].contiguous(), start.contiguous())
    return clusters, n_tri, c_area


def _safe_vertices(v: torch.Tensor) -> torch.Tensor:
    """a mesh without vertices has no valid triangle; the kernels want one row to point at"""
    return v if v.shape[0] else torch.zeros(1, 3, dtype=torch.float32, device=v.device)


def cluster_connected_triangles(vertices, triangles=None, slots: Optional[int] = None, device: int = 0):
    """Open3D's cluster_connected_triangles -> (triangle_clusters int32 [T], cluster_n_triangles int32 [C], cluster_area fp64 [C]).  Two valid
    triangles are connected when they share an edge; a shared vertex alone does not connect.  Clusters are numbered in the order of their
    first triangle; an invalid triangle has cluster -1.  cluster_area: the fp64 areas of the kept triangles, each cluster summed in a fixed
    order (tests/_mesh_ops_ref.py wave_sum).  ``last_rounds`` holds the rounds the labelling took."""
    v, t = _as_mesh(vertices, triangles)
    slots = _check_slots(slots, 3 * int(t.shape[0]))
    dev = _device(v, t, device)
    with torch.cuda.device(dev):
        v, t = _on_device(v, t, dev)
        return _clusters(v, t, slots)


# ---- winding -------------------------------------------------------------------------------------------------------------------------------
def _orient(vertices, triangles, slots, device):
    """-> (triangles int32 [T, 3], flipped bool [T], triangle_components int32 [T], component_orientable bool [C]), device tensors"""
    global last_orient_rounds
    v, t = _as_mesh(vertices, triangles)
    slots = _check_slots(slots, 3 * int(t.shape[0]))
    dev = _device(v, t, device)
    with torch.cuda.device(dev):
        v, t = _on_device(v, t, dev)
        T = int(t.shape[0])
        i32 = dict(dtype=torch.int32, device=dev)
        last_orient_rounds = 0
        if T == 0:
            return t.clone(), torch.zeros(0, dtype=torch.bool, device=dev), torch.empty(0, **i32), torch.zeros(0, dtype=torch.bool, device=dev)
        me = _edge_rows(t, int(v.shape[0]), slots)
        word = torch.arange(T, **i32) * 2                                    # parent << 1 | parity: every triangle its own root
        changed = torch.zeros(1, **i32)
        for _ in range(T + 1):                       # every round that reports a change removes a root for good: at most T do
            changed.zero_()
            L.mesh_orient_hook(me, word, changed)
            L.mesh_orient_compress(word)
            last_orient_rounds += 1
            if int(changed.cpu()) == 0:
                break
        else:
            raise L.BodySlamHipError(f"orient_triangles: no fixed point after {T + 1} rounds")
        bad = torch.zeros(T, **i32)
        L.mesh_orient_check(me, word, bad)
        out, flipped = torch.empty_like(t), torch.empty(T, dtype=torch.uint8, device=dev)
        L.mesh_orient_flip(t, me.edge_of_half, word, bad, out, flipped)
        root = word >> 1                                                     # (the labels are plumbing: a scan and two gathers)
        is_root = (me.edge_of_half[0::3] >= 0) & (root == torch.arange(T, **i32))
        rank = torch.cumsum(is_root.to(torch.int32), 0).to(torch.int32)
        components = torch.where(me.edge_of_half[0::3] >= 0, rank[root.to(torch.int64)] - 1, torch.full((), -1, **i32)).to(torch.int32)
        return out, flipped.to(torch.bool), components, bad[is_root] == 0


def orient_triangles(vertices, triangles=None, slots: Optional[int] = None, device: int = 0):
    """Open3D's orient_triangles -> (triangles int32 [T, 3], flipped bool [T], orientable bool); restated, parity with Open3D unpinned, the
    statement is tests/_orient_ref.py.  Every edge of the edge table with exactly two triangles links them: they have one orientation when
    they run the edge in opposite directions (edge_forward == 1), so the link says flip(t) xor flip(u) = (edge_forward != 1).  An edge
    with any other count -- a boundary edge, or one with three triangles or more -- links nothing and connects nothing: the components
    here are those of the two-triangle edges, finer than cluster_connected_triangles' where such edges exist.  csrc/mesh_ops.hip: rounds
    of (hook with a parity bit, compress) over csrc/union_parity.h until nothing changes (``last_orient_rounds``), a launch that re-tests
    every link, a launch that flips.

    In an orientable component the triangle of smallest index keeps its winding and every other triangle is flipped when its parity to
    that one is 1; a flipped triangle [a, b, c] becomes [a, c, b].  A component with a link its parities cannot satisfy (a Moebius strip)
    is not orientable: it is returned unchanged, and orientable is False.  Invalid triangles are returned unchanged.  No outward
    orientation by signed volume is attempted.  ``orientable_components`` gives the verdict per component."""
    out, flipped, _, verdict = _orient(vertices, triangles, slots, device)
    return out, flipped, bool(verdict.all())


def orientable_components(vertices, triangles=None, slots: Optional[int] = None, device: int = 0):
    """-> (triangle_components int32 [T], component_orientable bool [C]): the components of ``orient_triangles`` -- valid triangles joined
    through edges of exactly two triangles --, numbered in the order of their first triangle as cluster_connected_triangles numbers its
    clusters, -1 for an invalid triangle; and whether each can be wound consistently."""
    _, _, components, verdict = _orient(vertices, triangles, slots, device)
    return components, verdict


def is_orientable(vertices, triangles=None, slots: Optional[int] = None, device: int = 0) -> bool:
    """Open3D's is_orientable: every component of ``orient_triangles`` can be wound consistently (an empty mesh can)"""
    return bool(_orient(vertices, triangles, slots, device)[3].all())


def get_surface_area(vertices, triangles=None, device: int = 0) -> float:
    """the sum of the fp64 areas of the kept triangles, in the fixed order of cluster_area over all triangles"""
    v, t = _as_mesh(vertices, triangles)
    dev = _device(v, t, device)
    with torch.cuda.device(dev):
        v, t = _on_device(v, t, dev)
        T = int(t.shape[0])
        if T == 0:
            return 0.0
        area = torch.empty(T, dtype=torch.float64, device=dev)
        L.mesh_triangle_geometry(_safe_vertices(v), t, area=area)
        return float(_segment_sums(area, torch.tensor([0, T], dtype=torch.int64, device=dev)).cpu()[0])


# ---- is the mesh a solid: vertex fans, intersecting pairs, volume (csrc/mesh_solid.hip) -------------------------------------------------------
def _fan_counts(t: torch.Tensor, n_vertices: int, me: MeshEdges) -> torch.Tensor:
    """int32 [V]: the classes of corners at every vertex.  A round that reports a change removes a root for good: the cap is 3 T + 1 rounds."""
    global last_fan_rounds
    dev, T = t.device, int(t.shape[0])
    parent = torch.arange(3 * T, dtype=torch.int32, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    last_fan_rounds = 0
    for _ in range(3 * T + 1):
        changed.zero_()
        L.mesh_fan_hook(t, me.edge_of_half, me.edge_first_triangle, parent, changed)
        L.mesh_fan_compress(parent)
        last_fan_rounds += 1
        if int(changed.cpu()) == 0:
            break
    else:
        raise L.BodySlamHipError(f"get_non_manifold_vertices: no fixed point after {3 * T + 1} rounds")
    count = torch.zeros(n_vertices, dtype=torch.int32, device=dev)
    L.mesh_fan_count(t, n_vertices, me.edge_of_half, parent, count)
    return count


def _non_manifold_vertices(v, t, slots) -> torch.Tensor:
    T, V = int(t.shape[0]), int(v.shape[0])
    if T == 0 or V == 0:
        return torch.empty(0, dtype=torch.int32, device=t.device)
    return torch.nonzero(_fan_counts(t, V, _edge_rows(t, V, slots)) > 1)[:, 0].to(torch.int32)


def get_non_manifold_vertices(vertices, triangles=None, slots: Optional[int] = None, device: int = 0) -> torch.Tensor:
    """Open3D's get_non_manifold_vertices -> int32 [n] vertex rows, ascending.  A vertex is manifold when the valid triangles that contain it
    form one set connected through shared edges that contain the vertex: one fan, closed or open (a boundary fan is manifold, and so is a
    vertex in no valid triangle).  A bow-tie -- two fans that meet in the vertex alone -- is reported.  An edge of three or more triangles
    connects all of them, so the end points of a non-manifold EDGE are not reported for that reason alone: ask get_non_manifold_edges.
    csrc/mesh_solid.hip: union by minimum over the 3 T corners, rounds of (hook, compress) until nothing changes (``last_fan_rounds``),
    then the classes per vertex counted with integer atomics.  The result does not depend on ``slots``."""
    v, t = _as_mesh(vertices, triangles)
    slots = _check_slots(slots, 3 * int(t.shape[0]))
    dev = _device(v, t, device)
    with torch.cuda.device(dev):
        v, t = _on_device(v, t, dev)
        return _non_manifold_vertices(v, t, slots)


def is_vertex_manifold(vertices, triangles=None, slots: Optional[int] = None, device: int = 0) -> bool:
    """Open3D's is_vertex_manifold: ``get_non_manifold_vertices`` is empty"""
    return int(get_non_manifold_vertices(vertices, triangles, slots, device).shape[0]) == 0


def _check_pair_args(method, cells):
    if method not in PAIR_METHODS:
        raise ValueError(f"unknown method {method!r}: one of {PAIR_METHODS}")
    if cells is not None:
        AR.integer(cells, "cells", 1, 1 << 20, "None or an integer in 1 .. 2^20")
    return method, cells


def _solid_records(v: torch.Tensor, t: torch.Tensor):
    """-> (records fp32 [T, 3, 4] with the vertex rows in the fourth lanes, the number of kept triangles)"""
    records = torch.empty(int(t.shape[0]), 3, 4, dtype=torch.float32, device=t.device)
    kept = torch.empty(1, dtype=torch.int32, device=t.device)
    L.mesh_solid_records(v, t, records, kept)
    return records, int(kept.cpu())


def _pair_grid(records: torch.Tensor, n_kept: int, cells: Optional[int]):
    """The scene's triangle grid over the kept triangles of `records` (raycasting.RaycastingScene._build_grid: bounds, padding, count, scan,
    scatter) -> (grid, cell_start, refs).  cells None: the scene's default cell size, grown by 1.25 until the limits hold; otherwise the
    cell edge is the box's longest extent over `cells` (a little more, so that cells = 1 is one cell), and a broken limit is a ValueError."""
    from . import pointcloud as PC
    from .raycasting import grid_padding, max_references
    dev, T = records.device, int(records.shape[0])
    pts = records[records[:, 0, 3].contiguous().view(torch.int32) >= 0][:, :, :3].reshape(-1, 3)
    lo, hi = pts.amin(0).cpu().numpy(), pts.amax(0).cpu().numpy()
    pad, _ = grid_padding(lo, hi)
    if cells is None:
        h = PC.default_cell_size(lo, hi, n_kept)
    else:
        ext = float((hi.astype(np.float32) - lo.astype(np.float32)).max())
        h = float(np.float32(ext / cells) * np.float32(1.0 + 2.0 ** -10)) if ext > 0.0 else 1.0
    cap = max_references(T)
    while True:
        dims = PC.grid_dims(lo, hi, h)
        n_cells, n_refs = PC.n_cells(dims), None
        if n_cells <= L.PC_MAX_CELLS:
            grid = (lo, hi, h, dims.astype(np.int32), pad)
            counts = torch.zeros(n_cells, dtype=torch.int32, device=dev)
            L.mesh_grid_count(records, T, grid, counts)
            n_refs = int(counts.sum(dtype=torch.int64).cpu())
            if n_refs <= cap:
                break
        if cells is not None:
            what = f"{n_cells} cells, at most 2^24" if n_refs is None else f"{n_refs} references, at most {cap}"
            raise ValueError(f"cells {cells}: a grid of {dims[0]} x {dims[1]} x {dims[2]} with {what}")
        h = float(np.float32(h * 1.25))
    cell_start = torch.zeros(n_cells + 1, dtype=torch.int32, device=dev)
    cell_start[1:] = torch.cumsum(counts, 0).to(torch.int32)                              # (the scan is plumbing: integer, exact)
    refs = torch.empty(max(n_refs, 1), dtype=torch.int32, device=dev)
    L.mesh_grid_scatter(records, T, grid, cell_start[:-1].clone(), refs)
    return grid, cell_start, refs


def _pairs(a, b, method: str, cells: Optional[int], want_list: bool, device: int):
    """the intersecting pairs of mesh a with itself (b None) or with mesh b -> int32 [n, 2] (want_list) or bool"""
    global last_fallback
    method, cells = _check_pair_args(method, cells)
    va, ta = _as_mesh(*a)
    vb, tb = _as_mesh(*b) if b is not None else (None, None)
    dev = _device(va, ta, device) if b is None else AR.device_for(va, ta, vb, tb, device=device)
    with torch.cuda.device(dev):
        i32 = dict(dtype=torch.int32, device=dev)
        last_fallback = 0
        none = torch.empty(0, 2, **i32) if want_list else False
        va, ta = _on_device(va, ta, dev)
        if b is not None:
            vb, tb = _on_device(vb, tb, dev)
        if min(ta.shape[0], va.shape[0]) == 0 or (b is not None and min(tb.shape[0], vb.shape[0]) == 0):
            return none
        q_rec, q_kept = _solid_records(va, ta)
        rec, kept = (q_rec, q_kept) if b is None else _solid_records(vb, tb)
        if q_kept == 0 or kept == 0:
            return none
        n_q, self_mode = int(q_rec.shape[0]), b is None
        if method == "auto":
            method = "brute" if n_q * int(rec.shape[0]) <= PAIR_AUTO_BRUTE else "grid"
        index = _pair_grid(rec, kept, cells) if method == "grid" else None

        def run(mode, out=None, row_start=None, keys=None, flag=None):
            global last_fallback
            if index is None:
                cursor = torch.empty(n_q, **i32) if mode == L.MESH_PAIRS_FILL else None
                L.mesh_pairs_brute(q_rec, None, n_q, rec, self_mode, mode, out, row_start, keys, cursor, flag)
                return
            grid, cell_start, refs = index
            fb_list, fb_count = torch.empty(n_q, **i32), torch.empty(1, **i32)
            L.mesh_pairs_grid(q_rec, rec, refs, cell_start, grid, self_mode, PAIR_CELL_CAP, mode, out, row_start, keys, flag, fb_list, fb_count)
            last_fallback = int(fb_count.cpu())
            if last_fallback:
                cursor = torch.empty(last_fallback, **i32) if mode == L.MESH_PAIRS_FILL else None
                L.mesh_pairs_brute(q_rec, fb_list, last_fallback, rec, self_mode, mode, out, row_start, keys, cursor, flag)

        if not want_list:
            flag = torch.zeros(1, **i32)
            run(L.MESH_PAIRS_ANY, flag=flag)
            return bool(int(flag.cpu()))
        counts = torch.zeros(n_q, **i32)
        run(L.MESH_PAIRS_COUNT, out=counts)
        splits = torch.zeros(n_q + 1, dtype=torch.int64, device=dev)
        splits[1:] = torch.cumsum(counts, 0, dtype=torch.int64)                           # (the scan is plumbing: integer, exact)
        total = int(splits[-1].cpu())
        if total > 2 ** 31 - 1:
            raise L.BodySlamHipError(f"intersecting triangles: {total} pairs, at most 2^31 - 1")
        if total == 0:
            return none
        keys, ordered = torch.empty(total, dtype=torch.int64, device=dev), torch.empty(total, dtype=torch.int64, device=dev)
        run(L.MESH_PAIRS_FILL, row_start=splits, keys=keys)
        L.pc_radius_sort(keys, splits, ordered)
        return torch.stack([ordered >> 32, ordered & 0xFFFFFFFF], 1).to(torch.int32)      # (unpacking the keys is plumbing)


def get_self_intersecting_triangles(vertices, triangles=None, method: str = "auto", cells: Optional[int] = None, device: int = 0) -> torch.Tensor:
    """Open3D's get_self_intersecting_triangles -> int32 [n, 2]: the pairs (i, j), i < j, of KEPT triangles that have a point in common,
    rows in ascending (i, j).  Triangles are closed sets: touching in one point counts.  Only pairs that share no vertex INDEX are tested
    (Open3D's rule): a triangle folded onto its neighbour is therefore not found, and a mesh that is not welded -- the same position under
    several vertex rows -- reports every seam.  Candidates are the pairs whose fp32 boxes overlap; the decision is Guigue & Devillers'
    test over the signs of orient3d, each computed once in fp64 in the order of the vertex rows, and an edge-separation test over
    orient2d for coplanar pairs (tests/_mesh_solid_ref.py): exact whenever a determinant exceeds 2^-50 of the sum
    of its products, and the stated arithmetic's answer otherwise.  method: "grid" walks the scene's triangle grid (cells: the cells
    along the box's longest side; None: the scene's default) and finishes the triangles whose cell box is too large by brute force
    (``last_fallback``); "brute" tests everything against everything; "auto" picks brute force for small inputs.  The method and the
    grid change the time, never the result.  More than 2^31 - 1 pairs: BodySlamHipError."""
    return _pairs((vertices, triangles), None, method, cells, True, device)


def is_self_intersecting(vertices, triangles=None, method: str = "auto", cells: Optional[int] = None, device: int = 0) -> bool:
    """Open3D's is_self_intersecting: ``get_self_intersecting_triangles`` is not empty, found by a search that stops at the first pair"""
    return _pairs((vertices, triangles), None, method, cells, False, device)


def _two(mesh_a, mesh_b):
    return tuple((m, None) if not isinstance(m, (tuple, list)) else tuple(m) for m in (mesh_a, mesh_b))


def get_intersecting_triangles(mesh_a, mesh_b, method: str = "auto", cells: Optional[int] = None, device: int = 0) -> torch.Tensor:
    """int32 [n, 2]: every pair (i of mesh_a, j of mesh_b) of kept triangles with a point in common, ascending; the predicate of
    ``get_self_intersecting_triangles`` (mesh_a is the lower mesh).  mesh_a, mesh_b: a tsdf.TriangleMesh or a (vertices, triangles)
    pair each.  The grid is mesh_b's."""
    a, b = _two(mesh_a, mesh_b)
    return _pairs(a, b, method, cells, True, device)


def is_intersecting(mesh_a, mesh_b, method: str = "auto", cells: Optional[int] = None, device: int = 0) -> bool:
    """Open3D's is_intersecting(other): a triangle of mesh_a and one of mesh_b have a point in common"""
    a, b = _two(mesh_a, mesh_b)
    return _pairs(a, b, method, cells, False, device)


def _component_volumes(v, t, slots):
    """-> (triangle_clusters int32 [T], volume fp64 [C], NaN where the cluster is not closed or not consistently wound)"""
    T = int(t.shape[0])
    bad_half = []

    def vol6(me, parent):
        e = me.edge_of_half.to(torch.int64).clamp(min=0)
        bad_half.append((me.edge_of_half >= 0) & ((me.edge_count[e] != 2) | (me.edge_forward[e] != 1)))
        out = torch.empty(T, dtype=torch.float64, device=t.device)
        L.mesh_signed_volume(_safe_vertices(v), t, parent, out)
        return out
    clusters, n_tri, six = _clusters(v, t, slots, vol6)
    if six.numel() == 0:
        return clusters, six
    bad = torch.zeros(six.numel(), dtype=torch.bool, device=t.device)                      # (integers and masks: plumbing)
    rows = bad_half[0].reshape(T, 3).any(1) & (clusters >= 0)
    bad[clusters[rows].to(torch.int64)] = True
    return clusters, torch.where(bad, torch.full_like(six, float("nan")), six * (1.0 / 6.0))


def component_volumes(vertices, triangles=None, slots: Optional[int] = None, device: int = 0):
    """-> (triangle_clusters int32 [T], volume fp64 [C]): the signed volume of every cluster of cluster_connected_triangles, positive when
    the cluster is wound outwards.  Per kept triangle a . (b x c) in fp64, a, b, c the differences of its vertices to the first vertex
    of the cluster's smallest triangle -- so a cluster's volume depends on no other cluster and not on where the mesh lies --, summed in
    cluster_area's fixed order and multiplied by 1 / 6.  NaN for a cluster that is not closed (an edge without exactly two triangles)
    or not consistently oriented: it has no volume."""
    v, t = _as_mesh(vertices, triangles)
    slots = _check_slots(slots, 3 * int(t.shape[0]))
    dev = _device(v, t, device)
    with torch.cuda.device(dev):
        v, t = _on_device(v, t, dev)
        return _component_volumes(v, t, slots)


def orient_outward(vertices, triangles=None, slots: Optional[int] = None, device: int = 0):
    """``orient_triangles``, then every closed, consistently wound cluster whose signed volume is negative is turned inside out: the last
    two corners of each of its triangles are swapped -> (triangles int32 [T, 3], flipped bool [T] against the input, solid bool [C]:
    whether the cluster -- cluster_connected_triangles' numbering -- has a volume and now a non-negative one).  A cluster that is open
    or cannot be wound consistently is left as ``orient_triangles`` leaves it and is reported False."""
    out, flipped, _ = orient_triangles(vertices, triangles, slots, device)
    v, t = _as_mesh(vertices, triangles)
    with torch.cuda.device(out.device):
        v = v.to(out.device).to(torch.float32).contiguous()
        clusters, vol = _component_volumes(v, out, _check_slots(slots, 3 * int(out.shape[0])))
        if vol.numel() == 0:
            return out, flipped, torch.zeros(0, dtype=torch.bool, device=out.device)
        turn = (clusters >= 0) & (vol[clusters.clamp(min=0).to(torch.int64)] < 0.0)
        out = torch.where(turn[:, None], out[:, [0, 2, 1]], out)                           # (swapping two columns is plumbing)
        return out, flipped ^ turn, ~torch.isnan(vol)


@dataclass
class SolidReport:
    """check_solid's result"""
    is_edge_manifold: bool              # every edge has exactly two triangles (Open3D's is_edge_manifold(allow_boundary_edges=False))
    is_vertex_manifold: bool
    is_self_intersecting: bool
    is_watertight: bool                 # edge-manifold without boundary, vertex-manifold, not self-intersecting
    is_consistently_oriented: bool
    n_boundary_edges: int
    n_non_manifold_edges: int           # edges with more than two triangles
    n_non_manifold_vertices: int
    n_intersecting_pairs: int
    volume: Optional[float]             # get_volume's value when the mesh is watertight and consistently oriented, else None


def is_watertight(vertices, triangles=None, method: str = "auto", cells: Optional[int] = None, slots: Optional[int] = None, device: int = 0) -> bool:
    """Open3D's is_watertight: edge-manifold with no boundary edge allowed, vertex-manifold, and not self-intersecting -- evaluated in that
    order, the cheap terms first, and no further than the first that fails"""
    _check_pair_args(method, cells)
    v, t = _as_mesh(vertices, triangles)
    slots = _check_slots(slots, 3 * int(t.shape[0]))
    dev = _device(v, t, device)
    with torch.cuda.device(dev):
        vd, td = _on_device(v, t, dev)
        T, V = int(td.shape[0]), int(vd.shape[0])
        if T and V:
            me = _edge_rows(td, V, slots)
            if not me.is_edge_manifold(False) or bool((_fan_counts(td, V, me) > 1).any()):
                return False
    return not is_self_intersecting(v, t, method, cells, device)


def _total_volume(vol: torch.Tensor) -> float:
    return abs(float(_segment_sums(vol.contiguous(), torch.tensor([0, vol.numel()], dtype=torch.int64, device=vol.device)).cpu()[0])) if vol.numel() else 0.0


def get_volume(vertices, triangles=None, method: str = "auto", cells: Optional[int] = None, slots: Optional[int] = None, device: int = 0) -> float:
    """Open3D's get_volume, with its precondition: ValueError naming the failed condition unless the mesh is watertight and consistently
    oriented; otherwise abs of the sum of ``component_volumes`` (in cluster_area's fixed order)"""
    r = check_solid(vertices, triangles, method, cells, slots, device)
    if r.volume is None:
        why = ("it has boundary or non-manifold edges" if not r.is_edge_manifold else "it has non-manifold vertices" if not r.is_vertex_manifold
               else "it intersects itself" if r.is_self_intersecting else "it is not consistently oriented")
        raise ValueError(f"get_volume: the mesh is not a watertight, consistently oriented solid: {why}")
    return r.volume


def check_solid(vertices, triangles=None, method: str = "auto", cells: Optional[int] = None, slots: Optional[int] = None, device: int = 0) -> SolidReport:
    """Everything a user should know before trusting a signed distance or a volume -> SolidReport: the five verdicts, the counts behind
    them, and the volume when the mesh has one.  An empty mesh is watertight and has volume 0."""
    _check_pair_args(method, cells)
    v, t = _as_mesh(vertices, triangles)
    slots = _check_slots(slots, 3 * int(t.shape[0]))
    dev = _device(v, t, device)
    with torch.cuda.device(dev):
        vd, td = _on_device(v, t, dev)
        T, V = int(td.shape[0]), int(vd.shape[0])
        me = _edge_rows(td, V, slots)
        n_boundary, n_nm_edges = int(me.get_boundary_edges().shape[0]), int(me.get_non_manifold_edges().shape[0])
        n_nm_vertices = int((_fan_counts(td, V, me) > 1).sum().cpu()) if T and V else 0
        oriented = me.is_consistently_oriented()
    n_pairs = int(get_self_intersecting_triangles(v, t, method, cells, device).shape[0])
    watertight = n_boundary == 0 and n_nm_edges == 0 and n_nm_vertices == 0 and n_pairs == 0
    volume = None
    if watertight and oriented:
        with torch.cuda.device(dev):
            volume = _total_volume(_component_volumes(vd, td, slots)[1])
    return SolidReport(n_boundary == 0 and n_nm_edges == 0, n_nm_vertices == 0, n_pairs > 0, watertight, oriented, n_boundary, n_nm_edges,
                       n_nm_vertices, n_pairs, volume)


# ---- normals -------------------------------------------------------------------------------------------------------------------------------
def compute_triangle_normals(vertices, triangles=None, device: int = 0) -> torch.Tensor:
    """fp32 [T, 3]: the unit (v1 - v0) x (v2 - v0) of every kept triangle -- the face normal sample_mesh returns, the same bits --, zero for
    the others"""
    v, t = _as_mesh(vertices, triangles)
    dev = _device(v, t, device)
    with torch.cuda.device(dev):
        v, t = _on_device(v, t, dev)
        out = torch.empty(int(t.shape[0]), 3, dtype=torch.float32, device=dev)
        if t.shape[0]:
            L.mesh_triangle_geometry(_safe_vertices(v), t, normals=out)
        return out


def compute_vertex_normals(vertices, triangles=None, device: int = 0) -> torch.Tensor:
    """fp32 [V, 3]: Open3D's compute_vertex_normals, area-weighted -- the unnormalised fp64 cross products of a vertex's kept triangles added
    in ascending corner number, normalised and rounded once; zero for a vertex without a kept triangle or with a vanishing sum"""
    v, t = _as_mesh(vertices, triangles)
    dev = _device(v, t, device)
    with torch.cuda.device(dev):
        v, t = _on_device(v, t, dev)
        V, T = int(v.shape[0]), int(t.shape[0])
        out = torch.zeros(V, 3, dtype=torch.float32, device=dev)
        if V == 0 or T == 0:
            return out
        flags = torch.empty(T, dtype=torch.int32, device=dev)
        cross = torch.empty(T, 3, dtype=torch.float64, device=dev)
        L.mesh_triangle_geometry(v, t, flags=flags, cross=cross)
        valid = (flags & L.MESH_TRIANGLE_VALID) != 0
        key = torch.where(valid[:, None], t.to(torch.int64), torch.full_like(t, V, dtype=torch.int64)).reshape(-1)      # (plumbing)
        order = torch.sort(key, stable=True)[1].contiguous()
        start = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(torch.bincount(key, minlength=V + 1)[:V], 0)]).contiguous()
        L.mesh_vertex_normals(cross, order, start, out)
        return out


# ---- smoothing -----------------------------------------------------------------------------------------------------------------------------
def _adjacency(me: MeshEdges, V: int):
    """(nbr_start int64 [V + 1], nbr int32 [2 E]): both directions of every unique edge sorted by (a, b) -- each vertex's neighbours ascending"""
    e = me.edges.to(torch.int64)
    a, b = torch.cat([e[:, 0], e[:, 1]]), torch.cat([e[:, 1], e[:, 0]])
    order = torch.sort((a << 32) | b)[1]
    start = torch.cat([torch.zeros(1, dtype=torch.int64, device=e.device), torch.cumsum(torch.bincount(a, minlength=V), 0)])
    return start.contiguous(), b[order].to(torch.int32).contiguous()


def _smooth(vertices, triangles, iterations, steps, vertex_colors, slots, device):
    from .pointcloud import _as_attribute
    v, t = _as_mesh(vertices, triangles)
    n = _check_iterations(iterations)
    c = _as_attribute(vertex_colors, "vertex_colors", int(v.shape[0]))
    slots = _check_slots(slots, 3 * int(t.shape[0]))
    dev = _device(v, t, device)
    with torch.cuda.device(dev):
        v, t = _on_device(v, t, dev)
        c = None if c is None else c.to(dev).to(torch.float32).contiguous()
        V = int(v.shape[0])
        if V == 0 or n == 0:
            return v.clone(), None if c is None else c.clone()
        start, nbr = _adjacency(_edge_rows(t, V, slots), V)

        def run(x, clamp):
            bufs, src, k = (torch.empty_like(x), torch.empty_like(x)), x, 0          # ping-pong: the input is never written
            for _ in range(n):
                for lam in steps:
                    L.mesh_laplacian_step(src, start, nbr, lam, clamp, bufs[k])
                    src, k = bufs[k], 1 - k
            return src
        return run(v, False), None if c is None else run(c, True)


def filter_smooth_laplacian(vertices, triangles=None, number_of_iterations: int = 1, lambda_filter: float = 0.5, vertex_colors=None,
                            slots: Optional[int] = None, device: int = 0):
    """Open3D's filter_smooth_laplacian -> (vertices fp32 [V, 3], colours fp32 [V, 3] or None).  Per iteration every vertex moves by
    lambda_filter towards the mean of its neighbours -- the other ends of its unique edges, added in ascending order in fp64 --:
    fl32(v + lambda (mean - v)); a vertex without neighbours stays.  vertex_colors take the same step and are clamped to [0, 1]."""
    lam = _check_factor(lambda_filter, "lambda_filter")
    return _smooth(vertices, triangles, number_of_iterations, (lam,), vertex_colors, slots, device)


def filter_smooth_taubin(vertices, triangles=None, number_of_iterations: int = 1, lambda_filter: float = 0.5, mu: float = -0.53, vertex_colors=None,
                         slots: Optional[int] = None, device: int = 0):
    """Open3D's filter_smooth_taubin: per iteration the Laplacian step with lambda_filter, then the one with mu (negative: it undoes the
    shrinkage) -> (vertices, colours or None)"""
    lam, mu = _check_factor(lambda_filter, "lambda_filter"), _check_factor(mu, "mu")
    return _smooth(vertices, triangles, number_of_iterations, (lam, mu), vertex_colors, slots, device)


# ---- removal (TriangleMesh in, TriangleMesh out; plain indexing) ----------------------------------------------------------------------------
def _is_host(mesh) -> bool:
    return isinstance(mesh.vertices, np.ndarray)


def _rows(a, idx):
    """rows idx (an int64 index or a bool mask, as a torch tensor) of a numpy array or a torch tensor, or None"""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a[idx.cpu().numpy()]
    return a[idx.to(a.device)]


def _as_mask(mask, n: int) -> torch.Tensor:
    if isinstance(mask, np.ndarray):
        mask = torch.from_numpy(np.ascontiguousarray(mask))
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or tuple(mask.shape) != (n,):
        raise ValueError(f"mask: expected a bool array or tensor of shape [{n}]")
    return mask


def _map_of(keep: torch.Tensor) -> torch.Tensor:
    """int32 [n]: the new row of every old row, -1 for a row that leaves"""
    return torch.where(keep, torch.cumsum(keep.to(torch.int64), 0) - 1, torch.full((), -1, dtype=torch.int64, device=keep.device)).to(torch.int32)


def _out(mesh, x):
    return x.cpu().numpy() if _is_host(mesh) and isinstance(x, torch.Tensor) else x


def remove_triangles_by_mask(mesh, mask):
    """Open3D's remove_triangles_by_mask: the triangles whose mask is True leave -> (TriangleMesh with the same vertices and the remaining
    triangles in their order, triangle normals carried along; triangle_map int32 [T]: the new row of every old row or -1)"""
    from .tsdf import TriangleMesh
    T = int(mesh.triangles.shape[0])
    m = _as_mask(mask, T)
    keep = ~m
    out = TriangleMesh(mesh.vertices, mesh.vertex_colors, _rows(mesh.triangles, keep), _rows(mesh.triangle_normals, keep), mesh.vertex_normals)
    return out, _out(mesh, _map_of(keep if _is_host(mesh) else keep.to(mesh.triangles.device)))


def remove_unreferenced_vertices(mesh):
    """Open3D's remove_unreferenced_vertices: the vertices no triangle names leave -> (TriangleMesh with the remaining vertices in their order
    -- colours and vertex normals carried along --, the triangles re-indexed; vertex_map int32 [V]).  An index outside [0, V) stays as it is."""
    from .tsdf import TriangleMesh
    V = int(mesh.vertices.shape[0])
    t = mesh.triangles
    tt = (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t).to(torch.int64)
    inside = (tt >= 0) & (tt < V)
    used = torch.zeros(V, dtype=torch.bool, device=tt.device)
    used[tt[inside]] = True
    vmap = _map_of(used)
    new_t = torch.where(inside, vmap.to(torch.int64)[torch.where(inside, tt, torch.zeros_like(tt))], tt).to(torch.int32) if V else tt.to(torch.int32)
    out = TriangleMesh(_rows(mesh.vertices, used), _rows(mesh.vertex_colors, used), _out(mesh, new_t), mesh.triangle_normals,
                       _rows(mesh.vertex_normals, used))
    return out, _out(mesh, vmap)


def remove_small_components(mesh, min_triangles: Optional[int] = None, min_area: Optional[float] = None, keep_largest: bool = False,
                            device: int = 0):
    """Drop the floating fragments: the invalid triangles and every cluster of cluster_connected_triangles with fewer than min_triangles
    triangles or less than min_area area; keep_largest: every cluster but the one of most triangles (ties go to the lower cluster id).
    -> (TriangleMesh, vertex_map int32 [V], triangle_map int32 [T]).  Order-preserving: the remaining triangles and vertices keep their
    order; colours and any normals are carried along."""
    if min_triangles is not None:
        AR.integer(min_triangles, "min_triangles", 0, None, "None or an integer >= 0")
    if min_area is not None:
        min_area = _check_factor(min_area, "min_area")
    if not isinstance(keep_largest, (bool, np.bool_)):
        raise ValueError(f"keep_largest {keep_largest!r}: expected a bool")
    clusters, n_tri, area = cluster_connected_triangles(mesh.vertices, mesh.triangles, device=device)
    drop = torch.zeros(n_tri.numel(), dtype=torch.bool, device=n_tri.device)
    if min_triangles is not None:
        drop |= n_tri < int(min_triangles)
    if min_area is not None:
        drop |= area < min_area
    if keep_largest and n_tri.numel():
        best = int(torch.nonzero(n_tri == n_tri.max())[0, 0].cpu())                    # the first maximum
        drop |= torch.arange(n_tri.numel(), device=n_tri.device) != best
    mask = torch.ones(clusters.numel(), dtype=torch.bool, device=clusters.device)
    if n_tri.numel():
        mask = torch.where(clusters >= 0, drop[clusters.clamp(min=0).to(torch.int64)], mask)
    if _is_host(mesh):
        mask = mask.cpu()
    m1, tmap = remove_triangles_by_mask(mesh, mask)
    m2, vmap = remove_unreferenced_vertices(m1)
    return m2, vmap, tmap
