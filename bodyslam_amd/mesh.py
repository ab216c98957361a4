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

Not built: Open3D's vertex-manifold and self-intersection tests and hence is_watertight, outward orientation of closed components by signed
volume, simplification, subdivision, hole filling, signed distance."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _args as AR
from . import _lib as L

last_rounds = 0          # the (hook, compress) rounds of the latest cluster_connected_triangles, the final unchanged one included
last_orient_rounds = 0   # the (hook, compress) rounds of the latest orient_triangles / is_orientable / orientable_components, likewise


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


def _clusters(v, t, slots):
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
        area = torch.empty(T, dtype=torch.float64, device=dev)
        L.mesh_triangle_geometry(_safe_vertices(v), t, area=area)
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
