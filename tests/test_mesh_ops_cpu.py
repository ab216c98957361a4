"""The statement of the mesh clean-up (tests/_mesh_ops_ref.py) against independent facts: the counts of the test meshes, scipy's connected
components, analytic areas, constructed cases, the face normals of the mesh scene, and the argument errors of bodyslam_amd/mesh.py.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mesh_ops_ref as R  # noqa: E402
import _mesh_scene_ref as MS  # noqa: E402

f32, f64, i32 = np.float32, np.float64, np.int32
# the worst angle between the statement's vertex normal and the radial direction on icosphere(2) is 1.3542 degrees (measured with the
# statement): the faces at a vertex of the subdivided icosahedron are not equal, so their area-weighted mean leans
ICOSPHERE_NORMAL_ANGLE_DEG = 1.36


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def flat_grid(n=9):
    x = np.arange(n) * 2.0 ** -8
    return MS.grid_patch(x, x, lambda X, Y: np.zeros_like(X))


def strip(n=1501, seed=0):
    """one strip of 2 (n - 1) triangles on a 2 x n lattice, its triangle rows permuted: the hard case for the hooking rounds"""
    v, t = MS.grid_patch(np.arange(n) * 2.0 ** -8, np.arange(2) * 2.0 ** -8, lambda X, Y: np.zeros_like(X))
    return v, t[np.random.default_rng(seed).permutation(len(t))]


def shifted_icosphere(offset=(4.0, 0.0, 0.0)):
    v, t = MS.icosphere(2)
    return (v.astype(f64) + np.array(offset)).astype(f32), t


def concat(*meshes):
    vs, ts, base = [], [], 0
    for v, t in meshes:
        vs.append(v)
        ts.append(t + base)
        base += len(v)
    return np.concatenate(vs).astype(f32), np.concatenate(ts).astype(i32)


FRAGMENT = (np.array([[9, 0, 0], [10, 0, 0], [9, 1, 0], [10, 1, 0], [11, 0, 0]], f32), np.array([[0, 1, 2], [1, 3, 2], [1, 4, 3]], i32))
UNIT = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1], [2, 0, 0]], f32)
# name -> (vertices, triangles): the constructed cases, shared with tests/test_mesh_ops_gpu.py
CONSTRUCTED = {
    "one vertex shared": (UNIT, np.array([[0, 1, 2], [0, 4, 5]], i32)),
    "three on an edge": (UNIT, np.array([[0, 1, 2], [1, 0, 4], [0, 1, 3]], i32)),
    "flipped neighbour": (UNIT, np.array([[0, 1, 2], [1, 2, 3]], i32)),
    "duplicate": (UNIT, np.array([[0, 1, 2], [0, 1, 2]], i32)),
    "invalid": (UNIT, np.array([[0, 1, 2], [1, 1, 3], [0, 6, 1], [1, 3, 2], [-1, 0, 2]], i32)),
    "zero area": (UNIT, np.array([[0, 1, 5], [1, 0, 2]], i32)),
}


# ---- the table of the issue ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,V,T,E,boundary,components", [("cube", 150, 192, 336, 96, 6), ("icosphere", 162, 320, 480, 0, 1),
                                                             ("height_field", 2806, 5400, 8205, 210, 1), ("grid", 81, 128, 208, 32, 1)])
def test_counts(name, V, T, E, boundary, components):
    v, t = {"cube": MS.cube, "icosphere": lambda: MS.icosphere(2), "height_field": MS.height_field, "grid": flat_grid}[name]()
    tab = R.edge_table(v, t)
    assert (len(v), len(t), len(tab["edges"]), len(R.boundary_edges(tab))) == (V, T, E, boundary)
    assert len(R.non_manifold_edges(tab)) == 0 and R.is_edge_manifold(tab) and R.is_consistently_oriented(tab) and tab["n_invalid"] == 0
    assert R.is_closed(tab) == (boundary == 0) and R.is_edge_manifold(tab, allow_boundary_edges=False) == (boundary == 0)
    cl, n_tri, area = R.cluster_connected_triangles(v, t)
    assert len(n_tri) == components and n_tri.sum() == T and cl.dtype == i32 and area.dtype == f64
    assert (tab["edges"][:, 0] < tab["edges"][:, 1]).all() and tab["edge_count"].sum() == 3 * T
    first = np.array([np.nonzero(tab["edge_of_half"] == e)[0][0] for e in range(E)])
    assert (np.diff(first) > 0).all() and np.array_equal(first // 3, tab["edge_first_triangle"])


@pytest.mark.parametrize("mesh", ["cube", "height_field", "strip", "mixed"])
def test_components_equal_scipy(mesh):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    v, t = {"cube": MS.cube, "height_field": MS.height_field, "strip": strip,
            "mixed": lambda: concat(MS.cube(), shifted_icosphere(), FRAGMENT)}[mesh]()
    T = len(t)
    by_edge = {}
    for i, (a, b, c) in enumerate(t.tolist()):
        for e in ((a, b), (b, c), (c, a)):
            by_edge.setdefault((min(e), max(e)), []).append(i)
    rows, cols = [], []
    for ts in by_edge.values():
        rows += ts[1:]
        cols += [ts[0]] * (len(ts) - 1)
    n, lab = connected_components(sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(T, T)), directed=False)
    cl, n_tri, _ = R.cluster_connected_triangles(v, t)
    assert len(n_tri) == n
    pairs = set(zip(cl.tolist(), lab.tolist()))
    assert len(pairs) == n                                                     # a bijection of the labels: the same partition
    first = [int(np.nonzero(cl == c)[0][0]) for c in range(n)]
    assert first == sorted(first)                                              # cluster ids ascend with the first triangle
    assert np.array_equal(n_tri, np.bincount(cl, minlength=n))


def test_cube_clusters_and_areas():
    v, t = MS.cube()
    cl, n_tri, area = R.cluster_connected_triangles(v, t)
    assert n_tri.tolist() == [32] * 6 and np.array_equal(cl, np.repeat(np.arange(6), 32).astype(i32))
    # a face is 32 triangles of area 0.125, computed from dyadic coordinates without a rounding; their sum of magnitude 4 in the statement's
    # order makes at most 32 + 6 additions, each off by at most 2^-53 of a partial sum <= 4: (T_face + 6) 4 2^-53
    bound = (32 + 6) * 4.0 * 2.0 ** -53
    assert np.abs(area - 4.0).max() <= bound
    assert abs(R.surface_area(v, t) - 24.0) <= (192 + 6) * 24.0 * 2.0 ** -53


# ---- constructed cases ---------------------------------------------------------------------------------------------------------------------
def test_constructed_cases():
    tab = {k: R.edge_table(*m) for k, m in CONSTRUCTED.items()}
    cc = {k: R.cluster_connected_triangles(*m) for k, m in CONSTRUCTED.items()}
    assert cc["one vertex shared"][0].tolist() == [0, 1] and cc["one vertex shared"][1].tolist() == [1, 1]
    assert len(R.non_manifold_edges(tab["three on an edge"])) == 1 and R.non_manifold_edges(tab["three on an edge"]).tolist() == [[0, 1]]
    assert cc["three on an edge"][0].tolist() == [0, 0, 0] and not R.is_edge_manifold(tab["three on an edge"])
    assert not R.is_consistently_oriented(tab["flipped neighbour"]) and cc["flipped neighbour"][1].tolist() == [2]
    assert R.is_consistently_oriented(R.edge_table(UNIT, np.array([[0, 1, 2], [2, 1, 3]], i32)))
    d = tab["duplicate"]
    assert d["edge_count"].tolist() == [2, 2, 2] and sorted(d["edge_forward"].tolist()) == [0, 2, 2] and not R.is_consistently_oriented(d)
    assert set(d["edge_forward"].tolist()) <= {0, 2}
    inv = tab["invalid"]
    assert inv["n_invalid"] == 3 and len(inv["edges"]) == 5 and cc["invalid"][0].tolist() == [0, -1, -1, 0, -1] and cc["invalid"][1].tolist() == [2]
    assert inv["edge_of_half"].reshape(-1, 3)[[1, 2, 4]].tolist() == [[-1] * 3] * 3 and (inv["edge_of_half"].reshape(-1, 3)[[0, 3]] >= 0).all()
    z = R.triangle_geometry(*CONSTRUCTED["zero area"])
    assert z[0].tolist() == [True, True] and z[1].tolist() == [False, True] and not z[2][0].any() and z[4][0] == 0.0
    assert cc["zero area"][0].tolist() == [0, 0] and cc["zero area"][2].tolist() == [0.5]


# ---- normals -------------------------------------------------------------------------------------------------------------------------------
def test_triangle_normals_are_the_scene_normals():
    for v, t in (MS.cube(), MS.icosphere(2), MS.height_field(), CONSTRUCTED["zero area"]):
        kept, unit = MS.kept_and_normals(*MS.corners(v, t))
        assert same_bits(R.triangle_normals(v, t), unit)
        if kept.all():
            _, _, nrm, tri = MS.sample_mesh(v, t, 500, seed=3)
            assert same_bits(R.triangle_normals(v, t)[tri], nrm)


def test_vertex_normals_icosphere():
    v, t = MS.icosphere(2)
    n = R.vertex_normals(v, t).astype(f64)
    radial = v.astype(f64) / np.linalg.norm(v.astype(f64), axis=1, keepdims=True)
    angle = np.degrees(np.arccos(np.clip((n * radial).sum(1), -1.0, 1.0)))
    print("worst angle to the radial direction:", angle.max(), "degrees")
    assert angle.max() <= ICOSPHERE_NORMAL_ANGLE_DEG and np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-6
    flat = R.vertex_normals(*flat_grid())
    assert same_bits(flat, np.tile(np.array([0, 0, 1], f32), (81, 1)))
    lone = R.vertex_normals(UNIT, np.array([[0, 1, 2]], i32))
    assert lone[:3].tolist() == [[0, 0, 1]] * 3 and not lone[3:].any()


# ---- removal -------------------------------------------------------------------------------------------------------------------------------
def test_remove_small_components():
    v, t = concat(MS.cube(), shifted_icosphere(), FRAGMENT)
    nv, nt, vmap, tmap = R.remove_small_components(v, t, min_triangles=4)
    assert len(nt) == len(t) - 3 and (tmap[-3:] == -1).all() and (tmap[:-3] == np.arange(len(t) - 3)).all()
    assert (vmap[-5:] == -1).all() and len(nv) == len(v) - 5
    keep_t, keep_v = tmap >= 0, vmap >= 0
    assert same_bits(nv, v[keep_v]) and np.array_equal(vmap[keep_v], np.arange(keep_v.sum()))          # old -> new -> the same rows, in order
    assert np.array_equal(nt, vmap[t[keep_t]]) and same_bits(nv[nt], v[t[keep_t]])
    assert np.array_equal(np.unique(nt), np.arange(len(nv)))                                            # no unreferenced vertex remains
    nv, nt, vmap, tmap = R.remove_small_components(v, t, keep_largest=True)
    iv, it = shifted_icosphere()
    assert same_bits(nv, iv) and np.array_equal(nt, it) and (tmap >= 0).sum() == 320
    nv, nt, _, _ = R.remove_small_components(v, t, min_area=5.0)                                        # the cube's faces have area 4
    assert same_bits(nv, iv) and np.array_equal(nt, it)
    nv, nt, _, _ = R.remove_small_components(*MS.cube(), keep_largest=True)                             # six equal clusters: the lowest id
    assert np.array_equal(nt, MS.cube()[1][:32]) and len(nv) == 25


# ---- smoothing -----------------------------------------------------------------------------------------------------------------------------
def test_laplacian_leaves_the_flat_interior():
    v, t = flat_grid()
    out, _ = R.filter_smooth_laplacian(v, t, 1, 1.0)
    i, j = np.meshgrid(np.arange(9), np.arange(9), indexing="xy")
    interior = ((i > 0) & (i < 8) & (j > 0) & (j < 8)).ravel()
    assert same_bits(out[interior], v[interior]) and not same_bits(out[~interior], v[~interior])
    start, nbr = R.adjacency(R.edge_table(v, t), len(v))
    assert (np.diff(start)[interior] == 6).all() and all((np.diff(nbr[start[k]:start[k + 1]]) > 0).all() for k in range(81))


def test_taubin_shrinks_less_than_laplacian():
    v, t = MS.icosphere(2)
    radius = lambda p: np.linalg.norm(p.astype(f64), axis=1).mean()  # noqa: E731
    lap, tau = R.filter_smooth_laplacian(v, t, 10, 0.5)[0], R.filter_smooth_taubin(v, t, 10, 0.5, -0.53)[0]
    print("mean radius:", radius(v), "Laplacian", radius(lap), "Taubin", radius(tau))
    assert abs(radius(tau) - radius(v)) < abs(radius(lap) - radius(v))
    col = np.linspace(-0.2, 1.2, 162 * 3).reshape(162, 3).astype(f32)
    c = R.filter_smooth_taubin(v, t, 2, 0.5, -0.53, vertex_colors=col)[1]
    assert c.min() >= 0.0 and c.max() <= 1.0 and c.dtype == f32


# ---- the argument errors of the product ----------------------------------------------------------------------------------------------------
def test_argument_errors():
    import torch
    import bodyslam_amd.mesh as M
    from bodyslam_amd.tsdf import TriangleMesh
    v, t = MS.cube()
    bad = [lambda: M.edge_topology(v.astype(np.float16), t), lambda: M.edge_topology(v, t.astype(f32)), lambda: M.edge_topology(v[:, :2], t),
           lambda: M.edge_topology(v, t[:, :2]), lambda: M.edge_topology("mesh", t), lambda: M.edge_topology(v, None),
           lambda: M.edge_topology(TriangleMesh(v, v, t), t), lambda: M.edge_topology(v, t, slots=100), lambda: M.edge_topology(v, t, slots=0),
           lambda: M.cluster_connected_triangles(v, t, slots=True), lambda: M.compute_vertex_normals(torch.from_numpy(v).to(torch.float16), t),
           lambda: M.filter_smooth_laplacian(v, t, -1), lambda: M.filter_smooth_laplacian(v, t, 1.5), lambda: M.filter_smooth_laplacian(v, t, 1, np.nan),
           lambda: M.filter_smooth_taubin(v, t, 1, 0.5, np.inf), lambda: M.filter_smooth_taubin(v, t, 1, 0.5, "mu"),
           lambda: M.filter_smooth_laplacian(v, t, 1, 0.5, vertex_colors=v[:10]),
           lambda: M.remove_triangles_by_mask(TriangleMesh(v, v, t), np.zeros(len(t), np.int32)),
           lambda: M.remove_triangles_by_mask(TriangleMesh(v, v, t), np.zeros(5, bool)),
           lambda: M.remove_small_components(TriangleMesh(v, v, t), min_triangles=-1),
           lambda: M.remove_small_components(TriangleMesh(v, v, t), min_triangles=2.5),
           lambda: M.remove_small_components(TriangleMesh(v, v, t), min_area=np.nan),
           lambda: M.remove_small_components(TriangleMesh(v, v, t), keep_largest=1),
           lambda: TriangleMesh(v, v, t).filter_smooth_laplacian(colors=1), lambda: TriangleMesh(v, v, t).filter_smooth_taubin(colors="yes")]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
        assert True, k
    assert M.edge_table_slots(192) == 1024 and M.edge_table_slots(5400) == 16384 and M.edge_table_slots(1) == 4
    m = TriangleMesh(v, v, t)                                                  # the two new arguments are optional and trailing
    assert m.triangle_normals is None and m.vertex_normals is None
    m = TriangleMesh(v, v, t, None, v)
    assert m.vertex_normals is v and TriangleMesh(vertices=v, vertex_colors=v, triangles=t, vertex_normals=v).vertex_normals is v
    # removal is plain indexing: a numpy mesh needs no GPU
    out, tmap = M.remove_triangles_by_mask(TriangleMesh(v, v, t, R.triangle_normals(v, t)), np.arange(len(t)) >= 32)
    assert np.array_equal(out.triangles, t[:32]) and out.triangle_normals.shape == (32, 3) and tmap.tolist() == list(range(32)) + [-1] * 160
    out2, vmap = M.remove_unreferenced_vertices(out)
    want_rows, want_t, want_map = R.remove_unreferenced_vertices(len(v), t[:32])
    assert same_bits(out2.vertices, v[want_rows]) and same_bits(out2.triangles, want_t) and same_bits(vmap, want_map)
    assert out2.triangle_normals.shape == (32, 3) and isinstance(vmap, np.ndarray)
