"""GPU checks of the mesh clean-up (csrc/mesh_ops.hip, bodyslam_amd/mesh.py): everything bit-equal to the statement tests/_mesh_ops_ref.py --
the edge table, the components, the areas, both normals and both smoothings on the four test meshes and the constructed cases, from numpy and
from device inputs, twice --, the hooking rounds on a permuted strip, every table size, a full table, permuted triangle rows, the removal of
small components, TSDF.extract_mesh(host=False) and the kinds the TriangleMesh methods return.  The largest input is height_field(): 5 400
triangles, 16 200 half-edges -- 63 blocks of 256 and a partial one."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mesh_ops_ref as R  # noqa: E402
import _mesh_scene_ref as MS  # noqa: E402
from test_mesh_ops_cpu import CONSTRUCTED, FRAGMENT, concat, flat_grid, same_bits, shifted_icosphere, strip  # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64, i32 = np.float32, np.float64, np.int32
EDGE_FIELDS = ("edges", "edge_count", "edge_forward", "edge_first_triangle", "edge_of_half")
MESHES = {"cube": MS.cube, "icosphere": lambda: MS.icosphere(2), "height_field": MS.height_field, "grid": flat_grid,
          **{k: (lambda m=m: m) for k, m in CONSTRUCTED.items()}}
_REF = {}


@pytest.fixture(scope="module")
def M():
    import bodyslam_amd.mesh as M
    return M


def colors_of(n):
    return ((np.arange(3 * n).reshape(n, 3) * 37 % 101) / 100.0).astype(f32)


def ref(name):
    """the statement's results for a named mesh, computed once"""
    if name not in _REF:
        v, t = MESHES[name]()
        col = colors_of(len(v))
        lap, tau = R.filter_smooth_laplacian(v, t, 2, 0.5, vertex_colors=col), R.filter_smooth_taubin(v, t, 2, 0.5, -0.53, vertex_colors=col)
        _REF[name] = dict(table=R.edge_table(v, t), clusters=R.cluster_connected_triangles(v, t), area=R.surface_area(v, t),
                          tn=R.triangle_normals(v, t), vn=R.vertex_normals(v, t), lap=lap, tau=tau)
    return _REF[name]


def host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def check_edges(me, table, what):
    for k in EDGE_FIELDS:
        got = host(getattr(me, k))
        assert same_bits(got, table[k]), (what, k, got.shape, table[k].shape)
    assert me.n_invalid_triangles == table["n_invalid"], what


# ---- 1: every output on every mesh, numpy and device inputs, twice ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MESHES))
def test_everything_equals_the_statement(M, name):
    v, t = MESHES[name]()
    col = colors_of(len(v))
    want = ref(name)
    for kind in ("numpy", "device", "device again"):
        a, b, c = (v, t, col) if kind == "numpy" else (torch.from_numpy(x).cuda() for x in (v, t, col))
        me = M.edge_topology(a, b)
        assert all(getattr(me, k).is_cuda and getattr(me, k).dtype == torch.int32 for k in EDGE_FIELDS)
        check_edges(me, want["table"], (name, kind))
        assert me.is_edge_manifold() == R.is_edge_manifold(want["table"]) and me.is_closed() == R.is_closed(want["table"])
        assert me.is_consistently_oriented() == R.is_consistently_oriented(want["table"])
        assert same_bits(host(me.get_boundary_edges()), R.boundary_edges(want["table"]))
        assert same_bits(host(me.get_non_manifold_edges(False)), R.non_manifold_edges(want["table"], False))
        cl, n_tri, area = M.cluster_connected_triangles(a, b)
        assert cl.dtype == torch.int32 and n_tri.dtype == torch.int32 and area.dtype == torch.float64 and area.is_cuda
        for got, exp, k in zip((cl, n_tri, area), want["clusters"], ("clusters", "n_triangles", "cluster_area")):
            assert same_bits(host(got), exp), (name, kind, k)
        assert 1 <= M.last_rounds <= len(t) + 1
        s = M.get_surface_area(a, b)
        assert isinstance(s, float) and same_bits(np.float64(s), np.float64(want["area"])), (name, kind, s, want["area"])
        assert same_bits(host(M.compute_triangle_normals(a, b)), want["tn"]), (name, kind)
        assert same_bits(host(M.compute_vertex_normals(a, b)), want["vn"]), (name, kind)
        lv, lc = M.filter_smooth_laplacian(a, b, 2, 0.5, vertex_colors=c)
        assert same_bits(host(lv), want["lap"][0]) and same_bits(host(lc), want["lap"][1]), (name, kind)
        tv, tc = M.filter_smooth_taubin(a, b, 2, 0.5, -0.53, vertex_colors=c)
        assert same_bits(host(tv), want["tau"][0]) and same_bits(host(tc), want["tau"][1]), (name, kind)
        assert M.filter_smooth_laplacian(a, b, 1)[1] is None
        if kind != "numpy":
            assert same_bits(host(a), v) and same_bits(host(c), col)                              # the inputs are never written


def test_literal_facts(M):
    """the issue's table and the exact Laplacian fixed point, on the device"""
    for name, E, boundary, comps in (("cube", 336, 96, 6), ("icosphere", 480, 0, 1), ("height_field", 8205, 210, 1), ("grid", 208, 32, 1)):
        v, t = MESHES[name]()
        me = M.edge_topology(v, t)
        assert (me.edges.shape[0], me.get_boundary_edges().shape[0], me.get_non_manifold_edges().shape[0]) == (E, boundary, 0)
        assert me.is_consistently_oriented() and M.cluster_connected_triangles(v, t)[1].numel() == comps
    v, t = flat_grid()
    out = host(M.filter_smooth_laplacian(v, t, 1, 1.0)[0])
    i, j = np.meshgrid(np.arange(9), np.arange(9), indexing="xy")
    interior = ((i > 0) & (i < 8) & (j > 0) & (j < 8)).ravel()
    assert same_bits(out[interior], v[interior])
    kept, unit = MS.kept_and_normals(*MS.corners(*MS.height_field()))
    assert kept.all() and same_bits(host(M.compute_triangle_normals(*MS.height_field())), unit)


def test_empty_meshes(M):
    v, t = MS.cube()
    none_t, none_v = np.zeros((0, 3), i32), np.zeros((0, 3), f32)
    me = M.edge_topology(v, none_t)
    assert me.edges.shape == (0, 2) and me.edge_of_half.numel() == 0 and me.is_closed() and me.is_edge_manifold()
    cl, n_tri, area = M.cluster_connected_triangles(v, none_t)
    assert cl.numel() == 0 and n_tri.numel() == 0 and area.numel() == 0 and M.get_surface_area(v, none_t) == 0.0
    assert M.compute_triangle_normals(v, none_t).shape == (0, 3) and not host(M.compute_vertex_normals(v, none_t)).any()
    assert same_bits(host(M.filter_smooth_taubin(v, none_t, 3)[0]), v)
    assert M.compute_vertex_normals(none_v, none_t).shape == (0, 3) and M.filter_smooth_laplacian(none_v, none_t)[0].shape == (0, 3)
    cl, n_tri, _ = M.cluster_connected_triangles(none_v, np.array([[0, 1, 2]], i32))                    # every index outside [0, 0)
    assert cl.tolist() == [-1] and n_tri.numel() == 0


# ---- 2: the hard case for the hooking ----------------------------------------------------------------------------------------------------
def test_permuted_strip(M):
    v, t = strip()
    assert len(t) == 3000
    cl, n_tri, area = M.cluster_connected_triangles(v, t)
    rounds = M.last_rounds
    want = R.cluster_connected_triangles(v, t)
    print("permuted strip of 3 000 triangles:", rounds, "rounds, the cap is", len(t) + 1)
    assert same_bits(host(cl), want[0]) and same_bits(host(n_tri), want[1]) and same_bits(host(area), want[2])
    assert n_tri.tolist() == [3000] and 1 <= rounds < len(t) + 1
    me = M.edge_topology(v, t)
    parent = M._labels(me, len(t))
    assert same_bits(host(parent), R.component_labels(R.edge_table(v, t), len(t)).astype(i32)) and not host(parent).any()


# ---- 3: the table size, through the bindings; a full table ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "height_field", "invalid"])
def test_table_sizes(M, name):
    from bodyslam_amd import _lib as L
    v, t = MESHES[name]()
    want = ref(name)
    E = len(want["table"]["edges"])
    tight, default = 1 << (E - 1).bit_length(), M.edge_table_slots(len(t))
    assert tight >= E and default > 3 * len(t) and default & (default - 1) == 0
    L.init(0)
    td = torch.from_numpy(t).cuda()
    for slots in (tight, default, 8 * default):
        check_edges(M._edge_rows(td, len(v), slots), want["table"], (name, slots))
        cl, n_tri, area = M.cluster_connected_triangles(v, t, slots=slots)
        assert all(same_bits(host(g), w) for g, w in zip((cl, n_tri, area), want["clusters"])), (name, slots)
        assert same_bits(host(M.filter_smooth_laplacian(v, t, 2, 0.5, slots=slots)[0]), want["lap"][0])
    if tight > 1:
        with pytest.raises(L.BodySlamHipError, match="full"):
            M._edge_rows(td, len(v), tight // 2 if tight // 2 < E else tight // 4)
        with pytest.raises(L.BodySlamHipError, match="full"):
            M.edge_topology(v, t, slots=1)
    check_edges(M.edge_topology(v, t), want["table"], (name, "after the full table"))


def test_bindings_directly(M):
    """the launches as a caller of _lib sees them"""
    from bodyslam_amd import _lib as L
    v, t = MS.cube()
    want = ref("cube")
    L.init(0)
    T, slots = len(t), 1024
    i32d = dict(dtype=torch.int32, device="cuda")
    td, vd = torch.from_numpy(t).cuda(), torch.from_numpy(v).cuda()
    keys = torch.full((slots,), L.MESH_EDGE_EMPTY_KEY, dtype=torch.int64, device="cuda")
    first = torch.full((slots,), L.MESH_EDGE_NO_HALF, **i32d)
    count, forward, status = torch.zeros(slots, **i32d), torch.zeros(slots, **i32d), torch.zeros(2, **i32d)
    slot, leader, flag, eoh = (torch.empty(3 * T, **i32d) for _ in range(4))
    L.mesh_edge_insert(td, len(v), keys, first, count, forward, slot, status)
    L.mesh_edge_flags(slot, first, leader, flag)
    rank = torch.cumsum(flag, 0).to(torch.int32)
    E = int(rank[-1])
    assert E == 336 and int((keys != L.MESH_EDGE_EMPTY_KEY).sum()) == E and status.tolist() == [0, 0] and int(count.sum()) == 3 * T
    edges, ec, ef, et = torch.empty(E, 2, **i32d), torch.empty(E, **i32d), torch.empty(E, **i32d), torch.empty(E, **i32d)
    L.mesh_edge_rows(td, slot, count, forward, leader, rank, edges, ec, ef, et, eoh)
    for got, k in zip((edges, ec, ef, et, eoh), EDGE_FIELDS):
        assert same_bits(host(got), want["table"][k]), k
    flags, nrm = torch.empty(T, **i32d), torch.empty(T, 3, device="cuda")
    cross, area = torch.empty(T, 3, dtype=torch.float64, device="cuda"), torch.empty(T, dtype=torch.float64, device="cuda")
    L.mesh_triangle_geometry(vd, td, flags=flags, normals=nrm, cross=cross, area=area)
    valid, kept, unit, n64, a64 = R.triangle_geometry(v, t)
    assert flags.tolist() == [3] * T and same_bits(host(nrm), unit) and same_bits(host(cross), n64) and same_bits(host(area), a64)
    out = torch.empty(3, dtype=torch.float64, device="cuda")
    L.mesh_segment_sum(area, torch.tensor([0, 0, 70, T], device="cuda"), out)                      # an empty segment, one of 70, one of 122
    assert same_bits(host(out), np.array([0.0, R.wave_sum(a64[:70]), R.wave_sum(a64[70:])]))


def promise_mesh():
    """32 vertices, 39 triangles: a 5 x 5 height field (32 ordinary triangles) and one triangle of every kind that is not kept"""
    g = np.arange(5, dtype=f32) * f32(0.25)
    grid = np.array([[x, y, f32(((7 * i + 13 * j) % 5) * 0.05)] for j, y in enumerate(g) for i, x in enumerate(g)], f32)
    extra = np.array([[0.5, 0.5, 0.5], [1, 1, 1], [2, 2, 2],            # 25, 26, 27: exactly collinear
                      [np.nan, 0, 0], [0, np.inf, 0],                   # 28, 29
                      [1e30, 0, 0], [0, 1e30, 0]], f32)                 # 30, 31: with vertex 0 a cross product of 1e60, inf in fp32
    quad = [(5 * j + i, 5 * j + i + 1, 5 * j + i + 5, 5 * j + i + 6) for j in range(4) for i in range(4)]
    ordinary = [tri for a, b, c, d in quad for tri in ((a, b, d), (a, d, c))]
    special = [(3, 3, 9), (7, 12, 12), (25, 26, 27), (0, 1, 28), (5, 29, 6), (0, 30, 31), (26, 25, 27)]
    return np.concatenate([grid, extra]), np.array(ordinary + special, i32)


def test_scene_and_mesh_keep_the_same_triangles(M):
    """the promise of csrc/triangle.h: RaycastingScene and mesh.py keep the same triangles and give the same normal bits"""
    from bodyslam_amd import _lib as L
    from bodyslam_amd import pointcloud as PC
    from bodyslam_amd.raycasting import RaycastingScene
    v, t = promise_mesh()
    T = len(t)
    # the two numpy statements first: the reference alone agrees with itself on this mesh
    valid, kept, unit, _, area = R.triangle_geometry(v, t)
    scene_kept, scene_unit = MS.kept_and_normals(*MS.corners(v, t))
    assert np.array_equal(kept, scene_kept) and same_bits(unit, scene_unit)
    assert kept[:32].all() and not kept[32:].any() and valid[32:].tolist() == [False, False, True, True, True, True, True]
    assert (area[:32] > 0).all() and (np.abs(np.linalg.norm(unit[:32].astype(f64), axis=1) - 1) < 1e-6).all()
    L.init(0)
    vd, td = torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()
    # (a) the kept set of the scene's records is the KEPT flag of the mesh's geometry, triangle for triangle
    records, n_kept = torch.empty(T, 3, 4, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    L.mesh_records(vd, td, records, n_kept)
    flags, nrm = torch.empty(T, dtype=torch.int32, device="cuda"), torch.empty(T, 3, device="cuda")
    L.mesh_triangle_geometry(vd, td, flags=flags, normals=nrm)
    rec_kept = host(records[:, 0, 3].contiguous().view(torch.int32) >= 0)
    flag_kept = (host(flags) & L.MESH_TRIANGLE_KEPT) != 0
    assert np.array_equal(rec_kept, flag_kept) and np.array_equal(flag_kept, kept) and int(n_kept) == 32
    nrm = host(nrm)
    assert same_bits(nrm, unit)
    # (b) a sample's normal is its triangle's row
    _, _, s_normals, s_index = PC.sample_mesh(v, t, 400, seed=3)
    s_index = host(s_index)
    assert len(s_index) == 400 and kept[s_index].all() and len(set(s_index.tolist())) >= 24
    assert same_bits(host(s_normals), nrm[s_index])
    # (c) a hit's primitive normal is that row too: one ray down onto the centroid of every triangle of the height field, and two misses
    centroid = v[t[:32]].astype(f64).mean(1)
    rays = np.concatenate([np.concatenate([centroid + [0, 0, 2], np.tile([0.0, 0, -1], (32, 1))], 1),
                           [[5, 5, 2, 0, 0, -1], [0.4, 0.4, 2, 0, 0, 1]]]).astype(f32)
    scene = RaycastingScene()
    scene.add_triangles(v, t)
    for method in ("grid", "brute"):
        out = scene.cast_rays(rays, method=method)
        prim, got = host(out["primitive_ids"]), host(out["primitive_normals"])
        assert prim[:32].tolist() == list(range(32)) and prim[32:].tolist() == [-1, -1], method
        assert same_bits(got[:32], nrm[prim[:32]]) and not got[32:].any(), method


# ---- 4: permuted triangle rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "height_field"])
def test_permuted_rows(M, name):
    v, t = MESHES[name]()
    perm = np.random.default_rng(5).permutation(len(t))
    me, mp = M.edge_topology(v, t), M.edge_topology(v, t[perm])
    rows = lambda e: sorted(map(tuple, host(e).tolist()))  # noqa: E731
    assert rows(me.edges) == rows(mp.edges)
    count = lambda m: dict(zip(map(tuple, host(m.edges).tolist()), zip(host(m.edge_count).tolist(), host(m.edge_forward).tolist())))  # noqa: E731
    assert count(me) == count(mp)
    cl, clp = host(M.cluster_connected_triangles(v, t)[0]), host(M.cluster_connected_triangles(v, t[perm])[0])
    pairs = set(zip(cl[perm].tolist(), clp.tolist()))
    assert len(pairs) == cl.max() + 1 == clp.max() + 1                                                   # the same partition
    assert same_bits(host(M.compute_vertex_normals(v, t[perm])), R.vertex_normals(v, t[perm]))


# ---- 5: removal -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_mesh", [False, True])
def test_remove_small_components(M, device_mesh):
    from bodyslam_amd.tsdf import TriangleMesh
    v, t = concat(MS.cube(), shifted_icosphere(), FRAGMENT)
    col = colors_of(len(v))
    to = (lambda x: torch.from_numpy(x).cuda()) if device_mesh else (lambda x: x)
    mesh = TriangleMesh(to(v), to(col), to(t))
    mesh.compute_triangle_normals()
    mesh.compute_vertex_normals()
    kind = torch.Tensor if device_mesh else np.ndarray
    clean, vmap, tmap = mesh.remove_small_components(min_triangles=4)
    wv, wt, wvm, wtm = R.remove_small_components(v, t, min_triangles=4)
    assert all(isinstance(x, kind) for x in (clean.vertices, clean.vertex_colors, clean.triangles, clean.triangle_normals, clean.vertex_normals,
                                             vmap, tmap))
    assert same_bits(host(clean.vertices), wv) and same_bits(host(clean.triangles), wt) and same_bits(host(vmap), wvm) and same_bits(host(tmap), wtm)
    assert (host(tmap)[-3:] == -1).all() and (host(tmap)[:-3] >= 0).all() and len(wt) == len(t) - 3            # exactly the fragment
    assert same_bits(host(clean.vertex_colors), col[wvm >= 0]) and same_bits(host(clean.triangle_normals), R.triangle_normals(v, t)[wtm >= 0])
    assert same_bits(host(clean.vertex_normals), R.vertex_normals(v, t)[wvm >= 0])
    assert np.array_equal(np.unique(host(clean.triangles)), np.arange(len(wv)))
    big, _, _ = mesh.remove_small_components(keep_largest=True)
    iv, it = shifted_icosphere()
    assert same_bits(host(big.vertices), iv) and same_bits(host(big.triangles), it) and big.is_closed() and big.is_consistently_oriented()
    by_area, _, _ = mesh.remove_small_components(min_area=5.0)
    assert same_bits(host(by_area.triangles), it)
    bad = concat((v, t), (np.zeros((0, 3), f32), np.array([[0, 0, 1], [0, 1, 9999]], i32)))                 # two invalid rows leave too
    got, _, tm = TriangleMesh(to(bad[0]), to(col), to(bad[1])).remove_small_components()
    assert same_bits(host(got.triangles), t) and host(tm)[-2:].tolist() == [-1, -1]


# ---- 6: the TriangleMesh methods and the TSDF mesh -----------------------------------------------------------------------------------------
def test_methods_return_the_kind_of_the_mesh(M):
    from bodyslam_amd.tsdf import TriangleMesh
    v, t = MS.icosphere(2)
    col = colors_of(len(v))
    for dev in (False, True):
        to = (lambda x: torch.from_numpy(x).cuda()) if dev else (lambda x: x)
        kind = torch.Tensor if dev else np.ndarray
        mesh = TriangleMesh(to(v), to(col), to(t))
        e = mesh.edge_topology()
        assert all(isinstance(getattr(e, k), kind) for k in EDGE_FIELDS)
        check_edges(e, ref("icosphere")["table"], dev)
        assert isinstance(mesh.get_boundary_edges(), kind) and isinstance(mesh.get_non_manifold_edges(), kind)
        assert mesh.is_edge_manifold() and mesh.is_edge_manifold(False) and mesh.is_closed() and mesh.is_consistently_oriented()
        cl = mesh.cluster_connected_triangles()
        assert all(isinstance(x, kind) for x in cl) and same_bits(host(cl[2]), ref("icosphere")["clusters"][2])
        assert same_bits(np.float64(mesh.get_surface_area()), np.float64(ref("icosphere")["area"]))
        tn, vn = mesh.compute_triangle_normals(), mesh.compute_vertex_normals()
        assert tn is mesh.triangle_normals and vn is mesh.vertex_normals and isinstance(tn, kind) and isinstance(vn, kind)
        assert same_bits(host(tn), ref("icosphere")["tn"]) and same_bits(host(vn), ref("icosphere")["vn"])
        lap, tau = mesh.filter_smooth_laplacian(2, 0.5, colors=True), mesh.filter_smooth_taubin(2, 0.5, -0.53)
        assert all(isinstance(x, kind) for x in (lap.vertices, lap.vertex_colors, lap.triangles, tau.vertices, tau.vertex_colors))
        assert same_bits(host(lap.vertices), ref("icosphere")["lap"][0]) and same_bits(host(lap.vertex_colors), ref("icosphere")["lap"][1])
        assert same_bits(host(tau.vertices), ref("icosphere")["tau"][0]) and same_bits(host(tau.vertex_colors), col)
        half = mesh.remove_triangles_by_mask(to(np.arange(320) >= 160))
        assert isinstance(half.triangles, kind) and same_bits(host(half.triangles), t[:160]) and not half.is_closed()
        assert isinstance(half.remove_unreferenced_vertices().vertices, kind)
        pcd, _ = mesh.sample_points_uniformly(100, seed=1)                    # the existing method takes the longer dataclass
        assert isinstance(pcd.points, kind)


def test_tsdf_extract_mesh_on_the_device():
    """extract_mesh(host=False) holds the rows of extract_mesh().  The vertices are merged by a sort of their cube-edge identities, so their
    rows are the same in every call; the order of the triangles inside a volume unit is the order the extraction's atomics gave, which
    differs from call to call (as extract_pcd's rows do), so the triangle rows are compared after sorting them."""
    from bodyslam_amd.tsdf import MAP, TSDF, PinholeCameraIntrinsic, RGBDImage
    from test_tsdf_gpu import H, K, W, scene
    tsdf = TSDF(0.01, 0.04, volume_unit_resolution=8, depth_sampling_stride=4)
    intr = PinholeCameraIntrinsic(W, H, *K)
    for seed in range(3):
        depth, color, E = scene(seed)
        tsdf.build_3D_map(RGBDImage(color, depth), intr, E)
    a, b = tsdf.extract_mesh(), tsdf.extract_mesh(host=False)
    assert all(isinstance(x, np.ndarray) for x in (a.vertices, a.vertex_colors, a.triangles)) and a.triangles.shape[0] > 1000
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in (b.vertices, b.vertex_colors, b.triangles))
    assert b.triangles.dtype == torch.int32 and b.triangles.is_contiguous() and b.triangle_normals is None and b.vertex_normals is None
    assert same_bits(host(b.vertices), a.vertices) and same_bits(host(b.vertex_colors), a.vertex_colors)
    rows = lambda t: t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]  # noqa: E731
    assert same_bits(rows(host(b.triangles)), rows(a.triangles))
    assert b.is_edge_manifold() and a.is_edge_manifold() and b.is_consistently_oriented()
    assert len(b.get_boundary_edges()) == len(a.get_boundary_edges()) > 0
    clean, vmap, tmap = b.remove_small_components(keep_largest=True)
    assert clean.triangles.is_cuda and clean.cluster_connected_triangles()[1].numel() == 1 and clean.compute_vertex_normals().shape == clean.vertices.shape
    empty = TSDF(0.01, 0.04, volume_unit_resolution=8, depth_sampling_stride=4).extract_mesh(host=False)
    assert empty.vertices.is_cuda and empty.triangles.shape == (0, 3) and empty.triangles.dtype == torch.int32
    assert empty.cluster_connected_triangles()[1].numel() == 0 and empty.is_edge_manifold()
    assert MAP.extract_mesh.__defaults__ == (True,) and TSDF.extract_mesh.__defaults__ == (True,)
