"""GPU checks of "is this mesh a solid" (csrc/mesh_solid.hip, bodyslam_amd/mesh.py): every result EQUAL to the statement
tests/_mesh_solid_ref.py -- and, on the integer-lattice meshes, to the exact oracle --: the intersecting pairs with method="grid" at three
cell counts (one cell, the default, far finer than the triangles) and with "brute", from numpy and from device inputs, twice; ANY equal to
COUNT > 0; the fallback path; rows that take no part; T = 0 and T = 1; the vertex fans, the volumes, orient_outward, is_watertight,
check_solid and the kinds the TriangleMesh methods return.  The largest input is 384 triangles; a cell of the one-cell grid lists all of
them, more than one block."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mesh_scene_ref as MS  # noqa: E402
import _mesh_solid_ref as S  # noqa: E402
import _orient_ref as O  # noqa: E402
import test_mesh_solid_cpu as C  # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64, i32 = np.float32, np.float64, np.int32
WAYS = (("grid", 1), ("grid", None), ("grid", 32), ("brute", None))
LATTICE = ("welded_cube", "interpenetrating", "corner_touching", "seams", "coplanar", "piercing", "nested")
OTHERS = dict(icosphere=lambda: MS.icosphere(2), torus=O.torus, soup=C.soup, soup_big=lambda: C.soup(big=True), promise=C.promise_mesh)
_REF = {}


@pytest.fixture(scope="module")
def M():
    import bodyslam_amd.mesh as M
    return M


def mesh_of(name):
    return C.lattice_mesh(name) if name in LATTICE else OTHERS[name]()


def ref_pairs(name):
    """the statement's pairs of a named mesh, computed once"""
    if name not in _REF:
        _REF[name] = S.intersecting_pairs(*mesh_of(name))
    return _REF[name]


def host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def same(a, b):
    a, b = host(a), host(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_all_ways(M, name, v, t, want, other=None):
    """the list and the flag, every method and grid, numpy and device inputs, twice"""
    fallbacks = {}
    for kind in ("numpy", "device", "device again"):
        a = (v, t) if kind == "numpy" else (torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda())
        b = None if other is None else (other if kind == "numpy" else tuple(torch.from_numpy(x).cuda() for x in other))
        for method, cells in WAYS:
            if other is None:
                got = M.get_self_intersecting_triangles(*a, method=method, cells=cells)
                fallbacks[(method, cells)] = M.last_fallback
                flag = M.is_self_intersecting(*a, method=method, cells=cells)
            else:
                got = M.get_intersecting_triangles(a, b, method=method, cells=cells)
                fallbacks[(method, cells)] = M.last_fallback
                flag = M.is_intersecting(a, b, method=method, cells=cells)
            assert got.is_cuda and got.dtype == torch.int32 and same(got, want), (name, kind, method, cells, got.shape, want.shape)
            assert flag is (len(want) > 0), (name, kind, method, cells)
    return fallbacks


# ---- intersecting pairs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LATTICE)
def test_lattice_meshes_equal_the_statement_and_the_exact_oracle(M, name):
    v, t = mesh_of(name)
    want = ref_pairs(name)
    assert C.same_pairs(want, S.intersecting_pairs(v, t, predicate=S.exact_predicate))
    if C.LATTICE_PAIRS.get(name) is not None:
        assert len(want) == C.LATTICE_PAIRS[name]
    else:
        assert len(want) > 0
    check_all_ways(M, name, v, t, want)


def test_two_meshes(M):
    (va, ta), (vb, tb) = C.welded_cube(), C.welded_cube((1, 1, 1))
    want = S.intersecting_pairs(va, ta, vb, tb)
    assert len(want) > 0 and C.same_pairs(want, S.intersecting_pairs(va, ta, vb, tb, predicate=S.exact_predicate))
    check_all_ways(M, "two cubes", va, ta, want, other=(vb, tb))
    far = (vb + f32(10), tb)
    check_all_ways(M, "apart", va, ta, np.zeros((0, 2), i32), other=far)
    # a soup against the icosphere: non-lattice, A's boxes partly outside B's grid
    (va, ta), (vb, tb) = C.soup(120, seed=3), MS.icosphere(1)
    va = (va * f32(3) - f32(1.5)).astype(f32)
    want = S.intersecting_pairs(va, ta, vb, tb)
    assert len(want) > 0
    check_all_ways(M, "soup x icosphere", va, ta, want, other=(vb, tb))


@pytest.mark.parametrize("name", ["icosphere", "torus", "soup", "soup_big", "promise"])
def test_other_meshes_equal_the_statement(M, name):
    v, t = mesh_of(name)
    want = ref_pairs(name)
    fallbacks = check_all_ways(M, name, v, t, want)
    if name in ("icosphere", "torus"):
        assert len(want) == 0
    if name == "soup":
        assert len(want) > 10 and fallbacks[("grid", 32)] == 0
    if name == "soup_big":
        big = len(t) - 1
        assert (want[:, 1] == big).sum() > 10 and len(want) > len(ref_pairs("soup"))
        assert fallbacks[("grid", 32)] == 1 and fallbacks[("grid", 1)] == 0 and fallbacks[("brute", None)] == 0
    if name == "promise":
        assert len(want) > 0 and (want[:, 1] == len(t) - 1).all()       # the rows that are invalid or not kept take no part


def test_edge_sizes_and_errors(M):
    v, t = C.welded_cube()
    none = np.zeros((0, 2), i32)
    for tt in (t[:0], t[:1]):
        for method, cells in WAYS:
            assert same(M.get_self_intersecting_triangles(v, tt, method=method, cells=cells), none)
            assert M.is_self_intersecting(v, tt, method=method, cells=cells) is False
    assert same(M.get_intersecting_triangles((v, t[:1]), (v + f32(1), t[:0])), none)
    assert same(M.get_intersecting_triangles((v, t[:1]), (v[:, [1, 2, 0]] + f32(0.5), t[:1]), method="grid"),
                S.intersecting_pairs(v, t[:1], v[:, [1, 2, 0]] + f32(0.5), t[:1]))
    assert same(M.get_self_intersecting_triangles(v, np.full((3, 3), 9, i32)), none)          # nothing valid
    assert same(M.get_self_intersecting_triangles(*C.interpenetrating_cubes(), method="auto"), ref_pairs("interpenetrating"))
    with pytest.raises(ValueError):
        M.get_self_intersecting_triangles(v, t, method="bvh")
    with pytest.raises(ValueError):
        M.get_self_intersecting_triangles(v, t, cells=0)
    with pytest.raises(ValueError):
        M.is_self_intersecting(v, t, cells=1.5)
    with pytest.raises(ValueError):
        M.get_self_intersecting_triangles(*MS.icosphere(2), method="grid", cells=4096)       # more than 2^24 cells


# ---- vertex fans ---------------------------------------------------------------------------------------------------------------------------
def test_vertex_fans(M):
    strip_v, strip_t, _ = O.long_strip(1000)
    cases = dict(bow_tie=C.bow_tie(), open_fan=C.open_fan(), shared_edge=C.cubes_sharing_an_edge(), promise=C.promise_mesh(), strip=(strip_v, strip_t),
                 book=O.book(), icosphere=MS.icosphere(2), corner=C.corner_touching_cubes(),
                 unreferenced=(np.zeros((8, 3), f32), np.array([[0, 1, 2], [0, 2, 3], [0, 4, 5]], i32)),
                 invalid_only=(C.welded_cube()[0], np.concatenate([C.welded_cube()[1][:3], [[7, 7, 6], [7, 99, 6]]]).astype(i32)))
    want = {k: S.non_manifold_vertices(*m) for k, m in cases.items()}
    assert want["bow_tie"].tolist() == [0] and want["unreferenced"].tolist() == [0] and want["promise"].tolist() == [0]
    assert all(len(want[k]) == 0 for k in ("open_fan", "shared_edge", "strip", "icosphere", "invalid_only", "corner", "book"))
    for name, (v, t) in cases.items():
        for kind in ("numpy", "device", "device again"):
            a = (v, t) if kind == "numpy" else (torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda())
            got = M.get_non_manifold_vertices(*a)
            assert got.is_cuda and got.dtype == torch.int32 and same(got, want[name]), (name, kind)
            assert M.is_vertex_manifold(*a) is (len(want[name]) == 0)
            assert 1 <= M.last_fan_rounds <= 3 * len(t) + 1
        if name in ("strip", "icosphere"):
            assert M.last_fan_rounds >= 2                      # a round that hooks, and the last one, which finds nothing to do
    v, t = C.bow_tie()
    for slots in (32, 64, 4096):
        assert same(M.get_non_manifold_vertices(v, t, slots=slots), want["bow_tie"])
    assert same(M.get_non_manifold_vertices(v, t[:0]), np.zeros(0, i32)) and M.is_vertex_manifold(v[:0], t[:0])


# ---- volume --------------------------------------------------------------------------------------------------------------------------------
def test_volumes(M):
    two = O.merged(C.welded_cube((5, 5, 5), 3), C.tetrahedron(), C.welded_cube(inward=True))
    strip_torus = O.merged(O.moebius_strip(), O.torus())
    cases = dict(cube=C.welded_cube(), inward=C.welded_cube(inward=True), tetrahedron=C.tetrahedron(), components=two, open=C.open_cube(),
                 strip_torus=strip_torus, icosphere=MS.icosphere(2), promise=C.promise_mesh(), bow_tie=C.bow_tie())
    for name, (v, t) in cases.items():
        want = S.component_volumes(v, t)
        for kind in ("numpy", "device", "device again"):
            a = (v, t) if kind == "numpy" else (torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda())
            cl, vol = M.component_volumes(*a)
            assert cl.dtype == torch.int32 and vol.dtype == torch.float64 and vol.is_cuda
            assert same(cl, want[0]) and same(vol, want[1]), (name, kind, host(vol), want[1])
    assert host(M.component_volumes(*cases["cube"])[1]).tolist() == [8.0]
    assert host(M.component_volumes(*cases["inward"])[1]).tolist() == [-8.0]
    assert host(M.component_volumes(*cases["tetrahedron"])[1]).tolist() == [30 * (1.0 / 6.0)]
    assert host(M.component_volumes(*two)[1]).tolist() == [27.0, 5.0, -8.0]
    assert np.isnan(host(M.component_volumes(*cases["open"])[1])).all()
    assert M.get_volume(*cases["cube"]) == 8.0 and M.get_volume(*cases["inward"]) == 8.0
    assert M.get_volume(*MS.icosphere(2)) == S.check_solid(*MS.icosphere(2))["volume"]
    for bad, word in ((cases["open"], "edges"), (C.bow_tie(), "vertices"), (C.interpenetrating_cubes(), "intersects"),
                      ((C.welded_cube()[0], O.flip_rows(C.welded_cube()[1], [3])), "oriented")):
        with pytest.raises(ValueError, match=word):
            M.get_volume(*bad)
    # orient_outward: the cube wound inwards, and a Moebius strip beside a torus
    v, t = cases["inward"]
    out, flipped, solid = M.orient_outward(v, t)
    want = S.orient_outward(v, t)
    assert all(same(g, w) for g, w in zip((out, flipped, solid), want))
    assert host(flipped).all() and host(solid).tolist() == [True] and host(M.component_volumes(v, out)[1]).tolist() == [8.0]
    v, t = strip_torus
    for tt in (t, O.flip_rows(t, [35, 40, 77]), np.concatenate([t[:32], t[32:][:, [0, 2, 1]]])):
        out, flipped, solid = M.orient_outward(torch.from_numpy(v).cuda(), torch.from_numpy(tt).cuda())
        want = S.orient_outward(v, tt)
        assert all(same(g, w) for g, w in zip((out, flipped, solid), want))
        assert host(solid).tolist() == [False, True] and same(out[:32], tt[:32])              # the strip is left alone and reported
        vol = host(M.component_volumes(v, out)[1])
        assert np.isnan(vol[0]) and vol[1] > 0 and same(vol, S.component_volumes(v, host(out))[1])
    out, flipped, solid = M.orient_outward(v[:0], t[:0])
    assert out.shape == (0, 3) and flipped.shape == (0,) and solid.shape == (0,)


# ---- is_watertight / check_solid -------------------------------------------------------------------------------------------------------------
def test_watertight_and_check_solid(M):
    cases = dict(icosphere=(MS.icosphere(2), True), torus=(O.torus(), True), open_cube=(C.open_cube(), False), bow_tie=(C.bow_tie(), False),
                 interpenetrating=(C.interpenetrating_cubes(), False), inward=(C.welded_cube(inward=True), True),
                 flipped=((C.welded_cube()[0], O.flip_rows(C.welded_cube()[1], [3])), True), shared_edge=(C.cubes_sharing_an_edge(), False))
    for name, ((v, t), ok) in cases.items():
        want = S.check_solid(v, t)
        assert want["watertight"] is ok, name
        for kind in ("numpy", "device"):
            a = (v, t) if kind == "numpy" else (torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda())
            assert M.is_watertight(*a) is ok, (name, kind)
            r = M.check_solid(*a)
            got = dict(edge_manifold=r.is_edge_manifold, vertex_manifold=r.is_vertex_manifold, self_intersecting=r.is_self_intersecting,
                       consistently_oriented=r.is_consistently_oriented, n_boundary_edges=r.n_boundary_edges, n_non_manifold_edges=r.n_non_manifold_edges,
                       n_non_manifold_vertices=r.n_non_manifold_vertices, n_intersecting_pairs=r.n_intersecting_pairs, watertight=r.is_watertight,
                       volume=r.volume)
            assert got == want, (name, kind, got, want)
    r = M.check_solid(*C.open_cube())
    assert not r.is_edge_manifold and r.n_boundary_edges == 3 and r.is_vertex_manifold and not r.is_self_intersecting and r.volume is None
    r = M.check_solid(*C.bow_tie())
    assert r.is_edge_manifold and not r.is_vertex_manifold and r.n_non_manifold_vertices == 1 and not r.is_self_intersecting
    r = M.check_solid(*C.interpenetrating_cubes())
    assert r.is_edge_manifold and r.is_vertex_manifold and r.is_self_intersecting and r.n_intersecting_pairs == len(ref_pairs("interpenetrating"))
    r = M.check_solid(*cases["flipped"][0])
    assert r.is_watertight and not r.is_consistently_oriented and r.volume is None
    r = M.check_solid(C.welded_cube()[0], C.welded_cube()[1][:0])
    assert r.is_watertight and r.volume == 0.0


# ---- the TriangleMesh methods ------------------------------------------------------------------------------------------------------------------
def test_methods_return_the_kind_of_the_mesh(M):
    from bodyslam_amd.tsdf import TriangleMesh
    v, t = C.interpenetrating_cubes()
    col = np.zeros_like(v)
    other = C.welded_cube((1, 0, 1))
    for kind, conv, typ in (("numpy", lambda x: x, np.ndarray), ("device", lambda x: torch.from_numpy(x).cuda(), torch.Tensor)):
        m = TriangleMesh(conv(v), conv(col), conv(t))
        o = TriangleMesh(conv(other[0]), conv(np.zeros_like(other[0])), conv(other[1]))
        results = dict(nmv=m.get_non_manifold_vertices(), pairs=m.get_self_intersecting_triangles(), pairs_grid=m.get_self_intersecting_triangles("grid", 8),
                       two=m.get_intersecting_triangles(o), clusters=m.component_volumes()[0], volumes=m.component_volumes()[1])
        m2, flipped, solid = m.orient_outward()
        results.update(flipped=flipped, solid=solid, triangles=m2.triangles)
        for k, x in results.items():
            assert isinstance(x, typ) and (typ is np.ndarray or x.is_cuda), (kind, k, type(x))
        assert same(results["pairs"], ref_pairs("interpenetrating")) and same(results["pairs_grid"], ref_pairs("interpenetrating"))
        assert same(results["two"], S.intersecting_pairs(v, t, *other)) and same(results["volumes"], np.array([8.0, 8.0]))
        assert m.is_vertex_manifold() is True and m.is_self_intersecting() is True and m.is_intersecting(o) is True and m.is_watertight() is False
        assert isinstance(m2, TriangleMesh) and m2.vertices is m.vertices and not host(flipped).any()
        assert m.check_solid() == M.check_solid(v, t) and m.check_solid().n_intersecting_pairs == len(ref_pairs("interpenetrating"))
        with pytest.raises(ValueError, match="intersects"):
            m.get_volume()
        assert o.get_volume() == 8.0 and o.is_watertight() is True
