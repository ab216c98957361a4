"""CPU checks of the statement tests/_mesh_solid_ref.py against independent exact oracles: on integer-lattice inputs every product of the
stated arithmetic is exact in fp64, so the statement's triangle / triangle predicate must be exactly right -- compared with Python-integer
segment / triangle tests on a few thousand random pairs from {0..3}^3 (full of touching, coplanar and collinear configurations) and on
the constructed meshes --; the vertex-fan statement against a plain search per vertex; volumes against exact rationals."""
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mesh_ops_ref as R  # noqa: E402
import _mesh_scene_ref as MS  # noqa: E402
import _mesh_solid_ref as S  # noqa: E402
import _orient_ref as O  # noqa: E402

f32, i32 = np.float32, np.int32


# ---- the meshes of the CPU and the GPU tests -----------------------------------------------------------------------------------------------
def welded_cube(lo=(0, 0, 0), side=2, inward=False):
    """8 vertices, 12 triangles wound outwards (inward: the other way); integer coordinates"""
    v = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], f32) * f32(side) + np.array(lo, f32)
    t = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]], i32)
    return v, (t[:, [0, 2, 1]] if inward else t).copy()


def tetrahedron(p=((0, 0, 0), (3, 0, 0), (0, 2, 0), (1, 1, 5))):
    return np.array(p, f32), np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], i32)


def bow_tie():
    """two tetrahedra that share vertex row 0 and nothing else"""
    va, ta = tetrahedron(((0, 0, 0), (1, 0, 1), (0, 1, 1), (1, 1, 3)))
    vb, tb = tetrahedron(((0, 0, 0), (-1, 0, -1), (0, -1, -1), (-1, -1, -3)))
    tb = np.where(tb == 0, 0, tb + 3)
    return np.concatenate([va, vb[1:]]), np.concatenate([ta, tb]).astype(i32)


def open_fan():
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [-1, 1, 0]], f32)
    return v, np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4]], i32)


def cubes_sharing_an_edge():
    """two welded cubes that share the two vertex rows of one edge: that edge has four triangles"""
    va, ta = welded_cube()
    vb, tb = welded_cube((2, 2, 0))
    # B's vertices 0 (2, 2, 0) and 4 (2, 2, 2) are A's 3 and 7
    remap = {0: 3, 4: 7}
    rows = [k for k in range(8) if k not in remap]
    new = {k: 8 + n for n, k in enumerate(rows)}
    tb = np.vectorize(lambda k: remap.get(k, new.get(k)))(tb)
    return np.concatenate([va, vb[rows]]), np.concatenate([ta, tb]).astype(i32)


def open_cube():
    v, t = welded_cube()
    return v, t[1:].copy()


def interpenetrating_cubes():
    return O.merged(welded_cube(), welded_cube((1, 1, 1)))


def corner_touching_cubes():
    return O.merged(welded_cube(), welded_cube((2, 2, 2)))


def nested_cubes():
    return O.merged(welded_cube((0, 0, 0), 8), welded_cube((3, 3, 3), 2))


def coplanar_pair():
    v = np.array([[0, 0, 1], [4, 0, 1], [0, 4, 1], [1, 1, 1], [5, 1, 1], [1, 5, 1]], f32)
    return v, np.array([[0, 1, 2], [3, 4, 5]], i32)


def piercing_pair():
    """the second triangle's vertex 3 lies in the interior of the first: one point in common"""
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [1, 1, 0], [1, 1, 3], [2, 1, 3]], f32)
    return v, np.array([[0, 1, 2], [3, 4, 5]], i32)


def promise_mesh():
    """a welded cube with rows that take no part: an index out of range, a repeated index, a degenerate triangle, a NaN vertex"""
    v, t = welded_cube()
    v = np.concatenate([v, np.array([[1, 1, 1], [1, 1, 1], [np.nan, 0, 0], [1, 1, -1], [1, 1, 3], [2, 1, 3]], f32)])
    extra = np.array([[0, 1, 99], [2, 2, 3], [8, 9, 0], [10, 1, 2], [-1, 0, 1], [11, 12, 13]], i32)
    return v, np.concatenate([extra[:3], t, extra[3:]]).astype(i32)


def soup(n=300, seed=11, big=False):
    """n small random fp32 triangles in the unit box; big: plus one that spans the whole box"""
    rng = np.random.default_rng(seed)
    c = rng.random((n, 1, 3))
    v = (c + (rng.random((n, 3, 3)) - 0.5) * 0.16).reshape(-1, 3)
    t = np.arange(3 * n).reshape(n, 3)
    if big:
        v = np.concatenate([v, [[-0.1, -0.1, -0.1], [1.1, 1.1, 0.4], [0.2, 1.1, 1.1]]])
        t = np.concatenate([t, [[3 * n, 3 * n + 1, 3 * n + 2]]])
    return v.astype(f32), t.astype(i32)


LATTICE = dict(welded_cube=welded_cube, interpenetrating=interpenetrating_cubes, corner_touching=corner_touching_cubes, seams=MS.cube,
               coplanar=coplanar_pair, piercing=piercing_pair, nested=nested_cubes)
LATTICE_PAIRS = dict(welded_cube=0, corner_touching=None, coplanar=1, piercing=1, nested=0)


def lattice_mesh(name):
    v, t = LATTICE[name]()
    if name == "seams":
        v = (v * f32(2)).astype(f32)               # pitch 0.5 -> integers
    return v, t


def same_pairs(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


# ---- the predicate -------------------------------------------------------------------------------------------------------------------------
def _nondegenerate(A):
    return any(S._crs(S._sub(A[1], A[0]), S._sub(A[2], A[0])))


def _check_pair(rng, A, B):
    ids = rng.permutation(6)                         # the canonical order must not matter
    T1 = [(int(ids[k]), *map(float, A[k])) for k in range(3)]
    T2 = [(int(ids[3 + k]), *map(float, B[k])) for k in range(3)]
    want = S.exact_tri_tri(A, B)
    assert S.tri_tri(T1, T2) == want, (A, B, ids, want)
    assert S.tri_tri(T2, T1) == want, (A, B, ids, want, "swapped")
    return want


def test_random_lattice_pairs_equal_the_exact_oracle():
    rng = np.random.default_rng(5)
    n = met = 0
    while n < 4000:
        P = rng.integers(0, 4, size=(6, 3))
        A, B = [tuple(int(c) for c in p) for p in P[:3]], [tuple(int(c) for c in p) for p in P[3:]]
        if not _nondegenerate(A) or not _nondegenerate(B):
            continue                                 # a degenerate triangle is not KEPT: it takes no part
        met += _check_pair(rng, A, B)
        n += 1
    assert 500 < met < 3500, met


def test_random_coplanar_lattice_pairs_equal_the_exact_oracle():
    """both triangles in one lattice plane o + a u + b w, a, b in 0 .. 3: every pair takes the two-dimensional test"""
    rng = np.random.default_rng(6)
    n = met = 0
    while n < 2000:
        o, u, w = rng.integers(-2, 3, size=(3, 3))
        if not any(S._crs(tuple(u), tuple(w))):
            continue
        P = [tuple(int(c) for c in o + a * u + b * w) for a, b in rng.integers(0, 4, size=(6, 2))]
        A, B = P[:3], P[3:]
        if not _nondegenerate(A) or not _nondegenerate(B):
            continue
        met += _check_pair(rng, A, B)
        n += 1
    assert 300 < met < 1900, met


def test_constructed_lattice_meshes_equal_the_exact_oracle():
    for name in LATTICE:
        v, t = lattice_mesh(name)
        got, want = S.intersecting_pairs(v, t), S.intersecting_pairs(v, t, predicate=S.exact_predicate)
        assert same_pairs(got, want), name
        if LATTICE_PAIRS.get(name) is not None:
            assert len(got) == LATTICE_PAIRS[name], (name, len(got))
    assert len(S.intersecting_pairs(*lattice_mesh("interpenetrating"))) > 0 and len(S.intersecting_pairs(*lattice_mesh("seams"))) > 0
    touching = S.intersecting_pairs(*lattice_mesh("corner_touching"))
    assert len(touching) > 0 and (touching[:, 0] < 12).all() and (touching[:, 1] >= 12).all()
    (va, ta), (vb, tb) = welded_cube(), welded_cube((1, 1, 1))
    two = S.intersecting_pairs(va, ta, vb, tb)
    assert same_pairs(two, S.intersecting_pairs(va, ta, vb, tb, predicate=S.exact_predicate)) and len(two) > 0
    one = S.intersecting_pairs(*interpenetrating_cubes())
    assert same_pairs(two + np.array([0, 12], i32), one)          # neither cube meets itself: the same pairs, B's rows shifted


def test_rows_that_take_no_part():
    v, t = promise_mesh()
    pairs = S.intersecting_pairs(v, t)
    assert same_pairs(pairs, S.intersecting_pairs(v, t, predicate=S.exact_predicate))
    assert len(pairs) > 0 and (pairs[:, 1] == len(t) - 1).all()    # only the last row, which pierces the cube's bottom and top


# ---- vertex fans ---------------------------------------------------------------------------------------------------------------------------
def test_vertex_fans_equal_a_plain_search():
    v, t, _ = O.long_strip(200)
    cases = dict(bow_tie=bow_tie(), open_fan=open_fan(), shared_edge=cubes_sharing_an_edge(), promise=promise_mesh(), strip=(v, t),
                 book=O.book(), icosphere=MS.icosphere(1), corner=corner_touching_cubes())
    for name, (v, t) in cases.items():
        got = S.non_manifold_vertices(v, t)
        assert got.dtype == i32 and np.array_equal(got, S.non_manifold_vertices_bfs(v, t)), name
    assert S.non_manifold_vertices(*bow_tie()).tolist() == [0]
    assert all(len(S.non_manifold_vertices(*cases[k])) == 0 for k in ("open_fan", "shared_edge", "strip", "icosphere"))
    assert S.non_manifold_vertices(*promise_mesh()).tolist() == [0]      # the valid, degenerate row [8, 9, 0] is a second fan at vertex 0
    # two fans that share only vertex 0, and an unreferenced vertex
    v = np.zeros((8, 3), f32)
    assert S.non_manifold_vertices(v, np.array([[0, 1, 2], [0, 2, 3], [0, 4, 5]], i32)).tolist() == [0]


# ---- volumes -------------------------------------------------------------------------------------------------------------------------------
def exact_volume(v, t):
    total = Fraction(0)
    for a, b, c in t:
        A, B, C = ([Fraction(float(x)) for x in v[k]] for k in (a, b, c))
        total += S._dt(A, S._crs(B, C))
    return total / 6


def test_volumes_equal_exact_rationals():
    cl, vol = S.component_volumes(*welded_cube())
    assert vol.tolist() == [8.0] and (cl == 0).all()
    assert S.component_volumes(*welded_cube(inward=True))[1].tolist() == [-8.0]
    v, t = tetrahedron()
    det = int(round(np.linalg.det(v[1:].astype(np.float64) - v[0])))
    assert det == 30 and S.component_volumes(v, t)[1].tolist() == [det * (1.0 / 6.0)] and exact_volume(v, t) == Fraction(det, 6)
    v, t = O.merged(welded_cube((5, 5, 5), 3), tetrahedron(), welded_cube(inward=True))
    assert S.component_volumes(v, t)[1].tolist() == [27.0, 5.0, -8.0]
    assert np.isnan(S.component_volumes(*open_cube())[1]).all()
    v, t = O.torus()
    vol = S.component_volumes(v, t)[1]
    assert abs(vol[0] - float(exact_volume(v, t))) < 1e-15 and vol[0] > 0
    out, flipped, solid = S.orient_outward(*welded_cube(inward=True))
    assert flipped.all() and solid.all() and S.component_volumes(welded_cube()[0], out)[1].tolist() == [8.0]
    v, t = O.merged(O.moebius_strip(), O.torus())
    out, flipped, solid = S.orient_outward(v, t)
    assert solid.tolist() == [False, True] and not flipped[:32].any() and np.array_equal(out[:32], t[:32])
    assert S.component_volumes(v, out)[1][1] > 0 and np.isnan(S.component_volumes(v, out)[1][0])


def test_check_solid():
    for mesh, ok in ((MS.icosphere(2), True), (O.torus(), True), (open_cube(), False), (bow_tie(), False), (interpenetrating_cubes(), False)):
        d = S.check_solid(*mesh)
        assert d["watertight"] == ok and (d["volume"] is not None) == ok
    assert S.check_solid(*open_cube())["n_boundary_edges"] == 3 and not S.check_solid(*open_cube())["edge_manifold"]
    d = S.check_solid(*bow_tie())
    assert d["edge_manifold"] and not d["vertex_manifold"] and d["n_non_manifold_vertices"] == 1 and not d["self_intersecting"]
    d = S.check_solid(*interpenetrating_cubes())
    assert d["edge_manifold"] and d["vertex_manifold"] and d["self_intersecting"] and d["n_intersecting_pairs"] > 0
