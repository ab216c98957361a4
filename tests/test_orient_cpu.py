"""CPU tests of the statement tests/_orient_ref.py and of the argument checks of orient_normals_consistent_tangent_plane and
orient_triangles (bodyslam_amd/pointcloud.py, bodyslam_amd/mesh.py): the statement does what DESIGN section 3.24 claims for it, the inputs
of tests/test_orient_gpu.py exercise what they are there for, and bad arguments raise before the device is touched."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_ref as K  # noqa: E402
import _orient_ref as O  # noqa: E402

f32 = np.float32
_CACHE = {}


def tube():
    if "tube" not in _CACHE:
        _CACHE["tube"] = O.tube()
    return _CACHE["tube"]


def estimated():
    """the tube's normals estimated at k = 10 under the largest-component rule"""
    if "est" not in _CACHE:
        _CACHE["est"] = K.estimate_normals(tube()[0], 10)[0]
    return _CACHE["est"]


def test_largest_component_rule_leaves_both_signs():
    pts, nrm = tube()
    assert pts.shape == (2806, 3) and pts.dtype == f32
    for normals in (O.axis_rule(nrm), estimated()):
        out = O.tube_outward(pts, normals)
        assert (out > 0).sum() >= 1000 and (out < 0).sum() >= 1000, ((out > 0).sum(), (out < 0).sum())


@pytest.mark.parametrize("k", [6, 10, 16])
def test_statement_orients_the_tube_from_random_signs(k):
    pts, nrm = tube()
    start = O.random_signs(nrm, 5)
    out, flipped, comps = O.orient_normals(pts, start, k)
    assert comps == 1
    assert (O.tube_outward(pts, out) > 0).all()
    assert np.array_equal(out.view(np.uint32), nrm.view(np.uint32))                            # the analytic normals, bit for bit
    assert np.array_equal(flipped, (start.view(np.uint32) != nrm.view(np.uint32)).any(1))


def test_statement_orients_estimated_normals():
    pts, nrm = tube()
    out, flipped, comps = O.orient_normals(pts, estimated(), 10)
    assert comps == 1 and (O.tube_outward(pts, out) > 0).all() and 1000 <= flipped.sum() <= 1806
    assert np.abs(O.dot64(out, nrm)).min() >= 0.994
    assert np.array_equal(np.abs(out), np.abs(estimated()))                                     # only signs change


def test_forest_weight_equals_scipy():
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import minimum_spanning_tree
    rng = np.random.default_rng(53)                                                             # 300 points in a cube, normals at random
    pts = rng.uniform(0.0, 1.0, (300, 3)).astype(f32)
    nrm = rng.normal(size=(300, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(f32)
    lo, hi, w, _ = O.knn_edges(pts, nrm, 8)
    assert len(np.unique(w)) == len(w) and (w > 0).all()                                         # no weight ties, and no zero scipy would drop
    assert O.orient_normals(pts, nrm, 8)[2] == 1                                                 # one tree
    tree = O.spanning_forest(len(pts), lo, hi, w)
    assert len(tree) == len(pts) - 1
    ref = minimum_spanning_tree(sp.coo_matrix((w.astype(np.float64), (lo, hi)), shape=(len(pts),) * 2).tocsr())
    assert ref.nnz == len(tree)
    assert float(w[tree].astype(np.float64).sum()) == pytest.approx(float(ref.sum()), rel=1e-12)
    got = set(zip(lo[tree].tolist(), hi[tree].tolist()))
    r = ref.tocoo()
    assert got == set(zip(np.minimum(r.row, r.col).tolist(), np.maximum(r.row, r.col).tolist()))  # without ties the tree itself is unique


def test_plane_lattice_is_decided_by_the_indices():
    pts, nrm = O.plane_lattice()
    out, flipped, comps, (lo, hi, w, s, tree, seeds) = O.orient_normals(pts, nrm, 5, details=True)
    assert len(lo) == 141 and (w == 0).all() and comps == 1 and len(tree) == 62 and seeds.tolist() == [0]
    assert (out[:, 2] == 1).all() and np.array_equal(flipped, nrm[:, 2] < 0) and 20 <= flipped.sum() <= 43
    order = np.lexsort((hi, lo))                                                                # Kruskal took the edges in index order
    by_index = order[O.spanning_forest(63, lo[order], hi[order], np.arange(len(lo)).astype(f32))]
    assert set(tree.tolist()) == set(by_index.tolist())


def test_moebius_cloud_is_inconsistent():
    """some cycle of the graph has odd sign parity: the answer depends on the tree, so the tree has to be the statement's"""
    pts, nrm = O.moebius_cloud()
    out, flipped, comps, (lo, hi, w, s, tree, _) = O.orient_normals(pts, nrm, 10, details=True)
    assert comps == 1 and len(pts) == 1500
    violated = (flipped[lo] ^ flipped[hi]) != s
    assert violated.any() and not violated[tree].any()


def test_bad_rows_and_components():
    pts, nrm, rows = O.bad_rows_tube()
    out, flipped, comps = O.orient_normals(pts, nrm, 10)
    assert np.array_equal(out[rows].view(np.uint32), nrm[rows].view(np.uint32)) and not flipped[rows].any()
    keep = np.setdiff1d(np.arange(len(pts)), rows)
    assert comps == 1 and (O.tube_outward(pts[keep], out[keep]) > 0).all()
    lo, hi, _, _ = O.knn_edges(pts, nrm, 10)
    assert not np.isin(lo, rows).any() and not np.isin(hi, rows).any()                             # never traversed
    two = np.concatenate([O.tube()[0], O.tube((0.0, 1.0, 0.0))[0]])
    nn = O.random_signs(np.concatenate([O.tube()[1]] * 2), 7)
    out, _, comps = O.orient_normals(two, nn, 10)
    assert comps == 2
    assert (O.tube_outward(two[:2806], out[:2806]) > 0).all() and (O.tube_outward(two[2806:], out[2806:], (0.0, 1.0, 0.0)) > 0).all()


def test_winding_statement():
    v, t = O.torus()
    assert len(t) == 384 and O.consistently_oriented(len(v), t)
    rows = np.nonzero(np.random.default_rng(1).random(len(t)) < 1 / 3)[0]
    rows = rows[rows != 0]
    out, flipped, ok, comp, verdict = O.orient_triangles(v, O.flip_rows(t, rows))
    assert ok and np.array_equal(out, t) and np.array_equal(np.nonzero(flipped)[0], rows) and (comp == 0).all() and verdict.tolist() == [True]
    v, t = O.moebius_strip()
    out, flipped, ok, comp, verdict = O.orient_triangles(v, t)
    assert len(t) == 32 and not ok and np.array_equal(out, t) and not flipped.any() and verdict.tolist() == [False]
    v, t, good = O.long_strip()
    out, flipped, ok, _, _ = O.orient_triangles(v, t)
    assert ok and flipped.sum() in (499, 500, 501) and O.consistently_oriented(len(v), out) and not O.consistently_oriented(len(v), t)
    v, t = O.book()
    out, flipped, ok, comp, verdict = O.orient_triangles(v, t)
    assert ok and comp.tolist() == [0, 0, 1, 1, 2, 2] and not flipped[[0, 2, 4]].any()            # no link across the spine


# ---- argument checks: ValueError before any GPU call ---------------------------------------------------------------------------------------
def test_orient_normals_argument_errors():
    import bodyslam_amd.pointcloud as PC
    pts, nrm = tube()
    p, n = pts[:50], nrm[:50]
    for k in (1, 33, 0, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            PC.orient_normals_consistent_tangent_plane(p, n, k)
    for bad in (n[:49], n.astype(np.int32), n[:, :2], None, "n"):
        with pytest.raises(ValueError):
            PC.orient_normals_consistent_tangent_plane(p, bad, 10)
    for bad in (None, (0, 0), (0, 0, np.nan), "up", (1, 2, 3, 4)):
        with pytest.raises(ValueError):
            PC.orient_normals_consistent_tangent_plane(p, n, 10, direction=bad)
    for bad in (0.0, -1.0, np.inf, "h"):
        with pytest.raises(ValueError):
            PC.orient_normals_consistent_tangent_plane(p, n, 10, cell_size=bad)
    with pytest.raises(ValueError):
        PC.orient_normals_consistent_tangent_plane(p[:, :2], n, 10)
    with pytest.raises(ValueError):
        PC.orient_normals_consistent_tangent_plane(np.zeros((0, 3), f32), np.zeros((0, 3), f32), 10)
    assert PC._check_items(2 ** 30, "points") == 2 ** 30
    with pytest.raises(ValueError):
        PC._check_items(2 ** 30 + 1, "points")


def test_orient_triangles_argument_errors():
    import bodyslam_amd.mesh as M
    from bodyslam_amd.tsdf import PointCloud
    v, t = O.torus()
    for fn in (M.orient_triangles, M.is_orientable, M.orientable_components):
        for slots in (0, 3, 1000, 2.0, True):
            with pytest.raises(ValueError):
                fn(v, t, slots=slots)
        with pytest.raises(ValueError):
            fn(v, t.astype(np.float32))
        with pytest.raises(ValueError):
            fn(v[:, :2], t)
    with pytest.raises(ValueError):
        PointCloud(tube()[0], None, None).orient_normals_consistent_tangent_plane(10)             # no normals to orient
