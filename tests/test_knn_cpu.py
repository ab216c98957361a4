"""CPU checks of the k nearest neighbours, the normal estimation and the statistical outlier removal: the statement (tests/_knn_ref.py)
against closed forms, the conditions the GPU tests rely on (ties on the lattice, the eigenvalue gap on the bumpy target, the margin of the
planted outliers), the public signatures, argument validation before any device call, and no CPU fallback."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _icp_ref as I  # noqa: E402
import _knn_ref as K  # noqa: E402
import _pointcloud_ref as P  # noqa: E402

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import bodyslam_amd.pointcloud as PC
    import bodyslam_amd.tsdf as TS
    return PC, TS


@pytest.fixture(scope="module")
def bumpy():
    return I.bumpy_target()


# ---- the statement against closed forms ------------------------------------------------------------------------------------------------
def test_lattice_stencil_in_index_order():
    lat = K.tie_lattice()
    assert lat.shape == (189, 3) and lat.dtype == f32

    def at(x, y, z):
        return (z * 7 + y) * 9 + x
    c = at(4, 3, 1)                                                                # an interior point
    idx, d2, cnt = K.knn_brute(lat[c:c + 1], lat, 27)
    assert cnt[0] == 27 and idx[0, 0] == c and d2[0, 0] == 0.0
    axis = sorted(at(4 + a, 3 + b, 1 + d) for a, b, d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)))
    assert list(idx[0, 1:7]) == axis and np.all(d2[0, 1:7] == f32(2.0 ** -16))    # six at distance 1, ascending by index
    edge = sorted(at(4 + a, 3 + b, 1 + d) for a in (-1, 0, 1) for b in (-1, 0, 1) for d in (-1, 0, 1) if abs(a) + abs(b) + abs(d) == 2)
    assert list(idx[0, 7:19]) == edge and np.all(d2[0, 7:19] == f32(2.0 ** -15))
    corner = sorted(at(4 + a, 3 + b, 1 + d) for a in (-1, 1) for b in (-1, 1) for d in (-1, 1))
    assert list(idx[0, 19:27]) == corner and np.all(d2[0, 19:27] == f32(3 * 2.0 ** -16))
    # k = 8 cuts through the ties at distance sqrt(2): the 8th entry is the lowest index among the twelve
    i8, _, _ = K.knn_brute(lat[c:c + 1], lat, 8)
    assert list(i8[0]) == [c] + axis + [edge[0]]
    # hybrid search with the radius exactly the spacing: itself and the six axis neighbours, the ones AT the radius included
    ih, dh, ch = K.knn_brute(lat[c:c + 1], lat, 27, radius=2.0 ** -8)
    assert ch[0] == 7 and list(ih[0, :7]) == [c] + axis and np.all(ih[0, 7:] == -1) and np.all(np.isinf(dh[0, 7:]))


def test_lattice_has_ties_at_the_cut():
    """what makes the lattice a test of the strict stop and of the tie-break: for k = 8 nearly every row's 8th and 9th d2 are equal"""
    lat = K.tie_lattice()
    _, d2, _ = K.knn_brute(lat, lat, 9)
    frac = float((d2[:, 7] == d2[:, 8]).mean())
    print("rows whose 8th and 9th d2 are equal", frac)
    assert frac >= 0.9


def test_knn_edges_of_the_domain():
    rng = np.random.default_rng(3)
    t = rng.uniform(-1, 1, (40, 3)).astype(f32)
    t[7] = np.nan
    t[20, 1] = np.inf
    s = rng.uniform(-1, 1, (9, 3)).astype(f32)
    s[4, 2] = np.nan
    idx, d2, cnt = K.knn_brute(s, t, 5)
    assert cnt[4] == 0 and np.all(idx[4] == -1) and np.all(np.isnan(d2[4]))
    assert not np.isin(idx, (7, 20)).any() and np.all(np.delete(cnt, 4) == 5)
    assert np.all(np.diff(np.delete(d2, 4, 0), axis=1) >= 0)
    i1, d21, _ = P.nn_brute(s, t)
    i1k, d2k, _ = K.knn_brute(s, t, 1)
    assert np.array_equal(i1, i1k[:, 0]) and np.array_equal(d21.view(np.uint32), d2k[:, 0].view(np.uint32))     # k = 1 is the query
    idx, d2, cnt = K.knn_brute(s, t[:5], 8)                                                                       # more than there are
    assert np.all(np.delete(cnt, 4) == 5) and np.all(np.delete(idx, 4, 0)[:, 5:] == -1) and np.all(np.isinf(np.delete(d2, 4, 0)[:, 5:]))
    for k in (0, 33, -1):
        with pytest.raises(ValueError):
            K.knn_brute(s, t, k)


def test_radius_cutoff_is_the_same_predicate():
    rng = np.random.default_rng(4)
    for r in list(rng.uniform(1e-4, 2.0, 40).astype(f32)) + [f32(2.0 ** -8), f32(0.005), f32(0.008), f32(1e-20), f32(1e19)]:
        c = K.d2_cutoff(r)
        assert np.sqrt(c) <= r and (not np.isfinite(np.nextafter(c, f32(np.inf))) or np.sqrt(np.nextafter(c, f32(np.inf))) > r), (r, c)
    assert K.d2_cutoff(np.inf) == np.inf


def test_planar_cloud():
    x, y = np.meshgrid(np.arange(12) * 0.01, np.arange(9) * 0.01, indexing="ij")
    p = np.stack([x.ravel(), y.ravel(), np.zeros(x.size)], 1).astype(f32)
    n, ev = K.estimate_normals(p, k=9)
    assert np.abs(n - np.array([0, 0, 1], f32)).max() <= 1e-7 and np.all(ev[:, 0] == 0.0) and np.all(ev[:, 1] > 0)
    n2, _ = K.estimate_normals(p, k=9, direction=(0, 0, -1))
    assert np.abs(n2 - np.array([0, 0, -1], f32)).max() <= 1e-7
    n3, _ = K.estimate_normals(p, k=9, camera_location=(0.05, 0.04, -1.0))
    assert np.abs(n3 - np.array([0, 0, -1], f32)).max() <= 1e-7
    with pytest.raises(ValueError):
        K.estimate_normals(p, k=9, direction=(0, 0, 1), camera_location=(0, 0, 1))


def test_sphere_normals_are_radial():
    """points on a sphere of radius R: the fitted plane through neighbours within a cap of angular radius a deviates from the tangent
    plane by less than a (the discretisation angle)"""
    Rr, n_pts, k = 0.05, 4000, 12
    i = np.arange(n_pts) + 0.5
    phi, th = np.arccos(1 - 2 * i / n_pts), np.pi * (1 + 5 ** 0.5) * i            # the Fibonacci sphere: near-uniform
    p = (Rr * np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1)).astype(f32)
    idx, d2, cnt = K.knn_brute(p, p, k)
    n, _ = K.normals_from_knn(p, idx, cnt, camera_location=(0.0, 0.0, 0.0))
    radial = p.astype(f64) / np.linalg.norm(p.astype(f64), axis=1, keepdims=True)
    cosang = -(n.astype(f64) * radial).sum(1)                                      # oriented towards the centre
    cap = 2 * np.arcsin(np.sqrt(d2[:, -1].astype(f64)).max() / (2 * Rr))           # the angle the farthest neighbour subtends
    ang = np.arccos(np.clip(cosang, -1, 1))
    print("largest angle to the radial direction", ang.max(), "cap", cap)
    assert ang.max() < cap and np.abs(np.linalg.norm(n.astype(f64), axis=1) - 1).max() < 1e-6


def test_degenerate_neighbourhoods():
    same = np.full((10, 3), 0.25, f32)
    n, ev = K.estimate_normals(same, k=5)
    assert np.all(n == 0.0) and np.all(ev == 0.0)                                  # all points identical: no positive eigenvalue
    two = np.array([[0, 0, 0], [1, 2, 3]], f32)
    n, _ = K.estimate_normals(two, k=8)
    assert np.all(n == 0.0)                                                        # count < 3
    rng = np.random.default_rng(5)
    p = rng.uniform(-1, 1, (30, 3)).astype(f32)
    n, _ = K.estimate_normals(p, k=10, radius=1e-3)                                # every point alone within the radius
    assert np.all(n == 0.0)
    line = np.stack([np.arange(8) * 0.5, np.zeros(8), np.zeros(8)], 1).astype(f32)
    n, _ = K.estimate_normals(line, k=4)                                           # exactly collinear: unspecified, finite, unit or zero
    ln = np.linalg.norm(n.astype(f64), axis=1)
    assert np.isfinite(n).all() and np.all((np.abs(ln - 1) < 1e-6) | (ln == 0))
    p[3] = np.nan
    n, ev = K.estimate_normals(p, k=10)
    assert np.all(n[3] == 0.0) and np.isfinite(n).all()


def test_default_sign_is_deterministic():
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 0]], f32) @ np.array([[1, 0, 0], [0, 0.6, -0.8], [0, 0.8, 0.6]], f32)
    n, _ = K.estimate_normals(p, k=5)
    assert np.all(n[np.arange(5), np.argmax(np.abs(n), 1)] > 0)


@pytest.mark.parametrize("k", [6, 10, 30])
def test_bumpy_gap_condition(bumpy, k):
    """what the GPU test's 5e-7 on every normal component rests on: the relative gap (l1 - l0) / l2 is large on every row, so an fp64
    perturbation of the covariance of 1e-15 l2 moves the eigenvector by < 1e-14; and no normal's sign is marginal for direction = +z"""
    tgt, nrm = bumpy
    n, ev = K.estimate_normals(tgt, k=k, direction=(0, 0, 1))
    gap = (ev[:, 1] - ev[:, 0]) / ev[:, 2]
    ang = np.degrees(np.arccos(np.clip((n.astype(f64) * nrm.astype(f64)).sum(1), -1, 1)))
    print("k", k, "smallest relative gap", gap.min(), "smallest |n_z|", np.abs(n[:, 2]).min(), "largest angle to the analytic normal (deg)", ang.max())
    assert gap.min() >= 0.1 and np.abs(n[:, 2]).min() >= 0.5 and np.all(n[:, 2] > 0)
    assert np.abs(np.linalg.norm(n.astype(f64), axis=1) - 1).max() < 1e-6


def test_hybrid_counts_on_the_bumpy_target(bumpy):
    tgt, _ = bumpy
    _, _, c8 = K.knn_brute(tgt, tgt, 30, radius=0.008)
    _, _, c5 = K.knn_brute(tgt, tgt, 30, radius=0.005)
    print("radius 0.008: short rows", float((c8 < 30).mean()), "; radius 0.005: counts", c5.min(), "..", c5.max())
    assert 0.02 < (c8 < 30).mean() < 0.5 and c5.max() < 30 and c5.min() >= 3


# ---- outlier removal ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,ratio", [(20, 2.0), (8, 2.0)])
def test_planted_outliers(nb, ratio):
    pts, rows = K.planted_cloud()
    assert pts.shape == (I.N_TARGET, 3) and len(rows) == 12
    kept, mask, avg, thr = K.remove_statistical_outlier(pts, nb, ratio)
    margin = np.abs(avg.astype(f64) - thr).min() / thr
    print("nb_neighbors", nb, "removed", int((~mask).sum()), "threshold", thr, "closest avg relative to the threshold", margin)
    assert not mask[rows].any() and 12 <= (~mask).sum() <= 16                      # every planted point goes, and hardly anything else
    assert np.array_equal(kept, np.nonzero(mask)[0]) and kept.dtype == np.int64 and mask.dtype == bool
    assert margin >= 1e-3                                                          # a last-bit difference in std cannot flip a point
    bad = pts.copy()
    bad[11] = np.nan
    _, m2, a2, _ = K.remove_statistical_outlier(bad, nb, ratio)
    assert np.isnan(a2[11]) and not m2[11]
    # the rule itself, in closed form
    a = np.array([1, 1, 1, 1, 5], f32)
    mean, std, t = K.outlier_threshold(a, 1.0)
    assert mean == 1.8 and abs(std - np.std(a.astype(f64), ddof=1)) < 1e-15 and t == mean + std
    assert K.outlier_threshold(np.array([2.0], f32), 2.0) == (2.0, 0.0, 2.0)


# ---- the public interface --------------------------------------------------------------------------------------------------------------
def test_public_signatures(built):
    PC, TS = built

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert params(PC.NearestNeighbours.query_knn) == [("self", E), ("source", E), ("k", E), ("radius", None)]
    assert params(PC.estimate_normals) == [("points", E), ("k", 30), ("radius", None), ("direction", None), ("camera_location", None),
                                           ("cell_size", None), ("device", 0), ("return_eigenvalues", False)]
    assert params(TS.PointCloud.estimate_normals) == [("self", E), ("k", 30), ("radius", None), ("direction", None), ("camera_location", None)]
    assert params(PC.remove_statistical_outlier) == [("points", E), ("nb_neighbors", 20), ("std_ratio", 2.0), ("cell_size", None), ("device", 0)]
    assert params(TS.PointCloud.remove_statistical_outlier) == [("self", E), ("nb_neighbors", E), ("std_ratio", E)]
    # the pinned ones are as they were
    assert params(PC.NearestNeighbours.__init__) == [("self", E), ("target", E), ("cell_size", None), ("device", 0)]
    assert params(PC.NearestNeighbours.query) == [("self", E), ("source", E), ("max_distance", None), ("method", "grid")]
    assert [f.name for f in __import__("dataclasses").fields(TS.PointCloud)] == ["points", "colors", "normals"]
    from bodyslam_amd import _lib
    assert _lib.PC_KNN_MAX == K.KNN_MAX == 32


def test_argument_validation_before_any_device_call(built, bumpy, monkeypatch):
    PC, TS = built
    from bodyslam_amd import _lib
    tgt, _ = bumpy

    def touched(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "init", touched)
    cloud = TS.PointCloud(tgt, np.zeros_like(tgt))
    for k in (0, 33, -1, 2.5, "3", True, None):
        with pytest.raises(ValueError):
            PC.estimate_normals(tgt, k=k)
        with pytest.raises(ValueError):
            cloud.estimate_normals(k=k)
        with pytest.raises(ValueError):
            PC.remove_statistical_outlier(tgt, nb_neighbors=k)
        with pytest.raises(ValueError):
            cloud.remove_statistical_outlier(k, 2.0)
    for r in (0.0, -1.0, np.nan, np.inf, 1e-60, 1e60, "1", True):
        with pytest.raises(ValueError):
            PC.estimate_normals(tgt, radius=r)
        with pytest.raises(ValueError):
            cloud.estimate_normals(radius=r)
    for kw in (dict(direction=(0, 0, 1), camera_location=(0, 0, 0)), dict(direction=(0, np.nan, 1)), dict(camera_location=(np.inf, 0, 0)),
               dict(direction=(0, 1)), dict(camera_location="here"), dict(direction=np.zeros((3, 3)))):
        with pytest.raises(ValueError):
            PC.estimate_normals(tgt, **kw)
        with pytest.raises(ValueError):
            cloud.estimate_normals(**kw)
    for s in (np.nan, np.inf, -np.inf, "2", None, True):
        with pytest.raises(ValueError):
            PC.remove_statistical_outlier(tgt, std_ratio=s)
        with pytest.raises(ValueError):
            cloud.remove_statistical_outlier(20, s)
    for bad in (np.zeros((4, 2), f32), np.zeros((0, 3), f32), tgt.astype(np.int32), None):
        with pytest.raises(ValueError):
            PC.estimate_normals(bad)
        with pytest.raises(ValueError):
            PC.remove_statistical_outlier(bad)
    with pytest.raises(ValueError):
        PC.estimate_normals(tgt, cell_size=0.0)
    with pytest.raises(ValueError):
        PC.remove_statistical_outlier(tgt, cell_size=-1.0)
    # query_knn checks k and radius before it looks at its index (an index cannot exist without a device)
    nn = object.__new__(PC.NearestNeighbours)
    for k, r in ((0, None), (33, None), (True, None), (8, 0.0), (8, np.nan), (8, "r")):
        with pytest.raises(ValueError):
            PC.NearestNeighbours.query_knn(nn, tgt, k, r)
    with pytest.raises(ValueError):
        PC.NearestNeighbours.query_knn(nn, np.zeros((3, 2), f32), 8)


def test_no_cpu_fallback(built, bumpy):
    PC, TS = built
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from bodyslam_amd._lib import BodySlamHipError
    tgt, _ = bumpy
    cloud = TS.PointCloud(tgt, np.zeros_like(tgt))
    with pytest.raises(BodySlamHipError):
        PC.estimate_normals(tgt)
    with pytest.raises(BodySlamHipError):
        cloud.estimate_normals()
    with pytest.raises(BodySlamHipError):
        PC.remove_statistical_outlier(tgt)
    with pytest.raises(BodySlamHipError):
        cloud.remove_statistical_outlier(20, 2.0)
    assert cloud.normals is None
