"""Cloud-to-cloud distances without a GPU: the numpy statement against itself (the grid algorithm equals brute force bit for bit), the
statement's metrics on clouds whose answer is known in closed form, argument validation, the public signatures, and no CPU fallback."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pointcloud_ref as P  # noqa: E402

f32 = np.float32


def bits(a):
    return np.asarray(a, dtype=f32).view(np.uint32)


def same(a, b):
    """(index, d2, distance) triples are equal bit for bit"""
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(bits(a[2]), bits(b[2]))


@pytest.fixture(scope="module")
def base():
    tgt, src = P.base_target(), P.base_source()
    lo, hi = P.bounds(tgt)
    return tgt, src, P.nn_brute(src, tgt), P.default_cell_size(lo, hi, len(tgt))


def test_base_clouds(base):
    tgt, src, ref, h0 = base
    assert tgt.shape == (2806, 3) and src.shape == (1937, 3) and tgt.dtype == f32 and src.dtype == f32
    assert len(tgt) % 64 and len(tgt) % 256 and len(src) % 64 and len(src) % 256
    assert ref[0].min() >= 0 and ref[0].max() < len(tgt) and np.isfinite(ref[2]).all() and ref[2].max() < 0.003


@pytest.mark.parametrize("factor", [1.0, 0.25, 4.0])
def test_grid_equals_brute(base, factor):
    tgt, src, ref, h0 = base
    st = {}
    got = P.nn_grid(src, tgt, h0 * factor, shell_cap=8, stats_out=st)
    print("cell size", h0 * factor, "fallback", st["fallback"], "last shell histogram", np.bincount(st["shells"]))
    assert same(got, ref)
    assert st["fallback"] == 0


def test_grid_ties_far_sources_and_radius(base):
    tgt, src, ref, h0 = base
    tied = np.concatenate([tgt, tgt[:100]])
    rt = P.nn_brute(src, tied)
    assert same(rt, ref) and rt[0].max() < len(tgt)                # an exact tie goes to the lower index
    assert same(P.nn_grid(src, tied, h0), rt)
    far = (src + f32(0.5)).astype(f32)
    st = {}
    assert same(P.nn_grid(far, tgt, h0, shell_cap=8, stats_out=st), P.nn_brute(far, tgt))
    assert st["fallback"] == len(far)                              # 0.5 m is a hundred cells: every source passes the cap
    mixed = np.concatenate([far[:64], src[:64]])
    st = {}
    assert same(P.nn_grid(mixed, tgt, h0, shell_cap=8, stats_out=st), P.nn_brute(mixed, tgt))
    assert st["fallback"] == 64
    radius = 0.001
    assert np.abs(ref[2].astype(np.float64) - radius).min() > 1e-9
    rr = P.nn_brute(src, tgt, radius)
    miss = rr[0] < 0
    assert 0.2 < miss.mean() < 0.5 and np.isinf(rr[2][miss]).all() and np.array_equal(miss, ref[2] > f32(radius))
    assert same(P.nn_grid(src, tgt, h0, max_distance=radius), rr)
    assert same(P.nn_grid(src, tgt, h0 * 0.25, max_distance=radius), rr)


def test_grid_degenerate_shapes(base):
    tgt, src, ref, h0 = base
    one = tgt[:1]
    flat = tgt.copy()
    flat[:, 2] = f32(0.31)
    equal = np.repeat(tgt[:1], 50, 0)
    dirty_t = tgt[:300].copy()
    dirty_t[[3, 77], 1] = np.nan
    dirty_t[150, 0] = np.inf
    dirty_s = src[:200].copy()
    dirty_s[5, 2] = np.nan
    dirty_s[9, 0] = -np.inf
    for name, s, t in (("single-point target", src[:130], one), ("flat target", src, flat), ("all points equal", src[:130], equal),
                       ("one-point source", src[:1], tgt), ("NaN and inf rows", dirty_s, dirty_t)):
        b = P.nn_brute(s, t)
        assert same(P.nn_grid(s, t), b), name
        assert same(P.nn_grid(s, t, shell_cap=8), b), name
    b = P.nn_brute(dirty_s, dirty_t)
    assert b[0][5] == -1 and np.isnan(b[2][5]) and b[0][9] == -1 and np.isnan(b[2][9])
    assert not np.isin(b[0], [3, 77, 150]).any()
    empty = np.full((40, 3), np.nan, f32)
    b = P.nn_brute(dirty_s, empty)
    assert same(P.nn_grid(dirty_s, empty), b)
    ok = np.isfinite(dirty_s).all(1)
    assert (b[0] == -1).all() and np.isinf(b[2][ok]).all() and np.isnan(b[2][~ok]).all()


def test_grid_points_on_cell_faces():
    """a target on an exact lattice of pitch h with cell_size = h (every point on a cell corner), sources on the corners too"""
    h = 0.125
    ax = np.arange(6) * h
    tgt = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).astype(f32)
    src = np.stack(np.meshgrid(np.arange(-1, 8) * h, np.arange(-1, 8) * h, np.arange(0, 6, 2) * h, indexing="ij"), -1).reshape(-1, 3).astype(f32)
    b = P.nn_brute(src, tgt)
    for cell in (h, h / 2, 2 * h):
        assert same(P.nn_grid(src, tgt, cell), b)
    inside = ((src >= 0) & (src <= 5 * h)).all(1)
    assert (b[2][inside] == 0).all()


def lattices(offset=0.5):
    ax = np.arange(5) * 0.25
    x, y = np.meshgrid(ax, ax, indexing="ij")
    a = np.stack([x.ravel(), y.ravel(), np.zeros(25)], 1).astype(f32)
    b = a.copy()
    b[:, 2] = f32(offset)
    return a, b


def test_metrics_closed_form():
    """two parallel 5 x 5 lattices of pitch 0.25, 0.5 apart: every nearest neighbour is the point opposite, at exactly 0.5"""
    a, b = lattices()
    i, d2, d = P.nn_brute(a, b)
    assert np.array_equal(i, np.arange(25)) and (d2 == f32(0.25)).all() and (d == f32(0.5)).all()
    m = P.metrics(a, b, taus=(0.4, 0.5, 0.6))
    for side in ("accuracy", "completeness"):
        assert m[side] == dict(mean=0.5, median=0.5, rmse=0.5, max=0.5)
    assert m["chamfer"] == 0.5
    assert list(m["precision"]) == [0.0, 0.0, 1.0] and list(m["recall"]) == [0.0, 0.0, 1.0] and list(m["fscore"]) == [0.0, 0.0, 1.0]
    assert (m["n_pred"], m["n_gt"], m["n_unmatched_pred"], m["n_unmatched_gt"]) == (25, 25, 0, 0)
    # a similarity that puts the first lattice onto the second: distances 0
    T = (np.eye(3), 1.0, np.array([0.0, 0.0, 0.5]))
    m = P.metrics(a, b, taus=(0.1,), transform=T)
    assert m["accuracy"] == dict(mean=0.0, median=0.0, rmse=0.0, max=0.0) and m["chamfer"] == 0.0 and list(m["fscore"]) == [1.0]
    T4 = np.eye(4)
    T4[:3, :3] *= 2.0                                               # scale 2 about the origin, then 0.5 up: pitch 0.5 against 0.25
    T4[2, 3] = 0.5
    m = P.metrics(a, b, taus=(0.1,), transform=T4)
    assert m["accuracy"]["max"] == float(np.sqrt(f32(2.0))) and m["completeness"]["max"] == float(np.sqrt(f32(0.0625 + 0.0625)))
    # nothing within the radius: everything unmatched, precision and recall 0, F-score 0 by definition
    m = P.metrics(a, b, taus=(0.6,), max_distance=0.4)
    assert m["n_unmatched_pred"] == 25 and m["n_unmatched_gt"] == 25 and np.isnan(m["accuracy"]["mean"]) and np.isnan(m["chamfer"])
    assert list(m["precision"]) == [0.0] and list(m["recall"]) == [0.0] and list(m["fscore"]) == [0.0]


def test_stats_statement():
    d = np.array([0.5, np.inf, 0.25, np.nan, 1.0, 0.75], f32)
    r = P.stats(d, (0.5, 2.0))
    assert (r["n"], r["n_finite"], r["n_unmatched"], r["n_nan"]) == (6, 4, 1, 1)
    assert r["sum"] == 2.5 and r["sumsq"] == 0.25 + 0.0625 + 1.0 + 0.5625 and r["max"] == 1.0 and r["median"] == 0.625 and r["counts"] == [1, 4]
    r = P.stats(np.array([np.inf, np.nan], f32), (1.0,))
    assert r["n_finite"] == 0 and np.isnan(r["max"]) and np.isnan(r["median"]) and r["counts"] == [0]


# ---- the package, without a GPU ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import bodyslam_amd.evaluation as EV
    import bodyslam_amd.pointcloud as PC
    import bodyslam_amd.tsdf as TS
    return PC, EV, TS


def test_public_signatures(built):
    PC, EV, TS = built

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert params(PC.NearestNeighbours.__init__) == [("self", E), ("target", E), ("cell_size", None), ("device", 0)]
    assert params(PC.NearestNeighbours.query) == [("self", E), ("source", E), ("max_distance", None), ("method", "grid")]
    assert params(PC.point_cloud_distance)[:2] == [("source", E), ("target", E)]
    assert dict(params(PC.point_cloud_distance)[2:]) == dict(cell_size=None, device=0, max_distance=None, method="grid")
    assert params(EV.evaluate_reconstruction) == [("pred", E), ("gt", E), ("thresholds", (0.001, 0.002, 0.005)), ("transform", None),
                                                  ("max_distance", None)]
    assert params(TS.PointCloud.compute_point_cloud_distance) == [("self", E), ("target", E)]
    assert params(TS.TSDF.extract_pcd) == [("self", E), ("host", True)] and params(TS.MAP.extract_pcd) == [("self", E), ("host", True)]
    assert [f.name for f in __import__("dataclasses").fields(TS.PointCloud)] == ["points", "colors", "normals"]
    names = {f.name for f in __import__("dataclasses").fields(EV.ReconstructionMetrics)}
    assert {"accuracy", "completeness", "chamfer", "precision", "recall", "fscore", "n_pred", "n_gt", "n_unmatched_pred", "n_unmatched_gt"} <= names
    assert [f.name for f in __import__("dataclasses").fields(EV.DistanceStats)] == ["mean", "median", "rmse", "max"]
    assert callable(EV.ReconstructionMetrics.write_csv)


def test_argument_validation(built):
    PC, EV, TS = built
    a, b = lattices()
    bad_points = [np.zeros((4, 2), f32), np.zeros((0, 3), f32), np.zeros((4, 3), np.int32), np.zeros(3, f32), [[0.0, 0.0, 0.0]], None,
                  torch.zeros(4, 3, dtype=torch.float16), TS.PointCloud(np.zeros((0, 3), f32), np.zeros((0, 3), f32))]
    for bad in bad_points:
        with pytest.raises(ValueError):
            PC.NearestNeighbours(bad)
        with pytest.raises(ValueError):
            PC.point_cloud_distance(bad, b)
        with pytest.raises(ValueError):
            EV.evaluate_reconstruction(bad, b)
        with pytest.raises(ValueError):
            EV.evaluate_reconstruction(a, bad)
    for cell in (0.0, -1.0, np.nan, np.inf, 1e-60, "1", True):
        with pytest.raises(ValueError):
            PC.NearestNeighbours(b, cell_size=cell)
    for md in (-1.0, np.nan, "1", True):
        with pytest.raises(ValueError):
            PC.point_cloud_distance(a, b, max_distance=md)
        with pytest.raises(ValueError):
            EV.evaluate_reconstruction(a, b, max_distance=md)
    with pytest.raises(ValueError):
        PC.point_cloud_distance(a, b, method="kdtree")
    for taus in ((0.0,), (-1.0,), (np.nan,), tuple([0.1] * 9), ("a",), 0.1):
        with pytest.raises(ValueError):
            EV.evaluate_reconstruction(a, b, thresholds=taus)
    for T in (np.eye(3), np.zeros((4, 3)), (np.eye(3), 1.0), (np.eye(2), 1.0, np.zeros(3)), (np.eye(3), "s", np.zeros(3)), (np.eye(3), 1.0, np.zeros(2)),
              "T"):
        with pytest.raises(ValueError):
            EV.evaluate_reconstruction(a, b, transform=T)
    assert np.array_equal(PC.affine_rows((2.0 * np.eye(3)[[1, 0, 2]], 0.5, [1, 2, 3])), P.affine_rows((2.0 * np.eye(3)[[1, 0, 2]], 0.5, [1, 2, 3])))
    assert np.array_equal(PC.affine_rows(torch.eye(4, dtype=torch.float64)), np.eye(4)[:3])


def test_default_cell_size_matches_statement(built):
    PC, EV, TS = built
    tgt = P.base_target()
    lo, hi = P.bounds(tgt)
    h = PC.default_cell_size(lo, hi, len(tgt))
    assert h == P.default_cell_size(lo, hi, len(tgt)) and np.array_equal(PC.grid_dims(lo, hi, h), P.dims_for(lo, hi, h))
    assert 0.5 * len(tgt) <= PC.n_cells(PC.grid_dims(lo, hi, h)) <= 2 * len(tgt)           # about as many cells as points
    big_lo, big_hi = np.zeros(3, f32), np.full(3, 1000.0, f32)
    h = PC.default_cell_size(big_lo, big_hi, 10 ** 9)                                        # the 2^24 cap
    assert 2 ** 23 < PC.n_cells(PC.grid_dims(big_lo, big_hi, h)) <= 2 ** 24
    assert PC.default_cell_size(np.ones(3, f32), np.ones(3, f32), 5) == 1.0
    flat_hi = np.array([1.0, 2.0, 0.0], f32)
    assert list(PC.grid_dims(np.zeros(3, f32), flat_hi, PC.default_cell_size(np.zeros(3, f32), flat_hi, 200)))[2] == 1


def test_no_cpu_fallback(built):
    PC, EV, TS = built
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from bodyslam_amd._lib import BodySlamHipError
    a, b = lattices()
    with pytest.raises(BodySlamHipError):
        PC.NearestNeighbours(b)
    with pytest.raises(BodySlamHipError):
        PC.point_cloud_distance(a, b)
    with pytest.raises(BodySlamHipError):
        PC.transform_points(a, np.eye(4))
    with pytest.raises(BodySlamHipError):
        EV.evaluate_reconstruction(a, b)
    with pytest.raises(BodySlamHipError):
        EV.distance_stats_record(torch.zeros(4))
    with pytest.raises(BodySlamHipError):
        TS.PointCloud(a, np.zeros_like(a)).compute_point_cloud_distance(TS.PointCloud(b, np.zeros_like(b)))
