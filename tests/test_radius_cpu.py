"""CPU tests of the statement tests/_radius_ref.py and of the argument checks of the radius search, the radius outlier removal and DBSCAN
(bodyslam_amd/pointcloud.py): the inputs of tests/test_radius_gpu.py exercise what they claim, and bad arguments raise before the device
is touched."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_ref as K  # noqa: E402
import _radius_ref as R  # noqa: E402

f32 = np.float32
_CACHE = {}


def planted():
    if "planted" not in _CACHE:
        _CACHE["planted"] = K.planted_cloud()
    return _CACHE["planted"]


def dbscan(eps, min_points):
    key = ("dbscan", eps, min_points)
    if key not in _CACHE:
        _CACHE[key] = R.cluster_dbscan(planted()[0], eps, min_points, details=True)
    return _CACHE[key]


def test_statement_agrees_with_the_knn_statement():
    """where a row has at most 32 neighbours it is the hybrid search's row; everywhere the first 32 agree"""
    pts, _ = planted()
    src = pts[:600]
    row_start, index, d2 = R.radius_brute(src, pts, 0.008)
    idx, d2k, cnt = K.knn_brute(src, pts, 32, 0.008)
    c = np.diff(row_start)
    assert np.array_equal(np.minimum(c, 32), cnt) and c.max() > 32
    for i in range(len(src)):
        k = int(cnt[i])
        assert np.array_equal(index[row_start[i]:row_start[i] + k], idx[i, :k])
        assert np.array_equal(d2[row_start[i]:row_start[i] + k].view(np.uint32), d2k[i, :k].view(np.uint32))
    assert np.array_equal(index[row_start[:-1]], np.arange(len(src))) and np.all(d2[row_start[:-1]] == 0)       # itself first
    s5, i5, d5 = R.first_of_rows(row_start, index, d2, 5)
    assert np.all(np.diff(s5) == np.minimum(c, 5)) and np.array_equal(i5[s5[3]:s5[4]], index[row_start[3]:row_start[3] + 5])
    assert d5.dtype == f32 and i5.dtype == np.int32


def test_non_finite_rows_of_the_statement():
    pts, _ = planted()
    tgt = pts[:400].copy()
    tgt[7, 1], tgt[200, 0] = np.nan, np.inf
    src = tgt[:50].copy()
    row_start, index, _ = R.radius_brute(src, tgt, 0.008)
    c = np.diff(row_start)
    assert c[7] == 0 and c[6] > 0 and 7 not in index and 200 not in index                  # no row for it, and it is nobody's neighbour
    want = R.radius_brute(src, np.delete(tgt, [7, 200], 0), 0.008)[1]
    shifted = index - (index > 7) - (index > 200)
    assert np.array_equal(shifted, want)                                                       # indices refer to the target as given


def test_planted_rows_are_the_radius_outliers():
    pts, rows = planted()
    kept, mask, cnt = R.remove_radius_outlier(pts, 4, 0.004)
    moved = np.zeros(len(pts), bool)
    moved[rows] = True
    assert np.all(cnt[~moved] >= 5) and np.all(cnt[moved] == 1)
    assert np.array_equal(mask, ~moved) and np.array_equal(kept, np.nonzero(~moved)[0])


def test_a_radius_holds_more_than_the_knn_cap():
    pts, _ = planted()
    assert R.radius_count(pts, pts, 0.008).max() == 51 > K.KNN_MAX                             # why the feature exists


def test_dbscan_one_cluster():
    pts, rows = planted()
    labels, core, clusters, border = dbscan(0.005, 10)
    assert clusters == 1 and int(border.sum()) == 36
    assert np.array_equal(np.nonzero(labels < 0)[0], rows)
    assert np.all(labels[core] == 0) and np.all(labels[border] == 0)


def test_dbscan_many_clusters_and_borders_that_choose():
    pts, _ = planted()
    labels, core, clusters, border = dbscan(0.004, 10)
    assert (clusters, int(border.sum()), int((labels < 0).sum())) == (10, 857, 150)
    assert clusters >= 2 and border.sum() >= 100
    # clusters are numbered by their smallest core index
    firsts = [int(np.nonzero(core & (labels == c))[0][0]) for c in range(clusters)]
    assert firsts == sorted(firsts)
    # borders with core neighbours in two clusters: if the cloud has none, the two-plate case carries that rule alone
    row_start, index, _ = R.radius_brute(pts, pts, 0.004)
    choosing = 0
    for i in np.nonzero(border)[0]:
        nb = index[row_start[i]:row_start[i + 1]]
        seen = np.unique(labels[nb[core[nb]]])
        choosing += len(seen) >= 2
        assert labels[i] == seen.min()
    _CACHE["choosing"] = choosing
    assert choosing >= 1, "no border of this cloud chooses between clusters: the two-plate case carries that rule alone"


def test_tie_lattice_has_targets_at_exactly_the_radius():
    lat = K.tie_lattice()
    for radius, most in ((f32(2.0 ** -8), 7), (f32(np.sqrt(2.0) * 2.0 ** -8), 19)):
        cut = K.d2_cutoff(radius)
        assert np.sqrt(cut) <= radius < np.sqrt(np.nextafter(cut, f32(np.inf)))
        row_start, index, d2 = R.radius_brute(lat, lat, radius)
        cnt = np.diff(row_start)
        assert cnt.max() == most                                                              # itself, 6 along the axes, 12 across the faces
        at = np.sqrt(d2) == radius
        on_rim = np.add.reduceat(at.astype(np.int64), row_start[:-1])
        assert np.all(on_rim >= 3) and d2.max() == d2[at].max() <= cut                        # every point has targets at exactly the radius
        # "<" instead of "<=", or a cut-off one ulp lower, loses exactly those: every count changes
        lower = np.nextafter(d2[at].max(), f32(0.0))
        assert np.array_equal(np.add.reduceat((d2 <= lower).astype(np.int64), row_start[:-1]), cnt - on_rim)
        assert np.array_equal(R.radius_count(lat, lat, np.nextafter(radius, f32(0.0))), cnt - on_rim)


def test_two_plates():
    pts, b, contact0, contact1 = R.two_plates()
    eps, mp = R.PLATES_EPS, R.PLATES_MIN_POINTS
    labels, core, clusters, border = R.cluster_dbscan(pts, eps, mp, details=True)
    row_start, index, d2 = R.radius_brute(pts, pts, eps)
    nb, nd = index[row_start[b]:row_start[b + 1]], d2[row_start[b]:row_start[b + 1]]
    assert clusters == 2 and not core[b] and border[b] and len(nb) == 3                        # B: itself and the two contacts
    core_nb = nb[core[nb]]
    assert sorted(core_nb) == [contact1, contact0] and np.all(np.sqrt(nd[core[nb]]) == eps)    # both at exactly eps
    assert core[0] and labels[0] == 0 and labels[contact0] == 0 and labels[contact1] == 1
    assert contact0 == len(pts) - 1 and contact1 < contact0                                    # cluster 0 touches B through its highest index
    assert labels[b] == 0
    nearest = core_nb[np.lexsort((core_nb, nd[core[nb]]))[0]]                                  # the two wrong rules give 1 here
    assert labels[nearest] == 1 and labels[core_nb.min()] == 1
    assert int(border.sum()) == 9 and int((labels < 0).sum()) == 0                             # the eight corners and B


def test_chain():
    pts = R.chain()
    labels, core, clusters, border = R.cluster_dbscan(pts, R.CHAIN_EPS, 3, details=True)
    ends = np.nonzero((pts[:, 0] == 0) | (pts[:, 0] == pts[:, 0].max()))[0]
    assert clusters == 1 and np.all(labels == 0) and np.array_equal(np.nonzero(border)[0], np.sort(ends)) and core.sum() == R.CHAIN_N - 2
    assert not np.array_equal(pts[:, 0], np.sort(pts[:, 0]))                                   # shuffled: neighbours lie blocks apart
    labels, core, clusters, border = R.cluster_dbscan(pts, R.CHAIN_EPS, 4, details=True)
    assert clusters == 0 and not core.any() and np.all(labels == -1)


def test_every_finite_point_its_own_cluster():
    pts = planted()[0][:40].copy()
    pts[3, 0], pts[17, 2] = np.nan, -np.inf
    labels = R.cluster_dbscan(pts, 1e-6, 1)
    fin = np.isfinite(pts).all(1)
    assert np.array_equal(labels[fin], np.arange(fin.sum())) and np.all(labels[~fin] == -1)


def test_arguments_raise_before_the_device(monkeypatch):
    import bodyslam_amd.pointcloud as PC
    import bodyslam_amd.tsdf as TS
    from bodyslam_amd import _lib

    def touched(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "init", touched)
    pts = planted()[0]
    cloud = TS.PointCloud(pts, np.zeros_like(pts))
    nn = object.__new__(PC.NearestNeighbours)                  # the checks come before the index is looked at (none exists without a device)
    for r in (0.0, -1.0, np.nan, np.inf, 1e-60, 1e60, "1", True, None):
        with pytest.raises(ValueError):
            PC.NearestNeighbours.query_radius(nn, pts, r)
        with pytest.raises(ValueError):
            PC.NearestNeighbours.count_radius(nn, pts, r)
        with pytest.raises(ValueError):
            PC.remove_radius_outlier(pts, 4, r)
        with pytest.raises(ValueError):
            cloud.remove_radius_outlier(4, r)
        with pytest.raises(ValueError):
            PC.cluster_dbscan(pts, r, 10)
        with pytest.raises(ValueError):
            cloud.cluster_dbscan(r, 10)
        with pytest.raises(ValueError):
            PC.NearestNeighbours.for_radius(pts, r)
    for mp in (0, -1, 2.5, "3", True, None, 2 ** 31):
        with pytest.raises(ValueError):
            PC.cluster_dbscan(pts, 0.005, mp)
        with pytest.raises(ValueError):
            cloud.cluster_dbscan(0.005, mp)
    for nb in (-1, 2.5, "3", True, None):
        with pytest.raises(ValueError):
            PC.remove_radius_outlier(pts, nb, 0.004)
        with pytest.raises(ValueError):
            cloud.remove_radius_outlier(nb, 0.004)
    for k in (0, -1, 2.5, "3", True):
        with pytest.raises(ValueError):
            PC.NearestNeighbours.query_radius(nn, pts, 0.004, max_nn=k)
    for bad in (np.zeros((4, 2), f32), np.zeros((0, 3), f32), pts.astype(np.int32), None):
        with pytest.raises(ValueError):
            PC.remove_radius_outlier(bad, 4, 0.004)
        with pytest.raises(ValueError):
            PC.cluster_dbscan(bad, 0.005, 10)
        with pytest.raises(ValueError):
            PC.NearestNeighbours.query_radius(nn, bad, 0.004)
    for h in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError):
            PC.remove_radius_outlier(pts, 4, 0.004, cell_size=h)
        with pytest.raises(ValueError):
            PC.cluster_dbscan(pts, 0.005, 10, cell_size=h)


def test_radius_cell_size():
    import bodyslam_amd.pointcloud as PC
    lo, hi = np.zeros(3, f32), np.array([1.0, 0.5, 0.25], f32)
    assert PC.radius_cell_size(lo, hi, 0.01) == float(f32(0.01))                               # the radius itself while the grid fits
    h = PC.radius_cell_size(lo, hi, 1e-4)                                                      # 1.25e11 cells at the radius: grown by 1.25s
    assert h > 1e-4 and PC.n_cells(PC.grid_dims(lo, hi, h)) <= 2 ** 24 < PC.n_cells(PC.grid_dims(lo, hi, float(f32(h / 1.25))))
