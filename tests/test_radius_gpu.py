"""GPU tests of the radius search, the radius outlier removal and DBSCAN (csrc/radius.hip, bodyslam_amd/pointcloud.py) against the statement
tests/_radius_ref.py: bit-equal, at every cell size.  The clouds are those of tests/test_knn_gpu.py -- the planted cloud of 2 806 points
(eleven blocks of 256, the last one partial) and the 9 x 7 x 3 tie lattice -- and the two constructed cases of _radius_ref.py;
tests/test_radius_cpu.py asserts that they exercise what is claimed for them."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_ref as K  # noqa: E402
import _radius_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
R_SMALL, R_LARGE = 0.004, 0.008
TIE_RADII = (f32(2.0 ** -8), f32(np.sqrt(2.0) * 2.0 ** -8))


@pytest.fixture(scope="module")
def PC():
    import bodyslam_amd.pointcloud as PC
    return PC


@pytest.fixture(scope="module")
def data():
    planted, rows = K.planted_cloud()
    return dict(planted=planted, planted_rows=rows, lattice=K.tie_lattice())


_REF = {}


def ref(kind, name, *args):
    """the statement's result, computed once per case and left unchanged"""
    key = (kind, name) + tuple(float(a) if isinstance(a, (float, np.floating)) else a for a in args[1:] if not isinstance(a, np.ndarray))
    if key not in _REF:
        _REF[key] = {"radius": R.radius_brute, "dbscan": R.cluster_dbscan, "outlier": R.remove_radius_outlier}[kind](*args)
    return _REF[key]


def cells(cloud, radius):
    """None (the radius, as far as the grid allows), a quarter of it, four times it, and one cell for the whole cloud"""
    fin = cloud[np.isfinite(cloud).all(1)]
    one = float(2.0 * (fin.max(0) - fin.min(0)).max() + 1.0)
    return (None, float(radius) / 4, float(radius) * 4, one)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def host(ts):
    return tuple(t.cpu().numpy() for t in ts)


def check_rows(got, want, what):
    for g, w, name in zip(got, want, ("row_start", "index", "d2")):
        assert same_bits(g, w), (what, name, g[:8], w[:8])


def check_query(PC, src, tgt, radius, want, what):
    """count_radius and the sorted query_radius at every cell size, bit-equal to the statement"""
    for h in cells(tgt, radius):
        nn = PC.NearestNeighbours.for_radius(tgt, radius, cell_size=h)
        cnt = nn.count_radius(src, radius).cpu().numpy()
        assert same_bits(cnt, np.diff(want[0]).astype(np.int32)), (what, h)
        got = host(nn.query_radius(src, radius))
        assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == f32
        check_rows(got, want, (what, h))


# ---- 1: counts and lists against the statement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [R_SMALL, R_LARGE])
def test_self_query(PC, data, radius):
    p = data["planted"]
    want = ref("radius", "planted", p, p, radius)
    check_query(PC, p, p, radius, want, "planted")
    assert np.array_equal(want[1][want[0][:-1]], np.arange(len(p))) and np.all(want[2][want[0][:-1]] == 0.0)     # itself first, d2 = 0
    if radius == R_LARGE:
        assert np.diff(want[0]).max() > K.KNN_MAX


@pytest.mark.parametrize("radius", TIE_RADII)
def test_tie_lattice(PC, data, radius):
    lat = data["lattice"]
    check_query(PC, lat, lat, radius, ref("radius", "lattice", lat, lat, radius), "lattice")


def test_unsorted_rows_are_the_same_sets(PC, data):
    p = data["planted"]
    want = ref("radius", "planted", p, p, R_LARGE)
    for h in (None, R_LARGE * 4):
        row_start, index, d2 = host(PC.NearestNeighbours.for_radius(p, R_LARGE, cell_size=h).query_radius(p, R_LARGE, sort=False))
        assert same_bits(row_start, want[0])
        key = lambda i, d: (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | i.astype(np.uint64)          # noqa: E731
        got, exp = key(index, d2), key(want[1], want[2])
        row = np.repeat(np.arange(len(p)), np.diff(row_start))
        assert np.array_equal(got[np.lexsort((got, row))], exp)                                                # each row equal as a set


def test_max_nn_keeps_the_first_of_each_sorted_row(PC, data):
    p = data["planted"]
    want = R.first_of_rows(*ref("radius", "planted", p, p, R_LARGE), 5)
    for sort in (True, False):                                                                                 # max_nn implies the sort
        check_rows(host(PC.NearestNeighbours.for_radius(p, R_LARGE).query_radius(p, R_LARGE, max_nn=5, sort=sort)), want, ("max_nn", sort))
    lat = data["lattice"]
    few = host(PC.NearestNeighbours(lat).query_radius(lat, TIE_RADII[0], max_nn=100))                          # above every count: all of it
    check_rows(few, ref("radius", "lattice", lat, lat, TIE_RADII[0]), "max_nn above the counts")


# ---- 2: agreement with what exists -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [R_SMALL, R_LARGE])
def test_agrees_with_the_hybrid_search(PC, data, radius):
    p = data["planted"]
    nn = PC.NearestNeighbours(p)
    idx, d2k, cnt = host(nn.query_knn(p, 32, radius))
    row_start, index, d2 = host(nn.query_radius(p, radius))
    c = np.diff(row_start)
    assert np.array_equal(cnt, np.minimum(c, 32))
    col = np.arange(32)[None, :]
    pos = np.minimum(row_start[:-1, None] + col, len(index) - 1)
    got = col < cnt[:, None]
    assert np.array_equal(np.where(got, index[pos], -1), idx)                                                  # rows of <= 32: the whole row
    assert np.array_equal(np.where(got, d2[pos], f32(np.inf)).view(np.uint32), d2k.view(np.uint32))


@pytest.mark.parametrize("nb_points", [0, 4, 31])
def test_outlier_mask_agrees_with_the_hybrid_search(PC, data, nb_points):
    p = data["planted"]
    kept, mask = PC.remove_radius_outlier(p, nb_points, R_LARGE)
    cnt = PC.NearestNeighbours(p).query_knn(p, nb_points + 1, R_LARGE)[2]
    assert torch.equal(mask, cnt > nb_points) and torch.equal(kept, torch.nonzero(mask).reshape(-1))


# ---- 3: the edges --------------------------------------------------------------------------------------------------------------------------
def test_non_finite_sources_and_targets(PC, data):
    tgt = data["planted"][:600].copy()
    tgt[7, 1], tgt[200, 0], tgt[599, 2] = np.nan, np.inf, -np.inf
    src = tgt[:300].copy()
    src[11, 2] = np.inf
    want = R.radius_brute(src, tgt, R_LARGE)
    check_query(PC, src, tgt, R_LARGE, want, "non-finite")
    c = np.diff(want[0])
    assert c[7] == 0 and c[11] == 0 and c[12] > 0 and not np.isin([7, 200, 599], want[1]).any() and want[1].max() > 200


def test_far_source_has_no_neighbours(PC, data):
    p = data["planted"]
    src = np.concatenate([p[:3], p[:2] + f32(10.0), -p[:1] - f32(50.0)]).astype(f32)
    want = R.radius_brute(src, p, R_SMALL)
    assert np.all(np.diff(want[0])[3:] == 0)
    check_query(PC, src, p, R_SMALL, want, "far")


def test_one_source_one_target(PC, data):
    p = data["planted"]
    for src, tgt in ((p[5:6], p), (p[:300], p[5:6]), (p[5:6], p[5:6]), (p[6:7], p[5:6])):
        check_query(PC, src, tgt, R_LARGE, R.radius_brute(src, tgt, R_LARGE), (len(src), len(tgt)))


def test_radius_larger_than_the_cloud(PC, data):
    lat = data["lattice"].copy()
    lat[50, 0] = np.nan
    want = R.radius_brute(lat, lat, 1.0)
    c = np.diff(want[0])
    assert np.all(np.delete(c, 50) == len(lat) - 1) and c[50] == 0                                             # the whole finite target: rows of 188
    for h in (None, 2.0 ** -8, 0.25):
        nn = PC.NearestNeighbours.for_radius(lat, 1.0, cell_size=h)
        check_rows(host(nn.query_radius(lat, 1.0)), want, ("whole", h))


@pytest.mark.parametrize("m", [255, 256, 257])
def test_block_edge(PC, data, m):
    p = data["planted"]
    full = ref("radius", "planted", p, p, R_LARGE)
    e = full[0][m]
    want = (full[0][:m + 1], full[1][:e], full[2][:e])
    nn = PC.NearestNeighbours.for_radius(p, R_LARGE)
    check_rows(host(nn.query_radius(p[:m], R_LARGE)), want, m)
    assert same_bits(nn.count_radius(p[:m], R_LARGE).cpu().numpy(), np.diff(want[0]).astype(np.int32))


@pytest.mark.parametrize("copies", [63, 64, 65, 66, 130])
def test_wave_edge_of_the_sort(PC, data, copies):
    """a point repeated at distinct indices, scattered among others: the row of a source there holds exactly `copies` keys of d2 = 0 that only
    the index orders, and with the larger radius one more"""
    p = data["planted"]
    rng = np.random.default_rng(copies)
    spot = np.array([[2.0, 2.0, 2.0]], f32)
    tgt = np.concatenate([p[:200], np.repeat(spot, copies, 0), spot + np.array([2.0 ** -6, 0, 0], f32)]).astype(f32)
    tgt = tgt[rng.permutation(len(tgt))]
    src = np.concatenate([spot, p[:3]])
    for radius, n_row in ((2.0 ** -8, copies), (2.0 ** -6, copies + 1)):
        want = R.radius_brute(src, tgt, radius)
        assert np.diff(want[0])[0] == n_row and np.all(np.diff(want[1][:copies]) > 0)
        for h in (None, 1.0, 8.0):
            check_rows(host(PC.NearestNeighbours.for_radius(tgt, radius, cell_size=h).query_radius(src, radius)), want, (copies, radius, h))


def test_total_at_2_31_is_refused_before_the_fill(PC):
    n = 46400                                                                                                   # n * n = 2 152 960 000 >= 2^31
    pts = np.zeros((n, 3), f32)
    nn = PC.NearestNeighbours(pts)
    assert int(nn.count_radius(pts[:4], 1.0).min()) == n
    with pytest.raises(ValueError, match=str(n * n)):
        nn.query_radius(pts, 1.0)


# ---- 4: the radius outlier removal ---------------------------------------------------------------------------------------------------------
def test_remove_radius_outlier_drops_the_planted_rows(PC, data):
    p, rows = data["planted"], data["planted_rows"]
    want = ref("outlier", "planted", p, 4, R_SMALL)
    for h in cells(p, R_SMALL):
        kept, mask = host(PC.remove_radius_outlier(p, 4, R_SMALL, cell_size=h))
        assert kept.dtype == np.int64 and mask.dtype == bool and same_bits(kept, want[0]) and same_bits(mask, want[1]), h
    assert np.array_equal(np.nonzero(~want[1])[0], rows)


def test_remove_radius_outlier_above_the_knn_cap(PC, data):
    p = data["planted"]
    want = R.remove_radius_outlier(p, 60, 0.01)
    assert 0 < want[1].sum() < len(p)
    kept, mask = host(PC.remove_radius_outlier(p, 60, 0.01))
    assert same_bits(kept, want[0]) and same_bits(mask, want[1])


def test_point_cloud_methods(PC, data):
    from bodyslam_amd.tsdf import PointCloud
    p, rows = data["planted"], data["planted_rows"]
    colors = np.linspace(0, 1, 3 * len(p), dtype=f32).reshape(-1, 3)
    cloud = PointCloud(p, colors)
    out, ind = cloud.remove_radius_outlier(4, R_SMALL)
    want = ref("outlier", "planted", p, 4, R_SMALL)[0]
    assert isinstance(ind, np.ndarray) and np.array_equal(ind, want) and same_bits(out.points, p[want]) and same_bits(out.colors, colors[want])
    labels = cloud.cluster_dbscan(0.005, 10)
    assert isinstance(labels, np.ndarray) and same_bits(labels, ref("dbscan", "planted", p, 0.005, 10))
    dev = PointCloud(torch.from_numpy(p).cuda(), torch.from_numpy(colors).cuda())
    assert torch.equal(dev.cluster_dbscan(0.005, 10).cpu(), torch.from_numpy(labels))


# ---- 5: DBSCAN -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.005, 0.004])
def test_dbscan_planted(PC, data, eps):
    p = data["planted"]
    want = ref("dbscan", "planted", p, eps, 10)
    for h in cells(p, eps):
        labels = PC.cluster_dbscan(p, eps, 10, cell_size=h).cpu().numpy()
        assert same_bits(labels, want), (eps, h, np.nonzero(labels != want)[0][:8])
        assert PC.last_clusters == want.max() + 1 and PC.last_rounds >= 2
    assert want.max() + 1 == (1 if eps == 0.005 else 10)


def test_dbscan_two_plates(PC):
    pts, b, contact0, contact1 = R.two_plates()
    want = R.cluster_dbscan(pts, R.PLATES_EPS, R.PLATES_MIN_POINTS)
    for h in cells(pts, R.PLATES_EPS):
        labels = PC.cluster_dbscan(pts, R.PLATES_EPS, R.PLATES_MIN_POINTS, cell_size=h).cpu().numpy()
        assert same_bits(labels, want) and labels[b] == 0 and labels[contact0] == 0 and labels[contact1] == 1, (h, labels)


def test_dbscan_chain(PC):
    pts = R.chain()
    for h in cells(pts, R.CHAIN_EPS):
        labels = PC.cluster_dbscan(pts, R.CHAIN_EPS, 3, cell_size=h).cpu().numpy()
        assert labels.dtype == np.int32 and np.all(labels == 0), h                                             # one cluster, the ends its borders
        assert PC.last_clusters == 1 and 2 <= PC.last_rounds <= R.CHAIN_N, PC.last_rounds
    labels = PC.cluster_dbscan(pts, R.CHAIN_EPS, 4).cpu().numpy()                                              # nobody is core
    assert np.all(labels == -1) and PC.last_clusters == 0


def test_dbscan_every_finite_point_its_own_cluster(PC, data):
    pts = data["planted"][:700].copy()
    pts[3, 0], pts[300, 2], pts[699, 1] = np.nan, -np.inf, np.inf
    labels = PC.cluster_dbscan(pts, 1e-6, 1).cpu().numpy()
    fin = np.isfinite(pts).all(1)
    assert np.array_equal(labels[fin], np.arange(fin.sum())) and np.all(labels[~fin] == -1) and PC.last_clusters == fin.sum()
    assert same_bits(labels, R.cluster_dbscan(pts, 1e-6, 1))


def test_two_runs_give_the_same_bits(PC, data):
    p = data["planted"]
    a = PC.cluster_dbscan(p, 0.004, 10)
    b = PC.cluster_dbscan(p, 0.004, 10)
    assert torch.equal(a, b)
    nn = PC.NearestNeighbours.for_radius(p, R_LARGE)
    for x, y in zip(nn.query_radius(p, R_LARGE), nn.query_radius(p, R_LARGE)):
        assert torch.equal(x, y)
