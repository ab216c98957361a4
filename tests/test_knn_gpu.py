"""GPU tests of the k nearest neighbours, the normal estimation and the statistical outlier removal (csrc/knn.hip, bodyslam_amd/pointcloud.py)
against the statement tests/_knn_ref.py.  The base cloud is the bumpy target of tests/_icp_ref.py: 2 806 points = eleven blocks of 256, the
last one partial.  The tie cloud is the 9 x 7 x 3 integer lattice scaled by 2^-8: for k = 8, 96 % of its rows have the 8th and 9th d2 equal
(tests/test_knn_cpu.py asserts it), so a stop that is not strict, or a tie-break not by index, fails there."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _icp_ref as I  # noqa: E402
import _knn_ref as K  # noqa: E402
import _pointcloud_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
RECOVERY_BOUND = 5e-5            # tests/test_icp_gpu.py's bound for analytic normals; the statement with estimated normals measures 1.25e-5 m
EIG_TOL = 1e-12                  # of the largest eigenvalue: an fp64 sum of <= 32 terms in the same order leaves only the Jacobi's rounding
NORMAL_TOL = 5e-7                # two fp32 roundings of a unit vector (1.2e-7) plus the eigenvector's sensitivity (the gap: test_knn_cpu.py)


@pytest.fixture(scope="module")
def PC():
    import bodyslam_amd.pointcloud as PC
    return PC


@pytest.fixture(scope="module")
def data():
    tgt, nrm = I.bumpy_target()
    lo, hi = P.bounds(tgt)
    planted, rows = K.planted_cloud()
    return dict(tgt=tgt, nrm=nrm, h0=P.default_cell_size(lo, hi, len(tgt)), lattice=K.tie_lattice(), true=I.bumpy_source_true(),
                planted=planted, planted_rows=rows)


_REF = {}


def ref_knn(name, src, tgt, k, radius=None):
    """the statement's result, computed once per case"""
    key = (name, k, radius)
    if key not in _REF:
        _REF[key] = K.knn_brute(src, tgt, k, radius)
    return _REF[key]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_knn(PC, name, src, tgt, k, radius, cells):
    """the device result at every cell size, bit-equal to the statement (hence to each other) -> the statement's result"""
    want = ref_knn(name, src, tgt, k, radius)
    for h in cells:
        nn = PC.NearestNeighbours(tgt, cell_size=h)
        idx, d2, cnt = (t.cpu().numpy() for t in nn.query_knn(src, k, radius))
        assert idx.dtype == np.int32 and d2.dtype == f32 and cnt.dtype == np.int32 and idx.shape == (len(src), k) == d2.shape
        bad = np.nonzero((idx != want[0]).any(1) | (cnt != want[2]))[0]
        assert same_bits(cnt, want[2]) and same_bits(idx, want[0]), (name, k, radius, h, bad[:5], idx[bad[:2]], want[0][bad[:2]])
        assert same_bits(d2, want[1]), (name, k, radius, h)
    return want


# ---- 1: the self-query against the statement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 8, 30, 32])
def test_self_query(PC, data, k):
    tgt, h0 = data["tgt"], data["h0"]
    idx, d2, cnt = check_knn(PC, "self", tgt, tgt, k, None, (h0, h0 * 0.25, h0 * 4.0))
    assert np.all(cnt == k) and np.array_equal(idx[:, 0], np.arange(len(tgt))) and np.all(d2[:, 0] == 0.0)       # a point is its own first neighbour
    if k == 1:
        dist, index = (t.cpu().numpy() for t in PC.NearestNeighbours(tgt).query(tgt))
        assert same_bits(index, idx[:, 0]) and same_bits(dist, np.sqrt(d2[:, 0]))


# ---- 2: the tie lattice ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 7, 8, 27])
def test_tie_lattice(PC, data, k):
    lat = data["lattice"]
    check_knn(PC, "lattice", lat, lat, k, None, (2.0 ** -8, 3 * 2.0 ** -8, 1.0))          # one point per cell ... a single cell


# ---- 3: the edges of the domain ------------------------------------------------------------------------------------------------------------
def test_fewer_targets_than_k(PC, data):
    tgt = data["tgt"]
    idx, d2, cnt = check_knn(PC, "five", tgt[:300], tgt[:5], 8, None, (None, 1e-3))
    assert np.all(cnt == 5) and np.all(idx[:, 5:] == -1) and np.all(np.isposinf(d2[:, 5:]))


def test_non_finite_rows(PC, data):
    tgt = data["tgt"].copy()
    tgt[17] = np.nan
    tgt[1200, 2] = np.inf
    src = data["tgt"][::3].copy()
    src[5, 0] = np.nan
    src[400] = np.inf
    idx, d2, cnt = check_knn(PC, "nonfinite", src, tgt, 8, None, (None, data["h0"] * 0.25))
    assert cnt[5] == 0 and cnt[400] == 0 and np.all(idx[5] == -1) and np.all(np.isnan(d2[400]))
    assert not np.isin(idx, (17, 1200)).any()


def test_sources_outside_the_box(PC, data):
    src = P.base_source() + f32(0.05)
    lo, hi = P.bounds(data["tgt"])
    assert ((src < lo) | (src > hi)).any(1).all()
    check_knn(PC, "outside", src, data["tgt"], 8, None, (None, data["h0"] * 0.25))


def test_another_source(PC, data):
    src = data["true"].astype(f32)
    assert len(src) == 1937
    check_knn(PC, "true", src, data["tgt"], 8, None, (None, data["h0"] * 0.25, data["h0"] * 4.0))
    nn = PC.NearestNeighbours(data["tgt"])
    a = nn.query_knn(torch.from_numpy(src).cuda(), 8)                                     # a device tensor, and a second run: the same bits
    b = nn.query_knn(src.astype(f64), 8)
    assert all(torch.equal(x, y) for x, y in zip(a[:1] + a[2:], b[:1] + b[2:])) and same_bits(a[1].cpu().numpy(), b[1].cpu().numpy())


# ---- 4: hybrid search ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0.008, 0.005])
def test_hybrid(PC, data, radius):
    tgt, h0 = data["tgt"], data["h0"]
    _, _, cnt = check_knn(PC, "self", tgt, tgt, 30, radius, (h0, h0 * 0.25, h0 * 4.0))
    short = float((cnt < 30).mean())
    print("radius", radius, "short rows", short, "counts", cnt.min(), "..", cnt.max())
    assert (0.0 < short < 1.0) if radius == 0.008 else (short == 1.0 and cnt.min() >= 1)


def test_hybrid_radius_is_inclusive(PC, data):
    lat = data["lattice"]
    idx, d2, cnt = check_knn(PC, "lattice", lat, lat, 27, 2.0 ** -8, (2.0 ** -8, 3 * 2.0 ** -8, 1.0))
    c = (1 * 7 + 3) * 9 + 4                                                               # an interior point: itself and its six axis neighbours
    assert cnt[c] == 7 and np.all(d2[c, 1:7] == f32(2.0 ** -16)) and cnt.min() == 4 and cnt.max() == 7


# ---- 5: normals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [6, 10, 30])
def test_normals(PC, data, k):
    tgt, h0 = data["tgt"], data["h0"]
    idx, _, cnt = ref_knn("self", tgt, tgt, k)
    want_n, want_ev = K.normals_from_knn(tgt, idx, cnt, direction=(0, 0, 1))
    first = None
    for h in (h0, h0 * 0.25, h0 * 4.0, h0):                                               # three cell sizes and a second run
        n, ev = PC.estimate_normals(tgt, k=k, direction=(0, 0, 1), cell_size=h, return_eigenvalues=True)
        n, ev = n.cpu().numpy(), ev.cpu().numpy()
        assert n.shape == (len(tgt), 3) and n.dtype == f32 and ev.shape == (len(tgt), 3) and ev.dtype == f64
        if first is None:
            first = (n, ev)
        assert same_bits(first[0], n) and same_bits(first[1], ev), f"the bits depend on the cell size or the run ({h})"
    n, ev = first
    d_ev = (np.abs(ev - want_ev) / want_ev[:, 2:3]).max()
    d_n = np.abs(n.astype(f64) - want_n.astype(f64)).max()                                # every row, every component
    print("k", k, "largest eigenvalue difference relative to the largest eigenvalue", d_ev, "largest normal component difference", d_n)
    assert np.all(np.diff(ev, axis=1) >= 0) and d_ev <= EIG_TOL
    assert d_n <= NORMAL_TOL
    assert np.all(n[:, 2] > 0) and np.abs(np.linalg.norm(n.astype(f64), axis=1) - 1).max() < 1e-6
    plain = PC.estimate_normals(tgt, k=k)
    assert isinstance(plain, torch.Tensor) and plain.is_cuda and plain.dtype == torch.float32


def test_normals_orientation_modes(PC, data):
    tgt = data["tgt"]
    idx, _, cnt = ref_knn("self", tgt, tgt, 10)
    cam = (0.01, -0.02, 1.0)
    for kw in (dict(), dict(direction=(0.0, 0.0, -1.0)), dict(direction=np.array([0.3, -0.2, 1.0])), dict(camera_location=cam),
               dict(camera_location=torch.tensor([0.0, 0.0, -1.0]))):
        want, _ = K.normals_from_knn(tgt, idx, cnt, **{k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})
        got = PC.estimate_normals(tgt, k=10, **kw).cpu().numpy()
        d = np.abs(got.astype(f64) - want.astype(f64)).max()
        print(sorted(kw), "largest normal component difference", d)
        assert d <= NORMAL_TOL
    towards = PC.estimate_normals(tgt, k=10, camera_location=cam).cpu().numpy().astype(f64)
    assert np.all((towards * (np.array(cam) - tgt.astype(f64))).sum(1) > 0)
    away = PC.estimate_normals(tgt, k=10, direction=(0, 0, -1)).cpu().numpy()
    assert np.all(away[:, 2] < 0)


def test_normals_planar_lattice_and_degenerate(PC, data):
    lat = data["lattice"]
    plane = lat[lat[:, 2] == 0]
    assert len(plane) == 63
    n, ev = PC.estimate_normals(plane, k=9, return_eigenvalues=True)
    n, ev = n.cpu().numpy(), ev.cpu().numpy()
    assert np.abs(n - np.array([0, 0, 1], f32)).max() <= 1e-7 and np.all(ev[:, 0] == 0.0)
    want, want_ev = K.estimate_normals(plane, k=9)
    assert np.abs(n - want).max() <= 1e-7 and (np.abs(ev - want_ev) / want_ev[:, 2:3]).max() <= EIG_TOL
    same = np.full((10, 3), 0.25, f32)
    assert torch.count_nonzero(PC.estimate_normals(same, k=5)) == 0                       # all points identical
    assert torch.count_nonzero(PC.estimate_normals(data["tgt"][:2], k=8)) == 0             # count < 3
    assert torch.count_nonzero(PC.estimate_normals(data["tgt"], k=10, radius=1e-4)) == 0   # every point alone within the radius
    src = data["tgt"].copy()
    src[9] = np.nan
    got = PC.estimate_normals(src, k=10, direction=(0, 0, 1)).cpu().numpy()
    want, _ = K.estimate_normals(src, k=10, direction=(0, 0, 1))
    assert np.all(got[9] == 0.0) and np.isfinite(got).all() and np.abs(got.astype(f64) - want.astype(f64)).max() <= NORMAL_TOL


# ---- 6: outlier removal ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,ratio,removed", [(20, 2.0, 13), (8, 2.0, 12)])
def test_outlier_removal(PC, data, nb, ratio, removed):
    import bodyslam_amd.tsdf as TS
    pts, rows = data["planted"], data["planted_rows"]
    kept, mask, avg, thr = K.remove_statistical_outlier(pts, nb, ratio)
    assert (~mask).sum() == removed and not mask[rows].any()
    got_avg = PC.knn_mean_distance(pts, nb).cpu().numpy()
    assert same_bits(got_avg, avg)
    ind, m = PC.remove_statistical_outlier(pts, nb_neighbors=nb, std_ratio=ratio)
    assert ind.is_cuda and ind.dtype == torch.int64 and m.dtype == torch.bool and tuple(m.shape) == (len(pts),)
    assert np.array_equal(ind.cpu().numpy(), kept) and np.array_equal(m.cpu().numpy(), mask)
    ind2, _ = PC.remove_statistical_outlier(pts, nb_neighbors=nb, std_ratio=ratio, cell_size=data["h0"] * 4.0)
    assert torch.equal(ind, ind2)
    colors = np.random.default_rng(1).uniform(0, 1, pts.shape).astype(f32)
    cloud = TS.PointCloud(pts, colors, data["nrm"])
    out, i_np = cloud.remove_statistical_outlier(nb, ratio)
    assert isinstance(i_np, np.ndarray) and np.array_equal(i_np, kept)
    assert same_bits(out.points, pts[kept]) and same_bits(out.colors, colors[kept]) and same_bits(out.normals, data["nrm"][kept])
    dev = TS.PointCloud(torch.from_numpy(pts).cuda(), torch.from_numpy(colors).cuda(), None)
    out_d, i_d = dev.remove_statistical_outlier(nb, ratio)
    assert i_d.is_cuda and out_d.normals is None and same_bits(out_d.points.cpu().numpy(), pts[kept]) and same_bits(out_d.colors.cpu().numpy(), colors[kept])
    bad = pts.copy()
    bad[11] = np.nan
    _, m_bad = PC.remove_statistical_outlier(bad, nb_neighbors=nb, std_ratio=ratio)
    assert np.array_equal(m_bad.cpu().numpy(), K.remove_statistical_outlier(bad, nb, ratio)[1]) and not bool(m_bad[11])


# ---- 7: end to end: what the feature is for --------------------------------------------------------------------------------------------
def test_estimated_normals_register_point_to_plane(PC, data):
    import bodyslam_amd.evaluation as EV
    import bodyslam_amd.registration as REG
    import bodyslam_amd.tsdf as TS
    tgt, true = data["tgt"], data["true"]
    medium = I.displaced(true, I.MEDIUM)
    normals = PC.estimate_normals(tgt, k=10)
    got = REG.registration_icp(medium, tgt, I.RADIUS, estimation="point_to_plane", target_normals=normals)
    err = np.linalg.norm(I.moved(medium, got.transformation) - true, axis=1).max()
    print("estimated normals, k = 10:", got.status, got.iterations, "largest distance to the true position", err)
    assert got.status == "converged" and err <= RECOVERY_BOUND
    gt = TS.PointCloud(tgt, np.zeros_like(tgt))
    assert gt.normals is None
    n = gt.estimate_normals(k=10)
    assert isinstance(n, np.ndarray) and n is gt.normals and same_bits(n, normals.cpu().numpy())
    m = EV.evaluate_reconstruction_aligned(medium, gt, icp=dict(max_correspondence_distance=I.RADIUS, estimation="point_to_plane"))
    err = np.linalg.norm(I.moved(medium, m.alignment.transformation) - true, axis=1).max()
    print("through evaluate_reconstruction_aligned:", m.alignment.status, "largest distance to the true position", err)
    assert m.alignment.status == "converged" and err <= RECOVERY_BOUND
    dev = TS.PointCloud(torch.from_numpy(tgt).cuda(), torch.zeros(len(tgt), 3).cuda())
    nd = dev.estimate_normals(k=10)
    assert isinstance(nd, torch.Tensor) and nd.is_cuda and nd is dev.normals and torch.equal(nd, normals)
