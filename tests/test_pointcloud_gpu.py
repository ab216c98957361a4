"""Cloud-to-cloud distances on the device against the numpy statement (tests/_pointcloud_ref.py): distance and index bit for bit on every
path (grid, brute force, fallback, radius, degenerate shapes, cell faces), the statistics record, evaluate_reconstruction, and a map built
with true and with drifting poses."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pointcloud_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def bits(a):
    return np.asarray(a, dtype=f32).view(np.uint32)


def dev_pair(res):
    d, i = res
    assert d.is_cuda and i.is_cuda and d.dtype == torch.float32 and i.dtype == torch.int32 and d.shape == i.shape and d.dim() == 1
    return d.cpu().numpy(), i.cpu().numpy()


def assert_equals_statement(res, ref, what=""):
    d, i = dev_pair(res)
    wrong = np.nonzero((i != ref[0]) | (bits(d) != bits(ref[2])))[0]
    assert len(wrong) == 0, f"{what}: {len(wrong)} of {len(d)} differ, first at {wrong[0]}: device ({d[wrong[0]]!r}, {i[wrong[0]]}), statement " \
                            f"({ref[2][wrong[0]]!r}, {ref[0][wrong[0]]})"


@pytest.fixture(scope="module")
def PC():
    import bodyslam_amd.pointcloud as PC
    return PC


@pytest.fixture(scope="module")
def base():
    tgt, src = P.base_target(), P.base_source()
    return tgt, src, P.nn_brute(src, tgt)


# ---- 1: the base pair on every path -------------------------------------------------------------------------------------------------------
def test_base_pair_all_paths(PC, base):
    tgt, src, ref = base
    nn = PC.NearestNeighbours(tgt)
    h0 = nn.cell_size
    lo, hi = P.bounds(tgt)
    assert np.array_equal(nn.lo, lo) and np.array_equal(nn.hi, hi) and nn.n_finite == len(tgt) and h0 == P.default_cell_size(lo, hi, len(tgt))
    results = {"grid": nn.query(src), "brute": nn.query(src, method="brute")}
    assert nn.last_fallback == 0
    for name, factor in (("default", 1.0), ("quarter", 0.25), ("four times", 4.0)):
        results[name] = PC.point_cloud_distance(src, tgt, cell_size=h0 * factor)
    for name, res in results.items():
        assert_equals_statement(res, ref, name)
    d0, i0 = results["grid"]
    for name, (d, i) in results.items():
        assert torch.equal(d.view(torch.int32), d0.view(torch.int32)) and torch.equal(i, i0), name
    # inputs: fp64 is rounded to fp32 once; device tensors are read where they lie
    assert_equals_statement(PC.point_cloud_distance(src.astype(np.float64), tgt.astype(np.float64)), ref, "fp64")
    assert_equals_statement(PC.point_cloud_distance(torch.from_numpy(src).cuda(), torch.from_numpy(tgt)), ref, "tensors")


# ---- 2: exact ties ---------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_index(PC, base):
    tgt, src, ref = base
    tied = np.concatenate([tgt, tgt[:100]])
    rt = P.nn_brute(src, tied)
    assert np.array_equal(rt[0], ref[0])
    for method in ("grid", "brute"):
        res = PC.NearestNeighbours(tied).query(src, method=method)
        assert_equals_statement(res, rt, method)
        assert int(res[1].max()) < len(tgt)


# ---- 3: sources far outside the box: the fallback ----------------------------------------------------------------------------------------
def test_far_sources_take_the_fallback(PC, base):
    tgt, src, ref = base
    nn = PC.NearestNeighbours(tgt)
    far = (src + f32(0.5)).astype(f32)
    assert_equals_statement(nn.query(far), P.nn_brute(far, tgt), "all far")
    assert nn.last_fallback == len(far)
    mixed = np.concatenate([far[:64], src[:64]])
    assert_equals_statement(nn.query(mixed), P.nn_brute(mixed, tgt), "mixed")
    assert nn.last_fallback == 64
    # a larger target: the brute-force kernel's chunks and tiles (2806 * 5 records: 14 tiles, the last one partial)
    big = np.concatenate([tgt + f32(k * 1e-4) for k in range(5)]).astype(f32)
    nb = PC.NearestNeighbours(big)
    assert_equals_statement(nb.query(mixed), P.nn_brute(mixed, big), "mixed, 5 x target")
    assert_equals_statement(nb.query(src[:100], method="brute"), P.nn_brute(src[:100], big), "brute, 5 x target")


# ---- 4: a radius ---------------------------------------------------------------------------------------------------------------------------
def test_max_distance(PC, base):
    tgt, src, ref = base
    radius = 0.001
    assert np.abs(ref[2].astype(np.float64) - radius).min() > 1e-9          # (measured on the statement: 1.2e-7)
    rr = P.nn_brute(src, tgt, radius)
    print("fraction without a neighbour within the radius:", (rr[0] < 0).mean())
    assert 0.2 < (rr[0] < 0).mean() < 0.5
    nn = PC.NearestNeighbours(tgt)
    for method in ("grid", "brute"):
        res = nn.query(src, max_distance=radius, method=method)
        assert_equals_statement(res, rr, method)
        d, i = dev_pair(res)
        assert np.array_equal(np.isinf(d), rr[0] < 0) and np.array_equal(i == -1, rr[0] < 0)
    assert_equals_statement(PC.point_cloud_distance(src, tgt, cell_size=nn.cell_size * 0.25, max_distance=radius), rr, "quarter cells")
    far = (src[:100] + f32(0.5)).astype(f32)
    assert_equals_statement(nn.query(far, max_distance=radius), P.nn_brute(far, tgt, radius), "far, radius")


# ---- 5: degenerate shapes -------------------------------------------------------------------------------------------------------------------
def degenerate_cases(tgt, src):
    flat = tgt.copy()
    flat[:, 2] = f32(0.31)
    dirty_t = tgt[:300].copy()
    dirty_t[[3, 77], 1] = np.nan
    dirty_t[150, 0] = np.inf
    dirty_s = src[:200].copy()
    dirty_s[5, 2] = np.nan
    dirty_s[9, 0] = -np.inf
    return {"single-point target": (src[:130], tgt[:1]), "flat target": (src, flat), "all points equal": (src[:130], np.repeat(tgt[:1], 50, 0)),
            "one-point source": (src[:1], tgt), "NaN and inf rows": (dirty_s, dirty_t), "all-NaN target": (dirty_s, np.full((40, 3), np.nan, f32))}


@pytest.mark.parametrize("case", ["single-point target", "flat target", "all points equal", "one-point source", "NaN and inf rows", "all-NaN target"])
def test_degenerate_shapes(PC, base, case):
    tgt, src, ref = base
    s, t = degenerate_cases(tgt, src)[case]
    want = P.nn_brute(s, t)
    nn = PC.NearestNeighbours(t)
    for method in ("grid", "brute"):
        assert_equals_statement(nn.query(s, method=method), want, f"{case}, {method}")
    if case == "flat target":
        assert nn.dims[2] == 1
    if case == "NaN and inf rows":
        d, i = dev_pair(nn.query(s))
        assert np.isnan(d[[5, 9]]).all() and (i[[5, 9]] == -1).all() and nn.n_finite == 297
    if case == "all-NaN target":
        d, i = dev_pair(nn.query(s))
        ok = np.isfinite(s).all(1)
        assert (i == -1).all() and np.isposinf(d[ok]).all() and np.isnan(d[~ok]).all() and nn.n_finite == 0


# ---- 6: points exactly on cell faces ------------------------------------------------------------------------------------------------------
def test_points_on_cell_faces(PC):
    h = 0.125
    ax = np.arange(6) * h
    tgt = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).astype(f32)
    src = np.stack(np.meshgrid(np.arange(-1, 8) * h, np.arange(-1, 8) * h, np.arange(0, 6, 2) * h, indexing="ij"), -1).reshape(-1, 3).astype(f32)
    want = P.nn_brute(src, tgt)
    for cell in (h, h / 2, 2 * h):
        nn = PC.NearestNeighbours(tgt, cell_size=cell)
        assert nn.cell_size == cell
        assert_equals_statement(nn.query(src), want, f"cell {cell}")


# ---- 7: statistics -----------------------------------------------------------------------------------------------------------------------------
def check_record(rec, want, taus):
    """counts, max and median exactly; sums within 1e-12 relative (n <= 4096 terms of one sign in fp64: n 2^-53 < 5e-13)"""
    print("device", rec.tolist(), "statement", want)
    assert (rec[0], rec[1], rec[2], rec[3]) == (want["n"], want["n_finite"], want["n_unmatched"], want["n_nan"])
    assert list(rec[8:8 + len(taus)]) == want["counts"] and not rec[8 + len(taus):].any()
    if want["n_finite"]:
        assert rec[6] == want["max"] and rec[7] == want["median"]
        assert abs(rec[4] - want["sum"]) <= 1e-12 * want["sum"] and abs(rec[5] - want["sumsq"]) <= 1e-12 * want["sumsq"]
    else:
        assert np.isnan(rec[6]) and np.isnan(rec[7]) and rec[4] == 0 and rec[5] == 0


@pytest.mark.parametrize("case", ["odd", "even", "holes", "unaligned", "tiny", "nothing finite"])
def test_statistics(base, case):
    from bodyslam_amd.evaluation import distance_stats_record
    tgt, src, ref = base
    assert len(src) <= 4096
    d = ref[2].copy()                                                       # 1937 distances: an odd count
    if case == "even":
        d = d[:-1]
    elif case == "holes":
        d[::7] = np.inf
        d[3::11] = np.nan
    elif case == "tiny":
        d = d[:2]
    elif case == "nothing finite":
        d = np.array([np.inf, np.nan, np.inf], f32)
    taus = (0.0005, 0.001, float(np.median(d[np.isfinite(d)])) if np.isfinite(d).any() else 1.0, 10.0)
    t = torch.from_numpy(d).cuda()
    if case == "unaligned":
        t = torch.from_numpy(np.concatenate([[f32(0)], d])).cuda()[1:]      # 4 bytes past a 16-byte boundary: the element-load path
        assert t.data_ptr() % 16 == 4
    rec = distance_stats_record(t, taus)
    check_record(rec, P.stats(d, taus), taus)
    again = distance_stats_record(t, taus)
    assert np.array_equal(rec.view(np.uint64), again.view(np.uint64))
    if case == "unaligned":
        assert np.array_equal(rec.view(np.uint64), distance_stats_record(torch.from_numpy(d).cuda(), taus).view(np.uint64))


# ---- 8: evaluate_reconstruction -----------------------------------------------------------------------------------------------------------
def check_metrics(got, want, taus):
    print(got.as_dict())
    for side in ("accuracy", "completeness"):
        g, w = getattr(got, side), want[side]
        assert g.max == w["max"] and g.median == w["median"]
        assert abs(g.mean - w["mean"]) <= 1e-12 * w["mean"] and abs(g.rmse - w["rmse"]) <= 1e-12 * w["rmse"]
    assert abs(got.chamfer - want["chamfer"]) <= 1e-12 * want["chamfer"]
    assert np.array_equal(got.precision, want["precision"]) and np.array_equal(got.recall, want["recall"])
    assert np.allclose(got.fscore, want["fscore"], rtol=1e-15, atol=0)
    assert (got.n_pred, got.n_gt, got.n_unmatched_pred, got.n_unmatched_gt) == (want["n_pred"], want["n_gt"], want["n_unmatched_pred"],
                                                                                 want["n_unmatched_gt"])
    assert got.thresholds == tuple(float(f32(t)) for t in taus)


def test_evaluate_reconstruction(PC, base, tmp_path):
    import bodyslam_amd.evaluation as EV
    from bodyslam_amd.tsdf import PointCloud, TriangleMesh
    tgt, src, ref = base
    taus = (0.0005, 0.001, 0.002)
    got = EV.evaluate_reconstruction(src, tgt, thresholds=taus)
    check_metrics(got, P.metrics(src, tgt, taus), taus)
    again = EV.evaluate_reconstruction(src, tgt, thresholds=taus)
    assert got.as_dict() == again.as_dict()                                 # (floats compare by value: the same bits, no NaN here)
    # a similarity: the source scaled down and turned, brought back by (R, s, t); and the same as a 4 x 4
    a = 0.3
    Rm = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    s, t = 1.04, np.array([0.01, -0.02, 0.005])
    away = ((src.astype(np.float64) - t) @ Rm / s)                          # fp64 points: R^T (p - t) / s
    for transform in ((Rm, s, t), np.vstack([np.concatenate([s * Rm, t[:, None]], 1), [0, 0, 0, 1]])):
        want = P.metrics(away, tgt, taus, transform=transform)
        assert want["accuracy"]["mean"] < 1.001 * P.metrics(src, tgt, taus)["accuracy"]["mean"]
        check_metrics(EV.evaluate_reconstruction(away, tgt, thresholds=taus, transform=transform), want, taus)
        moved = PC.transform_points(away, transform)
        assert np.array_equal(bits(moved.cpu().numpy()), bits(P.apply_transform(away, transform)))
    # a radius: unmatched points both ways
    want = P.metrics(src, tgt, taus, max_distance=0.001)
    assert want["n_unmatched_pred"] > 100 and want["n_unmatched_gt"] > 100
    check_metrics(EV.evaluate_reconstruction(src, tgt, thresholds=taus, max_distance=0.001), want, taus)
    # Open3D's method on the dataclass, and a mesh's vertices as the cloud
    pc_s, pc_t = PointCloud(src, np.zeros_like(src)), PointCloud(tgt, np.zeros_like(tgt))
    d = pc_s.compute_point_cloud_distance(pc_t)
    assert d.dtype == np.float64 and np.array_equal(d, ref[2].astype(np.float64))
    mesh = TriangleMesh(tgt, np.zeros_like(tgt), np.zeros((1, 3), np.int32))
    assert_equals_statement(PC.point_cloud_distance(pc_s, mesh), ref, "PointCloud against TriangleMesh")
    assert EV.evaluate_reconstruction(pc_s, mesh, thresholds=taus).as_dict() == got.as_dict()
    path = got.write_csv(str(tmp_path / "reconstruction.csv"))
    rows = open(path).read().splitlines()
    assert rows[0] == "Metric,Value" and rows[1].startswith("accuracy_mean,") and len(rows) == 1 + len(got.as_dict())


# ---- 9: end to end on a map ---------------------------------------------------------------------------------------------------------------
# Eight 64 x 48 renderings of tests/_render.py's height field, voxels of 2 mm, integrated with the true poses and with poses that drift by
# three voxel lengths per frame; both maps against 6 000 samples of the true surface, tau = 2 voxels.
# CPU precheck (oracle/tsdf_ref.py's TSDFRef for the points, the statement for the metrics):
#   true poses       25 374 points, accuracy mean 2.2548e-03, completeness mean 1.5089e-03, chamfer 1.8818e-03, F-score 0.9265
#   drifting poses   28 432 points, accuracy mean 6.4168e-03, completeness mean 4.0475e-03, chamfer 5.2322e-03, F-score 0.4208
#   the accuracy means differ by a factor of 2.85 (at least 2 is asked for before the ordering is relied upon)
# MEASURED on the device (MI355X), the same two maps through TSDF.build_3D_map and evaluate_reconstruction -- the point counts are the
# oracle's, the means agree with the precheck to eight digits; the test asserts the ordering only, no absolute number:
MEASURED = {"true": dict(n_pred=25374, accuracy_mean=2.254753e-03, completeness_mean=1.508853e-03, chamfer=1.881803e-03, fscore=0.926529),
            "drift": dict(n_pred=28432, accuracy_mean=6.416834e-03, completeness_mean=4.047519e-03, chamfer=5.232177e-03, fscore=0.420838)}


def assert_same_cloud(host, dev):
    """extract_pcd() and extract_pcd(host=False) hold the same rows (point | colour | normal, 36 bytes) bit for bit.  The rows of one
    volume unit come out in the order its extraction atomics gave, which differs from call to call, so the rows are compared sorted."""
    rows = []
    for pcd in (host, dev):
        for name in ("points", "colors", "normals"):
            v = getattr(pcd, name)
            assert (isinstance(v, np.ndarray) if pcd is host else isinstance(v, torch.Tensor) and v.is_cuda) and v.dtype in (np.float32, torch.float32)
        r = np.concatenate([bits(v if pcd is host else v.cpu().numpy()) for v in (pcd.points, pcd.colors, pcd.normals)], 1)
        assert r.shape == (len(host.points), 9)
        rows.append(r[np.lexsort(r.T[::-1])])
    assert np.array_equal(rows[0], rows[1])


def assert_same_metrics(a, b):
    """two evaluations of one cloud whose rows are ordered differently: counts, max and median exactly; each fp64 sum of n terms of one
    sign is within n 2^-53 relative of the true sum, so two orders differ by at most n 2^-52"""
    tol = max(a.n_pred, a.n_gt) * 2.0 ** -52
    for side in ("accuracy", "completeness"):
        x, y = getattr(a, side), getattr(b, side)
        assert x.max == y.max and x.median == y.median and abs(x.mean - y.mean) <= tol * y.mean and abs(x.rmse - y.rmse) <= tol * y.rmse
    assert abs(a.chamfer - b.chamfer) <= tol * b.chamfer
    assert np.array_equal(a.precision, b.precision) and np.array_equal(a.recall, b.recall) and np.allclose(a.fscore, b.fscore, rtol=1e-15, atol=0)
    assert (a.n_pred, a.n_gt, a.n_unmatched_pred, a.n_unmatched_gt) == (b.n_pred, b.n_gt, b.n_unmatched_pred, b.n_unmatched_gt)


def test_map_with_true_poses_beats_drifting_poses(PC):
    import bodyslam_amd.evaluation as EV
    from bodyslam_amd.tsdf import MAP, TSDF, PinholeCameraIntrinsic, RGBDImage
    frames = P.map_frames()
    gt = P.map_gt_samples()
    intr = PinholeCameraIntrinsic(P.MAP_W, P.MAP_H, *P.MAP_K)
    tau = 2.0 * P.MAP_VL
    out = {}
    for drift in (False, True):
        m = TSDF(P.MAP_VL, P.MAP_TRUNC, volume_unit_resolution=P.MAP_RES, depth_sampling_stride=P.MAP_STRIDE, slab_bytes=1 << 24, max_units=8192)
        for (col, dep, _), E in zip(frames, P.map_extrinsics(frames, drift)):
            m.build_3D_map(RGBDImage(col, dep), intr, E)
        host, dev = m.extract_pcd(), m.extract_pcd(host=False)
        assert_same_cloud(host, dev)
        res = EV.evaluate_reconstruction(m, gt, thresholds=(tau,))
        assert res.n_pred == len(host.points) and res.n_gt == len(gt)
        assert_same_metrics(res, EV.evaluate_reconstruction(host, gt, thresholds=(tau,)))
        print("drift" if drift else "true ", res.as_dict())
        out[drift] = res
    good, bad = out[False], out[True]
    assert good.accuracy.mean < bad.accuracy.mean and good.chamfer < bad.chamfer and good.fscore[0] > bad.fscore[0]
    # the reference's second map class hands the flag through
    mp = MAP(P.MAP_W, P.MAP_H, intr, 0, 1000.0, voxel_size=P.MAP_VL, block_count=4096)
    mp.integrate(RGBDImage(frames[0][0], frames[0][1]), 0, frames[0][2])
    host, dev = mp.extract_pcd(), mp.extract_pcd(host=False)
    assert len(host.points) > 1000
    assert_same_cloud(host, dev)
    assert_same_metrics(EV.evaluate_reconstruction(mp, gt, thresholds=(tau,)), EV.evaluate_reconstruction(host, gt, thresholds=(tau,)))
