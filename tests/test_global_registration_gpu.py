"""Global registration on the device against the numpy statement (tests/_global_registration_ref.py), stage by stage, each stage fed with the
device's previous one where the stages chain: SPFH counts, FPFH rows, the feature match, RANSAC over planted correspondences, and the
recipe end to end with the reconstruction evaluation that uses it.  Integers are compared exactly, under the condition that
_global_registration_ref.assert_clear states and every test here that has a threshold asserts on its own input (the feature match has none:
its distances are fp32 sums in one order on both sides, its ties exact); the entry points one
at a time, at their edges and on their thresholds: tests/test_global_registration_stages_gpu.py."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _global_registration_ref as G  # noqa: E402
import _icp_ref as I  # noqa: E402
from test_global_registration_cpu import MEASURED, RECIPE_SEED, TAU, VOXEL  # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
T_TOL = 1e-9                     # tests/test_loop_closure_gpu.py: Jacobi against LAPACK and another order of the fp64 sums
RECOVERY_BOUND = 5e-5            # tests/test_icp_gpu.py holds its aligned evaluation to this
E2E_ITERATIONS = 16384           # four chunks: bounds the runs that cannot succeed (mirrored or flipped features)


@pytest.fixture(scope="module")
def REG():
    import bodyslam_amd.registration as REG
    return REG


@functools.lru_cache(maxsize=None)
def pair(name):
    return G.bumpy_pair(G.POSE_50 if name == "50" else G.POSE_170)


@functools.lru_cache(maxsize=None)
def statement(radius, max_nn):
    """the statement's lists, counts and k of the bumpy target, computed once"""
    tgt, tn = I.bumpy_target()
    ls = G.lists(tgt, radius, max_nn)
    counts, k, margins = G.spfh(tgt, tn, *ls)
    G.assert_clear(margins)
    return ls, counts, k


@functools.lru_cache(maxsize=None)
def device(radius, max_nn, cell):
    import bodyslam_amd.registration as REG
    tgt, tn = I.bumpy_target()
    f, s = REG._fpfh(tgt, tn, radius, max_nn, cell, 0)
    return f.cpu().numpy(), s.cpu().numpy()


def cells(radius):
    return (None, radius / 4.0, 4.0 * radius, 1.0)                        # the default, finer, coarser, one cell for the whole cloud


def split_spfh(s):
    assert s.shape[1] == 36 and not s[:, 34:].any()
    return s[:, :33].astype(np.int64), s[:, 33].astype(np.int64)


# ---- 5: SPFH --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_nn", [None, 100, 16])
@pytest.mark.parametrize("radius", [0.010, 0.004])
def test_spfh_counts_are_the_statements(radius, max_nn):
    ls, counts, k = statement(radius, max_nn)
    assert len(k) == 2806 == 10 * 256 + 246                               # eleven blocks of 256 rows' worth of waves, the last one partial
    for cell in cells(radius):
        got, gk = split_spfh(device(radius, max_nn, cell)[1])
        assert np.array_equal(gk, k) and np.array_equal(got, counts), (radius, max_nn, cell)
    print(radius, max_nn, "pairs counted", int(k.sum()), "rows", int(np.diff(ls[0]).min()), "..", int(np.diff(ls[0]).max()))


def test_spfh_constructed_rows(REG):
    pts, nrm, rows = G.constructed_cloud()
    r = G.CONSTRUCTED_RADIUS
    for max_nn in (None, 100):
        want = G.compute_fpfh(pts, nrm, r, max_nn)
        G.assert_clear(want["margins"])
        for cell in (None, r / 4.0):
            f, s = REG._fpfh(pts, nrm, r, max_nn, cell, 0)
            got, gk = split_spfh(s.cpu().numpy())
            assert np.array_equal(gk, want["k"]) and np.array_equal(got, want["counts"])
            assert np.array_equal(f.cpu().numpy().view(np.uint32), want["features"].view(np.uint32))
    k = want["k"]
    assert k[rows["alone"]] == 0 and k[rows["twins"]:rows["twins"] + 3].tolist() == [1, 1, 2]
    assert k[rows["normals"]:rows["normals"] + 5].tolist() == [0, 0, 2, 2, 2] and k[rows["nan"]:rows["nan"] + 3].tolist() == [0, 1, 1]
    assert (k[rows["k63"]:rows["k64"]] == 63).all() and (k[rows["k64"]:rows["k65"]] == 64).all() and (k[rows["k65"]:rows["along"]] == 65).all()
    assert k[rows["along"]:rows["along"] + 3].tolist() == [1, 1, 2]
    zero = np.nonzero(k == 0)[0]
    assert len(zero) == 4 and not f.cpu().numpy()[zero].any()


# ---- 6: FPFH --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_nn", [None, 100, 16])
@pytest.mark.parametrize("radius", [0.010, 0.004])
def test_fpfh_rows_are_the_statements_bit_for_bit(radius, max_nn):
    """the statement restates the order of the sums exactly (lane partials, the xor butterfly, the symmetric block sum): bit equality"""
    ls, _, _ = statement(radius, max_nn)
    f0, s0 = device(radius, max_nn, None)
    want, _ = G.fpfh_from_spfh(*split_spfh(s0), *ls)                         # from the device's own SPFH
    assert np.array_equal(f0.view(np.uint32), want.view(np.uint32))
    for cell in cells(radius)[1:]:
        assert np.array_equal(device(radius, max_nn, cell)[0].view(np.uint32), f0.view(np.uint32))


def test_fpfh_repeats_chunks_and_the_method(REG, monkeypatch):
    import bodyslam_amd.tsdf as TS
    tgt, tn = I.bumpy_target()
    f0 = device(0.010, 100, None)[0]
    again = REG.compute_fpfh_feature(tgt, tn, 0.010).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), f0.view(np.uint32))         # two calls, the same bits
    monkeypatch.setattr(REG, "LIST_BUDGET", 50000)                           # several source chunks: the lists are queried again for the second pass
    chunked = REG.compute_fpfh_feature(tgt, tn, 0.010).cpu().numpy()
    assert np.array_equal(chunked.view(np.uint32), f0.view(np.uint32))
    monkeypatch.undo()
    m = TS.PointCloud(tgt, np.zeros_like(tgt), tn).compute_fpfh_feature(0.010)
    assert isinstance(m, np.ndarray) and np.array_equal(m.view(np.uint32), f0.view(np.uint32))
    bad = tgt.copy()
    bad[7] = np.nan                                                          # a non-finite point: a zero row, and nobody's neighbour
    fb = REG.compute_fpfh_feature(bad, tn, 0.010).cpu().numpy()
    want = G.compute_fpfh(bad, tn, 0.010)
    G.assert_clear(want["margins"])
    want = want["features"]
    assert not fb[7].any() and np.array_equal(fb.view(np.uint32), want.view(np.uint32))
    fm = REG.mirror_fpfh(REG.compute_fpfh_feature(tgt, tn, 0.010))
    fn = REG.compute_fpfh_feature(tgt, -tn, 0.010)
    assert np.array_equal(fm.cpu().numpy().view(np.uint32), fn.cpu().numpy().view(np.uint32))


# ---- 7: matching ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_features(name):
    """the device's features of the pair: (source [1937, 33], target [2806, 33]) as numpy"""
    import bodyslam_amd.registration as REG
    p = pair(name)
    r = 0.010 if name == "50" else 0.008
    return REG.compute_fpfh_feature(p["src"], p["sn"], r).cpu().numpy(), REG.compute_fpfh_feature(p["tgt"], p["tn"], r).cpu().numpy()


def check_match(REG, s, t, splits=(None, 1, 3)):
    for mutual in (False, True):
        want = G.match_features(s, t, mutual)[0]
        for sp in splits:
            got = REG.match_features(s, t, mutual, _splits=sp)
            assert got.dtype == __import__("torch").int32 and got.is_cuda and np.array_equal(got.cpu().numpy(), want), (mutual, sp)
    return want


def test_match_on_the_pair(REG):
    s, t = pair_features("50")
    want = check_match(REG, s, t, splits=(None, 1, 7))
    assert len(want) == 750                                                   # the mutual matches of the last call
    assert np.array_equal(REG.match_features(t, s).cpu().numpy(), G.match_features(t, s)[0])


@pytest.mark.parametrize("m,n", [(255, 63), (256, 64), (257, 65), (1, 1), (300, 1), (3, 200)])
def test_match_constructed(REG, m, n):
    rng = np.random.default_rng(100 * m + n)
    t = rng.integers(0, 50, (n, 33)).astype(f32)                             # small integers: many exact ties in the distance
    s = rng.integers(0, 50, (m, 33)).astype(f32)
    if n >= 63:
        t[40] = t[12]                                                         # a duplicated target row: the tie goes to the lower index
        s[0] = t[40]
        t[n - 1, 3] = np.nan
        t[5, 32] = np.inf
    if m >= 255:
        s[m - 1, 0] = np.nan
        s[17, 32] = -np.inf
    want = check_match(REG, s, t)
    fwd = G.match_features(s, t)[1]
    if n >= 63:
        assert fwd[0] == 12 and not np.isin(fwd, [n - 1, 5]).any()
    if m >= 255:
        assert fwd[m - 1] == -1 and fwd[17] == -1 and not np.isin(want[:, 0], [m - 1, 17]).any()


def test_match_empty_and_all_nan(REG):
    t = np.random.default_rng(1).uniform(0, 1, (5, 33)).astype(f32)
    for a, b in ((np.zeros((0, 33), f32), t), (t, np.zeros((0, 33), f32)), (np.full((4, 33), np.nan, f32), t), (t, np.full((4, 33), np.nan, f32))):
        for mutual in (False, True):
            got = REG.match_features(a, b, mutual)
            assert tuple(got.shape) == (0, 2) and got.is_cuda


# ---- 8: RANSAC on planted correspondences ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_total,max_iteration", [(1000, 100000), (5000, 20000)])
def test_ransac_on_planted_correspondences(REG, monkeypatch, n_total, max_iteration):
    p = pair("50")
    cr = G.planted(p, 300, n_total, 5)
    want = G.ransac(p["src"].astype(f64)[cr[:, 0]], p["tgt"].astype(f64)[cr[:, 1]], TAU, max_iteration=max_iteration)
    G.assert_clear(want["margin"])
    monkeypatch.setattr(REG, "keep_tables", True)
    got = REG.registration_ransac_based_on_correspondence(p["src"], p["tgt"], cr, TAU, max_iteration=max_iteration)
    valid = np.concatenate([v for v, _ in REG.last_tables])
    scores = np.concatenate([s for _, s in REG.last_tables])
    print(n_total, got.status, "h", got.h, "inliers", got.inliers, "hypotheses", got.hypotheses, "valid", int(valid.sum()), "dT",
          np.abs(got.transformation - want["T"]).max(), "rmse", got.inlier_rmse, want["rmse"])
    assert len(REG.last_tables) == want["chunks"] and got.hypotheses == want["hypotheses"] and got.status == want["status"]
    assert np.array_equal(valid, want["valid"]) and np.array_equal(scores, want["scores"])
    assert got.h == want["h"] and np.array_equal(got.inlier_mask.cpu().numpy(), want["mask"]) and got.inliers == want["inliers"]
    assert np.abs(got.transformation - want["T"]).max() <= T_TOL and abs(got.inlier_rmse - want["rmse"]) <= T_TOL
    assert got.fitness == want["inliers"] / n_total and np.array_equal(got.correspondences.cpu().numpy(), cr)
    assert isinstance(got, REG.RegistrationResult)
    again = REG.registration_ransac_based_on_correspondence(p["src"], p["tgt"], cr, TAU, max_iteration=max_iteration)
    assert np.array_equal(again.transformation, got.transformation) and again.inlier_rmse == got.inlier_rmse and again.h == got.h


def test_ransac_degenerate(REG):
    p = pair("50")
    two = REG.registration_ransac_based_on_correspondence(p["src"], p["tgt"], np.array([[0, 0], [1, 1]], np.int32), TAU)
    line = np.stack([np.arange(50.0) * 0.001, np.zeros(50), np.zeros(50)], 1)
    cr = np.stack([np.arange(50), np.arange(50)], 1).astype(np.int32)
    col = REG.registration_ransac_based_on_correspondence(line, line + 0.1, cr, TAU, max_iteration=4096)
    none = REG.registration_ransac_based_on_correspondence(p["src"], p["tgt"], np.zeros((0, 2), np.int32), TAU)
    for r, c in ((two, 2), (col, 50), (none, 0)):
        assert r.status == "degenerate" and r.h == -1 and np.array_equal(r.transformation, np.eye(4)) and r.fitness == 0.0 and r.inlier_rmse == 0.0
        assert tuple(r.inlier_mask.shape) == (c,) and not r.inlier_mask.any() and r.inliers == 0
    assert col.hypotheses == 4096 and two.hypotheses == 0


def test_ransac_on_feature_matching(REG):
    p = pair("170")
    s, t = pair_features("170")
    want, corres = G.ransac_on_features(p["src"], p["tgt"], s, t, False, TAU, max_iteration=4096)
    G.assert_clear(want["margin"])
    got = REG.registration_ransac_based_on_feature_matching(p["src"], p["tgt"], s, t, False, TAU, max_iteration=4096)
    assert np.array_equal(got.correspondences.cpu().numpy(), corres) and got.h == want["h"] == MEASURED["raw_170"]["h"]
    assert got.inliers == want["inliers"] == MEASURED["raw_170"]["inliers"] and np.abs(got.transformation - want["T"]).max() <= T_TOL


# ---- 9: end to end ----------------------------------------------------------------------------------------------------------------------------------
def errors(p, T, pose):
    return float(np.linalg.norm(I.moved(p["src"], T) - p["true"], axis=1).max()), G.rotation_error_degrees(T, pose)


@pytest.mark.parametrize("name", ["50", "170"])
def test_registration_global(REG, name):
    import bodyslam_amd.pointcloud as PC
    p, pose = pair(name), (G.POSE_50 if name == "50" else G.POSE_170)
    kw = dict(seed=RECIPE_SEED[name], max_iteration=E2E_ITERATIONS)
    got = REG.registration_global(p["src"], p["tgt"], VOXEL, source_normals=p["sn"], target_normals=p["tn"], **kw)
    a = PC.voxel_down_sample(p["src"], VOXEL, normals=p["sn"], unit_normals=True)          # the statement on the device's thinned clouds
    b = PC.voxel_down_sample(p["tgt"], VOXEL, normals=p["tn"], unit_normals=True)
    want, corres, mirrored = G.recipe_on_thinned(*(x.cpu().numpy() for x in (a.points, a.normals, b.points, b.normals)), VOXEL, "given", **kw)
    G.assert_clear(want["margin"])
    err, rot = errors(p, got.transformation, pose)
    m = MEASURED[f"recipe_{name}"]
    print(name, got.status, "h", got.h, "inliers", got.inliers, "of", len(corres), "err", err, "rot", rot)
    assert REG.last_global is got and got.status == "converged"
    assert err <= 1.5 * m["err"] and rot <= 1.5 * m["rot"]
    assert got.h == want["h"] == m["h"] and got.inliers == want["inliers"] == m["inliers"]
    assert np.array_equal(got.correspondences.cpu().numpy(), corres) and np.abs(got.transformation - want["T"]).max() <= T_TOL
    # the source normals negated: "either" finds the same inliers through the mirrored features, "given" finds next to nothing
    either = REG.registration_global(p["src"], p["tgt"], VOXEL, source_normals=-p["sn"], target_normals=p["tn"], normal_sign="either", **kw)
    given = REG.registration_global(p["src"], p["tgt"], VOXEL, source_normals=-p["sn"], target_normals=p["tn"], normal_sign="given", **kw)
    print("flipped: either", either.inliers, "given", given.inliers)
    assert either.inliers == got.inliers and either.h == got.h and 5 * given.inliers < got.inliers


def test_evaluation_with_a_global_alignment(REG):
    import bodyslam_amd.evaluation as EV
    import bodyslam_amd.tsdf as TS
    p = pair("50")
    gt = TS.PointCloud(p["tgt"], np.zeros_like(p["tgt"]), p["tn"])
    moved = TS.PointCloud(p["src"], np.zeros_like(p["src"]), p["sn"])
    best = EV.evaluate_reconstruction(p["true"].astype(f32), gt)                            # the source where it belongs
    got = EV.evaluate_reconstruction_aligned(moved, gt, align="global", icp=dict(max_correspondence_distance=0.005, voxel_size=0.002))
    err = np.linalg.norm(I.moved(p["src"], got.alignment.transformation) - p["true"], axis=1).max()
    print("accuracy mean: in place", best.accuracy.mean, "global + icp", got.accuracy.mean, "largest distance to the true place", err, "global h",
          REG.last_global.h, "inliers", REG.last_global.inliers)
    assert got.alignment.status == "converged" and not isinstance(got.alignment, REG.GlobalRegistrationResult)
    assert abs(got.accuracy.mean - best.accuracy.mean) <= RECOVERY_BOUND and err <= RECOVERY_BOUND
    assert REG.last_global.h == MEASURED["recipe_50"]["h"] and REG.last_global.inliers == MEASURED["recipe_50"]["inliers"]
    surf = EV.evaluate_reconstruction_surface(moved, gt, align="global", icp=dict(max_correspondence_distance=0.005, voxel_size=0.002), gt_mesh="vertices")
    assert surf.accuracy.mean == got.accuracy.mean and np.array_equal(surf.alignment.transformation, got.alignment.transformation)
    # what the feature adds: ICP from the identity does not get there from this pose
    icp = EV.evaluate_reconstruction_aligned(moved, gt, align="icp", icp=dict(max_correspondence_distance=0.005, voxel_size=0.002))
    print("icp from the identity:", icp.alignment.status, "accuracy mean", icp.accuracy.mean)
    assert not abs(icp.accuracy.mean - best.accuracy.mean) <= RECOVERY_BOUND
