"""Global registration without a GPU: the numpy statement (tests/_global_registration_ref.py) recovers the pose of the bumpy pair, every
discrete decision of the clouds the GPU tests use lies away from its threshold, the closed forms, the public signatures, the argument
checks before any device call, and no CPU fallback."""
import functools
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _global_registration_ref as G  # noqa: E402
import _icp_ref as I  # noqa: E402
import _voxel_ref as V  # noqa: E402

f32, f64 = np.float32, np.float64
MARGIN = 1e-10
POSES = {"50": (G.POSE_50, 0.010, 0), "170": (G.POSE_170, 0.008, 0)}      # pose, feature radius of the raw runs, seed
RECIPE_SEED = {"50": 0, "170": 1}                                          # (170 degrees, seed 0: two hypotheses share the best score -- replaced, not tolerated)
TAU, VOXEL = 0.004, 0.002
# What the statement itself reaches, measured 2026-10-21 (the largest distance of a moved source point from its true place in m, the rotation
# error in degrees, the inliers, the winner).  raw: the 1 937 x 2 806 pair with analytic normals, nearest-feature correspondences (no mutual
# filter), tau = 4 mm, 4 096 hypotheses.  recipe: registration_global's steps at voxel_size = 2 mm (thinned clouds, features at 10 mm, mutual
# matches, tau = 3 mm).  The issue's prototype measured 0.66 mm / 0.57 deg and 0.84 mm / 0.53 deg with another draw function.
MEASURED = {
    "raw_50": dict(err=5.450e-04, rot=0.4798, inliers=489, h=3520), "raw_170": dict(err=3.307e-04, rot=0.1275, inliers=344, h=2817),
    "recipe_50": dict(err=7.005e-04, rot=0.4433, inliers=156, h=487), "recipe_170": dict(err=2.152e-04, rot=0.1232, inliers=172, h=3295),
}
TRUE_BOUND = 0.002                                                        # the issue's bound: about 2.5 x the prototype's 0.84 mm, because the draws differ


@functools.lru_cache(maxsize=None)
def pair(name):
    return G.bumpy_pair(POSES[name][0])


@functools.lru_cache(maxsize=None)
def features(name, which):
    p = pair(name)
    return G.compute_fpfh(p["src"], p["sn"], POSES[name][1]) if which == "src" else G.compute_fpfh(p["tgt"], p["tn"], POSES[name][1])


def errors(p, T, pose):
    return float(np.linalg.norm(I.moved(p["src"], T) - p["true"], axis=1).max()), G.rotation_error_degrees(T, pose)


# ---- 1: the statement recovers the pose -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["50", "170"])
def test_statement_recovers_the_pose(name):
    p, pose = pair(name), POSES[name][0]
    r, corres = G.ransac_on_features(p["src"], p["tgt"], features(name, "src")["features"], features(name, "tgt")["features"], False, TAU,
                                     max_iteration=4096, seed=0)
    err, rot = errors(p, r["T"], pose)
    true = np.linalg.norm(p["true"][corres[:, 0]] - p["tgt"].astype(f64)[corres[:, 1]], axis=1) < 0.005
    print(name, "correspondences", len(corres), "true", true.mean(), "valid", int(r["valid"].sum()), "h", r["h"], "inliers", r["inliers"], "err", err, "rot",
          rot, "margin", r["margin"], "unique", r["unique"], r["status"])
    m = MEASURED[f"raw_{name}"]
    assert len(corres) == len(p["src"]) and r["hypotheses"] == 4096
    assert err <= TRUE_BOUND
    assert r["inliers"] == m["inliers"] and r["h"] == m["h"] and err <= 1.001 * m["err"] and rot <= 1.001 * m["rot"]
    assert r["margin"] >= MARGIN and r["unique"]


@pytest.mark.parametrize("name", ["50", "170"])
def test_recipe_statement(name):
    p, pose = pair(name), POSES[name][0]
    r, corres, mirrored = G.recipe(p, VOXEL, "either", seed=RECIPE_SEED[name])
    err, rot = errors(p, r["T"], pose)
    print(name, "correspondences", len(corres), "h", r["h"], "inliers", r["inliers"], "err", err, "rot", rot, "margin", r["margin"], r["unique"])
    m = MEASURED[f"recipe_{name}"]
    assert not mirrored and err <= TRUE_BOUND
    assert r["inliers"] == m["inliers"] and r["h"] == m["h"] and err <= 1.001 * m["err"] and rot <= 1.001 * m["rot"]
    assert r["margin"] >= MARGIN and r["unique"]
    # the source normals negated: "either" finds the same result through the mirrored features, bit for bit
    f, cf, mf = G.recipe(p, VOXEL, "either", flip_source=True, seed=RECIPE_SEED[name])
    assert mf and f["h"] == r["h"] and f["inliers"] == r["inliers"] and np.array_equal(f["T"], r["T"]) and np.array_equal(cf, corres)


# ---- 2: margins of every cloud the GPU tests use ------------------------------------------------------------------------------------------------
def check_margins(m, what):
    print(what, m)
    assert min(m.values()) >= MARGIN, (what, m)


def test_feature_margins():
    tgt, tn = I.bumpy_target()
    for r in (0.010, 0.004):
        check_margins(G.spfh(tgt, tn, *G.lists(tgt, r))[2], f"target at {r}")         # (max_nn keeps a subset of these pairs)
    for name in POSES:
        check_margins(features(name, "src")["margins"], f"source {name}")
        p = pair(name)
        for cloud, nrm in ((p["src"], p["sn"]), (p["tgt"], p["tn"])):
            t = V.voxel_down_sample(cloud, VOXEL, normals=nrm, unit_normals=True)
            check_margins(G.compute_fpfh(t["points"], t["normals"], 5.0 * VOXEL)["margins"], f"thinned {name}")
    pts, nrm, _ = G.constructed_cloud()
    check_margins(G.compute_fpfh(pts, nrm, G.CONSTRUCTED_RADIUS, None)["margins"], "constructed")


@pytest.mark.parametrize("n_total,max_iteration", [(1000, 100000), (5000, 20000)])
def test_planted_margins(n_total, max_iteration):
    p = pair("50")
    cr = G.planted(p, 300, n_total, 5)
    r = G.ransac(p["src"].astype(f64)[cr[:, 0]], p["tgt"].astype(f64)[cr[:, 1]], TAU, max_iteration=max_iteration)
    print(n_total, r["status"], "h", r["h"], "inliers", r["inliers"], "hypotheses", r["hypotheses"], "chunks", r["chunks"], "valid", int(r["valid"].sum()),
          "margin", r["margin"], r["unique"])
    assert r["margin"] >= MARGIN and r["unique"] and r["inliers"] >= 250
    assert (r["chunks"] == 1 and r["status"] == "converged") if n_total == 1000 else (r["chunks"] == 5 and r["hypotheses"] == 20000)


def test_sector_is_the_atan2_bin():
    f = features("50", "tgt")
    rs, idx, d2 = f["lists"]
    tgt, tn = I.bumpy_target()
    rows = np.repeat(np.arange(len(tgt)), np.diff(rs))
    keep = d2 != 0
    P, N = tgt.astype(f64), tn.astype(f64)
    pf = G.pair_features(P[rows[keep]], N[rows[keep]], P[idx[keep]], N[idx[keep]])
    c = pf["counted"]
    assert c.sum() > 100000 and np.array_equal(pf["bins"][c, 0], G.sector_atan2(pf["xy"][c, 0], pf["xy"][c, 1]))
    th = np.linspace(-np.pi, np.pi, 100001)[1:-1]
    assert np.array_equal(G.sector(np.cos(th), np.sin(th)), G.sector_atan2(np.cos(th), np.sin(th)))
    assert G.sector(np.array([1.0, -1.0, -1.0]), np.array([0.0, 0.0, -1e-300])).tolist() == [5, 10, 0]


def test_the_draw_is_loop_closures():
    import _loop_closure_ref as LC
    ids = [LC.sample(7, 0, h, 10) for h in range(200)]
    assert all(len(set(i)) == 3 and max(i) < 10 for i in ids) and len(set(ids)) > 100


# ---- 3: closed forms ----------------------------------------------------------------------------------------------------------------------------
def test_plane_with_parallel_normals():
    x, y = np.meshgrid(np.arange(12) * 0.002, np.arange(9) * 0.002, indexing="ij")
    pts = np.stack([x.ravel(), y.ravel(), np.full(x.size, 0.3)], 1).astype(f32)
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], f32), (len(pts), 1))
    r = G.compute_fpfh(pts, nrm, 0.005)
    centre = np.zeros(33, bool)
    centre[[5, 16, 27]] = True
    assert (r["k"] > 0).all() and (r["counts"][:, centre] == r["k"][:, None]).all() and (r["counts"][:, ~centre] == 0).all()
    assert np.array_equal(r["features"][:, centre], np.full((len(pts), 3), 200.0, f32)) and not r["features"][:, ~centre].any()


def test_mirror_is_the_negated_normals_bit_for_bit():
    tgt, tn = I.bumpy_target()
    a = features("50", "tgt")
    b = G.compute_fpfh(tgt, -tn, 0.010)
    assert np.array_equal(G.mirror(a["features"]), b["features"]) and np.array_equal(G.mirror(a["exact"]), b["exact"])
    assert np.array_equal(G.mirror(G.mirror(a["features"])), a["features"]) and not np.array_equal(G.mirror(a["features"]), a["features"])


def test_features_are_invariant_under_a_rigid_motion():
    tgt, tn = I.bumpy_target()
    a = features("50", "tgt")
    T = G.POSE_170
    P, N = tgt.astype(f64) @ T[:3, :3].T + T[:3, 3], tn.astype(f64) @ T[:3, :3].T
    counts, k, _ = G.spfh(P, N, *a["lists"])
    _, exact = G.fpfh_from_spfh(counts, k, *a["lists"])
    assert np.abs(exact - a["exact"]).max() <= 1e-9


def test_matching_rules():
    rng = np.random.default_rng(3)
    t = rng.uniform(0, 100, (70, 33)).astype(f32)
    t[40] = t[12]                                                              # a duplicated row: the tie goes to the lower index
    s = t[[12, 40, 3, 69]].copy()
    s[2, 5] = np.nan
    t[69, 0] = np.inf
    corres, fwd, mutual = G.match_features(s, t, False)
    assert fwd[:3].tolist() == [12, 12, -1] and fwd[3] not in (-1, 69) and corres[:, 0].tolist() == [0, 1, 3]
    assert G.match_features(s, t, True)[0][:, 0].tolist()[:1] == [0] and not mutual[1]
    assert G.match_features(np.zeros((0, 33), f32), t)[0].shape == (0, 2) and G.match_features(s, np.zeros((0, 33), f32))[0].shape == (0, 2)


def test_degenerate_statement():
    p = pair("50")
    two = G.ransac(p["src"][:2], p["tgt"][:2], TAU)
    line = np.stack([np.arange(50.0) * 0.001, np.zeros(50), np.zeros(50)], 1)
    col = G.ransac(line, line + 0.1, TAU, max_iteration=4096)
    for r in (two, col):
        assert r["status"] == "degenerate" and r["h"] == -1 and not r["mask"].any() and np.array_equal(r["T"], np.eye(4))
    assert col["hypotheses"] == 4096 and not col["valid"].any()


# ---- 4: the public layer --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import bodyslam_amd.evaluation as EV
    import bodyslam_amd.registration as REG
    import bodyslam_amd.tsdf as TS
    return REG, EV, TS


def test_public_signatures(built):
    REG, EV, TS = built

    def sig(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    ransac = [("edge_length_threshold", 0.9), ("max_iteration", 100000), ("confidence", 0.999), ("n_refit", 2), ("seed", 0), ("device", 0)]
    assert sig(REG.compute_fpfh_feature) == [("points", E), ("normals", E), ("radius", E), ("max_nn", 100), ("cell_size", None), ("device", 0)]
    assert sig(REG.match_features)[:3] == [("source_features", E), ("target_features", E), ("mutual_filter", False)]
    assert sig(REG.registration_ransac_based_on_correspondence) == [("source", E), ("target", E), ("corres", E), ("max_correspondence_distance", E)] + ransac
    assert sig(REG.registration_ransac_based_on_feature_matching) == [("source", E), ("target", E), ("source_feature", E), ("target_feature", E),
                                                                      ("mutual_filter", E), ("max_correspondence_distance", E)] + ransac
    assert sig(REG.registration_global) == [("source", E), ("target", E), ("voxel_size", E), ("source_normals", None), ("target_normals", None),
                                            ("feature_radius", None), ("max_correspondence_distance", None), ("normal_sign", "either"), ("ransac", E)]
    assert sig(TS.PointCloud.compute_fpfh_feature) == [("self", E), ("radius", E), ("max_nn", 100)]
    assert issubclass(REG.GlobalRegistrationResult, REG.RegistrationResult)
    names = [f.name for f in __import__("dataclasses").fields(REG.GlobalRegistrationResult)]
    assert names[:6] == ["transformation", "fitness", "inlier_rmse", "iterations", "status", "log"]
    assert names[6:] == ["correspondences", "inlier_mask", "hypotheses", "h"]
    assert REG.RANSAC_CHUNK == G.CHUNK
    from bodyslam_amd import _lib
    assert (_lib.FPFH_DIM, _lib.FPFH_ROW) == (G.DIM, 36)


def test_mirror_fpfh_is_the_statements(built):
    REG = built[0]
    import torch
    f = np.arange(4 * 33, dtype=f32).reshape(4, 33)
    assert np.array_equal(REG.mirror_fpfh(f), G.mirror(f)) and np.array_equal(REG.mirror_fpfh(torch.from_numpy(f)).numpy(), G.mirror(f))
    with pytest.raises(ValueError):
        REG.mirror_fpfh(np.zeros((4, 32), f32))


def test_stop_rule_is_the_statements(built):
    REG = built[0]
    for best, c, conf in ((3, 1000, 0.999), (302, 1000, 0.999), (1000, 1000, 0.5), (322, 5000, 0.9)):
        assert REG._stop_need(best, c, conf) == G.stop_need(best, c, conf)


def test_argument_validation_before_any_device_call(built, monkeypatch):
    REG, EV, TS = built
    from bodyslam_amd import _lib

    def touched(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "init", touched)
    tgt, tn = I.bumpy_target()
    src = pair("50")["src"]
    fs, ft = np.zeros((len(src), 33), f32), np.zeros((len(tgt), 33), f32)
    cr = np.array([[0, 0], [1, 1], [2, 2]], np.int32)
    V_ = ValueError
    for radius in (0.0, -1.0, np.nan, np.inf, 1e-60, 1e60, "1", True, None):
        with pytest.raises(V_):
            REG.compute_fpfh_feature(tgt, tn, radius)
        with pytest.raises(V_):
            REG.registration_ransac_based_on_correspondence(src, tgt, cr, radius)
        with pytest.raises(V_):
            REG.registration_ransac_based_on_feature_matching(src, tgt, fs, ft, True, radius)
        with pytest.raises(V_):
            REG.registration_global(src, tgt, radius)
        with pytest.raises(V_):
            REG.registration_global(src, tgt, 0.002, feature_radius=0.0 if radius is None else radius)
    for max_nn in (0, -1, 1.5, "3", True):
        with pytest.raises(V_):
            REG.compute_fpfh_feature(tgt, tn, 0.01, max_nn=max_nn)
    for normals in (None, tn[:-1], tn[:, :2], "n"):
        with pytest.raises(V_):
            REG.compute_fpfh_feature(tgt, normals, 0.01)
    with pytest.raises(V_):
        REG.compute_fpfh_feature(tgt, tn, 0.01, cell_size=0.0)
    with pytest.raises(V_):
        TS.PointCloud(tgt, np.zeros_like(tgt)).compute_fpfh_feature(0.01)
    for a, b in ((fs[:, :32], ft), (fs, ft.reshape(-1)), (fs.astype(np.int32), ft), ("f", ft)):
        with pytest.raises(V_):
            REG.match_features(a, b)
        with pytest.raises(V_):
            REG.registration_ransac_based_on_feature_matching(src, tgt, a, b, False, 0.004)
    with pytest.raises(V_):
        REG.match_features(fs, ft, mutual_filter=1)
    with pytest.raises(V_):
        REG.registration_ransac_based_on_feature_matching(src, tgt, fs[:-1], ft, False, 0.004)      # one row per point
    for bad in (np.array([[0, len(tgt)]]), np.array([[len(src), 0]]), np.array([[-1, 0]]), np.zeros((3, 3), np.int32), np.zeros((3, 2), f32), "c"):
        with pytest.raises(V_):
            REG.registration_ransac_based_on_correspondence(src, tgt, bad, 0.004)
    for kw in (dict(confidence=0.0), dict(confidence=1.0), dict(confidence=np.nan), dict(edge_length_threshold=0.0), dict(edge_length_threshold=1.01),
               dict(max_iteration=0), dict(max_iteration=1.5), dict(n_refit=-1), dict(seed=-1), dict(seed=0.5)):
        with pytest.raises(V_):
            REG.registration_ransac_based_on_correspondence(src, tgt, cr, 0.004, **kw)
        with pytest.raises(V_):
            REG.registration_global(src, tgt, 0.002, **kw)
        with pytest.raises(V_):
            EV.evaluate_reconstruction_aligned(src, tgt, align="global", icp=dict(max_correspondence_distance=0.005, voxel_size=0.002, ransac=kw))
    with pytest.raises(V_):
        REG.registration_global(src, tgt, 0.002, normal_sign="both")
    with pytest.raises(V_):
        REG.registration_global(src, tgt, 0.002, ransac_n=4)
    with pytest.raises(V_):
        REG.registration_global(src, tgt, 0.002, source_normals=tn)
    icp = dict(max_correspondence_distance=0.005, voxel_size=0.002)
    for bad in (dict(max_correspondence_distance=0.005), dict(icp, init=np.eye(4)), dict(icp, ransac=dict(ransac_n=4)), dict(icp, ransac=3),
                dict(icp, ransac=dict(normal_sign="both")), dict(icp, ransac=dict(feature_radius=-1.0)), dict(icp, foo=1)):
        with pytest.raises(V_):
            EV.evaluate_reconstruction_aligned(src, tgt, align="global", icp=bad)
        with pytest.raises(V_):
            EV.evaluate_reconstruction_surface(src, tgt, align="global", icp=bad, gt_mesh="vertices")
    with pytest.raises(V_):
        EV.evaluate_reconstruction_aligned(src, tgt, align="icp", icp=dict(max_correspondence_distance=0.005, ransac=dict(seed=1)))   # "global" only
    with pytest.raises(V_):
        EV.evaluate_reconstruction_aligned(src, tgt, align="fgr", icp=icp)


def test_no_cpu_fallback(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    REG, EV, TS = built
    from bodyslam_amd._lib import BodySlamHipError
    tgt, tn = I.bumpy_target()
    p = pair("50")
    fs, ft = np.zeros((len(p["src"]), 33), f32), np.zeros((len(tgt), 33), f32)
    calls = [lambda: REG.compute_fpfh_feature(tgt, tn, 0.01), lambda: REG.match_features(fs, ft),
             lambda: REG.registration_ransac_based_on_correspondence(p["src"], tgt, np.zeros((5, 2), np.int32), 0.004),
             lambda: REG.registration_ransac_based_on_feature_matching(p["src"], tgt, fs, ft, True, 0.004),
             lambda: REG.registration_global(p["src"], tgt, 0.002, source_normals=p["sn"], target_normals=tn),
             lambda: TS.PointCloud(tgt, np.zeros_like(tgt), tn).compute_fpfh_feature(0.01),
             lambda: EV.evaluate_reconstruction_aligned(p["src"], tgt, align="global", icp=dict(max_correspondence_distance=0.005, voxel_size=0.002))]
    for call in calls:
        with pytest.raises(BodySlamHipError):
            call()
