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


# ---- 3b: the statement in stages --------------------------------------------------------------------------------------------------------------------
FROZEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "global_registration_ransac.npz")
FROZEN_T_TOL = 1e-12      # T and the RMSE only: the refit now adds in reduce.h's order (the order the device is held to bit for bit), numpy's pairwise
#                           one when the copy was frozen; Kabsch's S = sum q p^T - (sum q) mean(p)^T cancels two digits.  Measured 5.1e-14 and 2.8e-18.


@pytest.mark.parametrize("n_total,max_iteration", [(1000, 100000), (5000, 20000)])
def test_ransac_composed_of_stages_is_the_frozen_copy(n_total, max_iteration):
    """golden/global_registration_ransac.npz holds what ransac() returned on the two planted cases while it was one function"""
    p = pair("50")
    cr = G.planted(p, 300, n_total, 5)
    r = G.ransac(p["src"].astype(f64)[cr[:, 0]], p["tgt"].astype(f64)[cr[:, 1]], TAU, max_iteration=max_iteration)
    with np.load(FROZEN) as z:
        want = {k[len(f"c{n_total}_"):]: z[k] for k in z.files if k.startswith(f"c{n_total}_")}
    got = [r["h"], r["inliers"], r["hypotheses"], r["chunks"], int(r["status"] == "converged"), int(r["unique"])]
    print(n_total, got, "dT", np.abs(r["T"] - want["T"]).max(), "drmse", abs(r["rmse"] - want["floats"][0]))
    assert got == want["scalars"].tolist()
    assert np.array_equal(np.packbits(r["valid"]), want["valid"]) and np.array_equal(r["scores"], want["scores"])
    assert np.array_equal(np.packbits(r["mask"]), want["mask"])
    assert r["fitness"] == want["floats"][1] and r["margin"] == want["floats"][2]
    assert np.abs(r["T"] - want["T"]).max() <= FROZEN_T_TOL and abs(r["rmse"] - want["floats"][0]) <= FROZEN_T_TOL


def test_winner_key_round_trip_and_order():
    top = (1 << 31) - 2
    for h in (0, top):
        key = G.winner_key(0, [7], h)
        assert key == (7 << 32) | (0xffffffff - h) and G.decode(key) == (7, h)
    assert G.winner_key(0, [0, 0, 0], 5) == 0                                            # a score of zero never enters
    key = G.winner_key(0, [0, 4, 9, 9, 2], 100)                                          # a tie inside a chunk: the lower h
    assert G.decode(key) == (9, 102)
    assert G.winner_key(key, [9, 9], 4096) == key                                        # a tie in a later chunk does not displace
    assert G.decode(G.winner_key(key, [3, 10], 4096)) == (10, 4097)                      # a larger score does
    assert G.winner_key(key, [0, 0], 4096) == key
    assert G.decode(G.winner_key(0, [1] * 257, top + 1 - 257)) == (1, top + 1 - 257) and G.decode(G.winner_key(0, [0] * 256 + [1], top + 1 - 257)) == (1, top)


def test_refit_partials_add_the_plain_terms():
    """c = 16385: 65 partial rows, the second trip of column_sum.  The fixed-order sums against numpy's of the same terms."""
    c, n_true = G.STAGE_PLANTED[-1]
    assert c == 16385 and -(-c // 256) == 65
    P, Q = G.planted_scene(c, n_true)
    mask, partial = G.refit_partials(P, Q, G.STAGE_POSE, G.STAGE_TAU)
    r2 = np.sum((P @ G.STAGE_POSE[:3, :3].T + G.STAGE_POSE[:3, 3] - Q) ** 2, 1)
    assert np.array_equal(mask, r2 < G.STAGE_TAU ** 2) and n_true <= mask.sum() < n_true + 50 and partial.shape == (65, 17)
    terms = np.concatenate([np.ones((c, 1)), P, Q, (Q[:, :, None] * P[:, None, :]).reshape(c, 9), r2[:, None]], 1)[mask]
    assert np.array_equal(partial[:, 0], np.add.reduceat(mask.astype(f64), np.arange(0, c, 256)))
    assert partial[64, 0] == 1.0 and (partial[:, 0] > 0).all()                           # the 65th row is a true correspondence: lane 0's second row counts
    assert np.allclose(partial.sum(0), terms.sum(0), rtol=1e-12, atol=0.0)
    state = np.zeros(16)
    state[:12], state[12] = G.STAGE_POSE[:3].reshape(12), 1.0
    fin = G.refit_finish(partial, state, True)
    assert fin[13] == mask.sum() and fin[15] == 1.0 and np.array_equal(fin[:13], state[:13])
    assert abs(fin[14] - np.sqrt(r2[mask].mean())) <= 1e-12 * fin[14]
    tot = np.array([G.wave_sum(partial[:, k]) for k in range(17)])
    assert np.allclose(tot, terms.sum(0), rtol=1e-12, atol=0.0)
    fit = G.refit_finish(partial, state, False)
    want = G.LC.kabsch(P[mask], Q[mask])
    assert fit[12] == 1.0 and fit[15] == 1.0 and np.abs(fit[:12].reshape(3, 4) - np.concatenate([want[0], want[1][:, None]], 1)).max() <= 1e-12


def test_refit_state_machine_of_the_statement():
    P, Q = G.exact_scene()
    state = np.zeros(16)
    state[:12], state[12] = np.eye(4)[:3].reshape(12), 1.0
    line = P.copy()
    line[:5] = np.arange(5.0)[:, None] * np.array([1.0, 2.0, -1.0]) / 1024.0
    lq = line + 1.0
    lq[:5] = line[:5]
    for PP, QQ, want in ((P[:3], P[:3], 1.0), (P[:3], np.concatenate([P[:2], P[2:3] + 1.0]), 0.0), (line, lq, 0.0)):
        mask, partial = G.refit_partials(PP, QQ, np.eye(4), G.STAGE_TAU)
        for final in (False, True):
            out = G.refit_finish(partial, state, final)
            assert out[12] == (1.0 if final and mask.sum() >= 3 else want) and out[15] == 1.0
            if out[12] == 0.0:
                assert np.array_equal(out[:12], state[:12]) and out[13] == 0.0 and out[14] == 0.0
    dead = state.copy()
    dead[12] = 0.0
    assert np.array_equal(G.refit_finish(partial, dead, False), dead)


@pytest.mark.parametrize("c,n_true", G.STAGE_PLANTED)
def test_stage_scenes_are_clear(c, n_true):
    """every planted scene of the stage tests converges with every decision clear of its threshold, in one chunk"""
    P, Q = G.planted_scene(c, n_true)
    r = G.ransac(P, Q, G.STAGE_TAU, max_iteration=512 if c > 2000 else 4096)
    print(c, n_true, r["status"], "h", r["h"], "inliers", r["inliers"], "valid", int(r["valid"].sum()), "margin", r["margin"])
    G.assert_clear(r["margin"])
    assert r["status"] == "converged" and r["chunks"] == 1 and n_true <= r["inliers"] <= n_true + 50
    if c >= 255:                                                                        # (three noisy points fix a rotation to noise / extent only)
        assert np.abs(r["T"] - G.STAGE_POSE).max() <= 1e-3


def test_exact_scene_sits_on_the_edge_length_threshold():
    P, Q = G.exact_scene()
    assert len(np.unique(P, axis=0)) == G.EXACT_C and np.array_equal(P * 1024.0, np.round(P * 1024.0)) and MARGIN == G.MARGIN
    for s in (0.9, 1.0):
        r = G.ransac(P, Q, G.STAGE_TAU, edge_length_threshold=s, max_iteration=4096)
        print(s, r["status"], r["h"], r["inliers"], r["margin"])
        assert r["valid"].all() and len(r["valid"]) == 4096 and (r["scores"] == G.EXACT_C).all() and r["h"] == 0 and r["inliers"] == G.EXACT_C
        assert (r["margin"] == 0.0) if s == 1.0 else (r["margin"] >= MARGIN)
    grown = Q * (1.0 + 2.0 ** -20)                                                       # exact: no edge pair is congruent any more
    assert np.array_equal(grown - Q, Q * 2.0 ** -20)
    ids, valid, fits, margin = G.hypotheses(P, grown, 0, 0, 4096, 1.0, G.STAGE_TAU)
    assert not valid.any() and margin >= MARGIN and np.array_equal(fits, np.tile(np.eye(4)[:3], (4096, 1, 1)))
    assert G.hypotheses(P, grown, 0, 0, 4096, 0.9, G.STAGE_TAU)[3] >= MARGIN


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
