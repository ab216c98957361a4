"""Loop closure on the device (bs_orb_lift, bs_orb_match_pairs, bs_loop_register through bodyslam_amd.loop_closure) against the numpy
statement tests/_loop_closure_ref.py: the integer stages bit for bit, the registration within the fp64 bars of tests/test_trajectory_eval_gpu.py
(rtol 1e-9, atol 1e-9 on rotation entries), every decision exactly.

A comparison that rests on a floating-point decision (a residual against tau) first asserts ON THE STATEMENT that no residual of any
hypothesis or refit round lies within 1e-10 m of tau: the device's Jacobi SVD and LAPACK differ by about 1e-9 relative on millimetre
residuals, i.e. 5e-12 m, so with that margin both sides take the same decisions and a borderline input fails here on the CPU side
instead of flaking.  With the margin the scores are the same integers on both sides, so the tie rule (the lowest h) picks the same
winner whether or not the winning score is unique; uniqueness is asserted on the rendered frames.  On the synthetic sets it cannot
hold: the inliers are exact, so every sample without an outlier reaches the same score.

Frames are tests/_loop_scene.py's at 200 x 152; the statement of every frame is computed once per module."""

import numpy as np
import pytest

import _corner_scene as S
import _loop_closure_ref as LR
import _loop_scene as LS
import _orb_ref as R
from _render import small_pose
from test_loop_closure_cpu import MEASURED, SEED

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from bodyslam_amd import _lib as L  # noqa: E402
from bodyslam_amd import loop_closure as LC  # noqa: E402
from bodyslam_amd import scaling_system as SS  # noqa: E402
from bodyslam_amd.posegraph import PoseGraph, update_global_extrinsic  # noqa: E402

TAU = 0.005
NF = SS.MAX_FEATURES


@pytest.fixture(scope="module")
def views():
    """the rendered frames and their statement: key (the origin), revisit, other (another place, the keyframe's pose), other2 (a third
    place from a second pose), blank"""
    fr = dict(key=LS.render(LS.ORIGIN), revisit=LS.render(LS.REVISIT), other=LS.render(LS.ORIGIN, 1), other2=LS.render(LS.ELSEWHERE, 2), blank=S.blank())
    return {k: dict(color=c, depth=d, **LR.frame(c, d, LS.K)) for k, (c, d) in fr.items()}


def device_features(names, views):
    eng = SS.SparseScale(LS.K)
    return eng, eng.features(np.stack([views[n]["color"] for n in names]))


def match_pairs(s, pairs):
    dev = s["desc"].device
    P = len(pairs)
    m = torch.zeros(P, NF, 4, dtype=torch.int32, device=dev)
    c = torch.zeros(P, dtype=torch.int32, device=dev)
    pr = torch.tensor(pairs, dtype=torch.int32, device=dev)
    L.check(L.load_library().bs_orb_match_pairs(L.p(s["desc"]), L.p(s["counts"]), s["n"], L.p(pr), P, L.p(m), L.p(c), L.stream_ptr()), "bs_orb_match_pairs")
    return m, c


# ---- bs_orb_match_pairs -----------------------------------------------------------------------------------------------------------------
def test_match_pairs_bit_equal_to_the_statement_and_to_bs_orb_match(views):
    names = ["key", "revisit", "other", "blank"]
    eng, s = device_features(names, views)
    pairs = [(0, 2), (2, 0), (1, 1), (3, 0), (0, 3), (0, 1), (7, 0), (0, -1)]
    m, c = match_pairs(s, pairs)
    m, c = m.cpu().numpy(), c.cpu().numpy()
    want = LR.match_pairs([views[n]["desc"] for n in names], pairs[:6])
    assert [len(w) for w in want[:3]] == [int(v) for v in c[:3]] and min(len(w) for w in want[:3]) > 50
    for p, w in enumerate(want):
        assert int(c[p]) == len(w) and np.array_equal(m[p, :len(w), :3], w), p
        assert not m[p, len(w):].any() and not m[p, :, 3].any()
    assert len(want[2]) > 300 and list(c[3:5]) == [0, 0]                                    # a frame against itself; a blank frame either side
    assert list(c[6:]) == [0, 0] and not m[6:].any()                                        # a pair that leaves the arrays reads nothing
    # pairs (p, p + 1) are bs_orb_match
    m2, c2 = match_pairs(s, [(0, 1), (1, 2), (2, 3)])
    eng.match(s)
    assert torch.equal(m2, s["matches"]) and torch.equal(c2, s["match_counts"])


def test_bs_orb_match_still_equals_the_statement_on_the_plane_pair():
    prev, curr, _ = S.pair("plane")
    want = R.match(R.extract(prev[0])["desc"], R.extract(curr[0])["desc"])
    eng = SS.SparseScale(S.K)
    s = eng.match(eng.features(np.stack([prev[0], curr[0]])))
    assert len(want) > 100 and int(s["match_counts"][0]) == len(want)
    assert np.array_equal(s["matches"][0, :len(want), :3].cpu().numpy(), want) and not s["matches"][0, len(want):].any()


# ---- bs_orb_lift --------------------------------------------------------------------------------------------------------------------------
def test_lift_bit_equal_with_zero_and_nan_depth(views):
    v = views["revisit"]
    depth = v["depth"].copy()
    for k, bad in ((0, 0.0), (5, np.nan), (17, 0.0), (40, np.inf)):
        x, y = v["pt"][k]
        depth[int(y), int(x)] = bad
    want = LR.lift(v["pt"], depth, LS.K)
    n = len(want)
    assert n - int(want[:, 3].sum()) >= 4 and want[:, 3].sum() > 300
    eng, s = device_features(["revisit"], views)
    xyz = torch.full((1, NF, 4), -1.0, dtype=torch.float64, device=eng.dev)
    d = torch.from_numpy(depth).to(eng.dev)
    L.check(L.load_library().bs_orb_lift(L.p(s["pt"]), L.p(s["counts"]), L.p(d), 1, LS.H, LS.W, SS._ptr(eng.K), L.p(xyz), L.stream_ptr()), "bs_orb_lift")
    got = xyz[0].cpu().numpy()
    assert np.array_equal(got[:n].view(np.uint64), want.view(np.uint64)) and not got[n:].any()


# ---- register_points on synthetic data ------------------------------------------------------------------------------------------------------
T_SYN = small_pose(0.3, -0.2, 0.5, 0.05, -0.02, 0.08)


def synthetic(C, share, seed):
    """exact inliers under T_SYN; the planted outliers are displaced by at least 10 tau along every axis"""
    rng = np.random.default_rng(1000 * seed + C)
    P = rng.uniform(-0.2, 0.2, size=(C, 3)) + (0.0, 0.0, 0.5)
    Q = P @ T_SYN[:3, :3].T + T_SYN[:3, 3]
    planted = np.ones(C, dtype=bool)
    planted[rng.permutation(C)[:int(share * C)]] = False
    n_out = int((~planted).sum())
    Q[~planted] += rng.choice([-1.0, 1.0], size=(n_out, 3)) * rng.uniform(10 * TAU, 0.2, size=(n_out, 3))
    return P, Q, planted


@pytest.mark.parametrize("share", [0.0, 0.3, 0.6])
@pytest.mark.parametrize("C", [3, 4, 63, 64, 65, 257, 500])
def test_register_points_synthetic(C, share):
    P, Q, planted = synthetic(C, share, 7)
    ref = LR.register(P, Q, TAU, seed=11)
    print("C", C, "share", share, "planted inliers", int(planted.sum()), "statement: status", ref["status"], "inliers", ref["inliers"], "h", ref["h"],
          "margin", ref["margin"])
    assert ref["margin"] >= 1e-10
    out = [LC.register_points(P, Q, TAU, seed=11) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*out))                                    # the same bits in every call
    T, mask, info, rmse, h = (o.cpu().numpy() for o in out[0])
    print("device: h", int(h), "inliers", int(mask.sum()), "max |T - statement|", np.abs(T - ref["T"]).max(), "rmse", float(rmse))
    assert int(h) == ref["h"] and np.array_equal(mask, ref["mask"])
    if planted.sum() >= 3:
        assert ref["status"] == 1 and np.array_equal(mask, planted) and info[5, 5] == planted.sum()
        assert np.allclose(T[:3, :3], T_SYN[:3, :3], rtol=1e-9, atol=1e-9) and np.allclose(T[:3, 3], T_SYN[:3, 3], rtol=1e-9, atol=0.0)
        assert float(rmse) < 1e-12
    else:
        assert ref["status"] == 0 and int(h) == -1                                        # two inliers among three or four points: no fit
    assert np.allclose(T[:3, :3], ref["T"][:3, :3], rtol=1e-9, atol=1e-9) and np.allclose(T[:3, 3], ref["T"][:3, 3], rtol=1e-9, atol=0.0)
    assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])
    assert np.allclose(info, ref["info"], rtol=1e-9, atol=0.0) and np.array_equal(info, info.T)


# ---- rejections -----------------------------------------------------------------------------------------------------------------------------
def assert_rejected(T, mask, info, rmse, h):
    assert np.array_equal(T.cpu().numpy(), np.eye(4)) and not mask.any() and not info.any() and int(h) == -1 and float(rmse) == 0.0


@pytest.mark.parametrize("case", ["C0", "C1", "C2", "collinear", "coincident"])
def test_rejections(case):
    rng = np.random.default_rng(5)
    if case[0] == "C":
        P = rng.uniform(-0.2, 0.2, size=(int(case[1]), 3))
    elif case == "collinear":
        P = np.outer(np.linspace(0.0, 1.0, 50), (0.3, -0.2, 0.1)) + (0.1, 0.2, 0.3)
    else:
        P = np.tile((0.1, 0.2, 0.3), (50, 1))
    assert LR.register(P, P, TAU)["status"] == 0
    assert_rejected(*LC.register_points(P, P, TAU))


def test_every_match_above_max_hamming_is_a_rejection():
    rng = np.random.default_rng(6)
    dev = torch.device("cuda", 0)
    L.init(0)
    xyz = torch.zeros(2, NF, 4, dtype=torch.float64, device=dev)
    xyz[:, :100, :3] = torch.from_numpy(rng.uniform(-0.2, 0.2, size=(100, 3))).to(dev)
    xyz[:, :100, 3] = 1.0
    matches = torch.zeros(1, NF, 4, dtype=torch.int32, device=dev)
    matches[0, :, 0] = matches[0, :, 1] = torch.arange(NF, dtype=torch.int32, device=dev)
    matches[0, :, 2] = 65
    pairs = torch.tensor([[0, 1]], dtype=torch.int32, device=dev)
    count = torch.tensor([100], dtype=torch.int32, device=dev)
    rec, mask = LC._register(xyz, pairs, matches, count, 64, TAU, 256, 2, 0, 0)
    r = LC._records(rec.cpu().numpy())
    assert r["status"][0] == 0 and r["correspondences"][0] == 0 and r["matches"][0] == 100 and r["h"][0] == -1
    assert np.array_equal(r["T"][0], np.eye(4)) and not r["information"].any() and not mask.any()
    rec, mask = LC._register(xyz, pairs, matches, count, 65, TAU, 256, 2, 0, 0)            # at the threshold they count
    r = LC._records(rec.cpu().numpy())
    assert r["status"][0] == 1 and r["correspondences"][0] == 100 and r["inliers"][0] == 100 and int(mask.sum()) == 100


# ---- LoopCloser on rendered frames ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def revisit_ref(views):
    """the statement of the pair (revisit -> key); the margin assertion that the device comparisons rest on"""
    m = LR.match_pairs([views["revisit"]["desc"], views["key"]["desc"]], [(0, 1)])[0]
    r = LR.register_pair(views["revisit"]["xyz"], views["key"]["xyz"], m, 64, TAU, min_matches=30, seed=SEED, pair=0)
    assert r["margin"] >= 1e-10 and r["unique"] and r["status"] == 1
    return r


def make_closer(views, **kw):
    closer = LC.LoopCloser(LS.K, seed=SEED, **kw)
    for index, name in ((0, "key"), (10, "blank"), (20, "other")):
        closer.add_keyframe(index, views[name]["color"], views[name]["depth"])
    return closer


def test_loop_closer_finds_the_revisit_and_nothing_else(views, revisit_ref):
    closer = make_closer(views, min_gap=20)
    edges = closer.detect(40, views["revisit"]["color"], views["revisit"]["depth"])
    rec = closer.last_records
    print("keyframes", rec["keyframe"], "matches", rec["matches"], "C", rec["correspondences"], "inliers", rec["inliers"], "h", rec["h"], "rmse", rec["rmse"])
    assert len(edges) == 1 and edges[0][:2] == (40, 0)
    T, info = edges[0][2], edges[0][3]
    ref = revisit_ref
    assert list(rec["keyframe"]) == [0, 10, 20] and rec["h"][0] == ref["h"] and rec["inliers"][0] == ref["inliers"] == MEASURED["revisit"]["inliers"]
    assert rec["correspondences"][0] == ref["C"] and rec["matches"][0] == ref["matches"]
    assert np.array_equal(rec["mask"][0].cpu().numpy() != 0, ref["mask_rows"])
    assert np.allclose(T[:3, :3], ref["T"][:3, :3], rtol=1e-9, atol=1e-9) and np.allclose(T[:3, 3], ref["T"][:3, 3], rtol=1e-9, atol=0.0)
    assert np.allclose(info, ref["info"], rtol=1e-9, atol=0.0) and info[5, 5] == rec["inliers"][0]
    assert abs(rec["rmse"][0] - ref["rmse"]) <= 1e-9 * ref["rmse"]
    # against the rendered motion: 1.5 times the statement's own measured error (set by the integer keypoint positions, not by the device)
    truth = LS.motion(LS.REVISIT)
    et, eR = np.linalg.norm(T[:3, 3] - truth[:3, 3]), np.abs(T[:3, :3] - truth[:3, :3]).max()
    print("error against the rendered motion: t", et, "R", eR)
    assert et <= 1.5 * MEASURED["revisit"]["t"] and eR <= 1.5 * MEASURED["revisit"]["R"]
    # the blank keyframe has nothing to match; the other place passes the descriptor gate and fails the geometry
    assert rec["matches"][1] == 0 and rec["status"][1] == 0 and rec["correspondences"][2] >= 30 and rec["inliers"][2] <= MEASURED["elsewhere_max_inliers"]
    # zero false closures: a view of a third place, and a blank frame
    assert closer.detect(41, views["other2"]["color"], views["other2"]["depth"]) == []
    assert closer.last_records["inliers"].max() <= MEASURED["elsewhere_max_inliers"] and closer.last_records["correspondences"].max() >= 30
    assert closer.detect(42, views["blank"]["color"], views["blank"]["depth"]) == []
    assert not closer.last_records["matches"].any()


def test_min_gap_keeps_young_keyframes_out(views):
    closer = make_closer(views, min_gap=50)
    assert closer.detect(40, views["revisit"]["color"], views["revisit"]["depth"]) == [] and closer.last_records is None
    assert [e[:2] for e in closer.detect(50, views["revisit"]["color"], views["revisit"]["depth"])] == [(50, 0)]
    assert list(closer.last_records["keyframe"]) == [0]


def test_store_growth_leaves_earlier_keyframes_unchanged(views, monkeypatch):
    monkeypatch.setattr(LC, "CHUNK", 2)
    closer = LC.LoopCloser(LS.K, seed=SEED, min_gap=1)
    assert closer.cap == 2
    closer.add_keyframe(0, views["key"]["color"], views["key"]["depth"])
    closer.add_keyframe(1, views["other"]["color"], views["other"]["depth"])
    e1 = closer.detect(40, views["revisit"]["color"], views["revisit"]["depth"])
    a = closer.last_records
    closer.add_keyframe(40)                                                                # the frame detect looked at: across the chunk boundary
    closer.add_keyframe(41, views["blank"]["color"], views["blank"]["depth"])
    assert closer.cap == 4 and closer.n == 4
    e2 = closer.detect(80, views["revisit"]["color"], views["revisit"]["depth"])
    b = closer.last_records
    assert list(b["keyframe"]) == [0, 1, 40, 41]
    for k in ("T", "inliers", "correspondences", "h", "rmse", "status", "matches", "information"):
        assert np.array_equal(a[k], b[k][:2]), k
    assert torch.equal(a["mask"], b["mask"][:2]) and torch.equal(a["matches_dev"], b["matches_dev"][:2])
    assert e1[0][:2] == (40, 0) and e2[0][:2] == (80, 40)                                  # its own stored copy is the best closure
    # the frame against its own stored copy: every usable match is an inlier of the identity
    assert b["inliers"][2] == b["correspondences"][2] > 150 and np.allclose(b["T"][2], np.eye(4), atol=1e-9)
    with pytest.raises(ValueError):
        closer.add_keyframe(7)


# ---- the graph ------------------------------------------------------------------------------------------------------------------------------------
def drifted_chain():
    """nine true poses from the origin to LS.REVISIT along one screw, and the chain an odometry with a constant bias would give"""
    w, t = np.array([0.02, -0.03, 0.05]), np.array([0.010, -0.006, 0.008])
    true = [small_pose(*(w * (k / 8.0)), *(t * (k / 8.0))) for k in range(9)]
    bias = small_pose(0.0015, -0.001, 0.0012, 4e-4, -3e-4, 2e-4)
    rel = [np.linalg.inv(true[k - 1]) @ true[k] @ bias for k in range(1, 9)]
    chain = [np.eye(4)]
    for T in rel:
        chain.append(chain[-1] @ T)
    return true, rel, chain


def test_detected_closure_pulls_a_drifted_chain(views):
    """The shape of test_sequence_with_posegraph_relinearisation with the edge found instead of given.  PoseGraph's line process keeps an
    uncertain edge whose residual e^T Lambda e stays near mu = preference * max_correspondence_distance^2 * Lambda[5, 5]; with Lambda = sum G^T G
    both sides grow with the inlier count, so what the edge survives does not: a disagreement with the chain of the order of
    sqrt(preference) * 5 mm per point, 0.5 mm at the reference's preference 0.01.  The drift planted here (4.3 mm and 0.012 in a rotation
    entry at node 8) is several times the closure's own error (0.43 mm, 3.6e-3: MEASURED) so that "closer than before" has a meaning; at
    preference 0.01 the line process switches such an edge off (measured on the CPU with the statement's edge), so the graph is built
    with preference 1.0: a closure may disagree with the chain by about the correspondence distance itself."""
    true, rel, chain = drifted_chain()
    closer = LC.LoopCloser(LS.K, seed=SEED, min_gap=8)
    closer.add_keyframe(0, views["key"]["color"], views["key"]["depth"])
    edges = closer.detect(8, views["revisit"]["color"], views["revisit"]["depth"])
    assert len(edges) == 1 and edges[0][:2] == (8, 0)
    pg = PoseGraph(preference_loop_closure=1.0)
    pg.add_node(chain[0])
    for i in range(1, 9):
        pg.add_node(chain[i])
        pg.add_edge(rel[i - 1], i, i - 1, False)
    pg.add_edge(edges[0][2], 8, 0, True, edges[0][3])
    pg.optimize()
    X = np.stack(update_global_extrinsic(pg.pose_graph))
    err = lambda A, B: (np.linalg.norm(A[:3, 3] - B[:3, 3]), np.abs(A[:3, :3] - B[:3, :3]).max())
    before, after = err(chain[8], true[8]), err(X[8], true[8])
    print("node 8 against its true pose (t, R): before", before, "after", after, "log", pg.last_log)
    assert before[0] > 5 * MEASURED["revisit"]["t"] and before[1] > 3 * MEASURED["revisit"]["R"]
    assert after[0] < before[0] and after[1] < before[1]
    assert np.array_equal(X[0], chain[0])
    assert len([e for e in pg.pose_graph.edges if e.uncertain]) == 1                       # the closure was kept
    Rg = X[:, :3, :3]
    assert np.abs(Rg @ Rg.transpose(0, 2, 1) - np.eye(3)).max() < 1e-9


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------------------
def test_run_slam_loop_finds_the_closure_of_a_repeated_frame():
    """the small pipeline of test_sequence_with_posegraph_relinearisation; frame 8 is a copy of frame 0 and both carry the tiled corner
    texture, so ORB has keypoints.  Identical frames give identical depth, the lifted points coincide and T is the identity whatever the
    random-weight network predicts."""
    import dataclasses
    from bodyslam_amd.pipeline import BodySlamPipeline
    from bodyslam_amd.synthetic import make_sequence
    from bodyslam_amd.zoedepth import ZoeConfig
    from oracle import cyclepose_ref as CP
    from oracle import zoedepth_ref as Z
    cfg_o = Z.ZoeConfig(hidden=128, layers=4, heads=2, intermediate=256, taps=(1, 2, 3, 4), image_size=64)
    names = {f.name for f in dataclasses.fields(ZoeConfig)}
    cfg_p = ZoeConfig(**{k: v for k, v in dataclasses.asdict(cfg_o).items() if k in names})
    pipe = BodySlamPipeline(Z.synth_weights(cfg_o, seed=2), CP.synth_weights(seed=2), cfg_p, batch=4, target_hw=(64, 96))
    frames = np.array(make_sequence(9, 160, 192, seed=5))
    tex = S.render(np.eye(4), "plane", K=(200.0, 200.0, 96.0, 80.0), H=160, W=192)[0]
    frames[0, 8:152, 8:184] = tex[8:152, 8:184]
    frames[8] = frames[0]
    a = pipe.run_slam_loop(frames)
    assert pipe.perform_loop_closure is False and pipe.num_closure == 10000 and pipe.global_key_frame_indices == [] and pipe.loop_closures_found == []
    pipe.perform_loop_closure, pipe.num_closure, pipe.loop_closure_options = True, 8, dict(min_gap=8)
    b = pipe.run_slam_loop(frames)
    assert pipe.global_key_frame_indices == [0, 8] and len(pipe.loop_closures_found) == 1
    s_, t_, T, info = pipe.loop_closures_found[0]
    print("closure", s_, t_, "inliers", info[5, 5], "max |T - I|", np.abs(T - np.eye(4)).max())
    assert (s_, t_) == (8, 0) and info[5, 5] >= 30 and np.abs(T - np.eye(4)).max() <= 1e-9
    assert torch.equal(a.g_abs, b.g_abs)                                                   # (no optimisation asked for: the poses stand)
    pipe.perform_loop_closure = False
    c = pipe.run_slam_loop(frames)
    assert torch.equal(a.g_abs, c.g_abs) and torch.equal(a.depth_u16, c.depth_u16) and torch.equal(a.t_rel, c.t_rel)
    assert torch.equal(a.point_counts, c.point_counts)
