"""The inputs of tests/test_orb_stages_gpu.py meet, ON THE STATEMENT (tests/_orb_ref.py), the conditions they were built for.  No GPU.

A builder of tests/_orb_cases.py that stops reaching its cap, tie or edge fails here and not in the GPU file, where it would pass without
testing anything.  The counts are the statement's, measured on the CPU."""
import numpy as np
import pytest

import _orb_cases as C
import _orb_ref as R
from bodyslam_amd import orb_tables as T

NFEAT = [109, 90, 75, 63, 52, 44, 36, 31]


def counts(name, frame=0):
    return [int(v) for v in C.statement(name)[0][frame]["counts"]]


def test_features_per_level_and_caps():
    assert list(T.features_per_level()) == NFEAT and sum(NFEAT) == C.NF == 500 and 2 * max(NFEAT) <= 256


def test_full_fills_all_500_keypoints_in_both_frames():
    """gap: a frame that fills ORB_KP = 500 (every level full, match with n1 = n2 = 500, displacement with M above one 256-wide pass)"""
    f, m = C.statement("full")
    assert counts("full", 0) == NFEAT and counts("full", 1) == NFEAT
    assert all(c > n for c, n in zip(C.candidates(f[0])[:7], NFEAT))            # every level but the last also cuts by response
    assert len(f[0]["desc"]) == len(f[1]["desc"]) == 500
    assert len(m) == 332 and len(m) > 256                                         # two passes of displacement's scan loop
    (_, d0), (_, d1) = C.full_pair()
    for a in ("reference", "matched"):
        mean, cnt = R.displacement(f[0]["pt"], f[1]["pt"], m, d0, d1, C.FULL_K, a)
        assert cnt[:3] == (500, 500, 332) and cnt[5] > 256 and np.all(np.isfinite(mean)) and np.max(np.abs(mean)) <= 1.0


def test_blocks_sizes_reach_their_edges():
    """gaps: a level whose interior is one pixel thick; a portrait frame; (no interior at all; far below every cut)"""
    assert counts("blocks_83x97", 0) == [32, 7, 0, 0, 0, 0, 0, 0] and counts("blocks_83x97", 1) == [36, 8, 0, 0, 0, 0, 0, 0]
    f = C.statement("blocks_83x97")[0][0]
    assert C.candidates(f) == counts("blocks_83x97") and all(c < n for c, n in zip(counts("blocks_83x97"), NFEAT))
    one = C.statement("blocks_63x200")[0][0]
    assert 63 - 2 * T.EDGE_THRESHOLD == 1 and counts("blocks_63x200") == [7, 0, 0, 0, 0, 0, 0, 0]
    assert set(one["kp"][:, 2]) == {31}                                            # the one interior row
    assert counts("blocks_62x200") == [0] * 8 and all(not s.any() for s in C.statement("blocks_62x200")[0][0]["score"])
    rgb, _ = C.frames("blocks_230x141")
    assert rgb.shape[1] > rgb.shape[2] and counts("blocks_230x141") == NFEAT[:4] + [17, 0, 0, 0]


def test_periodic_has_ties_duplicates_and_a_level_with_exactly_n_candidates():
    """gaps: the Harris tie rule; the lowest-index rule of the match on equal distances, both directions; a level with exactly n_l candidates"""
    f, m = C.statement("periodic")
    assert C.equal_responses(f[0]) == 91 and C.duplicate_descriptors(f[0]) == 91
    assert C.candidates(f[0])[5] == NFEAT[5] == 44 and counts("periodic")[5] == 44   # cand == n: neither cut removes anything
    assert counts("periodic") == NFEAT[:6] + [2, 0]
    # against the rolled copy the best distance of many queries is shared by two or more trains, and of many trains by two or more queries
    assert C.shared_best(f[0]["desc"], f[1]["desc"]) >= 91 and C.shared_best(f[1]["desc"], f[0]["desc"]) >= 91
    # a period's shift leaves the frame as it is: of every group of equal descriptors the lowest index alone survives the cross-check
    assert np.array_equal(f[0]["desc"], f[1]["desc"]) and len(m) == len(f[0]["desc"]) - 91 and not m[:, 2].any()
    assert np.array_equal(m[:, 0], m[:, 1]) and np.all(np.diff(m[:, 0]) > 0)


def test_mirror_and_checker_have_equal_responses():
    """gap: the Harris tie rule in select_kernel (equal response, lower pixel index first)"""
    m = C.statement("mirror")[0][0]
    assert C.equal_responses(m) == 92 and C.duplicate_descriptors(m) == 0
    c = C.statement("checker")[0][0]
    assert C.equal_responses(c) == 92 and C.duplicate_descriptors(c) == 72
    assert counts("checker") == [0, 90, 48, 10, 0, 0, 0, 0] and C.candidates(c)[1] == 120          # level 0 empty, level 1 full


def test_noise_and_constant_frames():
    rgb, _ = C.frames("noise_rgb")
    assert not np.array_equal(rgb[..., 0], rgb[..., 2])
    a, b = C.statement("noise_rgb")[0][0], C.statement("noise_bgr")[0][0]
    assert not np.array_equal(a["grey"][0], b["grey"][0]) and counts("noise_rgb")[:2] == [109, 90]
    for name, v in (("white", 255), ("black", 0)):
        f = C.statement(name)[0][0]
        assert all(np.all(g == v) for g in f["grey"]) and all(np.all(s == v) for s in f["smooth"]) and counts(name) == [0] * 8


def test_both_residues_of_the_level_size_occur_at_populated_levels():
    """the selector reads 16 score bytes at a time: a populated level with W H a multiple of 16 and one with a tail"""
    seen = set()
    for name in C.FRAMES:
        rgb, _ = C.frames(name)
        for (w, h), n in zip(T.level_sizes(*rgb.shape[1:3]), counts(name)):
            if n:
                seen.add((w * h) % 16 != 0)
    assert seen == {False, True}


@pytest.mark.parametrize("name", sorted(C.SELECT_CASES))
def test_crafted_score_maps_meet_their_cut(name):
    """gap: the cut's tie list across several 4096-pixel chunks with `need` below the number of ties"""
    g, score, hist = C.select_case(name)
    n = NFEAT[0]
    e = T.EDGE_THRESHOLD
    s0 = score[0]
    assert not s0[:e].any() and not s0[-e:].any() and not s0[:, :e].any() and not s0[:, -e:].any()       # interior only
    assert all(np.array_equal(hist[l, 1:], np.bincount(score[l].reshape(-1), minlength=256)[1:]) for l in range(8))
    T_, need, ties = C.cut_of(s0, n)
    k = int((s0 > 0).sum())
    want = {"ties_300": (300, 50, 218, 300), "exactly_2n": (218, 50, 218, 218), "exactly_n": (109, 0, 0, 0), "one": (1, 0, 0, 0),
            "need_1": (267, 50, 1, 50)}[name]
    assert (k, T_, need, ties) == want
    sel = R.select(g[0], s0, n)
    assert len(sel) == min(k, n)
    if name in ("ties_300", "need_1"):
        assert need < ties
        tie_px = np.flatnonzero(s0.reshape(-1) == T_)
        assert len(np.unique(tie_px // C.CHUNK)) >= 4                                 # the tie list runs over several chunks
        taken, dropped = tie_px[:need], tie_px[need:]
        assert len(np.unique(dropped // C.CHUNK)) >= 2
        chosen = {y * C.SEL_W + x for (x, y, s, _) in sel if s == T_}
        assert chosen <= set(taken.tolist()) and not chosen & set(dropped.tolist())
    if name == "ties_300":
        assert len(np.unique(np.flatnonzero(s0.reshape(-1))[:218] // C.CHUNK)) >= 3   # the winners themselves span chunks


@pytest.mark.parametrize("name", C.MATCH_CASES)
def test_crafted_descriptor_sets(name):
    """gaps: n1 != n2 by a wide margin, n1 = 0 or n2 = 0; the lowest-index rule on equal distances; the stable order"""
    desc, cnt = C.match_case(name)
    assert desc.shape[1:] == (500, 8) and desc.dtype == np.uint32
    sets = C.clamped(desc, cnt)
    m = R.match(sets[0], sets[1])
    if name.startswith("random_"):
        assert len(m) > 0 or 0 in cnt
        assert len(m) <= min(cnt)
    if name == "identical_64":
        assert m.tolist() == [[0, 0, 0]]
    if name == "triples":
        assert C.shared_best(sets[0], sets[1]) == 480 and C.shared_best(sets[1], sets[0]) == 480 and len(m) == 160 and not m[:, 2].any()
    if name == "one_distance":
        assert len(m) == 400 and set(m[:, 2]) == {3} and np.array_equal(m[:, 0], np.arange(400)) and np.any(np.diff(m[:, 1]) < 0)
    if name == "clamped_counts":
        assert [len(s) for s in sets] == [500, 300, 0] and len(m) > 100


@pytest.mark.parametrize("name", C.DISP_CASES)
def test_crafted_displacement_inputs(name):
    """gaps: displacement with M = 500; a NaN depth"""
    c = C.displacement_case(name)
    W = C.FULL_W
    assert np.abs(c["pt"][..., 0].astype(np.float64) - c["K"][2]).max() / c["K"][0] <= 1.0 and np.nanmax(c["depth"]) <= 1.0
    assert c["pt"][0, 1, 0] == W - 0.5 and c["pt"][0, 2, 0] == W and c["pt"][0, 4, 0] == -0.5
    ref, cr = C.displacement_statement(c, "reference")
    mat, cm = C.displacement_statement(c, "matched")
    if name == "zeros":
        assert cr[2] == 500 and cr[3] != cr[4] and 250 < min(cr[3], cr[4]) < 400 and cr[5] == min(cr[3], cr[4])      # nA != nB: the zip misaligns
        assert 100 < cm[5] < cr[5] and np.all(np.isfinite(ref)) and np.all(np.isfinite(mat))
        assert cr[3] == 500 - 167 - 1                                                  # a third dropped, and the point at x = W
    if name == "nan":
        assert cr == C.displacement_statement(C.displacement_case("zeros"), "reference")[1]       # NaN is not 0: the same counters
        assert np.all(np.isnan(ref)) and np.all(np.isnan(mat)) and cm[5] > 0
        assert np.isnan(c["depth"]).sum() == 4
    if name in ("no_match", "all_zero"):
        assert cr[5] == cm[5] == 0 and np.all(np.isnan(ref)) and np.all(np.isnan(mat))
        assert cr[2] == (0 if name == "no_match" else 500)
    if name == "fewer_curr":
        assert cr[:3] == (500, 300, 300) and (c["matches"][:, 0] >= 300).sum() > 50 and cr[4] < cr[3]
