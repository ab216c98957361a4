"""Every bs_orb_* entry point (csrc/sparse_features.hip, csrc/orb_match.h through bs_orb_match and bs_orb_match_pairs) against the numpy
statement tests/_orb_ref.py BIT FOR BIT, at the caps, ties and frame edges that tests/_corner_scene.py's 200 x 152 pair does not reach.
The inputs are tests/_orb_cases.py's; that each reaches what it is for is asserted on the statement in tests/test_orb_stages_cpu.py.

Whole frames go through SparseScale.features / .match; hand-written score maps, descriptor sets and displacement inputs go to the entry
points through the library handle, every output prefilled with a sentinel that rows at and behind the count must keep.  The refusals are
host-side: nothing is launched and every buffer stays as it was.  The only out-of-range data any test passes is a keypoint count outside
0 .. 500, which orb_match_pair clamps before it reads.

The one tolerance is the displacement's mean, 1e-12: at most 500 terms of magnitude <= 1 m summed in another order differ by at most
500 * 2^-53 = 5.6e-14; a dropped or doubled term of a millimetre moves the mean by 2e-6.  Everything else is equality."""
import functools

import numpy as np
import pytest

import _orb_cases as C
import _orb_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from bodyslam_amd import _lib as L  # noqa: E402
from bodyslam_amd import orb_tables as T  # noqa: E402
from bodyslam_amd import scaling_system as SS  # noqa: E402

NF, NL, OUTF = SS.MAX_FEATURES, SS.MAX_LEVELS, SS.OUT_FIELDS
SENT = -77                                          # the sentinel: no keypoint field, index, distance, count or byte pattern of a result


def engine(association="reference"):
    return SS.SparseScale(C.FULL_K, association=association)


def host(s):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in s.items()}


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")        # (a copy: the shared inputs are read-only)


def filled(shape, dtype, value=SENT):
    return torch.full(shape, value, dtype=dtype, device="cuda:0")


@functools.lru_cache(maxsize=None)
def device_stages(name):
    """the stage outputs of FRAMES[name] through SparseScale.features (and .match for a pair), read back once"""
    rgb, bgr = C.frames(name)
    e = engine()
    s = e.features(dev(rgb), bgr=bgr)
    if len(rgb) == 2:
        e.match(s)
    return host(s)


# ---- whole frames ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.FRAMES))
def test_image_stages_and_histogram_bit_equal(name):
    """gaps: a level whose interior is one pixel thick (blocks_63x200), a portrait frame (blocks_230x141), the rounding at 0 and 255"""
    st, (f, _) = device_stages(name), C.statement(name)
    for frame, want in enumerate(f):
        for l in range(NL):
            for stage in ("grey", "smooth", "score"):
                got = C.level_view(st, stage, frame, l)
                assert got.shape == want[stage][l].shape and np.array_equal(got, want[stage][l]), (stage, frame, l, int((got != want[stage][l]).sum()))
            h = np.bincount(want["score"][l].reshape(-1), minlength=256)
            assert np.array_equal(st["hist"][frame, l, 1:], h[1:]) and st["hist"][frame, l, 0] == 0, (frame, l)


@pytest.mark.parametrize("name", sorted(C.FRAMES))
def test_keypoints_responses_positions_descriptors_bit_equal(name):
    """gaps: a frame that fills ORB_KP = 500 (full); the Harris tie rule, equal response -> lower pixel index first (periodic, mirror,
    checker); a level with exactly n_l candidates (periodic, level 5); a level whose interior is one pixel thick (blocks_63x200: its 7
    keypoints lie on the row y = 31); a portrait frame (blocks_230x141)"""
    st, (f, _) = device_stages(name), C.statement(name)
    for frame, want in enumerate(f):
        n = int(want["counts"].sum())
        assert list(st["counts"][frame]) == list(want["counts"]) + [n], (frame, st["counts"][frame])
        assert np.array_equal(st["kp"][frame, :n, :7], want["kp"]), frame
        assert not st["kp"][frame, :n, 7].any()
        assert np.array_equal(st["resp"][frame, :n].view(np.uint64), want["resp"].view(np.uint64)), frame
        assert np.array_equal(st["pt"][frame, :n].view(np.uint32), want["pt"].view(np.uint32)), frame
        assert np.array_equal(st["desc"][frame, :n].view(np.uint32), want["desc"]), frame


@pytest.mark.parametrize("name", C.PAIRS)
def test_matches_of_the_pairs_bit_equal(name):
    """gaps: match with n1 = n2 = 500 (full); the lowest-index rule on equal Hamming distances in both directions of the cross-check
    (periodic against its copy: of every group of equal descriptors only the lowest index survives)"""
    st, (_, m) = device_stages(name), C.statement(name)
    assert int(st["match_counts"][0]) == len(m)
    assert np.array_equal(st["matches"][0, :len(m), :3], m) and not st["matches"][0, :len(m), 3].any()


@pytest.mark.parametrize("association", ["reference", "matched"])
def test_displacement_of_the_full_pair(association):
    """gap: displacement with more matches than one 256-wide pass of its scan loop (M = 332 between 500 and 500 keypoints)"""
    (c0, d0), (c1, d1) = C.full_pair()
    f, m = C.statement("full")
    want, counts = R.displacement(f[0]["pt"], f[1]["pt"], m, d0, d1, C.FULL_K, association)
    e = engine(association)
    got = e.displacements_block(np.stack([c0, c1]), np.stack([d0, d1]))[0]
    print(association, "device", got, "statement", want, "counts", e.last_counts[0], counts)
    assert list(e.last_counts[0]) == list(counts) and counts[5] > 256
    assert got.dtype == np.float64 and np.max(np.abs(got - want)) <= 1e-12


# ---- the entry points through the library handle ----------------------------------------------------------------------------------------------
def flat(levels_of_frames, layout, stride, fill=0):
    """uint8 [frames, stride]: every frame's levels at their offsets"""
    out = np.full((len(levels_of_frames), stride), fill, dtype=np.uint8)
    for f, lv in enumerate(levels_of_frames):
        for (w, h, off), a in zip(layout, lv):
            out[f, off:off + w * h] = a.reshape(-1)
    return out


def call_select(g, score, hist):
    H, W = g[0].shape
    layout, stride = T.level_layout(H, W)
    grey, sc, hs = dev(flat([g], layout, stride)), dev(flat([score], layout, stride)), dev(hist[None])
    kp, resp, counts = filled((1, NF, 8), torch.int32), filled((1, NF), torch.float64), filled((1, NL + 1), torch.int32)
    nfeat = T.features_per_level()
    L.check(L.load_library().bs_orb_select(L.p(grey), L.p(sc), L.p(hs), 1, H, W, SS._ptr(layout), len(layout), stride, SS._ptr(nfeat), L.p(kp), L.p(resp),
                                           L.p(counts), L.stream_ptr()), "bs_orb_select")
    return kp[0].cpu().numpy(), resp[0].cpu().numpy(), counts[0].cpu().numpy()


@pytest.mark.parametrize("name", sorted(C.SELECT_CASES))
def test_select_on_crafted_score_maps(name):
    """gaps: the cut's tie list across several 4096-pixel chunks with `need` below the number of ties (ties_300, need_1); a level with
    exactly n_l candidates (exactly_n) and with exactly 2 n_l (exactly_2n)"""
    L.init(0)
    g, score, hist = C.select_case(name)
    want = R.select(g[0], score[0], int(T.features_per_level()[0]))
    kp, resp, counts = call_select(g, score, hist)
    n = len(want)
    assert list(counts) == [n] + [0] * (NL - 1) + [n]                                  # (the prefilled total is overwritten)
    assert kp[:n, :4].tolist() == [[0, x, y, s] for (x, y, s, _) in want]
    assert np.array_equal(resp[:n].view(np.uint64), np.array([r for (*_, r) in want], dtype=np.float64).view(np.uint64))
    assert not kp[:n, 4:].any() and np.all(kp[n:] == SENT) and np.all(resp[n:] == SENT)


def call_match(desc, counts):
    frames = len(desc)
    cnt = np.zeros((frames, NL + 1), dtype=np.int32)
    cnt[:, NL] = counts
    d, c = dev(desc.view(np.int32)), dev(cnt)
    m, mc = filled((frames - 1, NF, 4), torch.int32), filled((frames - 1,), torch.int32)
    L.check(L.load_library().bs_orb_match(L.p(d), L.p(c), frames, L.p(m), L.p(mc), L.stream_ptr()), "bs_orb_match")
    return d, c, m.cpu().numpy(), mc.cpu().numpy()


def call_match_pairs(d, c, frames, pairs):
    P = len(pairs)
    m, mc = filled((P + 1, NF, 4), torch.int32), filled((P + 1,), torch.int32)
    pr = dev(np.array(pairs, dtype=np.int32))
    L.check(L.load_library().bs_orb_match_pairs(L.p(d), L.p(c), frames, L.p(pr), P, L.p(m), L.p(mc), L.stream_ptr()), "bs_orb_match_pairs")
    return m.cpu().numpy(), mc.cpu().numpy()


def assert_match_rows(got, count, want, where):
    M = len(want)
    assert int(count) == M, (where, int(count), M)
    assert np.array_equal(got[:M, :3], want) and not got[:M, 3].any(), where
    assert np.all(got[M:] == SENT), where                                             # nothing written behind the matches


@pytest.mark.parametrize("name", C.MATCH_CASES)
def test_match_and_match_pairs_on_crafted_descriptor_sets(name):
    """gaps: match with n1 = n2 = 500 and every LDS array used to its last element; n1 != n2 by a wide margin, n1 = 0 or n2 = 0 with the
    other side non-zero; the lowest-index rule on equal distances in both directions (identical_64, triples); the stable order
    (one_distance).  bs_orb_match_pairs runs every ordered pair of the frames -- (i, i), (j, i) after (i, j) -- and one pair twice; each
    row is the statement's and, for (p, p + 1), bs_orb_match's bit for bit."""
    L.init(0)
    desc, counts = C.match_case(name)
    sets = C.clamped(desc, counts)
    frames = len(desc)
    want = functools.lru_cache(maxsize=None)(lambda a, b: R.match(sets[a], sets[b]))
    d, c, m, mc = call_match(desc, counts)
    for p in range(frames - 1):
        assert_match_rows(m[p], mc[p], want(p, p + 1), ("match", p))
    pairs = [(a, b) for a in range(frames) for b in range(frames)] + [(0, 1)]
    pm, pc = call_match_pairs(d, c, frames, pairs)
    for k, (a, b) in enumerate(pairs):
        assert_match_rows(pm[k], pc[k], want(a, b), ("match_pairs", a, b))
        if b == a + 1:
            assert np.array_equal(pm[k], m[a]) and pc[k] == mc[a]
    assert np.all(pm[len(pairs)] == SENT) and pc[len(pairs)] == SENT                  # the rows of a pair that was not asked for


def call_displacement(c, mode, pairs_behind=2):
    cnt = np.zeros((2, NL + 1), dtype=np.int32)
    cnt[:, NL] = c["counts"]
    mt = np.full((1, NF, 4), SENT, dtype=np.int32)                                    # rows at and behind M are not matches: not to be read
    mt[0, :c["M"], :3] = c["matches"][:c["M"]]
    mt[0, :c["M"], 3] = 0
    out = filled((1 + pairs_behind, OUTF), torch.float64)
    K = np.array(c["K"], dtype=np.float64)
    H, W = c["depth"].shape[1:]
    args = [dev(c["pt"]), dev(cnt), dev(mt), dev(np.array([c["M"]], dtype=np.int32)), dev(c["depth"])]
    L.check(L.load_library().bs_orb_displacement(*[L.p(a) for a in args], 2, H, W, SS._ptr(K), SS.ASSOCIATIONS[mode], L.p(out), L.stream_ptr()),
            "bs_orb_displacement")
    return out.cpu().numpy()


@pytest.mark.parametrize("association", ["reference", "matched"])
@pytest.mark.parametrize("name", C.DISP_CASES)
def test_displacement_on_crafted_inputs(name, association):
    """gaps: displacement with M = 500 (two passes of the scan loop, the LDS lists to their last element); a NaN depth (it is not 0: the
    pair counts and the mean is NaN).  Also x = W - 0.5, x = W, x = -0.5, no match, no depth, and n2 < n1 in the reference mode."""
    L.init(0)
    c = C.displacement_case(name)
    want, counts = C.displacement_statement(c, association)
    out = call_displacement(c, association)
    print(name, association, "device", out[0], "statement", want, counts)
    assert out[0, 3:].tolist() == [float(v) for v in counts]
    assert np.array_equal(np.isnan(out[0, :3]), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.all(np.abs(out[0, :3][ok] - want[ok]) <= 1e-12)
    assert np.all(out[1:] == SENT)                                                    # the out rows of other pairs


# ---- nothing written behind the outputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blocks_83x97", "blocks_62x200", "checker"])
def test_nothing_is_written_behind_the_counts(name):
    """every stage into prefilled buffers: the slack between the levels, the rows at and behind a frame's keypoint count and behind a
    pair's match count keep the sentinel, counts[BS_ORB_MAX_LEVELS] is overwritten, and the results are the statement's"""
    L.init(0)
    rgb, bgr = C.frames(name)
    f, _ = C.statement(name)
    n, H, W = rgb.shape[:3]
    e = engine()
    layout, stride = T.level_layout(H, W)
    lib, st, lp, nl = L.load_library(), L.stream_ptr(), SS._ptr(layout), len(layout)
    color = dev(rgb)
    grey, smooth, score = (filled((n, stride), torch.uint8, 0xAB) for _ in range(3))
    hist = filled((n, NL, 256), torch.int32)
    kp, resp, counts = filled((n, NF, 8), torch.int32), filled((n, NF), torch.float64), filled((n, NL + 1), torch.int32)
    pt, desc = filled((n, NF, 2), torch.float32), filled((n, NF, 8), torch.int32)
    L.check(lib.bs_orb_pyramid(L.p(color), n, H, W, int(bgr), lp, nl, stride, L.p(grey), L.p(smooth), st), "bs_orb_pyramid")
    L.check(lib.bs_orb_fast(L.p(grey), n, H, W, lp, nl, stride, L.p(score), L.p(hist), st), "bs_orb_fast")
    L.check(lib.bs_orb_select(L.p(grey), L.p(score), L.p(hist), n, H, W, lp, nl, stride, SS._ptr(e._nfeat), L.p(kp), L.p(resp), L.p(counts), st), "bs_orb_select")
    L.check(lib.bs_orb_describe(L.p(grey), L.p(smooth), n, H, W, lp, nl, stride, SS._ptr(e._scales), L.p(e._cos_sin), L.p(e._pattern), L.p(kp), L.p(counts),
                                L.p(pt), L.p(desc), st), "bs_orb_describe")
    slack = np.ones(stride, dtype=bool)
    for (w, h, off) in layout:
        slack[off:off + w * h] = False
    assert slack.sum() >= 16 * nl
    for nm, buf in (("grey", grey), ("smooth", smooth), ("score", score)):
        b = buf.cpu().numpy()
        assert np.all(b[:, slack] == 0xAB), nm
        for frame in range(n):
            assert all(np.array_equal(b[frame, off:off + w * h].reshape(h, w), f[frame][nm][l]) for l, (w, h, off) in enumerate(layout)), (nm, frame)
    kp_h, resp_h, counts_h, pt_h, desc_h = (t.cpu().numpy() for t in (kp, resp, counts, pt, desc))
    for frame in range(n):
        k = int(f[frame]["counts"].sum())
        assert list(counts_h[frame]) == list(f[frame]["counts"]) + [k]
        assert np.array_equal(kp_h[frame, :k, :7], f[frame]["kp"]) and not kp_h[frame, :k, 7].any()
        assert np.array_equal(desc_h[frame, :k].view(np.uint32), f[frame]["desc"])
        assert np.all(kp_h[frame, k:] == SENT) and np.all(resp_h[frame, k:] == SENT) and np.all(pt_h[frame, k:] == SENT) and np.all(desc_h[frame, k:] == SENT)
    if n == 2:
        m, mc = filled((1, NF, 4), torch.int32), filled((1,), torch.int32)
        L.check(lib.bs_orb_match(L.p(desc), L.p(counts), 2, L.p(m), L.p(mc), st), "bs_orb_match")
        assert_match_rows(m[0].cpu().numpy(), int(mc[0]), C.statement(name)[1], name)


# ---- batch invariance -----------------------------------------------------------------------------------------------------------------------------
PER_FRAME = ("grey", "smooth", "score", "hist", "kp", "resp", "counts", "pt", "desc")


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32) if t.dtype == torch.float32 else t


def test_a_batch_of_five_is_bit_equal_to_the_single_calls():
    """every stage of every frame and every pair of one batch against the one-frame and one-pair calls, in both association modes; three
    of the four pairs touch a frame without keypoints (gap: n1 = 0 or n2 = 0 with the other side non-zero)"""
    rgb = C.batch_of_five()
    depth = dev((0.3 + 0.5 * np.random.default_rng(9).random(size=rgb.shape[:3])).astype(np.float32))
    for association in ("reference", "matched"):
        e = engine(association)
        s = e.match(e.features(rgb))
        out = e._displacement(s, depth)
        totals = s["counts"][:, NL].cpu().tolist()
        assert totals[1] == 0 and totals[4] == 0 and min(totals[0], totals[2], totals[3]) > 100 and int(s["match_counts"][2]) > 20
        pixels = torch.zeros(s["stride"], dtype=torch.bool, device="cuda:0")           # (the slack between the levels is never written)
        for (w, h, off) in s["levels"]:
            pixels[off:off + w * h] = True
        for i in range(5):
            one = e.features(rgb[i:i + 1])
            for k in PER_FRAME:
                a, b = (one[k][0][pixels], s[k][i][pixels]) if k in ("grey", "smooth", "score") else (one[k][0], s[k][i])
                assert torch.equal(bits(a), bits(b)), (association, k, i)
        for p in range(4):
            two = e.match(e.features(rgb[p:p + 2]))
            o = e._displacement(two, depth[p:p + 2])
            assert torch.equal(two["matches"][0], s["matches"][p]) and int(two["match_counts"][0]) == int(s["match_counts"][p]), (association, p)
            assert torch.equal(bits(o[0]), bits(out[p])), (association, p, o[0], out[p])
        assert torch.isnan(out[[0, 1, 3], :3]).all() and (out[[0, 1, 3], 8] == 0).all() and out[2, 8] > 0


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
ENTRY_ARGS = {
    "bs_orb_pyramid": ("color", "batch", "H", "W", "bgr", "levels", "nl", "stride", "grey", "smooth"),
    "bs_orb_fast": ("grey", "batch", "H", "W", "levels", "nl", "stride", "score", "hist"),
    "bs_orb_select": ("grey", "score", "hist", "batch", "H", "W", "levels", "nl", "stride", "nfeat", "kp", "resp", "counts"),
    "bs_orb_describe": ("grey", "smooth", "batch", "H", "W", "levels", "nl", "stride", "scales", "cos_sin", "pattern", "kp", "counts", "pt", "desc"),
    "bs_orb_match": ("desc", "counts", "batch", "matches", "match_counts"),
    "bs_orb_displacement": ("pt", "counts", "matches", "match_counts", "depth", "batch", "H", "W", "K", "mode", "out"),
    "bs_orb_match_pairs": ("desc", "counts", "batch", "pairs", "P", "matches", "match_counts"),
}
SCALARS = ("batch", "H", "W", "bgr", "nl", "stride", "mode", "P")
WITH_LEVELS = ("bs_orb_pyramid", "bs_orb_fast", "bs_orb_select", "bs_orb_describe")


class Rig:
    """valid arguments of every entry point for two 83 x 97 frames; every device buffer prefilled"""

    def __init__(self):
        L.init(0)
        e = engine()
        H, W, n = 83, 97, 2
        self.layout, stride = T.level_layout(H, W)
        self.host = dict(levels=self.layout, nfeat=T.features_per_level(), scales=T.level_scales(), K=np.array(C.FULL_K, dtype=np.float64))
        self.val = dict(batch=n, H=H, W=W, bgr=0, nl=len(self.layout), stride=stride, mode=0, P=1)
        self.t = dict(color=filled((n, H, W, 3), torch.uint8, 7), grey=filled((n + 1, stride), torch.uint8, 7), smooth=filled((n + 1, stride), torch.uint8, 7),
                      score=filled((n + 1, stride), torch.uint8, 0), hist=filled((n, NL, 256), torch.int32, 0), kp=filled((n, NF, 8), torch.int32),
                      resp=filled((n, NF), torch.float64), counts=filled((n, NL + 1), torch.int32, 0), pt=filled((n, NF, 2), torch.float32),
                      desc=filled((n, NF, 8), torch.int32), matches=filled((n, NF, 4), torch.int32), match_counts=filled((n,), torch.int32, 0),
                      depth=filled((n, H, W), torch.float32, 1), out=filled((n, OUTF), torch.float64), pairs=filled((1, 2), torch.int32, 0),
                      cos_sin=e._cos_sin, pattern=e._pattern)
        self.before = {k: v.clone() for k, v in self.t.items()}

    def value(self, name):
        if name in SCALARS:
            return self.val[name]
        return SS._ptr(self.host[name]) if name in self.host else L.p(self.t[name])

    def refused(self, entry, **override):
        """call `entry` with its valid arguments but for `override`: refused with a text that names it, every buffer as before"""
        lib = L.load_library()
        keep = [v for v in override.values() if isinstance(v, np.ndarray)]             # (host arrays stay alive over the call)
        args = [SS._ptr(override[a]) if isinstance(override.get(a), np.ndarray) else override[a] if a in override else self.value(a) for a in ENTRY_ARGS[entry]]
        rc = getattr(lib, entry)(*args, L.stream_ptr())
        text = lib.bs_last_error().decode(errors="replace")
        torch.cuda.synchronize()
        assert rc != 0 and entry in text, (entry, sorted(override), rc, text)
        for k, v in self.t.items():
            assert torch.equal(bits(v), bits(self.before[k])), (entry, sorted(override), k)
        del keep
        return text


@pytest.fixture(scope="module")
def rig():
    return Rig()


def bad_levels(rig):
    lay = rig.layout
    edit = lambda l, c, v: np.array([[v if (i, j) == (l, c) else lay[i, j] for j in range(3)] for i in range(len(lay))], dtype=np.int32)
    nine = np.concatenate([lay, [[lay[7, 0], lay[7, 1], rig.val["stride"]]]]).astype(np.int32)
    seven = lay.copy()
    seven[7, :2] = 7
    return {
        "a stride that is no multiple of 16": dict(stride=rig.val["stride"] + 8),
        "level 0 is not the frame": dict(levels=edit(0, 0, int(lay[0, 0]) - 1)),
        "a level offset inside the previous level": dict(levels=edit(1, 2, 16)),
        "a level larger than its parent": dict(levels=edit(1, 0, int(lay[0, 0]) + 1)),
        "9 levels": dict(levels=nine, nl=9),
        "a 7 x 7 level": dict(levels=seven),
    }


@pytest.mark.parametrize("entry", WITH_LEVELS)
def test_make_levels_refusals(rig, entry):
    """gap: any refusal of make_levels, from each of the four entry points that build the level table"""
    for what, override in bad_levels(rig).items():
        text = rig.refused(entry, **override)
        print(entry, "|", what, "|", text)


def test_select_match_displacement_refusals(rig):
    nf = T.features_per_level()
    many, total = nf.copy(), nf.copy()
    many[0], total[7] = 129, nf[7] + 1
    assert int(total.sum()) == 501 and total.max() <= 128
    off4 = lambda name: L.p(rig.t[name]) + 4
    for entry, override in (("bs_orb_select", dict(nfeat=many)), ("bs_orb_select", dict(nfeat=total)), ("bs_orb_select", dict(score=off4("score"))),
                            ("bs_orb_match", dict(desc=off4("desc"))), ("bs_orb_match_pairs", dict(desc=off4("desc"))), ("bs_orb_match", dict(batch=1)),
                            ("bs_orb_displacement", dict(batch=1)), ("bs_orb_displacement", dict(mode=7))):
        text = rig.refused(entry, **override)
        print(entry, "|", sorted(override), "|", text)


@pytest.mark.parametrize("entry", sorted(ENTRY_ARGS))
def test_null_pointer_refusals(rig, entry):
    for a in ENTRY_ARGS[entry]:
        if a not in SCALARS:
            assert "null" in rig.refused(entry, **{a: None}), (entry, a)
