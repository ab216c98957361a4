"""The RANSAC and FPFH entry points of csrc/global_registration.hip one at a time, called through bodyslam_amd._lib, each against its stage of
the numpy statement (tests/_global_registration_ref.py: hypotheses, score, winner_key, refit_partials, refit_finish, spfh, fpfh_from_spfh):
correspondences at the tile and block edges (3, 4, 255, 256, 257, 513, 1025), several LDS tiles per split in the score, 65 partial rows in
the refit (the second trip of column_sum), chunk offsets up to the cap h0 + count = 2^31 - 1, the winner's key across chunks, decisions
exactly ON their thresholds (inputs whose arithmetic is exact), the refit state machine, bad entries in the CSR lists and in the score's
list, and the refusals.  Every output has a poisoned tail (NaN, 0x5a5a5a5a) beyond the rows the call owns, which must stay as it was.

Integers and fixed-order fp64 sums are compared exactly -- after `G.assert_clear` has shown that every decision of the input lies clear of
its threshold (tests/test_global_registration_cpu.py shows the same on the CPU) --, transforms that went through the SVD (Jacobi on the
device, LAPACK in the statement) within test_global_registration_gpu.py's T_TOL."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _global_registration_ref as G  # noqa: E402
from test_global_registration_gpu import T_TOL  # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
TAU, SEED = G.STAGE_TAU, 5
SENTINEL = 0x5a5a5a5a
TOP = (1 << 31) - 1                                                        # the cap: h0 + count <= TOP
PLANTED = dict(G.STAGE_PLANTED)
IDENTITY = np.eye(4)[:3]


@pytest.fixture(scope="module")
def L():
    from bodyslam_amd import _lib
    _lib.init(0)
    return _lib


def dev():
    return torch.device("cuda:0")


def up(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev())


def nan64(n):
    return torch.full((n,), float("nan"), dtype=torch.float64, device=dev())


def mark32(n):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=dev())


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def poisoned(t):
    """a tail (or a whole buffer) still holds what nan64 / mark32 put there"""
    if t.dtype == torch.int32:
        return bool((t == SENTINEL).all())
    return same_bits(t, torch.full_like(t, float("nan")))


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (P, Q, the [c, 6] table on the device)"""
    if name == "blocks":
        P, Q = G.blocks_scene()
    elif name == "exact":
        P, Q = G.exact_scene()
    else:
        P, Q = G.planted_scene(int(name), PLANTED[int(name)])
    P.setflags(write=False)
    Q.setflags(write=False)
    return P, Q, up(np.concatenate([P, Q], 1))


@functools.lru_cache(maxsize=None)
def found(name):
    """the statement's whole run on a planted scene, once"""
    P, Q, _ = scene(name)
    r = G.ransac(P, Q, TAU, max_iteration=512 if len(P) > 2000 else 4096)
    G.assert_clear(r["margin"])
    return r


def run_hypotheses(L, corr, h0, count, s, tau=TAU, seed=SEED, spare=3):
    fits, valid = nan64(12 * (count + spare)), mark32(count + spare)
    L.gr_hypotheses(corr, seed, h0, count, s, tau, fits, valid)
    assert poisoned(fits[12 * count:]) and poisoned(valid[count:]), "rows >= count were written"
    return fits[:12 * count].cpu().numpy().reshape(count, 3, 4), valid[:count].cpu().numpy()


def check_hypotheses(got_fits, got_valid, fits, valid, what):
    """valid exact; the identity bit for bit where the statement has no fit (edge-length checker or rank test), T_TOL elsewhere"""
    assert np.array_equal(got_valid, valid.astype(np.int32)), what
    fitted = ~(fits == IDENTITY).all((1, 2))
    assert same_bits(got_fits[~fitted], np.tile(IDENTITY, (int((~fitted).sum()), 1, 1))), what
    err = float(np.abs(got_fits[fitted] - fits[fitted]).max(initial=0.0))
    assert err <= T_TOL, (what, err)
    return err, int(fitted.sum())


# ---- A: hypotheses ------------------------------------------------------------------------------------------------------------------------------
CHUNKS = ((0, 1), (0, 255), (0, 256), (0, 257), (4096, 257), (TOP - 257, 257))


@pytest.mark.parametrize("name", ["3", "4", "255", "257", "513", "blocks"])
def test_hypotheses_at_the_edges(L, name):
    P, Q, corr = scene(name)
    worst = 0.0
    for s in (0.9, 0.5):
        for h0, count in CHUNKS:
            ids, valid, fits, margin = G.hypotheses(P, Q, SEED, h0, count, s, TAU)
            G.assert_clear(margin)
            got_fits, got_valid = run_hypotheses(L, corr, h0, count, s)
            err, fitted = check_hypotheses(got_fits, got_valid, fits, valid, (name, s, h0, count))
            worst = max(worst, err)
            if name == "blocks" and count == 257:                                       # the degenerate samples are there and have no fit
                line, point = (ids < 6).all(1), ((ids >= 6) & (ids < 9)).sum(1) >= 2
                assert line.sum() >= 3 and point.sum() >= 3 and not valid[line | point].any() and (fits[line | point] == IDENTITY).all()
            if (h0, count, s) == (0, 257, 0.9):
                assert valid.any() or name == "blocks"
                again = run_hypotheses(L, corr, h0, count, s)
                assert same_bits(again[0], got_fits) and np.array_equal(again[1], got_valid)
    print(name, "largest |fit - statement|", worst)


def test_hypotheses_on_the_edge_length_threshold(L):
    """the exact scene: at edge_length_threshold = 1 every check is ls == lt, which `>=` passes; Q grown by exactly 1 + 2^-20 passes none"""
    P, Q, corr = scene("exact")
    count = 1025
    for s in (1.0, 0.9):
        ids, valid, fits, margin = G.hypotheses(P, Q, SEED, 0, count, s, TAU)
        assert valid.all() and ((margin == 0.0) if s == 1.0 else (margin >= G.MARGIN))
        got_fits, got_valid = run_hypotheses(L, corr, 0, count, s)
        assert got_valid.all()
        check_hypotheses(got_fits, got_valid, fits, valid, s)
    grown = Q * (1.0 + 2.0 ** -20)
    ids, valid, fits, margin = G.hypotheses(P, grown, SEED, 0, count, 1.0, TAU)
    G.assert_clear(margin)
    assert not valid.any() and (fits == IDENTITY).all()
    got_fits, got_valid = run_hypotheses(L, up(np.concatenate([P, grown], 1)), 0, count, 1.0)
    assert not got_valid.any() and same_bits(got_fits, fits)


# ---- B: score -------------------------------------------------------------------------------------------------------------------------------------
LEAD = 4                                                                   # rows in front of and behind the tables: a true fit each, so that a
SPLITS = (1, 2, 3, 5, 65535)                                               # list entry that slips past its check counts inliers where it must not


def run_score(L, corr, fits, lst, count, splits, tau):
    """fits [count, 3, 4] -> int64 [count]; the tables lie inside larger buffers whose other rows hold a true pose and the sentinel"""
    fbuf = up(np.concatenate([np.tile(G.STAGE_POSE[:3], (LEAD, 1, 1)), fits, np.tile(G.STAGE_POSE[:3], (LEAD, 1, 1))]).reshape(-1))
    sbuf = mark32(count + 2 * LEAD)
    score = sbuf[LEAD:LEAD + count]
    score.zero_()
    L.gr_score(corr, fbuf[12 * LEAD:12 * (LEAD + count)], up(lst, np.int32), count, splits, tau, score)
    assert poisoned(sbuf[:LEAD]) and poisoned(sbuf[LEAD + count:]), "a score outside 0 .. count - 1 was written"
    return score.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("name", ["3", "255", "256", "257", "513", "1025"])
def test_score_tiles_splits_and_lists(L, name):
    """splits = 1 at c = 513 and 1025 walks three and five LDS tiles in one block; 65535 splits leave most blocks without a row"""
    P, Q, corr = scene(name)
    count = 300
    rng = np.random.default_rng(int(name))
    fits = G.hypotheses(P, Q, SEED, 0, count, 0.5, TAU)[2]                  # every hypothesis is scored, valid or not: the kernel does not ask
    near = np.tile(G.STAGE_POSE[:3], (count // 2, 1, 1))                    # every other one: the true pose moved by about tau, which counts
    near[:, :, 3] += rng.normal(0.0, 0.6 * TAU, (count // 2, 3))            # some of the true rows of every tile
    fits[1::2] = near
    margins = []
    full = G.score(P, Q, fits, np.arange(count), TAU, margins)
    G.assert_clear(min(margins))
    assert full.max() >= 0.9 * PLANTED[int(name)] and len(np.unique(full)) >= min(20, PLANTED[int(name)])
    order = rng.permutation(count)
    padded = np.concatenate([order[:40], [-1, count, count + LEAD - 1], order[40:90]])   # (out of range, but inside the buffers)
    for lst in (order[:1], order[:256], order[:257], rng.permutation(padded)):
        want = G.score(P, Q, fits, lst, TAU)
        assert np.array_equal(want, np.where(np.isin(np.arange(count), lst), full, 0))
        for splits in SPLITS:
            got = run_score(L, corr, fits, lst, count, splits, TAU)
            assert np.array_equal(got, want), (name, len(lst), splits, np.nonzero(got != want)[0][:8], got[got != want][:8], want[got != want][:8])


def test_score_on_the_distance_threshold(L):
    """r^2 < tau^2 is strict: the identity fit, tau = 2^-9, Q - P = (2^-9, 0, 0) / (2^-9 - 2^-30, 0, 0) / (0, 0, -2^-9) in turn: only the second
    kind counts.  259 rows: a second tile."""
    P = scene("exact")[0][:259]
    step = np.array([[2.0 ** -9, 0.0, 0.0], [2.0 ** -9 - 2.0 ** -30, 0.0, 0.0], [0.0, 0.0, -2.0 ** -9]])
    Q = P + step[np.arange(259) % 3]
    assert np.array_equal(Q - P, step[np.arange(259) % 3])                              # exact
    fits = np.tile(IDENTITY, (4, 1, 1))
    want = G.score(P, Q, fits, [0, 1, 2, 3], 2.0 ** -9)
    assert want.tolist() == [86] * 4 and int((np.arange(259) % 3 == 1).sum()) == 86
    corr = up(np.concatenate([P, Q], 1))
    for splits in (1, 2):
        assert np.array_equal(run_score(L, corr, fits, [3, 1, 0, 2], 4, splits, 2.0 ** -9), want)


# ---- C: the winner -------------------------------------------------------------------------------------------------------------------------------
def run_winner(L, best, scores, h0):
    count = len(scores)
    buf = up(np.concatenate([scores, [1 << 30] * 3]), np.int32)                           # (a score past `count` would win at once)
    L.gr_winner(buf, count, h0, best)
    return int(best.cpu()) & ((1 << 64) - 1)


@pytest.mark.parametrize("count", [1, 255, 256, 257])
def test_winner_key(L, count):
    """integers only: ties inside a chunk and across chunks, a larger score later, zeros, the last hypothesis below the cap"""
    first = np.arange(count) % 7
    first[[0, count // 2, count - 1]] = 9                                                # a tie: the lowest h wins
    best = torch.zeros(1, dtype=torch.int64, device=dev())
    key = G.winner_key(0, first, 0)
    assert run_winner(L, best, first, 0) == key and G.decode(key) == (9, 0)
    tie = np.zeros(count, np.int64)
    tie[count - 1] = 9
    assert run_winner(L, best, tie, 4096) == key == G.winner_key(key, tie, 4096)          # an equal best in a later chunk does not displace
    more = tie + (np.arange(count) == count // 2)
    more[count - 1] = 10
    key2 = G.winner_key(key, more, 8192)
    assert run_winner(L, best, more, 8192) == key2 and G.decode(key2) == (10, 8192 + count - 1)
    assert run_winner(L, best, np.zeros(count, np.int64), 12288) == key2                 # zeros never enter
    fresh = torch.zeros(1, dtype=torch.int64, device=dev())
    assert run_winner(L, fresh, np.zeros(count, np.int64), 0) == 0
    last = np.zeros(count, np.int64)
    last[[count - 1, count // 2]] = 2
    key3 = G.winner_key(0, last, TOP - count)
    assert run_winner(L, fresh, last, TOP - count) == key3 and G.decode(key3) == (2, TOP - count + count // 2)
    only = np.zeros(count, np.int64)
    only[count - 1] = 2
    assert run_winner(L, fresh, only, TOP - count) == key3                               # h = 2^31 - 2, the same score: the lower h stays
    only[count - 1] = 3
    assert G.decode(run_winner(L, fresh, only, TOP - count)) == (3, TOP - 1)


def test_winner_fit_is_stage_a_bit_for_bit(L):
    P, Q, corr = scene("blocks")
    ids, valid, fits, margin = G.hypotheses(P, Q, SEED, 0, 257, 0.9, TAU)
    G.assert_clear(margin)
    line = (ids < 6).all(1)
    edge = ((ids >= 6) & (ids < 9)).sum(1) >= 2
    table_fits, table_valid = run_hypotheses(L, corr, 0, 257, 0.9)
    picks = [int(np.nonzero(valid)[0][0]), int(np.nonzero(edge)[0][0]), int(np.nonzero(line)[0][0]), 256, TOP - 1]
    for h in picks:
        one_fit, one_valid = run_hypotheses(L, corr, h, 1, 0.9)
        state = nan64(16 + 4)
        L.gr_winner_fit(corr, SEED, h, 0.9, TAU, state)
        assert poisoned(state[16:])
        got = state[:16].cpu().numpy()
        assert same_bits(got[:12], one_fit.reshape(12)) and got[12] == float(one_valid[0]) and same_bits(got[13:], np.zeros(3))
        if h < 257:
            assert same_bits(got[:12], table_fits[h].reshape(12)) and got[12] == float(table_valid[h]) == float(valid[h])
    assert valid[picks[0]] and not valid[picks[1]] and not valid[picks[2]]


# ---- D: the refit ----------------------------------------------------------------------------------------------------------------------------------
def make_state(T, status=1.0, rounds=0.0):
    s = np.zeros(16)
    s[:12], s[12], s[15] = np.asarray(T)[:3].reshape(12), status, rounds
    return s


def run_step(L, corr, state, tau, c):
    """-> (mask int32 [c], partial float64 [nb, 17]) with the tails checked; state [>= 16] on the device"""
    nb = -(-c // 256)
    mbuf, pbuf = mark32(c + 5), nan64((nb + 2) * 17)
    L.gr_refit_step(corr, state, tau, mbuf[:c], pbuf)
    assert poisoned(mbuf[c:]) and poisoned(pbuf[nb * 17:]), "the refit step wrote past its rows"
    return mbuf[:c], pbuf[:nb * 17]


@pytest.mark.parametrize("name", ["3", "255", "256", "257", "16385"])
def test_refit_step_partials_bit_for_bit(L, name):
    P, Q, corr = scene(name)
    c = len(P)
    T = found(name)["T"]
    margins = []
    mask, partial = G.refit_partials(P, Q, T, TAU, margins)
    G.assert_clear(min(margins))
    state = up(make_state(T))
    got_mask, got_partial = run_step(L, corr, state, TAU, c)
    assert np.array_equal(got_mask.cpu().numpy(), mask.astype(np.int32)) and mask.sum() == found(name)["inliers"]
    got = got_partial.cpu().numpy().reshape(-1, 17)
    diff = np.abs(got - partial).max()
    print(name, "inliers", int(mask.sum()), "partial rows", len(partial), "largest |partial - statement|", diff)
    assert same_bits(got, partial), (name, diff, np.argwhere(bits(got) != bits(partial))[:8])
    assert same_bits(state, make_state(T))                                                # (the step reads the state only)


@pytest.mark.parametrize("name", ["257", "16385"])
def test_refit_finish(L, name):
    """16385 correspondences are 65 partial rows: lane 0 of column_sum adds a second row"""
    P, Q, corr = scene(name)
    c = len(P)
    T = found(name)["T"]
    before = make_state(T, rounds=2.0)
    partial = run_step(L, corr, up(before), TAU, c)[1]
    rows = partial.cpu().numpy().reshape(-1, 17)
    assert len(rows) == -(-c // 256) and (name != "16385" or len(rows) == 65)
    for final in (1, 0):
        want = G.refit_finish(rows, before, final)
        state = torch.cat([up(before), nan64(4)])
        L.gr_refit_finish(partial, c, final, state)
        got = state[:16].cpu().numpy()
        assert poisoned(state[16:]) and got[15] == 3.0 == want[15] and got[12] == 1.0 == want[12]
        if final:
            assert same_bits(got[:13], before[:13]) and same_bits(got[13:15], want[13:15]) and got[13] == found(name)["inliers"]
        else:
            err = np.abs(got[:12] - want[:12]).max()
            print(name, "refit |T - statement|", err)
            assert err <= T_TOL and same_bits(got[13:15], before[13:15]) and not same_bits(got[:12], before[:12])


def refit_round(L, P, Q, tau, before, final):
    """one step + finish from the state `before` -> (the state after, mask, the statement's state after)"""
    c = len(P)
    corr = up(np.concatenate([P, Q], 1))
    state = torch.cat([up(before), nan64(4)])
    mask, partial = run_step(L, corr, state, tau, c)
    smask, spartial = G.refit_partials(P, Q, before[:12].reshape(3, 4), tau)
    assert np.array_equal(mask.cpu().numpy(), smask.astype(np.int32)) and same_bits(partial.cpu().numpy().reshape(-1, 17), spartial)
    L.gr_refit_finish(partial, c, final, state)
    assert poisoned(state[16:])
    return state[:16].cpu().numpy(), smask, G.refit_finish(spartial, before, final)


def test_refit_state_machine(L):
    """exact inputs, the identity as the state: Q - P = (d, 0, 0) with d = 0, 1, 2 and then 3 .. 7 in units of 1 / 1024; tau = 2.5 / 1024 has
    exactly three inliers, tau = 1.5 / 1024 exactly two"""
    P = scene("exact")[0]
    c = len(P)
    d = np.where(np.arange(c) < 3, np.arange(c), 3 + np.arange(c) % 5) / 1024.0
    Q = P + np.stack([d, np.zeros(c), np.zeros(c)], 1)
    before = make_state(np.eye(4), rounds=1.0)
    for final in (0, 1):
        got, mask, want = refit_round(L, P, Q, 2.5 / 1024.0, before, final)           # three inliers: the fit stands
        assert mask.sum() == 3 and got[12] == 1.0 == want[12] and got[15] == 2.0 == want[15]
        assert (same_bits(got[:13], before[:13]) and same_bits(got[13:15], want[13:15]) and got[13] == 3.0) if final else \
            (np.abs(got[:12] - want[:12]).max() <= T_TOL and same_bits(got[13:15], before[13:15]))
        got, mask, want = refit_round(L, P, Q, 1.5 / 1024.0, before, final)           # two: degenerate, the transform left alone, the round counted
        assert mask.sum() == 2 and got[12] == 0.0 == want[12] and got[15] == 2.0 == want[15]
        assert same_bits(got[:12], before[:12]) and same_bits(got[13:15], before[13:15])
    line = P.copy()                                                                     # five collinear inliers: the rank test
    line[:5] = np.arange(5.0)[:, None] * np.array([1.0, 2.0, -1.0]) / 1024.0
    lq = line + 1.0
    lq[:5] = line[:5]
    got, mask, want = refit_round(L, line, lq, TAU, before, 0)
    assert mask.sum() == 5 and got[12] == 0.0 == want[12] and got[15] == 2.0 and same_bits(got[:12], before[:12]) and same_bits(got[13:15], before[13:15])
    got, mask, want = refit_round(L, line, lq, TAU, before, 1)                           # (the final round does not fit: five inliers stand)
    assert got[12] == 1.0 == want[12] and got[13] == 5.0 and same_bits(got[13:15], want[13:15])
    dead = make_state(np.eye(4), status=0.0, rounds=1.0)                                 # a status-0 state: nobody writes anything
    corr = up(np.concatenate([P, P], 1))
    nb = -(-c // 256)
    state = torch.cat([up(dead), nan64(4)])
    mbuf, pbuf = mark32(c), nan64(nb * 17)
    L.gr_refit_step(corr, state, TAU, mbuf, pbuf)
    assert poisoned(mbuf) and poisoned(pbuf)
    sums = up(G.refit_partials(P, P, np.eye(4), TAU)[1].reshape(-1))                     # (partials that WOULD give a fit)
    for final in (0, 1):
        L.gr_refit_finish(sums, c, final, state)
        assert same_bits(state[:16], dead) and poisoned(state[16:])
    for status in (2.0, -1.0, float("nan")):                                             # (anything but 1 is not a standing fit)
        other = make_state(np.eye(4), status=status)
        state = up(other)
        L.gr_refit_step(corr, state, TAU, mbuf, pbuf)
        L.gr_refit_finish(sums, c, 0, state)
        assert poisoned(mbuf) and poisoned(pbuf) and same_bits(state, other)


# ---- FPFH on lists edited by hand ----------------------------------------------------------------------------------------------------------------
SPARE = 2                                                                  # rows beyond n in every table: a neighbour that slips past its check
#                                                                            reads them (mapped memory, and values that count) instead of faulting


def sanitised(row_start, index, d2, n, first, m):
    """what the header promises: a row whose bounds are not 0 <= b <= e <= total is empty; an entry outside 0 .. n - 1 takes part in nothing
    but keeps its place in the row (the place decides which lane adds an entry: the statement's own rule for d2 == 0) -> CSR lists over
    all n rows, empty outside first .. first + m - 1"""
    total = len(index)
    rs, ii, dd = [0], [], []
    for i in range(n):
        if first <= i < first + m:
            b, e = int(row_start[i - first]), int(row_start[i - first + 1])
            if 0 <= b <= e <= total:
                bad = (index[b:e] < 0) | (index[b:e] >= n)
                ii.append(np.where(bad, 0, index[b:e]))
                dd.append(np.where(bad, f32(0), d2[b:e]))
        rs.append(sum(len(a) for a in ii))
    return np.array(rs, np.int64), np.concatenate(ii).astype(np.int32), np.concatenate(dd).astype(f32)


@functools.lru_cache(maxsize=None)
def edited_lists():
    pts, nrm, rows = G.constructed_cloud()
    n = len(pts)
    rs, idx, d2 = (np.array(a) for a in G.lists(pts, G.CONSTRUCTED_RADIUS))
    rs, idx, d2 = rs.astype(np.int64), idx.astype(np.int32), d2.astype(f32)
    total = len(idx)
    a, b, e = rows["k64"] + 3, rows["k65"] + 2, rows["k63"] + 10
    assert rs[a + 1] - rs[a] == 65 and rs[b + 1] - rs[b] == 66 and rs[e + 1] - rs[e] == 64
    assert d2[rs[a] + 1] != 0 and d2[rs[a] + 5] != 0 and d2[rs[a] + 64] != 0
    idx[rs[a] + 1], idx[rs[a] + 5], idx[rs[a] + 64] = -1, n, n + 1                       # (the last one in lane 0's second trip)
    rs[b + 1] = rs[b] - 3                                                               # row b decreases; row b + 1 grows by row b and three entries
    rs[e + 1] = total + 7                                                               # rows e and e + 1 reach past the lists
    twins, zero_normal = rows["twins"], rows["normals"]
    assert (d2[rs[twins]:rs[twins + 1]] == 0).sum() == 2                                 # an entry with d2 = 0 besides the point itself
    assert zero_normal in idx[rs[zero_normal + 2]:rs[zero_normal + 3]]                  # a neighbour whose SPFH k is 0
    return pts, nrm, n, rs, idx, d2


def fpfh_tables(pts, nrm, n, counts, k):
    """the packed point table and the SPFH table with SPARE live rows beyond n: a copy of a dense cluster's point, counts that would add"""
    table = np.zeros((n + SPARE, 8), f32)
    table[:n, 0:3], table[:n, 4:7] = pts, nrm
    table[n:, 0:3], table[n:, 4:7] = pts[G.constructed_cloud()[2]["k64"] + 1] + f32(0.0005), [0.0, 0.6, 0.8]
    spfh = np.zeros((n + SPARE, 36), np.int32)
    spfh[:n, :33], spfh[:n, 33] = counts, k
    spfh[n:, :33], spfh[n:, 33] = 3, 33
    return table, spfh


@pytest.mark.parametrize("first,drop", [(0, 0), (7, 20)])
def test_fpfh_entries_on_edited_lists(L, first, drop):
    """bs_fpfh_spfh and bs_fpfh_features called directly: entries -1, n and n + 1, a decreasing row_start, a row_start past the lists, rows
    first .. first + m - 1 of n only"""
    pts, nrm, n, rs, idx, d2 = edited_lists()
    m = n - first - drop
    sub = rs[first:first + m + 1]
    clean = sanitised(sub, idx, d2, n, first, m)
    counts, k, margins = G.spfh(pts, nrm, *clean)
    G.assert_clear(margins)
    table, packed = fpfh_tables(pts, nrm, n, counts, k)
    lib = L.load_library()
    lists = (up(sub), up(idx), up(d2))
    own = slice(first, first + m)
    got = mark32((n + SPARE) * 36).reshape(n + SPARE, 36)
    t = up(table)
    L.check(lib.bs_fpfh_spfh(L.p(t), n, *(L.p(x) for x in lists), m, first, len(idx), L.p(got), L.stream_ptr()), "bs_fpfh_spfh")
    assert poisoned(got[:first]) and poisoned(got[first + m:]), "rows outside first .. first + m - 1 were written"
    g = got[own].cpu().numpy()
    assert np.array_equal(g[:, :33], counts[own]) and np.array_equal(g[:, 33], k[own]) and not g[:, 34:].any()
    emptied = [i for i in range(first, first + m) if clean[0][i + 1] == clean[0][i] and rs[i + 1] != rs[i]]
    assert len(emptied) == 3 and not k[emptied].any()                                    # the decreasing row and the two past the lists
    # the second pass on the statement's complete SPFH (every neighbour's row exists)
    full_counts, full_k, _ = G.spfh(pts, nrm, *sanitised(rs, idx, d2, n, 0, n))
    table, packed = fpfh_tables(pts, nrm, n, full_counts, full_k)
    want = G.fpfh_from_spfh(full_counts, full_k, *clean)[0]
    feat = torch.full(((n + SPARE), 33), float("nan"), dtype=torch.float32, device=dev())
    s = up(packed)
    L.check(lib.bs_fpfh_features(L.p(s), n, *(L.p(x) for x in lists), m, first, len(idx), L.p(feat), L.stream_ptr()), "bs_fpfh_features")
    assert bool(torch.isnan(feat[:first]).all()) and bool(torch.isnan(feat[first + m:]).all())
    assert same_bits(feat[own], want[own]) and np.abs(want[own]).max() > 0 and not want[emptied].any()
    assert same_bits(s, packed) and same_bits(t, table)


# ---- the refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(L):
    """every BS_REQUIRE of the nine entries -- null pointers, alignments, ranges --: the call fails, the library's message names the entry,
    nothing is written.  (What comes before them, "call bs_init first", cannot be reached in a process that has initialised the library.)"""
    from bodyslam_amd._lib import BodySlamHipError
    lib = L.load_library()
    P, Q, corr5 = scene("257")
    c, count = 257, 8
    fits, valid, score, best = nan64(12 * count), mark32(count), mark32(count), torch.zeros(1, dtype=torch.int64, device=dev())
    state, mask, partial = nan64(16), mark32(c), nan64(2 * 17)
    lst = up(np.arange(count), np.int32)
    shifted = torch.zeros(c * 6 + 2, dtype=torch.float64, device=dev())[1:1 + c * 6]     # 8 bytes past a 16-byte boundary
    assert shifted.data_ptr() % 16 == 8 and corr5.data_ptr() % 16 == 0
    # the CSR entries: a table of 10 points, 4 rows of lists; the match: 4 source rows, 5 target rows
    n, m = 10, 4
    table, packed = torch.zeros(n, 8, dtype=torch.float32, device=dev()), torch.zeros(n, 36, dtype=torch.int32, device=dev())
    rs, idx, d2 = up(np.array([0, 2, 4, 6, 8], np.int64)), up(np.arange(8) % n, np.int32), up(np.ones(8), f32)
    out_s, out_f = mark32(n * 36), torch.full((n * 33,), float("nan"), dtype=torch.float32, device=dev())
    src, tgt = torch.ones(4, 33, dtype=torch.float32, device=dev()), torch.ones(5, 33, dtype=torch.float32, device=dev())
    mbest = torch.full((4,), -1, dtype=torch.int64, device=dev())
    p, st = L.p, L.stream_ptr()
    ptr = dict(corr=p(corr5), fits=p(fits), valid=p(valid), score=p(score), best=p(best), state=p(state), mask=p(mask), partial=p(partial), lst=p(lst),
               table=p(table), packed=p(packed), rs=p(rs), idx=p(idx), d2=p(d2), out_s=p(out_s), out_f=p(out_f), src=p(src), tgt=p(tgt), mbest=p(mbest))
    assert all(v % 16 == 0 for v in ptr.values())
    inf, nan, big = float("inf"), float("nan"), 1.0 + 2.0 ** -20

    def hyp(c=c, h0=0, count=count, s=0.9, tau=TAU, **o):
        a = dict(ptr, **o)
        return lib.bs_gr_hypotheses(a["corr"], c, SEED, h0, count, s, tau, a["fits"], a["valid"], st)

    def sco(c=c, n_valid=count, count=count, splits=1, tau=TAU, **o):
        a = dict(ptr, **o)
        return lib.bs_gr_score(a["corr"], c, a["fits"], a["lst"], n_valid, count, splits, tau, a["score"], st)

    def win(count=count, h0=0, **o):
        a = dict(ptr, **o)
        return lib.bs_gr_winner(a["score"], count, h0, a["best"], st)

    def wfit(c=c, h=0, s=0.9, tau=TAU, **o):
        a = dict(ptr, **o)
        return lib.bs_gr_winner_fit(a["corr"], c, SEED, h, s, tau, a["state"], st)

    def step(c=c, tau=TAU, **o):
        a = dict(ptr, **o)
        return lib.bs_gr_refit_step(a["corr"], c, a["state"], tau, a["mask"], a["partial"], st)

    def fin(c=c, **o):
        a = dict(ptr, **o)
        return lib.bs_gr_refit_finish(a["partial"], c, 0, a["state"], st)

    def spf(n=n, m=m, first=0, total=8, **o):
        a = dict(ptr, **o)
        return lib.bs_fpfh_spfh(a["table"], n, a["rs"], a["idx"], a["d2"], m, first, total, a["out_s"], st)

    def fea(n=n, m=m, first=0, total=8, **o):
        a = dict(ptr, **o)
        return lib.bs_fpfh_features(a["packed"], n, a["rs"], a["idx"], a["d2"], m, first, total, a["out_f"], st)

    def mat(m=4, n=5, splits=1, **o):
        a = dict(ptr, **o)
        return lib.bs_feature_match(a["src"], m, a["tgt"], n, splits, a["mbest"], st)
    calls = []
    for fn, name in ((hyp, "bs_gr_hypotheses"), (sco, "bs_gr_score"), (wfit, "bs_gr_winner_fit"), (step, "bs_gr_refit_step")):
        calls += [(name, fn, dict(c=2)), (name, fn, dict(corr=p(shifted)))] + [(name, fn, dict(tau=t)) for t in (0.0, -1.0, nan, inf)]
    calls += [("bs_gr_refit_finish", fin, dict(c=2))]
    for fn, name in ((hyp, "bs_gr_hypotheses"), (wfit, "bs_gr_winner_fit")):
        calls += [(name, fn, dict(s=0.0)), (name, fn, dict(s=big)), (name, fn, dict(s=nan))]
    for fn, name in ((hyp, "bs_gr_hypotheses"), (win, "bs_gr_winner")):
        calls += [(name, fn, dict(count=0)), (name, fn, dict(count=(1 << 20) + 1)), (name, fn, dict(h0=TOP + 1 - 257, count=257)), (name, fn, dict(count=-1))]
    calls += [("bs_gr_score", sco, dict(count=0, n_valid=0)), ("bs_gr_score", sco, dict(count=(1 << 20) + 1)), ("bs_gr_score", sco, dict(n_valid=0)),
              ("bs_gr_score", sco, dict(n_valid=count + 1)), ("bs_gr_score", sco, dict(splits=0)), ("bs_gr_score", sco, dict(splits=65536)),
              ("bs_gr_winner_fit", wfit, dict(h=TOP + 1))]
    for fn, name in ((spf, "bs_fpfh_spfh"), (fea, "bs_fpfh_features")):
        calls += [(name, fn, kw) for kw in (dict(first=n - m + 1), dict(total=-1), dict(first=-1), dict(m=0), dict(n=0), dict(m=n + 1), dict(total=1 << 31))]
    calls += [("bs_feature_match", mat, kw) for kw in (dict(m=0), dict(n=0), dict(m=1 << 31), dict(splits=0), dict(splits=65536))]
    # a null pointer in every place that takes one
    for fn, name, takes in ((hyp, "bs_gr_hypotheses", "corr fits valid"), (sco, "bs_gr_score", "corr fits lst score"), (win, "bs_gr_winner", "score best"),
                            (wfit, "bs_gr_winner_fit", "corr state"), (step, "bs_gr_refit_step", "corr state mask partial"),
                            (fin, "bs_gr_refit_finish", "partial state"), (spf, "bs_fpfh_spfh", "table rs idx d2 out_s"),
                            (fea, "bs_fpfh_features", "packed rs idx d2 out_f"), (mat, "bs_feature_match", "src tgt mbest")):
        calls += [(name, fn, {k: None}) for k in takes.split()]
    # the alignments besides corr's: 16 bytes for the state and the packed tables, 8 for the two 64-bit keys
    calls += [("bs_gr_winner_fit", wfit, dict(state=ptr["state"] + 8)), ("bs_gr_winner", win, dict(best=ptr["best"] + 4)),
              ("bs_fpfh_spfh", spf, dict(table=ptr["table"] + 8)), ("bs_fpfh_spfh", spf, dict(out_s=ptr["out_s"] + 4)),
              ("bs_fpfh_features", fea, dict(packed=ptr["packed"] + 8)), ("bs_feature_match", mat, dict(mbest=ptr["mbest"] + 4))]
    for name, fn, kw in calls:
        with pytest.raises(BodySlamHipError) as err:
            L.check(fn(**kw), "the call")
        said = str(err.value).split(": ", 1)[1]
        assert name in said, (name, kw, str(err.value))
    torch.cuda.synchronize()
    for t in (fits, valid, score, state, mask, partial, out_s):
        assert poisoned(t)
    assert bool(torch.isnan(out_f).all()) and int(best.cpu()) == 0 and bool((mbest == -1).all())
    assert hyp() == 0 and sco() == 0 and spf() == 0 and fea() == 0 and mat() == 0            # (the same calls with good arguments go through)
    torch.cuda.synchronize()
    assert not poisoned(valid) and not poisoned(out_s) and not bool((mbest == -1).any())
