"""Numpy statement of the global registration (csrc/global_registration.hip, bodyslam_amd/registration.py) -- TEST
INFRASTRUCTURE ONLY, independent of the product code.

The roles are Open3D's ``compute_fpfh_feature`` and ``registration_ransac_based_on_feature_matching`` / ``_on_correspondence``.  Open3D is
not available and the reference only calls it: **parity unpinned**.  Restated from Rusu, Blodow & Beetz 2009 (FPFH), Fischler & Bolles 1981
(RANSAC), Kabsch 1976 / Arun, Huang & Blostein 1987 (the fit) and Open3D's documented meaning; the text below is the contract.

lists     the neighbours of point i are the row of `_radius_ref.radius_brute(cloud, cloud, radius)` (with max_nn its first max_nn entries):
          float32 d2, ascending (d2, index).  Entries with d2 == 0 -- the point itself, coincident points -- are left out of both passes but
          keep their place in the row (the place decides which lane adds an entry).
pairs     float64 from the float32 inputs, one operation at a time, the parentheses as written in `pair_features`: p1 = point i, p2 = the
          neighbour.  a1 = n1.dp / d, a2 = n2.dp / d.  |a1| < |a2| (strictly): n1 <-> n2, dp -> -dp, f3 = -a2; else f3 = a1.  v = dp x n1
          normalised (|v| = 0: skipped), w = n1 x v, f2 = v.n2, f1 = the angle of the vector (x, y) = (n1.n2, w.n2).  A zero or non-finite
          normal at either end skips the pair; a skipped pair is not counted in k.
bins      eleven per feature.  f2, f3: floor(11 (f + 1) / 2) clipped to 0 .. 10.  f1: floor(11 (atan2(y, x) + pi) / 2 pi) clipped, stated
          WITHOUT a transcendental function (`sector`): the ten inner edges are the directions +-(2 j + 1) pi / 11, j = 0 .. 4, held as the
          float64 constants EDGE_COS / EDGE_SIN; in the upper half plane (y >= 0) the bin is 5 + #{j: c_j y - s_j x >= 0}, in the lower one
          #{j: c_j y + s_j x >= 0}: half-open sectors.  `margins` measures every decision; `sector` equals the atan2 form wherever the
          margin is positive (asserted in tests/test_global_registration_cpu.py).
SPFH      33 integer counts and k per point: independent of the order of the row.  The value is 100 count / k, 0 for k = 0.
FPFH      acc = sum_j spfh(j) / (double) d2_ij: lane l of 64 adds the entries l, l + 64, ... of the row in order from +0, then the xor
          butterfly 32, 16, .., 1 (`lanes = lanes + lanes[lane ^ o]`), reduce.h's order; lane 0's total.  Each block of eleven is scaled
          to sum 100 when its sum s is positive, v = (acc * 100) / s, with s = (((((a0 + a10) + (a1 + a9)) + (a2 + a8)) + (a3 + a7)) +
          (a4 + a6)) + a5 -- symmetric, so that `mirror` commutes with everything bit for bit.  + spfh(i), one rounding to float32.  A point
          with k = 0 (a non-finite point has k = 0) has a zero row.  The float64 value before the rounding is returned too.
mirror    a global flip of the normals reverses blocks 1 and 3 (f1 -> -f1, f3 -> -f3) and leaves block 2.
match     distance = sum_k (a_k - b_k)^2 in float32, k = 0 .. 32 in order; the match is the minimum of (distance, target index); a row with a
          non-finite value neither matches nor is matched.  mutual: kept when the target row's match, roles exchanged, is that source row.
RANSAC    hypothesis h draws three distinct correspondences with `_loop_closure_ref.sample(seed, 0, h, c)`.  Edge-length checker (before any
          fit): every pair of the three has |ps| >= s |pt| and |pt| >= s |ps|.  Kabsch with its rank test (`_loop_closure_ref.kabsch`).
          Distance checker: the three residuals^2 < tau^2.  score = #(residual^2 < tau^2), 0 for a rejected hypothesis.  Hypotheses run in
          chunks of CHUNK; after a chunk, with best = the highest score so far, the run stops "converged" when
          log(1 - confidence) / log(1 - (best / c)^3) <= the hypotheses tried (best = c: 0), else "max_iteration" after max_iteration.  The
          winner: the highest score, the lowest h.  best < 3: "degenerate", identity, zero mask, h = -1.  Then n_refit rounds of (Kabsch over
          the inliers, recount); fewer than 3 inliers or a collinear set: degenerate.  fitness = inliers / c, inlier_rmse over the inliers.
stages    `ransac` is composed of one function per device entry, each comparable on its own: `hypotheses` (bs_gr_hypotheses and
          bs_gr_winner_fit: the fit is the identity where the edge-length checker or the rank test fails), `score` (bs_gr_score),
          `winner_key` / `decode` (bs_gr_winner: score << 32 | ~h, pure integers), `refit_partials` (bs_gr_refit_step: per block of 256 rows
          the 17 sums count, p, q, q p^T, r^2 over the inliers in the order of reduce.h's block_sum) and `refit_finish` (bs_gr_refit_finish:
          the columns in the order of reduce.h's column_sum, then Kabsch from the sums or the final RMSE, and the 16-field state).
The device computes singular vectors by Jacobi, the statement by LAPACK: transforms agree to about 1e-9, the refit's partial sums and the
RMSE bit for bit, every integer decision exactly as long as `margin` (relative to tau^2) is positive -- `assert_clear` is the condition the
tests hold an input to before they compare integers.  tau is rounded to float32 first, as the public layer rounds it.

Also here, shared by tests/test_global_registration_cpu.py, tests/test_global_registration_gpu.py and
tests/test_global_registration_stages_gpu.py: the inputs (the bumpy pair of tests/_icp_ref.py at two poses, the constructed cloud, the
planted correspondences, the recipe on thinned clouds, the planted / exact scenes of the stage tests)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _loop_closure_ref as LC  # noqa: E402
from _mesh_ops_ref import wave_sum  # noqa: E402
import _radius_ref as RR  # noqa: E402

f32, f64 = np.float32, np.float64
BINS, DIM = 11, 33
CHUNK = 4096
EDGE_COS = np.array([0.9594929736144975, 0.6548607339452851, 0.14231483827328512, -0.4154150130018863, -0.8412535328311811])
EDGE_SIN = np.array([0.2817325568414295, 0.7557495743542583, 0.9898214418809327, 0.9096319953545184, 0.5406408174555978])


# ---- lists ------------------------------------------------------------------------------------------------------------------------------------
def lists(points, radius, max_nn=None):
    """-> (row_start, index, d2) of the cloud on itself"""
    rs, idx, d2 = RR.radius_brute(points, points, radius)
    return (rs, idx, d2) if max_nn is None else RR.first_of_rows(rs, idx, d2, max_nn)


# ---- pair features ----------------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def bin11(f):
    return np.clip(np.floor((11.0 * (f + 1.0)) / 2.0), 0, 10).astype(np.int64)


def sector(x, y):
    x, y = np.asarray(x, f64), np.asarray(y, f64)
    up = np.zeros(x.shape, np.int64)
    dn = np.zeros(x.shape, np.int64)
    for j in range(5):
        up += (EDGE_COS[j] * y - EDGE_SIN[j] * x >= 0.0)
        dn += (EDGE_COS[j] * y + EDGE_SIN[j] * x >= 0.0)
    return np.where(y >= 0.0, 5 + up, dn)


def sector_atan2(x, y):
    """the same bin through atan2: for the cross-check only"""
    return np.clip(np.floor(11.0 * (np.arctan2(y, x) + np.pi) / (2.0 * np.pi)), 0, 10).astype(np.int64)


def _normal_ok(n):
    return np.isfinite(n).all(1) & (n != 0).any(1)


def _edge_distance(t, edges):
    return np.min(np.abs(t[:, None] - np.asarray(edges, f64)[None, :]), 1) if len(t) else np.zeros(0)


def pair_features(p1, n1, p2, n2):
    """float64 [P, 3] each -> dict(counted bool [P], bins int [P, 3] (f1, f2, f3), f [P, 3] (the angle f1, f2, f3), margins: the smallest
    distance of a counted pair's f1, f2, f3 to a bin edge in bin widths, and the smallest ||a1| - |a2||)"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = _normal_ok(n1) & _normal_ok(n2)
        dp = p2 - p1
        d = np.sqrt((dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1]) + dp[:, 2] * dp[:, 2])
        ok &= (d > 0.0) & np.isfinite(d)
        a1, a2 = _dot(n1, dp) / d, _dot(n2, dp) / d
        swap = np.abs(a1) < np.abs(a2)
        m1 = np.where(swap[:, None], n2, n1)
        m2 = np.where(swap[:, None], n1, n2)
        dp = np.where(swap[:, None], -dp, dp)
        f3 = np.where(swap, -a2, a1)
        v = _cross(dp, m1)
        vn = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        ok &= (vn > 0.0) & np.isfinite(vn)
        v = v / vn[:, None]
        w = _cross(m1, v)
        f2 = _dot(v, m2)
        y, x = _dot(w, m2), _dot(m1, m2)
        bins = np.stack([sector(x, y), bin11(f2), bin11(f3)], 1)
        theta = np.arctan2(y, x)
        c = ok
        margins = dict(
            f1=float(np.min(_edge_distance(11.0 * (theta[c] + np.pi) / (2.0 * np.pi), range(0, 12)), initial=np.inf)),
            f2=float(np.min(_edge_distance(11.0 * (f2[c] + 1.0) / 2.0, range(1, 11)), initial=np.inf)),
            f3=float(np.min(_edge_distance(11.0 * (f3[c] + 1.0) / 2.0, range(1, 11)), initial=np.inf)),
            swap=float(np.min(np.abs(np.abs(a1[c]) - np.abs(a2[c])), initial=np.inf)))
    return dict(counted=ok, bins=bins, f=np.stack([theta, f2, f3], 1), xy=np.stack([x, y], 1), margins=margins)


def spfh(points, normals, row_start, index, d2):
    """-> (counts int64 [n, 33], k int64 [n], margins).  points / normals: float32 (the contract) or float64 (for the invariance test)"""
    P, N = np.asarray(points).astype(f64), np.asarray(normals).astype(f64)
    n = len(P)
    rows = np.repeat(np.arange(n), np.diff(row_start))
    keep = (d2 != 0) & np.isfinite(P).all(1)[rows]
    rows, nb = rows[keep], index[keep].astype(np.int64)
    pf = pair_features(P[rows], N[rows], P[nb], N[nb])
    counts = np.zeros((n, DIM), np.int64)
    c = pf["counted"]
    for f in range(3):
        np.add.at(counts, (rows[c], f * BINS + pf["bins"][c, f]), 1)
    k = np.bincount(rows[c], minlength=n).astype(np.int64)
    return counts, k, pf["margins"]


def spfh_value(counts, k):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(k[:, None] > 0, (100.0 * counts.astype(f64)) / k[:, None].astype(f64), 0.0)


def block_sum(a):
    """[n, 11] -> the symmetric sum of a block"""
    return (((((a[:, 0] + a[:, 10]) + (a[:, 1] + a[:, 9])) + (a[:, 2] + a[:, 8])) + (a[:, 3] + a[:, 7])) + (a[:, 4] + a[:, 6])) + a[:, 5]


def fpfh_from_spfh(counts, k, row_start, index, d2):
    """-> (features float32 [n, 33], the same before the rounding float64 [n, 33])"""
    n = len(k)
    val = spfh_value(counts, k)
    acc = np.zeros((n, DIM), f64)
    lane = np.arange(64)
    for i in range(n):
        b, e = int(row_start[i]), int(row_start[i + 1])
        if e == b:
            continue
        dd = d2[b:e].astype(f64)
        with np.errstate(invalid="ignore", divide="ignore"):
            term = np.where((dd != 0)[:, None], val[index[b:e]] / dd[:, None], 0.0)
        pad = (-len(term)) % 64
        term = np.concatenate([term, np.zeros((pad, DIM))]).reshape(-1, 64, DIM)
        lanes = np.zeros((64, DIM), f64)
        for chunk in term:
            lanes = lanes + chunk
        for o in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[lane ^ o]
        acc[i] = lanes[0]
    out = np.zeros((n, DIM), f64)
    for f in range(3):
        a = acc[:, f * BINS:(f + 1) * BINS]
        s = block_sum(a)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[:, f * BINS:(f + 1) * BINS] = np.where(s[:, None] > 0.0, (a * 100.0) / s[:, None], a)
    out = np.where(k[:, None] > 0, out + val, 0.0)
    return out.astype(f32), out


def compute_fpfh(points, normals, radius, max_nn=100):
    """-> dict(features float32 [n, 33], exact float64, counts, k, margins)"""
    ls = lists(points, radius, max_nn)
    counts, k, margins = spfh(points, normals, *ls)
    feat, exact = fpfh_from_spfh(counts, k, *ls)
    return dict(features=feat, exact=exact, counts=counts, k=k, margins=margins, lists=ls)


def mirror(features):
    f = np.asarray(features)
    return np.concatenate([f[:, 10::-1], f[:, 11:22], f[:, 32:21:-1]], 1)


# ---- matching ---------------------------------------------------------------------------------------------------------------------------------
def nearest_feature(src, tgt):
    """-> index int64 [m], -1 where there is no match"""
    a, b = np.asarray(src).astype(f32).reshape(-1, DIM), np.asarray(tgt).astype(f32).reshape(-1, DIM)
    out = np.full(len(a), -1, np.int64)
    okb = np.isfinite(b).all(1)
    oka = np.isfinite(a).all(1)
    if not okb.any() or not oka.any():
        return out
    cols = np.nonzero(okb)[0]
    bb = b[cols]
    for lo in range(0, len(a), 512):
        aa = np.where(oka[lo:lo + 512, None], a[lo:lo + 512], f32(0))
        acc = np.zeros((len(aa), len(bb)), f32)
        with np.errstate(over="ignore"):
            for q in range(DIM):
                d = aa[:, q, None] - bb[None, :, q]
                acc = acc + d * d
        out[lo:lo + 512] = cols[np.argmin(acc, 1)]                        # (the first minimum: the lowest index)
    out[~oka] = -1
    return out


def match_features(src, tgt, mutual_filter=False):
    """-> (correspondences int32 [c, 2] ascending by source row, the forward match int64 [m], the mutual mask bool [m])"""
    fwd = nearest_feature(src, tgt)
    back = nearest_feature(tgt, src)
    rows = np.arange(len(fwd))
    mutual = (fwd >= 0) & (back[np.maximum(fwd, 0)] == rows) if len(back) else np.zeros(len(fwd), bool)
    keep = (fwd >= 0) & (mutual if mutual_filter else True)
    return np.stack([rows[keep], fwd[keep]], 1).astype(np.int32), fwd, mutual


# ---- RANSAC -----------------------------------------------------------------------------------------------------------------------------------
def stop_need(best, c, confidence):
    """the hypotheses Open3D's rule asks for at the score `best`"""
    ratio = best / c
    if ratio >= 1.0:
        return 0.0
    return math.log(1.0 - confidence) / math.log(1.0 - ratio ** 3)


def _res2(fit, P, Q):
    R, t = fit
    e = (((P[:, 0, None] * R[None, :, 0] + P[:, 1, None] * R[None, :, 1]) + P[:, 2, None] * R[None, :, 2]) + t[None, :]) - Q
    return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]


def degenerate(c, **kw):
    return dict(dict(status="degenerate", T=np.eye(4), mask=np.zeros(c, bool), h=-1, inliers=0, fitness=0.0, rmse=0.0, margin=np.inf, unique=True,
                     hypotheses=0, chunks=0, valid=np.zeros(0, bool), scores=np.zeros(0, np.int64)), **kw)


MARGIN = 1e-10


def assert_clear(margin):
    """The condition under which integers are compared exactly: every discrete decision of the input (a checker, an inlier, a bin) lies at
    least MARGIN from its threshold (RANSAC: relative to tau^2), far beyond what Jacobi against LAPACK or another order of the sums can
    move a value."""
    m = min(margin.values()) if isinstance(margin, dict) else float(margin)
    assert m >= MARGIN, f"a decision lies {m:.3e} from its threshold (the bar is {MARGIN:.0e}): integers cannot be compared exactly"


def _note(margins, r2, tau2):
    if margins is not None and len(r2):
        margins.append(float(np.min(np.abs(r2 - tau2)) / tau2))


def _fit34(fit):
    return np.concatenate([fit[0], fit[1][:, None]], 1)


IDENTITY34 = np.eye(4)[:3]


def hypotheses(P, Q, seed, h0, count, s_edge, tau):
    """stage A (gr_hypotheses_kernel) for the hypotheses h0 .. h0 + count - 1 -> (ids int64 [count, 3], valid bool [count], fits float64
    [count, 3, 4] = [R | t], margin).  The fit is the identity where the edge-length checker fails or Kabsch's rank test does, and Kabsch's
    where only the distance checker failed.  margin: the edge-length decisions of every hypothesis and the distance decisions of every
    fitted one, relative to tau^2."""
    P, Q = np.asarray(P, f64).reshape(-1, 3), np.asarray(Q, f64).reshape(-1, 3)
    c, s, tau2 = len(P), float(s_edge), float(tau) * float(tau)
    ids = np.array([LC.sample(seed, 0, h, c) for h in range(h0, h0 + count)], np.int64).reshape(count, 3)
    ok = np.ones(count, bool)
    margin = np.inf
    for a, b in ((0, 1), (0, 2), (1, 2)):
        ds, dt = P[ids[:, a]] - P[ids[:, b]], Q[ids[:, a]] - Q[ids[:, b]]
        ls = np.sqrt((ds[:, 0] * ds[:, 0] + ds[:, 1] * ds[:, 1]) + ds[:, 2] * ds[:, 2])
        lt = np.sqrt((dt[:, 0] * dt[:, 0] + dt[:, 1] * dt[:, 1]) + dt[:, 2] * dt[:, 2])
        ok &= (ls >= s * lt) & (lt >= s * ls)
        margin = min(margin, float(np.min(np.abs(ls * ls - (s * lt) ** 2)) / tau2), float(np.min(np.abs(lt * lt - (s * ls) ** 2)) / tau2))
    valid = np.zeros(count, bool)
    fits = np.tile(IDENTITY34, (count, 1, 1))
    for i in np.nonzero(ok)[0]:
        fit = LC.kabsch(P[ids[i]], Q[ids[i]])
        if fit is None:
            continue
        fits[i] = _fit34(fit)
        r3 = _res2(fit, P[ids[i]], Q[ids[i]])
        margin = min(margin, float(np.min(np.abs(r3 - tau2)) / tau2))
        valid[i] = bool((r3 < tau2).all())
    return ids, valid, fits, margin


def score(P, Q, fits, listed, tau, margins=None):
    """stage B (gr_score_kernel): fits [count, 3, 4], listed = the hypotheses to score (an entry outside 0 .. count - 1 is ignored) -> int64
    [count], the number of correspondences with residual^2 < tau^2 (strictly), zero for a hypothesis that is not listed.  margins: a list
    that receives the smallest |r^2 - tau^2| / tau^2 of every scored hypothesis."""
    P, Q = np.asarray(P, f64).reshape(-1, 3), np.asarray(Q, f64).reshape(-1, 3)
    fits = np.asarray(fits, f64).reshape(-1, 3, 4)
    tau2 = float(tau) * float(tau)
    out = np.zeros(len(fits), np.int64)
    for i in np.asarray(listed, np.int64).reshape(-1):
        if 0 <= i < len(fits):
            r2 = _res2((fits[i, :, :3], fits[i, :, 3]), P, Q)
            _note(margins, r2, tau2)
            out[i] = int((r2 < tau2).sum())
    return out


def winner_key(best_key, scores, h0):
    """stage C (gr_winner_kernel), pure integers: the maximum of best_key and (score << 32 | ~(h0 + t) mod 2^32) over the scores > 0 of a
    chunk that starts at hypothesis h0 -- the highest score, then the lowest h; a score of zero never enters"""
    key = int(best_key)
    for t, sc in enumerate(np.asarray(scores, np.int64).reshape(-1).tolist()):
        if sc > 0:
            key = max(key, (sc << 32) | (~(int(h0) + t) & 0xffffffff))
    return key


def decode(key):
    """-> (score, h) of a winner key"""
    return int(key) >> 32, ~int(key) & 0xffffffff


REFIT_BLOCK, REFIT_SUMS = 256, 17


def refit_partials(P, Q, T, tau, margins=None):
    """stage D, gr_refit_step_kernel: T [3 or 4, 4] -> (mask bool [c], partial float64 [ceil(c / 256), 17]).  A row of `partial` is a block's
    sum of (1, p, q, q p^T row-major, r^2) over its inliers (r^2 < tau^2, r^2 in `_res2`'s order), each term started from +0.0 as kabsch_add
    starts it, in the order of reduce.h's block_sum<17, 4>: inside each wave of 64 rows the xor butterfly 32, 16, .., 1, then the four waves
    in order; a row that is absent or no inlier contributes +0.0."""
    P, Q = np.asarray(P, f64).reshape(-1, 3), np.asarray(Q, f64).reshape(-1, 3)
    T = np.asarray(T, f64)
    c, tau2 = len(P), float(tau) * float(tau)
    r2 = _res2((T[:3, :3], T[:3, 3]), P, Q)
    _note(margins, r2, tau2)
    mask = r2 < tau2
    nb = -(-c // REFIT_BLOCK)
    v = np.zeros((nb * REFIT_BLOCK, REFIT_SUMS), f64)
    terms = np.concatenate([np.ones((c, 1)), 0.0 + P, 0.0 + Q, 0.0 + (Q[:, :, None] * P[:, None, :]).reshape(c, 9), r2[:, None]], 1)
    v[:c] = np.where(mask[:, None], terms, 0.0)
    v = v.reshape(nb, REFIT_BLOCK // 64, 64, REFIT_SUMS)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    w = v[:, :, 0]
    partial = w[:, 0]
    for i in range(1, REFIT_BLOCK // 64):
        partial = partial + w[:, i]
    return mask, partial


def kabsch_from_sums(s, n):
    """rigid3.h's kabsch_from_sums with LAPACK's SVD: s = (sum p, sum q, sum q p^T row-major) over n pairs -> (R, t) or None where the second
    singular value of S = sum q p^T - (sum q) mean(p)^T is below RANK_EPS"""
    s = np.asarray(s, f64)
    mp, mq = s[0:3] / n, s[3:6] / n
    S = s[6:15].reshape(3, 3) - s[3:6, None] * mp[None, :]
    if not np.all(np.isfinite(S)):
        return None
    U, d, Vt = np.linalg.svd(S)
    if not d[1] >= LC.RANK_EPS:
        return None
    U, V = U.copy(), Vt.T.copy()
    U[:, 2] = np.cross(U[:, 0], U[:, 1])
    V[:, 2] = np.cross(V[:, 0], V[:, 1])
    R = U @ V.T
    return R, mq - R @ mp


def refit_finish(partial, state, final):
    """stage D, gr_refit_finish_kernel: partial [nblocks, 17], state [16] = (0-11 the rows of [R | t], 12 status, 13 inliers, 14 RMSE, 15 rounds)
    -> the new state.  A status other than 1 on entry: nothing changes.  The columns are added as reduce.h's column_sum adds them (lane l
    adds rows l, l + 64, ... in order from +0.0, then the butterfly: `wave_sum`); rounds + 1; fewer than 3 inliers: status 0.  final: inliers
    and sqrt(sum r^2 / inliers).  Otherwise Kabsch from the sums replaces the transform, or status 0 where its rank test fails; the
    transform stays as it was whenever the status is cleared."""
    state = np.array(state, f64).reshape(16)
    if state[12] != 1.0:
        return state
    partial = np.asarray(partial, f64).reshape(-1, REFIT_SUMS)
    tot = np.array([wave_sum(partial[:, k]) for k in range(REFIT_SUMS)], f64)
    state[15] = state[15] + 1.0
    if not tot[0] >= 3.0:
        state[12] = 0.0
    elif final:
        state[13], state[14] = tot[0], np.sqrt(tot[16] / tot[0])
    else:
        fit = kabsch_from_sums(tot[1:16], tot[0])
        if fit is None:
            state[12] = 0.0
        else:
            state[:12] = _fit34(fit).reshape(12)
    return state


def ransac(src, dst, tau, edge_length_threshold=0.9, max_iteration=100000, confidence=0.999, n_refit=2, seed=0):
    """RANSAC over the correspondences src[i] -> dst[i] ([c, 3] each), composed of the stages above -> dict(status, T, mask, h, inliers,
    fitness, rmse, hypotheses, chunks, valid bool [hypotheses], scores int64 [hypotheses], margin = the smallest distance of any decision to
    its threshold relative to tau^2 (|r^2 - tau^2| / tau^2, |ls^2 - s^2 lt^2| / tau^2), unique = no second hypothesis reaches the winning
    score)"""
    P, Q = np.asarray(src, f64).reshape(-1, 3), np.asarray(dst, f64).reshape(-1, 3)
    tau = float(f32(tau))                                                  # (the public layer rounds the distance to float32 first, as registration_icp does)
    c, s = len(P), float(edge_length_threshold)
    if c < 3:
        return degenerate(c)
    margins, tried, chunks, key, status = [], 0, 0, 0, "max_iteration"
    valid_all, score_all = [], []
    while tried < max_iteration:
        cnt = min(CHUNK, max_iteration - tried)
        ids, valid, fits, m = hypotheses(P, Q, seed, tried, cnt, s, tau)
        margins.append(m)
        sc = score(P, Q, fits, np.nonzero(valid)[0], tau, margins)
        key = winner_key(key, sc, tried)
        valid_all.append(valid)
        score_all.append(sc)
        tried += cnt
        chunks += 1
        best = decode(key)[0]
        if best > 0 and stop_need(best, c, confidence) <= tried:
            status = "converged"
            break
    valid, scores = np.concatenate(valid_all), np.concatenate(score_all)
    common = dict(hypotheses=tried, chunks=chunks, valid=valid, scores=scores)
    best, h = decode(key)
    if best < 3:
        return degenerate(c, margin=min(margins), **common)
    unique = int((scores == best).sum()) == 1
    state = np.zeros(16)
    state[:12] = hypotheses(P, Q, seed, h, 1, s, tau)[2].reshape(12)       # (gr_winner_fit: the same code path as stage A)
    state[12] = 1.0
    for rnd in range(n_refit + 1):
        mask, partial = refit_partials(P, Q, state[:12].reshape(3, 4), tau, margins)
        state = refit_finish(partial, state, rnd == n_refit)
        if state[12] != 1.0:
            return degenerate(c, margin=min(margins), **common)
    T = np.eye(4)
    T[:3] = state[:12].reshape(3, 4)
    return dict(status=status, T=T, mask=mask, h=h, inliers=int(state[13]), fitness=float(state[13]) / c, rmse=float(state[14]),
                margin=min(margins), unique=unique, **common)


def ransac_on_features(src, dst, src_feat, dst_feat, mutual_filter, tau, **kw):
    """-> (ransac's dict, correspondences int32 [c, 2])"""
    corres = match_features(src_feat, dst_feat, mutual_filter)[0]
    r = ransac(np.asarray(src, f64)[corres[:, 0]], np.asarray(dst, f64)[corres[:, 1]], tau, **kw)
    return r, corres


# ---- the poses of the tests ---------------------------------------------------------------------------------------------------------------------
def axis_angle(axis, degrees, shift):
    """the 4 x 4 of a rotation by `degrees` about `axis` followed by the translation `shift`"""
    a = np.asarray(axis, f64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(degrees)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)
    T[:3, 3] = shift
    return T


AXIS, SHIFT = (0.3, -0.5, 0.8), (0.11, -0.07, 0.2)
POSE_50, POSE_170 = axis_angle(AXIS, 50.0, SHIFT), axis_angle(AXIS, 170.0, SHIFT)


def rotation_error_degrees(T, T_true):
    R = T[:3, :3] @ T_true[:3, :3].T
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))))


# ---- the inputs of the tests ----------------------------------------------------------------------------------------------------------------------
def bumpy_pair(pose):
    """the bumpy pair of tests/_icp_ref.py with analytic normals, the source moved by the inverse of `pose`: registering it finds `pose` ->
    dict(tgt, tn float32 [2806, 3], src, sn float32 [1937, 3], true float64 [1937, 3])"""
    import _icp_ref as I
    tgt, tn = I.bumpy_target()
    true = I.bumpy_source_true()
    Ti = np.linalg.inv(pose)
    src = (true @ Ti[:3, :3].T + Ti[:3, 3]).astype(f32)
    sn = (I.bumpy_normal(true[:, 0], true[:, 1]) @ Ti[:3, :3].T).astype(f32)
    return dict(tgt=tgt, tn=tn, src=src, sn=sn, true=true)


def planted(pair, n_true, n_total, seed):
    """n_true correspondences (a source row, the target point nearest to its true place) followed by n_total - n_true random ones, shuffled
    -> int32 [n_total, 2]"""
    rng = np.random.default_rng(seed)
    rows = rng.choice(len(pair["src"]), n_true, replace=False)
    d = np.linalg.norm(pair["true"][rows][:, None, :] - pair["tgt"].astype(f64)[None, :, :], axis=2)
    good = np.stack([rows, np.argmin(d, 1)], 1)
    bad = np.stack([rng.integers(0, len(pair["src"]), n_total - n_true), rng.integers(0, len(pair["tgt"]), n_total - n_true)], 1)
    return rng.permutation(np.concatenate([good, bad])).astype(np.int32)


# ---- the scenes of the stage tests (tests/test_global_registration_stages_gpu.py; shown fair in tests/test_global_registration_cpu.py) ----------
STAGE_POSE = axis_angle((0.3, -0.5, 0.8), 50.0, (0.02, -0.01, 0.03))
STAGE_TAU = float(f32(0.002))
STAGE_PLANTED = ((3, 3), (4, 3), (255, 90), (256, 90), (257, 90), (513, 150), (1025, 300), (16385, 5000))      # (c, n_true)


def planted_scene(c, n_true, blocks=True):
    """-> (P, Q float64 [c, 3]): P uniform in +-0.05 m; Q = STAGE_POSE P + N(0, 1e-4) on the first n_true rows, uniform on the rest.  With
    `blocks` and c >= 255, rows 0 .. 5 of P lie on one line (true correspondences: a sample of three of them passes the edge-length
    checker and fails the rank test) and the last three rows of P are one point (a sample with two of them fails the edge-length checker)."""
    rng = np.random.default_rng(1000 + c)
    P = rng.uniform(-0.05, 0.05, (c, 3))
    if blocks and c >= 255:
        P[:6] = P[0] + np.arange(6.0)[:, None] * np.array([0.004, -0.003, 0.002])
        P[c - 3:] = P[c - 3]
    Q = rng.uniform(-0.05, 0.05, (c, 3))
    Q[:n_true] = P[:n_true] @ STAGE_POSE[:3, :3].T + STAGE_POSE[:3, 3] + rng.normal(0.0, 1e-4, (n_true, 3))
    order = rng.permutation(c)                                             # the rows shuffled: true ones in every tile of 256, and in the last
    last = int(np.nonzero(order < n_true)[0][-1])                          # row, so that the last block's partial row (c = 16385: the 65th) is
    order[[last, c - 1]] = order[[c - 1, last]]                            # not zero
    return P[order], Q[order]


def blocks_scene():
    """16 correspondences in which the degenerate samples are frequent: rows 0 .. 5 on one line and rows 9 .. 15 in general position, all
    true; rows 6 .. 8 one point of P with three different targets"""
    rng = np.random.default_rng(77)
    P = rng.uniform(-0.05, 0.05, (16, 3))
    P[:6] = P[0] + np.arange(6.0)[:, None] * np.array([0.004, -0.003, 0.002])
    P[6:9] = P[6]
    Q = P @ STAGE_POSE[:3, :3].T + STAGE_POSE[:3, 3] + rng.normal(0.0, 1e-4, (16, 3))
    Q[6:9] = rng.uniform(-0.05, 0.05, (3, 3))
    return P, Q


EXACT_C = 300


def exact_scene():
    """-> (P, Q float64 [300, 3]) whose lengths, products and sums are exact in float64: P = distinct integer points of [-40, 40]^3 / 1024,
    Q = a quarter turn about z, (x, y, z) -> (-y, x, z), plus (3, -2, 5) / 1024.  Every edge-length decision at edge_length_threshold = 1
    sits exactly on ls == lt."""
    rng = np.random.default_rng(300)
    cells = rng.choice(81 ** 3, EXACT_C, replace=False)
    K = np.stack([cells // 6561, (cells // 81) % 81, cells % 81], 1).astype(f64) - 40.0
    P = K / 1024.0
    Q = np.stack([0.0 - P[:, 1], P[:, 0], P[:, 2]], 1) + np.array([3.0, -2.0, 5.0]) / 1024.0
    return P, Q


CONSTRUCTED_RADIUS = 0.01


def constructed_cloud():
    """Clusters one unit apart along x, searched at CONSTRUCTED_RADIUS -> (points float32 [n, 3], normals float32 [n, 3], rows: the first row of
    each cluster by name).  alone: no neighbour.  twins: two coincident points and a third.  normals: a zero normal, a NaN normal, three good
    points.  nan: a non-finite point beside two good ones.  k63 / k64 / k65: 64 / 65 / 66 points inside a ball of diameter 0.008, every point
    with exactly 63 / 64 / 65 counted pairs.  along: a neighbour on the normal's line (|v| = 0 from both ends) and a third point."""
    rng = np.random.default_rng(23)

    def unit(n):
        v = rng.normal(size=(n, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    def ball(n):
        return unit(n) * (0.004 * rng.uniform(0.2, 1.0, (n, 1)))
    pts, nrm, rows = [], [], {}

    def add(name, p, n):
        rows[name] = sum(len(a) for a in pts)
        pts.append(np.asarray(p, f64) + np.array([float(len(rows)), 0.0, 0.0]))
        nrm.append(np.asarray(n, f64))
    add("alone", [[0.0, 0.0, 0.0]], unit(1))
    add("twins", [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.003, 0.001, -0.002]], unit(3))
    n5 = unit(5)
    n5[0] = 0.0
    n5[1, 1] = np.nan
    add("normals", ball(5), n5)
    p3 = ball(3)
    p3[0, 0] = np.nan
    add("nan", p3, unit(3))
    for name, n in (("k63", 64), ("k64", 65), ("k65", 66)):
        add(name, ball(n), unit(n))
    add("along", [[0.0, 0.0, 0.0], [0.0, 0.0, 0.005], [0.002, -0.003, 0.001]], np.concatenate([[[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]], unit(1)]))
    return np.concatenate(pts).astype(f32), np.concatenate(nrm).astype(f32), rows


def recipe_on_thinned(ps, ns, pt, nt, voxel_size, normal_sign="either", **kw):
    """registration_global after its thinning: features at 5 voxel_size, the mutual matches, RANSAC at 1.5 voxel_size; with "either" a second
    run on the mirrored source features, the run with more inliers (a tie: the first) -> (ransac's dict, correspondences, mirrored bool)"""
    fs = compute_fpfh(ps, ns, 5.0 * voxel_size)["features"]
    ft = compute_fpfh(pt, nt, 5.0 * voxel_size)["features"]
    a, ca = ransac_on_features(ps, pt, fs, ft, True, 1.5 * voxel_size, **kw)
    if normal_sign == "either":
        b, cb = ransac_on_features(ps, pt, mirror(fs), ft, True, 1.5 * voxel_size, **kw)
        if b["inliers"] > a["inliers"]:
            return b, cb, True
    return a, ca, False


def recipe(pair, voxel_size, normal_sign="either", flip_source=False, **kw):
    """the whole of registration_global in numpy (the thinning is tests/_voxel_ref.py's) on a bumpy_pair"""
    import _voxel_ref as V
    sn = -pair["sn"] if flip_source else pair["sn"]
    a = V.voxel_down_sample(pair["src"], voxel_size, normals=sn, unit_normals=True)
    b = V.voxel_down_sample(pair["tgt"], voxel_size, normals=pair["tn"], unit_normals=True)
    return recipe_on_thinned(a["points"], a["normals"], b["points"], b["normals"], voxel_size, normal_sign, **kw)
