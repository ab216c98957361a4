"""The numpy statement of the loop-closure kernels (bodyslam_amd/csrc/loop_closure.hip): the keypoints' 3-D points, the match over a list
of frame pairs, and the RANSAC rigid registration with its information matrix.  Plain numpy; ORB and the match are tests/_orb_ref.py's.

Nothing here is the reference's code (3DM/slam.py:79-80 calls a ``_loop_closure`` that does not exist).  RANSAC (Fischler & Bolles 1981)
over three-point Kabsch fits (Kabsch 1976; Arun, Huang & Blostein 1987) and the information matrix in the form of Open3D's
``get_information_matrix_from_point_clouds`` (restated from its documentation) -- parity with Open3D UNPINNED.

Every choice that the device reproduces:
  * lift: depth at (int(y), int(x)) of a point inside the image (associate_depth's rule), valid when != 0 and finite; pixel_to_3d in fp64.
  * correspondences: the matches with distance <= max_hamming whose two points are valid, in match order.  C of them.
  * sampler: draw d of hypothesis h of pair p is the high 32 bits of splitmix64's finaliser applied to
    (seed ^ p * 0xD6E8FEB86659FD93) + 0x9E3779B97F4A7C15 * (3 h + d + 1) in 64-bit wrap-around arithmetic; i0 = r0 % C, i1 = r1 % (C - 1),
    i2 = r2 % (C - 2), each shifted past the earlier picks.  Integer arithmetic only: bit for bit.
  * Kabsch from sums: S = sum q p^T - (sum q)(sum p)^T / n; S = U diag(s) V^T; the directions of the smallest singular value are replaced
    by the cross product of the other two (the det sign fix of ensure_so3_v2, and the completion of a rank-2 sample); R = U V^T,
    t = mean q - R mean p.  A second singular value below RANK_EPS (collinear / coincident points): no fit, score 0.
  * score = #(|R p + t - q| < tau); the highest score wins, the lowest h among equals; a best score below 3 rejects.
  * refit: n_refit rounds of (Kabsch over the inliers, recount); fewer than 3 inliers or a collinear inlier set rejects.
  * information = sum G^T G over the inliers, G = [-[q]x | I3] from the TARGET (train-frame) points, rotation parameters first.
The device computes the singular vectors by a Jacobi iteration and its sums in another order: floating-point results agree to about 1e-9
relative, integer decisions exactly as long as no residual lies at the threshold -- which decision_margin measures."""
import numpy as np

import _orb_ref as R

MAX_FEATURES = 500
RANK_EPS = 1e-12
M64 = (1 << 64) - 1


# ---- lift and match -------------------------------------------------------------------------------------------------------------------------
def lift(pt, depth, K):
    """pt fp32 [n, 2], depth fp32 [H, W] -> fp64 [n, 4] = (x, y, z, valid); invalid rows are zero"""
    fx, fy, cx, cy = (np.float64(v) for v in K)
    H, W = depth.shape
    out = np.zeros((len(pt), 4), dtype=np.float64)
    for k, (u, v) in enumerate(np.asarray(pt, dtype=np.float32)):
        if not (u > np.float32(-1.0) and u < np.float32(W) and v > np.float32(-1.0) and v < np.float32(H)):
            continue
        d = np.float64(depth[int(v), int(u)])
        if d == 0.0 or not np.isfinite(d):
            continue
        out[k] = ((np.float64(u) - cx) * d / fx, (np.float64(v) - cy) * d / fy, d, 1.0)
    return out


def match_pairs(descs, pairs):
    """descs: the frames' descriptor arrays; pairs [(query frame, train frame)] -> [_orb_ref.match of each pair]"""
    return [R.match(descs[q], descs[t]) for q, t in pairs]


# ---- the sampler ----------------------------------------------------------------------------------------------------------------------------
def draw(seed, pair, h, d):
    z = ((seed ^ ((pair * 0xD6E8FEB86659FD93) & M64)) + 0x9E3779B97F4A7C15 * (3 * h + d + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z >> 32


def sample(seed, pair, h, C):
    """three distinct indices below C (C >= 3)"""
    i0 = draw(seed, pair, h, 0) % C
    i1 = draw(seed, pair, h, 1) % (C - 1)
    i2 = draw(seed, pair, h, 2) % (C - 2)
    if i1 >= i0:
        i1 += 1
    lo, hi = min(i0, i1), max(i0, i1)
    if i2 >= lo:
        i2 += 1
    if i2 >= hi:
        i2 += 1
    return int(i0), int(i1), int(i2)


# ---- the fit ----------------------------------------------------------------------------------------------------------------------------------
def kabsch(P, Q):
    """(R, t) with Q ~ R P + t, or None where the points are collinear / coincident"""
    n = np.float64(len(P))
    sp, sq = P.sum(0), Q.sum(0)
    S = Q.T @ P - np.outer(sq, sp / n)
    if not np.all(np.isfinite(S)):
        return None
    U, s, Vt = np.linalg.svd(S)
    if not s[1] >= RANK_EPS:
        return None
    V = Vt.T.copy()
    U = U.copy()
    U[:, 2] = np.cross(U[:, 0], U[:, 1])
    V[:, 2] = np.cross(V[:, 0], V[:, 1])
    Rm = U @ V.T
    return Rm, sq / n - Rm @ (sp / n)


def residuals(fit, P, Q):
    return np.linalg.norm(P @ fit[0].T + fit[1] - Q, axis=1)


def information(Q):
    """sum G^T G, G = [-[q]x | I3], over the rows of Q"""
    info = np.zeros((6, 6))
    for x, y, z in Q:
        G = np.array([[0.0, z, -y, 1.0, 0.0, 0.0], [-z, 0.0, x, 0.0, 1.0, 0.0], [y, -x, 0.0, 0.0, 0.0, 1.0]])
        info += G.T @ G
    return info


def rejected(C, margin=np.inf):
    return dict(status=0, T=np.eye(4), mask=np.zeros(C, dtype=bool), info=np.zeros((6, 6)), rmse=0.0, h=-1, inliers=0, C=C, margin=margin,
                unique=True, scores=None)


def register(src, dst, tau, n_hyp=256, n_refit=2, seed=0, pair=0, min_matches=0):
    """RANSAC registration of the correspondences src[i] -> dst[i] ([C, 3] each): dict(status, T with dst ~ T src, mask [C], info, rmse, h,
    inliers, C, margin = the smallest | |residual| - tau | over every hypothesis and every refit round, unique = no second hypothesis
    reaches the winning score, scores [n_hyp])"""
    P, Q = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(dst, dtype=np.float64).reshape(-1, 3)
    C = len(P)
    if C < max(3, min_matches):
        return rejected(C)
    margin = np.inf
    scores = np.zeros(n_hyp, dtype=np.int64)
    for h in range(n_hyp):
        ids = list(sample(seed, pair, h, C))
        fit = kabsch(P[ids], Q[ids])
        if fit is None:
            continue
        r = residuals(fit, P, Q)
        margin = min(margin, float(np.min(np.abs(r - tau))))
        scores[h] = int((r < tau).sum())
    best = int(scores.max())
    h = int(np.argmax(scores))                                         # (the first maximum: the lowest h)
    unique = int((scores == best).sum()) == 1
    if best < 3:
        return dict(rejected(C, margin), scores=scores)
    fit = kabsch(P[list(sample(seed, pair, h, C))], Q[list(sample(seed, pair, h, C))])
    for rnd in range(n_refit + 1):
        r = residuals(fit, P, Q)
        margin = min(margin, float(np.min(np.abs(r - tau))))
        mask = r < tau
        if mask.sum() < 3:
            return dict(rejected(C, margin), scores=scores)
        if rnd == n_refit:
            break
        fit = kabsch(P[mask], Q[mask])
        if fit is None:
            return dict(rejected(C, margin), scores=scores)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = fit
    return dict(status=1, T=T, mask=mask, info=information(Q[mask]), rmse=float(np.sqrt(np.mean(r[mask] ** 2))), h=h, inliers=int(mask.sum()),
                C=C, margin=margin, unique=unique, scores=scores)


def decision_margin(src, dst, tau, n_hyp=256, n_refit=2, seed=0, pair=0):
    """(the smallest | |residual| - tau | over every hypothesis and every refit round, whether the winning score is unique)"""
    r = register(src, dst, tau, n_hyp, n_refit, seed, pair)
    return r["margin"], r["unique"]


# ---- a pair of frames -------------------------------------------------------------------------------------------------------------------------
def correspondences(xyz_q, xyz_t, matches, max_hamming):
    """(match rows kept, source points, target points): distance <= max_hamming and both points valid, in match order"""
    rows = [m for m, (q, t, d) in enumerate(matches) if d <= max_hamming and xyz_q[q, 3] == 1.0 and xyz_t[t, 3] == 1.0]
    rows = np.array(rows, dtype=np.int64)
    if len(rows) == 0:
        return rows, np.zeros((0, 3)), np.zeros((0, 3))
    return rows, xyz_q[matches[rows, 0], :3], xyz_t[matches[rows, 1], :3]


def register_pair(xyz_q, xyz_t, matches, max_hamming, tau, n_hyp=256, n_refit=2, min_matches=0, seed=0, pair=0):
    """register() on a pair's correspondences; adds rows (the match rows of the correspondences) and mask_rows bool [MAX_FEATURES] by match row"""
    rows, P, Q = correspondences(xyz_q, xyz_t, matches, max_hamming)
    r = register(P, Q, tau, n_hyp, n_refit, seed, pair, min_matches)
    mask_rows = np.zeros(MAX_FEATURES, dtype=bool)
    mask_rows[rows[r["mask"]]] = True
    return dict(r, rows=rows, mask_rows=mask_rows, matches=len(matches))


def frame(color, depth, K):
    """ORB of a frame and its lifted points: dict(pt, desc, xyz)"""
    f = R.extract(color)
    return dict(pt=f["pt"], desc=f["desc"], xyz=lift(f["pt"], depth, K))
