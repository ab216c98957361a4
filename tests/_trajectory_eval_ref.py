"""A numpy restatement of the trajectory metrics, independent of the product code (bodyslam_amd.evaluation.evaluate_trajectory,
bs_trajectory_metrics, bs_similarity_fit).  Poses are [N, 4, 4] float64; Q is the ground truth, P the prediction.

umeyama(x, y)       the similarity with y ~ s R x + t over [n, 3] point sets (the reference's estimate_similarity_transformation,
                    BodySLAM_not_refactored/3DM/slam_utils.py:138-169, takes the transposes):
                        mx, my = the means; sigma_x = mean |x - mx|^2; Sxy = (1 / n) sum (y - my)(x - mx)^T = U D V^T
                        S = diag(1, 1, -1) when det(Sxy) < 0 ("reference" rule) or when det(U) det(V) < 0 ("evo" rule), else I
                        R = U S V^T, s = tr(D S) / sigma_x, t = my - s R mx
                    The two rules agree for a full-rank Sxy; with a planar point set det(Sxy) is round-off and only the evo rule
                    yields a proper rotation.

Protocol "evo": the reference's evaluation MPEM_Metrics.compute_pose_metrics (EVALUATION/evaluation_metrics.py:136-165), which is
pred.align_origin(gt), pred.align(gt, correct_scale=True), then evo's APE / RPE.  Restated from evo's published definitions; evo is not
installed where this runs, so parity with evo itself is unpinned.
    align_origin    P_i <- Q_0 P_0^-1 P_i                                 (inverses are [R^T | -R^T t] throughout)
    align           (R, s, t) = umeyama(positions of P, positions of Q), evo rule; s = 1 without correct_scale
                    trans P_i <- s trans P_i, then P_i <- [R | t] P_i
                    degenerate (evo raises): fewer than two singular values of Sxy above np.finfo(float64).eps, or sigma_x == 0
    ATE_i           |trans Q_i - trans P_i|
    ARE_i           the angle of Q_i^-1 P_i in degrees
    pairs           (i, i + delta) for i = 0, delta, 2 delta, ... (all_pairs=False) or for every i (all_pairs=True), i + delta < N
    E               (Q_i^-1 Q_j)^-1 (P_i^-1 P_j)
    RTE             |trans E|;  RRE = the angle of rot E in degrees
    angle(R)        arccos(clip((tr R - 1) / 2, -1, 1))
    statistics      rmse = sqrt(mean e^2), mean, std = np.std (population), min, max; the reference reports (rmse, std)

Protocol "training": the reference's own code, TrainingLoss.compute_scale_factor / compute_ARE_and_ATE / compute_RRE_and_RTE
(MPEM/training_utils.py:473-585).
    scale           sum trans Q_i . trans P_i / sum |trans P_i|^2
    ATE             mean |trans Q_i - scale trans P_i|
    ARE             mean arccos(clip((tr(rot Q_i rot P_i^T) - 1) / 2, -1, 1)) in radians
    RTE, RRE        means over every i < n - delta of the same two errors between inv(Q_i) Q_{i + delta} and inv(P_i) P_{i + delta}
                    (np.linalg.inv), on the UNSCALED poses
    The reference's compute_ARE_and_ATE multiplies the caller's prediction translations by the scale IN PLACE, so there a later
    compute_RRE_and_RTE on the same arrays sees scaled poses.  Nothing here (or in the product) writes to its inputs.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
STATS = ("rmse", "mean", "std", "min", "max")


class Degenerate(ValueError):
    pass


def umeyama(x, y, rule="reference", with_scale=True):
    """x, y: [n, 3] -> R [3, 3], s, t [3], info (sigma_x, rank)"""
    # (as [3, n] arrays, the reference's layout: for a planar point set the sign of det(Sxy) is round-off, and the "reference" rule
    # reproduces the reference's answer there only if the sums run in the reference's order)
    x = np.ascontiguousarray(np.asarray(x, np.float64).T)
    y = np.ascontiguousarray(np.asarray(y, np.float64).T)
    n = x.shape[1]
    mx, my = x.mean(axis=1), y.mean(axis=1)
    xc, yc = x - mx[:, None], y - my[:, None]
    sigma_x = np.mean(np.sum(xc ** 2, axis=0))
    Sxy = (yc @ xc.T) / n
    U, D, Vt = np.linalg.svd(Sxy)
    S = np.eye(3)
    if rule == "reference":
        flip = np.linalg.det(Sxy) < 0
    else:
        flip = np.linalg.det(U) * np.linalg.det(Vt) < 0
    if flip:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    with np.errstate(divide="ignore", invalid="ignore"):             # (sigma_x = 0: the callers report the fit as degenerate)
        s = np.trace(np.diag(D) @ S) / sigma_x if with_scale else 1.0
    t = my - s * (R @ mx)
    return R, s, t, (sigma_x, int(np.count_nonzero(D > EPS)))


def se3_inv(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def angle(R):
    return np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))


def stats(e):
    e = np.asarray(e, np.float64)
    return {"rmse": np.sqrt(np.mean(e * e)), "mean": np.mean(e), "std": np.std(e), "min": np.min(e), "max": np.max(e)}


def pair_ids(n, delta, all_pairs):
    if all_pairs:
        return [(i, i + delta) for i in range(n) if i + delta < n]
    ids = list(range(0, n, delta))
    return list(zip(ids, ids[1:]))


def align_evo(gt, pred, align_origin=True, align=True, correct_scale=True):
    """-> the aligned copy of pred, s, R, t.  Raises Degenerate where evo raises."""
    P = np.array(pred, np.float64, copy=True)
    Q = np.asarray(gt, np.float64)
    if align_origin:
        O = Q[0] @ se3_inv(P[0])
        P = np.array([O @ p for p in P])
    R, s, t = np.eye(3), 1.0, np.zeros(3)
    if align or correct_scale:
        Rf, sf, tf, (sigma_x, rank) = umeyama(P[:, :3, 3], Q[:, :3, 3], rule="evo", with_scale=correct_scale)
        if rank < 2 or not sigma_x > 0:
            raise Degenerate(f"degenerate alignment: {rank} singular values above eps, sigma_x {sigma_x}")
        if correct_scale:
            s = sf
        if align:
            R, t = Rf, tf
    P[:, :3, 3] *= s
    A = np.eye(4)
    A[:3, :3], A[:3, 3] = R, t
    P = np.array([A @ p for p in P])
    return P, s, R, t


def evaluate_evo(gt, pred, delta=1, all_pairs=False, align_origin=True, align=True, correct_scale=True):
    """-> dict: ate / are / rte / rre -> {rmse, mean, std, min, max}; scale, rotation, translation, n_poses, n_pairs"""
    Q = np.asarray(gt, np.float64)
    n = len(Q)
    if n < delta + 1:
        raise Degenerate(f"{n} poses: fewer than delta + 1 = {delta + 1}")
    P, s, R, t = align_evo(Q, pred, align_origin, align, correct_scale)
    ate = [np.linalg.norm(q[:3, 3] - p[:3, 3]) for q, p in zip(Q, P)]
    are = [np.degrees(angle((se3_inv(q) @ p)[:3, :3])) for q, p in zip(Q, P)]
    rte, rre = [], []
    pairs = pair_ids(n, delta, all_pairs)
    for i, j in pairs:
        E = se3_inv(se3_inv(Q[i]) @ Q[j]) @ (se3_inv(P[i]) @ P[j])
        rte.append(np.linalg.norm(E[:3, 3]))
        rre.append(np.degrees(angle(E[:3, :3])))
    return {"ate": stats(ate), "are": stats(are), "rte": stats(rte), "rre": stats(rre), "scale": s, "rotation": R, "translation": t,
            "n_poses": n, "n_pairs": len(pairs)}


def training_scale(gt, pred):
    Q, P = np.asarray(gt, np.float64), np.asarray(pred, np.float64)
    num = den = 0.0
    for q, p in zip(Q, P):
        num += np.dot(q[:3, 3], p[:3, 3])
        den += np.linalg.norm(p[:3, 3]) ** 2
    return num / den


def evaluate_training(gt, pred, delta=1):
    Q, P = np.asarray(gt, np.float64), np.asarray(pred, np.float64)
    n = len(Q)
    if n < delta + 1:
        raise Degenerate(f"{n} poses: fewer than delta + 1 = {delta + 1}")
    s = training_scale(Q, P)
    if not np.isfinite(s):
        raise Degenerate("the prediction has no translation")
    ate = [np.linalg.norm(q[:3, 3] - s * p[:3, 3]) for q, p in zip(Q, P)]
    are = [angle(q[:3, :3] @ p[:3, :3].T) for q, p in zip(Q, P)]
    rte, rre = [], []
    for i in range(n - delta):
        qr = np.linalg.inv(Q[i]) @ Q[i + delta]
        pr = np.linalg.inv(P[i]) @ P[i + delta]
        rte.append(np.linalg.norm(qr[:3, 3] - pr[:3, 3]))
        rre.append(angle(qr[:3, :3] @ pr[:3, :3].T))
    return {"ate": stats(ate), "are": stats(are), "rte": stats(rte), "rre": stats(rre), "scale": s, "rotation": np.eye(3),
            "translation": np.zeros(3), "n_poses": n, "n_pairs": n - delta}


def evaluate(gt, pred, protocol="evo", delta=1, **kw):
    if protocol == "evo":
        return evaluate_evo(gt, pred, delta=delta, **kw)
    if protocol == "training":
        return evaluate_training(gt, pred, delta=delta)
    raise ValueError(protocol)


# ---- test trajectories ------------------------------------------------------------------------------------------------------------------
def rot(axis, a):
    """Rodrigues: the rotation by a radians about `axis`"""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def random_walk(rng, n, step=0.02, turn=0.03):
    """[n, 4, 4]: a smooth 3-D path (not planar, not straight) of SE(3) poses"""
    T = np.eye(4)
    out = [T.copy()]
    for _ in range(n - 1):
        d = np.eye(4)
        d[:3, :3] = rot(rng.normal(size=3) + [0.3, 1.0, 0.2], turn * (1 + 0.5 * rng.normal()))
        d[:3, 3] = step * (np.array([0.2, 0.1, 1.0]) + 0.3 * rng.normal(size=3))
        T = T @ d
        out.append(T.copy())
    return np.array(out)


def perturbed(rng, gt, scale=0.37, rot_noise=2e-3, trans_noise=1e-3):
    """a prediction for gt: its relative motions with per-step noise (rotation errors well above 1e-4 rad), chained, translations
    divided by `scale`, then moved by a rigid transform"""
    n = len(gt)
    T = np.eye(4)
    out = [T.copy()]
    for i in range(1, n):
        d = np.linalg.inv(gt[i - 1]) @ gt[i]
        e = np.eye(4)
        e[:3, :3] = rot(rng.normal(size=3), rot_noise * (1.0 + rng.random()))
        e[:3, 3] = trans_noise * rng.normal(size=3)
        T = T @ d @ e
        out.append(T.copy())
    P = np.array(out)
    P[:, :3, 3] /= scale
    G = np.eye(4)
    G[:3, :3] = rot([0.5, -1.0, 0.8], 0.7)
    G[:3, 3] = [0.3, -1.2, 2.0]
    return np.array([G @ p for p in P])
