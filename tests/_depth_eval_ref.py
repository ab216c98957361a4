"""numpy fp64 restatement of the depth-evaluation contract (include/bodyslam_hip.h, bs_depth_metrics): the reference's MDEM protocol,
MDEM_eval.py:114-127,179-197 and evaluation_metrics.py:24-102, one frame at a time.  The yardstick of tests/test_depth_eval_*.py.

One deliberate choice: log(gt) is the correctly rounded fp32 logarithm, widened.  The reference takes np.log of a uint16 array, which
numpy evaluates in fp32 with SIMD loops that differ from the correctly rounded value by 1 ulp on some inputs, and differently on
different CPUs; the device computes the correctly rounded value, so the two agree bit for bit here and the golden file (made with
the reference's own np.log) is met to the rmse_log tolerance its 1-ulp differences need.
"""
import math

import numpy as np

PROTOCOLS = {"hamlyn": (1.0, 300.0), "scared": (0.0, math.inf), "endoslam": (-math.inf, math.inf)}
METRIC_NAMES = ("abs_rel_diff", "squared_rel_err", "rmse", "rmse_log", "accuracy_1.25", "accuracy_(1.25)^2", "accuracy_(1.25)^3")
PER_FRAME_NAMES = METRIC_NAMES + ("scale", "median_gt", "median_pred", "n_mask", "n_valid", "n_pos")


def log32(g):
    """correctly rounded fp32 log of integer values, widened to fp64"""
    return np.log(np.asarray(g, dtype=np.float64)).astype(np.float32).astype(np.float64)


def frame_metrics(pred, gt, lo, hi, scale=None):
    """one frame: pred, gt uint16 (or int16 storage) [H, W] -> dict over PER_FRAME_NAMES"""
    pred = np.asarray(pred).view(np.uint16)
    gt = np.asarray(gt).view(np.uint16)
    f64 = np.float64
    with np.errstate(all="ignore"):
        m = (gt.astype(f64) > lo) & (gt.astype(f64) < hi)                 # MDEM_eval.py:183,190: on GT only, open interval
        g_u, p_u = gt[m], pred[m]
        n = g_u.size
        med_g = f64(np.median(g_u)) if n else f64(np.nan)                 # :114-127 (np.median of an empty array is NaN)
        med_p = f64(np.median(p_u)) if n else f64(np.nan)
        s = med_g / med_p if scale is None else f64(scale)                # :196
        g = g_u.astype(f64)
        p = s * p_u.astype(f64)                                           # :197
        v = (g != 0) & ~np.isnan(p)                                       # evaluation_metrics.py:33,47,60 + nanmean's skip
        d = g[v] - p[v]
        nv = f64(np.count_nonzero(v))
        abs_rel = np.sum(np.abs(d) / g[v]) / nv
        sq_rel = np.sum(d * d / g[v]) / nv
        rmse = np.sqrt(np.sum(d * d) / nv)
        q = (g > 0) & (p > 0)                                             # :76-77,97
        npos = f64(np.count_nonzero(q))
        e = log32(g[q]) - np.log(p[q])
        rmse_log = np.sqrt(np.sum(e * e) / npos)
        r = np.maximum(g[q] / p[q], p[q] / g[q])
        acc = [f64(np.count_nonzero(r < c ** 2)) / npos for c in (1.25, 1.25 ** 2, 1.25 ** 3)]   # :101: criterion ** 2
    vals = [abs_rel, sq_rel, rmse, rmse_log] + acc + [s, med_g, med_p, f64(n), nv, npos]
    return {k: float(x) for k, x in zip(PER_FRAME_NAMES, vals)}


def evaluate(pred, gt, lo, hi, scale=None):
    """[B, H, W] (or [H, W]) -> name -> float64 [B]"""
    pred, gt = np.asarray(pred), np.asarray(gt)
    if pred.ndim == 2:
        pred, gt = pred[None], gt[None]
    rows = [frame_metrics(pred[i], gt[i], lo, hi, scale) for i in range(pred.shape[0])]
    return {k: np.array([r[k] for r in rows], dtype=np.float64) for k in PER_FRAME_NAMES}
