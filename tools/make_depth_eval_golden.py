"""Build-machine only: tests/golden/depth_eval.npz -- inputs and the reference's own depth metrics for a set of frames that cover the
MDEM protocol's cases (like oracle/make_golden.py for the networks; nothing on the GPU machine reads the reference).

    python tools/make_depth_eval_golden.py --ref <reference checkout> [--out PATH] [--check]

The metrics are the reference's MDEM_Metrics functions (BodySLAM_not_refactored/EVALUATION/evaluation_metrics.py, imported with `evo`
stubbed: MDEM_Metrics never touches it).  MDEM_eval.py itself cannot be imported (it runs an evaluation at import time), so its
masking and median lines (:114-127,179-197) are restated below with their line numbers.  --check compares a fresh run with the
committed file at the tolerances of tests/test_depth_eval_cpu.py instead of writing.
"""
import argparse
import math
import os
import sys
import warnings
from unittest import mock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "depth_eval.npz")
H, W = 48, 64
METRIC_NAMES = ("abs_rel_diff", "squared_rel_err", "rmse", "rmse_log", "accuracy_1.25", "accuracy_(1.25)^2", "accuracy_(1.25)^3")
EXTRA = ("scale", "median_gt", "median_pred", "n_mask", "n_valid", "n_pos")
HAMLYN, SCARED, ENDOSLAM = (1.0, 300.0), (0.0, math.inf), (-math.inf, math.inf)


def load_reference_metrics(ref):
    for m in ("evo", "evo.core", "evo.core.metrics", "evo.core.units", "evo.tools", "evo.tools.file_interface"):
        sys.modules.setdefault(m, mock.MagicMock())
    sys.path.insert(0, os.path.join(ref, "BodySLAM_not_refactored", "EVALUATION"))
    from evaluation_metrics import MDEM_Metrics
    return MDEM_Metrics()


def smooth(rng, lo, hi):
    """a smooth random surface in [lo, hi) (depth-like: neighbours share their high byte)"""
    y, x = np.mgrid[0:H, 0:W] / np.array([H, W])[:, None, None]
    a = rng.uniform(0, 2 * np.pi, 4)
    z = 0.5 + 0.25 * np.sin(3 * x + a[0]) * np.cos(2 * y + a[1]) + 0.2 * np.sin(5 * x * y + a[2]) + 0.05 * np.cos(7 * y + a[3])
    return np.clip(lo + (hi - lo) * z, lo, hi - 1).astype(np.uint16)


def frames():
    """(name, pred, gt, (lo, hi), scale or None)"""
    rng = np.random.default_rng(20260)
    from PIL import Image
    ref_png = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "reference_pair", "output_depth_map.png")), dtype=np.uint16)
    out = []
    # Hamlyn (1 < gt < 300 mm), odd and even masked counts
    g = smooth(rng, 0, 420)
    p = smooth(rng, 300, 900)
    m = (g > 1) & (g < 300)
    if np.count_nonzero(m) % 2 == 0:
        g[np.argwhere(m)[0][0], np.argwhere(m)[0][1]] = 500
    out.append(("hamlyn_odd", p, g, HAMLYN, None))
    g2 = g.copy()
    g2[np.argwhere((g2 > 1) & (g2 < 300))[0][0], np.argwhere((g2 > 1) & (g2 < 300))[0][1]] = 0
    out.append(("hamlyn_even", p.copy(), g2, HAMLYN, None))
    # SCARED-like sparse GT (about 8 % of pixels), gt > 0
    g = smooth(rng, 20, 180) * (rng.random((H, W)) < 0.08)
    out.append(("scared_sparse", smooth(rng, 200, 700), g.astype(np.uint16), SCARED, None))
    # EndoSlam: no mask, zeros of the GT inside its median
    g = smooth(rng, 0, 60000) * (rng.random((H, W)) < 0.7)
    out.append(("endoslam_zeros", smooth(rng, 100, 5000), g.astype(np.uint16), ENDOSLAM, None))
    # EndoSlam with the extreme values 0 and 65535 in both maps
    g = smooth(rng, 0, 65535)
    p = smooth(rng, 0, 65535)
    g[::7, ::5] = 65535
    g[3::11, ::3] = 0
    p[1::5, ::4] = 65535
    p[2::9, 1::6] = 0
    out.append(("endoslam_extremes", p, g, ENDOSLAM, None))
    # prediction zeros inside the mask (they scale to 0: counted by the first three metrics, not by rmse_log / accuracy)
    g = smooth(rng, 2, 299)
    p = smooth(rng, 50, 400)
    p[rng.random((H, W)) < 0.2] = 0
    out.append(("pred_zeros_in_mask", p, g, HAMLYN, None))
    # empty mask: NaN medians, NaN metrics
    out.append(("empty_mask", smooth(rng, 10, 500), smooth(rng, 300, 2000), HAMLYN, None))
    # median(pred) = 0: s = inf -> inf, inf, inf, inf, 0
    g = smooth(rng, 5, 290)
    p = smooth(rng, 10, 300)
    p[: H * 2 // 3] = 0
    out.append(("median_pred_zero", p, g, HAMLYN, None))
    # median(gt) = 0 (EndoSlam zeros): s = 0
    g = smooth(rng, 10, 3000)
    g[: H * 2 // 3] = 0
    out.append(("median_gt_zero", smooth(rng, 100, 900), g, ENDOSLAM, None))
    # one all-equal frame
    out.append(("all_equal", np.full((H, W), 77, np.uint16), np.full((H, W), 123, np.uint16), HAMLYN, None))
    # the reference's own depth output (metres * 256) and a GT in mm derived from it (SCARED-like holes), median-scaled and metric
    y0, x0 = 200, 260
    pc = ref_png[y0:y0 + H, x0:x0 + W].copy()
    gmm = np.rint(pc.astype(np.float64) / 256.0 * 1000.0 * (1.0 + 0.04 * (smooth(rng, 0, 1000) / 1000.0 - 0.5))).astype(np.uint16)
    gmm[rng.random((H, W)) < 0.1] = 0
    out.append(("reference_output_scared", pc, gmm, SCARED, None))
    out.append(("reference_output_metric", pc.copy(), gmm.copy(), SCARED, 1000.0 / 256.0))
    # a user range
    out.append(("user_range", smooth(rng, 100, 3000), smooth(rng, 0, 2500), (100.0, 2000.0), None))
    return out


def reference_record(M, pred, gt, rng_lohi, scale):
    """one frame through the reference's lines; returns the metrics and the extras"""
    lo, hi = rng_lohi
    prediction, ground_truth = pred, gt
    # MDEM_eval.py:181-192 -- Hamlyn: valid_mask = (ground_truth > 1.0) & (ground_truth < 300); SCARED: ground_truth > 0; EndoSlam:
    # no branch.  Restated as the open interval (lo, hi) on the GT
    if not (lo == -math.inf and hi == math.inf):
        valid_mask = np.logical_and(ground_truth > lo, ground_truth < hi)
        ground_truth = ground_truth[valid_mask]
        prediction = prediction[valid_mask]
    else:
        ground_truth = ground_truth.reshape(-1)
        prediction = prediction.reshape(-1)
    # :196-197 with compute_median_scale_factor (:114-127): s = np.median(ground_truth) / np.median(predictions)
    med_g, med_p = np.median(ground_truth), np.median(prediction)
    s = med_g / med_p if scale is None else np.float64(scale)
    prediction = s * prediction
    # :211-217
    vals = [M.abs_rel_diff(prediction, ground_truth), M.squared_rel_error(prediction, ground_truth), M.rmse(prediction, ground_truth),
            M.rmse_log(prediction, ground_truth)] + [M.accuracy_with_threshold(prediction, ground_truth, criterion=c)
                                                       for c in (1.25, 1.25 ** 2, 1.25 ** 3)]
    # the counts behind them (evaluation_metrics.py:33-35 with nanmean's skip; :76-77 / :97)
    mv = np.logical_and(ground_truth != 0, ~np.isnan(ground_truth))
    n_valid = np.count_nonzero(~np.isnan(np.abs(ground_truth[mv] - prediction[mv]) / ground_truth[mv]))
    n_pos = np.count_nonzero(np.logical_and(ground_truth > 0, prediction > 0))
    return [float(v) for v in vals] + [float(s), float(med_g), float(med_p), float(ground_truth.size), float(n_valid), float(n_pos)]


def make(ref):
    M = load_reference_metrics(ref)
    fr = frames()
    recs = []
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for name, p, g, lh, sc in fr:
            recs.append(reference_record(M, p, g, lh, sc))
    recs = np.array(recs, dtype=np.float64)
    d = {"names": np.array([f[0] for f in fr]), "pred": np.stack([f[1] for f in fr]).astype(np.uint16),
         "gt": np.stack([f[2] for f in fr]).astype(np.uint16), "gt_lo": np.array([f[3][0] for f in fr]),
         "gt_hi": np.array([f[3][1] for f in fr]), "scale_in": np.array([np.nan if f[4] is None else f[4] for f in fr])}
    for i, k in enumerate(METRIC_NAMES + EXTRA):
        d[k] = recs[:, i]
    return d


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ref", required=True, help="checkout of the reference (GuidoManni/BodySLAM)")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--check", action="store_true", help="compare with the committed file instead of writing")
    a = ap.parse_args()
    d = make(a.ref)
    if a.check:
        old = np.load(OUT)
        bad = []
        for k in d:
            x, y = d[k], old[k]
            if x.dtype.kind in "fc":
                tol = 1e-7 if k == "rmse_log" else 1e-12
                ok = np.allclose(x, y, rtol=tol, atol=0, equal_nan=True)
            else:
                ok = np.array_equal(x, y)
            if not ok:
                bad.append(k)
        print("depth_eval golden:", "reproduced" if not bad else f"DIFFERS in {bad}")
        sys.exit(1 if bad else 0)
    np.savez_compressed(a.out, **d)
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes, {len(d['names'])} frames)")
    for i, n in enumerate(d["names"]):
        print(f"  {n:26s} n_mask {int(d['n_mask'][i]):5d}  scale {d['scale'][i]:.6g}  " +
              "  ".join(f"{d[k][i]:.6g}" for k in METRIC_NAMES))


if __name__ == "__main__":
    main()
