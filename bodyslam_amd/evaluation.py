"""Depth-map evaluation with the reference's MDEM protocol, on the device.

The reference judges its depth module by BodySLAM_not_refactored/EVALUATION/MDEM_eval.py (compute_metrics_for, :130-259) over the
MDEM_Metrics functions of EVALUATION/evaluation_metrics.py:17-102: per frame the GT is masked by dataset, the prediction is scaled by
the ratio of the medians, and AbsRel, SqRel, RMSE, RMSE-log and three delta accuracies are averaged over the sequence.  This module
computes the same numbers with one call of bs_depth_metrics (include/bodyslam_hip.h) over depth maps that can stay in device memory
(SequenceResult.depth_u16).  There is no CPU fallback: without a GPU the call raises BodySlamHipError.
"""
from __future__ import annotations

import csv
import math
import os
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

# GT masks of MDEM_eval.py:179-192, as open intervals lo < gt < hi on the GT alone: Hamlyn `gt > 1.0 and gt < 300` (:183), SCARED
# `gt > 0` (:190); EndoSlam has no branch, so nothing is masked -- zeros in its GT are part of the median (and of no metric)
PROTOCOLS: Dict[str, Tuple[float, float]] = {"hamlyn": (1.0, 300.0), "scared": (0.0, math.inf), "endoslam": (-math.inf, math.inf)}

# the per-frame columns of the reference's results.csv, in its order (MDEM_eval.py:220-228)
METRIC_NAMES = ("abs_rel_diff", "squared_rel_err", "rmse", "rmse_log", "accuracy_1.25", "accuracy_(1.25)^2", "accuracy_(1.25)^3")
# and what else the record holds per frame: the scale applied, the two medians, the pixel counts (n_mask: pixels the mask keeps;
# n_valid: terms of the first three metrics, gt != 0 and s * pred not NaN; n_pos: terms of rmse_log and the accuracies, gt > 0 and
# s * pred > 0)
EXTRA_NAMES = ("scale", "median_gt", "median_pred", "n_mask", "n_valid", "n_pos")
PER_FRAME_NAMES = METRIC_NAMES + EXTRA_NAMES

_MAX_FRAMES_PER_LAUNCH = 65535          # bs_depth_metrics' grid limit; longer inputs go in slices (records do not depend on the batch)


@dataclass
class DepthMetrics:
    """per_frame: name -> float64 [B] for every name of PER_FRAME_NAMES."""
    per_frame: Dict[str, np.ndarray]

    def __len__(self) -> int:
        return len(self.per_frame[METRIC_NAMES[0]])

    def mean(self) -> Dict[str, float]:
        """The sequence mean of each metric, frames whose value is NaN left out (pandas DataFrame.mean() of results.csv,
        MDEM_eval.py:247-251); NaN where every frame is NaN."""
        out = {}
        for k in METRIC_NAMES:
            v = self.per_frame[k]
            ok = ~np.isnan(v)
            n = int(np.count_nonzero(ok))
            out[k] = float(np.sum(v[ok]) / n) if n else math.nan
        return out

    def write_csv(self, directory: str) -> Tuple[str, str]:
        """results.csv (one row per frame, csv.DictWriter as CSVIO.write_metrics_on_cvs writes it) and avg.csv (the
        Series.to_csv(header=True) layout of MDEM_eval.py:253-254) in `directory`; returns both paths."""
        os.makedirs(directory, exist_ok=True)
        results = os.path.join(directory, "results.csv")
        with open(results, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(METRIC_NAMES))
            w.writeheader()
            for i in range(len(self)):
                w.writerow({k: float(self.per_frame[k][i]) for k in METRIC_NAMES})
        avg = os.path.join(directory, "avg.csv")
        with open(avg, "w") as f:
            f.write(",0\n")
            for k, v in self.mean().items():
                f.write(f"{k},{'' if math.isnan(v) else repr(v)}\n")
        return results, avg


def _as_u16_frames(x, what: str):
    """-> (int16 torch tensor [B, H, W] holding the uint16 bits, on whatever device x is on); ValueError on anything else"""
    if isinstance(x, np.ndarray):
        if x.dtype not in (np.uint16, np.int16):
            raise ValueError(f"{what}: dtype {x.dtype}, expected uint16 (or int16 storage of uint16 values)")
        t = torch.from_numpy(np.ascontiguousarray(x).view(np.int16))
    elif isinstance(x, torch.Tensor):
        if x.dtype == torch.int16:
            t = x
        elif getattr(torch, "uint16", None) is not None and x.dtype == torch.uint16:
            t = x.view(torch.int16)
        else:
            raise ValueError(f"{what}: dtype {x.dtype}, expected torch.uint16 or torch.int16 storage of uint16 values")
    else:
        raise ValueError(f"{what}: expected a numpy array or a torch tensor, got {type(x).__name__}")
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"{what}: shape {tuple(x.shape)}, expected a non-empty [B, H, W] or [H, W]")
    return t


def _bounds(protocol: str, gt_range) -> Tuple[float, float]:
    if protocol not in PROTOCOLS:
        raise ValueError(f"unknown protocol {protocol!r}: one of {sorted(PROTOCOLS)}")
    if gt_range is None:
        return PROTOCOLS[protocol]
    try:
        lo, hi = (float(v) for v in gt_range)
    except (TypeError, ValueError):
        raise ValueError(f"gt_range {gt_range!r}: expected (lo, hi)") from None
    return lo, hi


def evaluate_depth(pred, gt, protocol: str = "hamlyn", gt_range: Optional[Sequence[float]] = None,
                   scale: Optional[float] = None) -> DepthMetrics:
    """MDEM metrics of every frame of `pred` against `gt` (MDEM_eval.py:179-228).

    pred: uint16 [B, H, W] or [H, W], depth in metres * 256 (int16 storage as in SequenceResult.depth_u16 is accepted); gt: uint16 of
    the same shape, in dataset units.  torch tensors (device or host) or numpy arrays; host inputs are uploaded once.
    protocol: the GT mask of the dataset ("hamlyn": 1 < gt < 300, "scared": gt > 0, "endoslam": none); gt_range=(lo, hi) replaces it
    by lo < gt < hi.  scale: None = the per-frame median scale median(gt) / median(pred) over the mask; a number = that scale for
    every frame (e.g. 1000 / 256 for metric evaluation against GT in mm).
    """
    lo, hi = _bounds(protocol, gt_range)
    if scale is not None:
        try:
            scale = float(scale)
        except (TypeError, ValueError):
            raise ValueError(f"scale {scale!r}: expected None or a number") from None
    p = _as_u16_frames(pred, "pred")
    g = _as_u16_frames(gt, "gt")
    if tuple(p.shape) != tuple(g.shape):
        raise ValueError(f"pred shape {tuple(p.shape)} and gt shape {tuple(g.shape)} differ")
    cuda = [t.device for t in (p, g) if t.is_cuda]
    if not torch.cuda.is_available():
        L.init(0)                              # raises BodySlamHipError: no CPU fallback
    dev = cuda[0] if cuda else torch.device("cuda", torch.cuda.current_device())
    B, H, W = p.shape
    with torch.cuda.device(dev):
        L.init(dev.index)
        p = p.to(dev, non_blocking=False).contiguous()
        g = g.to(dev, non_blocking=False).contiguous()
        nb = min(B, _MAX_FRAMES_PER_LAUNCH)
        ws = torch.empty(L.depth_metrics_workspace(nb, H, W), dtype=torch.uint8, device=dev)
        out = torch.empty(B, L.DEPTH_METRICS_FIELDS, dtype=torch.float64, device=dev)
        for b0 in range(0, B, nb):
            b1 = min(B, b0 + nb)
            L.depth_metrics(p[b0:b1], g[b0:b1], lo, hi, scale, ws, out[b0:b1])
        rec = out.cpu().numpy()
    return DepthMetrics({k: rec[:, i].copy() for i, k in enumerate(PER_FRAME_NAMES)})


def _read_u16_png(path: str) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("I;16", "I;16L", "I;16B"):
            raise ValueError(f"{path}: image mode {im.mode!r}; expected a single-channel 16-bit PNG (an 8-bit or multi-channel GT is not "
                             "supported: the reference takes np.log of a uint8 array in fp16 there)")
        return np.asarray(im, dtype=np.uint16)


def evaluate_depth_files(pred_paths: Sequence[str], gt_paths: Sequence[str], protocol: str = "hamlyn",
                         gt_range: Optional[Sequence[float]] = None, scale: Optional[float] = None, results_dir: Optional[str] = None,
                         batch: int = 64) -> DepthMetrics:
    """One sequence of (prediction, GT) PNG pairs, as compute_metrics_for walks a folder (MDEM_eval.py:160-254): single-channel 16-bit
    PNGs read with PIL (what DepthEstimator.save_depth_map writes; cv2.IMREAD_ANYDEPTH reads the same values), evaluated `batch`
    frames per call; with results_dir, results.csv and avg.csv are written there."""
    pred_paths, gt_paths = list(pred_paths), list(gt_paths)
    if len(pred_paths) != len(gt_paths) or not pred_paths:
        raise ValueError(f"{len(pred_paths)} predictions and {len(gt_paths)} GT files: expected the same, non-zero number")
    if batch < 1:
        raise ValueError(f"batch {batch}: expected >= 1")
    _bounds(protocol, gt_range)
    parts = []
    for b0 in range(0, len(pred_paths), batch):
        pp, gg = pred_paths[b0:b0 + batch], gt_paths[b0:b0 + batch]
        preds = [_read_u16_png(f) for f in pp]
        gts = [_read_u16_png(f) for f in gg]
        for fp, fg, a, b in zip(pp, gg, preds, gts):
            if a.shape != b.shape or a.shape != preds[0].shape:
                raise ValueError(f"{fp} {a.shape} / {fg} {b.shape}: every prediction and GT of a batch must have one shape")
        parts.append(evaluate_depth(np.stack(preds), np.stack(gts), protocol=protocol, gt_range=gt_range, scale=scale))
    res = DepthMetrics({k: np.concatenate([m.per_frame[k] for m in parts]) for k in PER_FRAME_NAMES})
    if results_dir is not None:
        res.write_csv(results_dir)
    return res
