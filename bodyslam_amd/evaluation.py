"""Evaluation on the device: depth maps (the reference's MDEM protocol), trajectories (its MPEM protocol) and the map against ground-truth
geometry (cloud-to-cloud distances).

Depth.  The reference judges its depth module by BodySLAM_not_refactored/EVALUATION/MDEM_eval.py (compute_metrics_for, :130-259) over the
MDEM_Metrics functions of EVALUATION/evaluation_metrics.py:17-102: per frame the GT is masked by dataset, the prediction is scaled by
the ratio of the medians, and AbsRel, SqRel, RMSE, RMSE-log and three delta accuracies are averaged over the sequence.  evaluate_depth
computes the same numbers with one call of bs_depth_metrics (include/bodyslam_hip.h) over depth maps that can stay in device memory
(SequenceResult.depth_u16).

Trajectories.  The reference judges its pose module by MPEM_Metrics.compute_pose_metrics (EVALUATION/evaluation_metrics.py:136-165): evo's
align_origin, align(correct_scale=True), then ATE, RTE and RRE; while training it monitors its own compute_ARE_and_ATE /
compute_RRE_and_RTE (MPEM/training_utils.py:473-585).  evaluate_trajectory computes either with one call of bs_trajectory_metrics over
poses that can stay in device memory (SequenceResult.g_abs); similarity_transform is the Umeyama fit on its own (bs_similarity_fit).

Reconstruction.  SCARED ships structured-light point clouds and EndoSLAM 3-D scans (the reference reads both, DatasetLoader.read_SCARED /
read_EndoSlam); its mapping module measures clouds against each other with Open3D's compute_point_cloud_distance
(3DM/mapping_module.py:45,48,62).  evaluate_reconstruction computes accuracy, completeness, chamfer distance and precision / recall /
F-score from the two nearest-neighbour distance arrays (bodyslam_amd/pointcloud.py), which stay in device memory;
evaluate_reconstruction_aligned refines the frame by rigid ICP first (bodyslam_amd/registration.py).

There is no CPU fallback: without a GPU the calls raise BodySlamHipError.
"""
from __future__ import annotations

import csv
import math
import os
from dataclasses import dataclass
from typing import TYPE_CHECKING, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _args as AR
from . import _lib as L

if TYPE_CHECKING:
    from .registration import RegistrationResult

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
    dev = AR.device_for(p, g)
    B, H, W = p.shape
    with torch.cuda.device(dev):
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


# ---- trajectories -----------------------------------------------------------------------------------------------------------------------
TRAJECTORY_PROTOCOLS = {"evo": L.TRAJ_EVO, "training": L.TRAJ_TRAINING}
STAT_NAMES = ("rmse", "mean", "std", "min", "max")
_TRAJ_STATUS = {L.TRAJ_DEGENERATE: "degenerate alignment (fewer than two singular values of the covariance above eps, or no spread / no "
                                   "translation in the prediction; evo raises here)",
                L.TRAJ_TOO_SHORT: "fewer than delta + 1 poses", L.TRAJ_BAD_OFFSETS: "bad offsets"}


@dataclass
class ErrorStats:
    """The statistics of one error over each sequence, float64 [S] each; std is the population std (np.std)."""
    rmse: np.ndarray
    mean: np.ndarray
    std: np.ndarray
    min: np.ndarray
    max: np.ndarray


@dataclass
class TrajectoryMetrics:
    """Per sequence: ate, are, rte, rre (ErrorStats); the applied scale [S], rotation [S, 3, 3], translation [S, 3]; n_poses and
    n_pairs [S].  Protocol "evo": ATE and RTE in the units of the ground truth, ARE and RRE in degrees; "training": radians."""
    ate: ErrorStats
    are: ErrorStats
    rte: ErrorStats
    rre: ErrorStats
    scale: np.ndarray
    rotation: np.ndarray
    translation: np.ndarray
    n_poses: np.ndarray
    n_pairs: np.ndarray
    protocol: str = "evo"

    def __len__(self) -> int:
        return len(self.scale)

    def as_reference_dict(self, i: int = 0) -> Dict[str, Tuple[float, float]]:
        """{"ATE": (rmse, std), "RTE": (rmse, std), "RRE": (rmse, std)} of sequence i, what compute_pose_metrics returns
        (evaluation_metrics.py:159-165), as Python floats."""
        return {k: (float(e.rmse[i]), float(e.std[i])) for k, e in (("ATE", self.ate), ("RTE", self.rte), ("RRE", self.rre))}

    def write_csv(self, path: str, i: int = 0) -> str:
        """The Metric,Value file of MPEM_eval.py:274-280 for sequence i: csv.DictWriter rows whose Value is the (rmse, std) tuple.  The
        tuple is written as Python floats: under numpy 2 the reference's own tuple of numpy scalars prints as
        "(np.float64(...), np.float64(...))", under numpy 1 as the plain numbers written here."""
        with open(path, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=["Metric", "Value"])
            w.writeheader()
            for k, v in self.as_reference_dict(i).items():
                w.writerow({"Metric": k, "Value": v})
        return path


def _metrics_from_records(rec: np.ndarray, protocol: str) -> TrajectoryMetrics:
    def st(base):
        return ErrorStats(*(rec[:, base + j].copy() for j in range(5)))
    return TrajectoryMetrics(ate=st(16), are=st(21), rte=st(26), rre=st(31), scale=rec[:, 3].copy(), rotation=rec[:, 4:13].reshape(-1, 3, 3).copy(),
                             translation=rec[:, 13:16].copy(), n_poses=rec[:, 0].astype(np.int64), n_pairs=rec[:, 1].astype(np.int64),
                             protocol=protocol)


def _as_poses(x, what: str) -> torch.Tensor:
    """-> float64 torch tensor [N, 16] (4x4 row-major) on whatever device x is on; ValueError on anything else"""
    if isinstance(x, np.ndarray):
        if x.dtype.kind != "f":
            raise ValueError(f"{what}: dtype {x.dtype}, expected a floating-point array")
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    elif isinstance(x, torch.Tensor):
        if not x.dtype.is_floating_point:
            raise ValueError(f"{what}: dtype {x.dtype}, expected a floating-point tensor")
        t = x.detach()
    else:
        raise ValueError(f"{what}: expected a numpy array or a torch tensor, got {type(x).__name__}")
    shape = tuple(t.shape)
    if t.dim() == 3 and shape[1:] == (4, 4):
        return t.to(torch.float64).reshape(shape[0], 16).contiguous()          # (g_abs itself when it is fp64 and contiguous: no copy)
    if (t.dim() == 3 and shape[1:] == (3, 4)) or (t.dim() == 2 and shape[1] == 12):
        full = torch.zeros(shape[0], 16, dtype=torch.float64, device=t.device)
        full[:, :12] = t.reshape(shape[0], 12)
        full[:, 15] = 1.0
        return full
    raise ValueError(f"{what}: shape {shape}, expected [N, 4, 4], [N, 3, 4] or [N, 12]")


def _check_trajectory_args(protocol, delta):
    if protocol not in TRAJECTORY_PROTOCOLS:
        raise ValueError(f"unknown protocol {protocol!r}: one of {sorted(TRAJECTORY_PROTOCOLS)}")
    AR.integer(delta, "delta", 1)


def evaluate_trajectory(pred, gt, protocol: str = "evo", delta: int = 1, all_pairs: bool = False, align_origin: bool = True,
                        align: bool = True, correct_scale: bool = True) -> TrajectoryMetrics:
    """Trajectory metrics of `pred` against `gt`.

    pred, gt: poses as [N, 4, 4], [N, 3, 4] or [N, 12] (a KITTI row per pose), or lists of such for a ragged batch of sequences; torch
    tensors (device or host) or numpy arrays.  A float64 [N, 4, 4] device tensor (SequenceResult.g_abs) is read where it lies; host
    inputs are uploaded once.  Nothing is written to the inputs (the reference's compute_ARE_and_ATE scales its predictions in place).
    protocol "evo": the reference's evaluation -- align_origin, then the similarity alignment (align, correct_scale), then ATE, ARE, RTE,
    RRE over the pose pairs (i, i + delta), i = 0, delta, 2 delta, ... (every i with all_pairs); angles in degrees.  Restated from evo's
    published definitions (include/bodyslam_hip.h spells them out); parity with evo itself is unpinned.
    protocol "training": the reference's training monitors -- the least-squares scale, no alignment (the four flags are not used), every
    i < n - delta a pair, angles in radians.
    Raises ValueError naming the sequence for a degenerate alignment (evo raises there too) or a sequence shorter than delta + 1.
    Degenerate is evo's absolute criterion, fewer than two singular values of the covariance above eps = 2.2e-16; round-off leaves about
    1e-16 of the largest in place of a vanishing one, so a collinear path with steps of metres sits at the threshold and may pass, in evo as
    here.  Do not rely on it to detect collinear paths.
    """
    _check_trajectory_args(protocol, delta)
    batched = isinstance(pred, (list, tuple))
    if batched != isinstance(gt, (list, tuple)):
        raise ValueError("pred and gt: both a list of sequences or both one sequence")
    preds, gts = (list(pred), list(gt)) if batched else ([pred], [gt])
    if len(preds) != len(gts) or not preds:
        raise ValueError(f"{len(preds)} predicted and {len(gts)} ground-truth sequences: expected the same, non-zero number")
    P = [_as_poses(x, f"pred[{i}]") for i, x in enumerate(preds)]
    G = [_as_poses(x, f"gt[{i}]") for i, x in enumerate(gts)]
    for i, (a, b) in enumerate(zip(P, G)):
        if a.shape[0] != b.shape[0]:
            raise ValueError(f"sequence {i}: {a.shape[0]} predicted and {b.shape[0]} ground-truth poses")
        if a.shape[0] < delta + 1:
            raise ValueError(f"sequence {i}: {a.shape[0]} poses, fewer than delta + 1 = {delta + 1}")
    lengths = [int(a.shape[0]) for a in P]
    if sum(lengths) >= 2 ** 31:
        raise ValueError(f"{sum(lengths)} poses in all: the offsets are int32")
    dev = AR.device_for(*P, *G)
    flags = ((L.TRAJ_ALIGN_ORIGIN if align_origin else 0) | (L.TRAJ_ALIGN if align else 0) | (L.TRAJ_CORRECT_SCALE if correct_scale else 0) |
             (L.TRAJ_ALL_PAIRS if all_pairs else 0))
    with torch.cuda.device(dev):
        P = [t.to(dev) for t in P]
        G = [t.to(dev) for t in G]
        p_all = P[0] if len(P) == 1 else torch.cat(P)
        g_all = G[0] if len(G) == 1 else torch.cat(G)
        offsets = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32).to(dev)
        out = torch.empty(len(lengths), L.TRAJ_FIELDS, dtype=torch.float64, device=dev)
        L.trajectory_metrics(g_all, p_all, offsets, TRAJECTORY_PROTOCOLS[protocol], int(delta), flags, out)
        rec = out.cpu().numpy()
    for i in range(len(lengths)):
        status = int(rec[i, 2])
        if status != L.TRAJ_OK:
            raise ValueError(f"sequence {i}: {_TRAJ_STATUS.get(status, f'status {status}')}")
    return _metrics_from_records(rec, protocol)


def read_kitti_poses(path: str, project_so3: bool = False) -> np.ndarray:
    """A KITTI pose file -> float64 [N, 4, 4]: 12 numbers per line, the top three rows of a pose (what save_poses_as_kitti writes and
    evo's read_kitti_poses_file reads).  project_so3: each rotation block goes through ensure_so3_v2 first, the reference's correct_poses
    for trajectories of other methods (EVALUATION/compute_pose_metrics_for_competitor.py:31-62); that runs on the device, one call and
    read-back per pose (slow for many thousands of poses)."""
    rows = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            tok = line.split()
            if not tok:
                continue
            if len(tok) != 12:
                raise ValueError(f"{path}:{ln}: {len(tok)} numbers, expected 12")
            try:
                rows.append([float(v) for v in tok])
            except ValueError:
                raise ValueError(f"{path}:{ln}: not a number in {line.strip()!r}") from None
    if not rows:
        raise ValueError(f"{path}: no poses")
    T = np.zeros((len(rows), 4, 4), np.float64)
    T[:, :3, :] = np.asarray(rows, np.float64).reshape(-1, 3, 4)
    T[:, 3, 3] = 1.0
    if project_so3:
        from .geom3d import ensure_so3_v2
        for i in range(len(T)):
            T[i, :3, :3] = ensure_so3_v2(T[i, :3, :3])
    return T


def evaluate_trajectory_files(pred_paths, gt_paths, protocol: str = "evo", delta: int = 1, all_pairs: bool = False, align_origin: bool = True,
                              align: bool = True, correct_scale: bool = True, project_so3: bool = False,
                              results_dir: Optional[str] = None) -> TrajectoryMetrics:
    """KITTI pose files, one (prediction, GT) pair per sequence, in one device call, as compute_metrics walks a dataset
    (MPEM_eval.py:255-280); a single path each is one sequence.  With results_dir, sequence i's Metric,Value file is written there under
    the prediction file's base name + ".csv"."""
    if isinstance(pred_paths, (str, os.PathLike)):
        pred_paths, gt_paths = [pred_paths], [gt_paths]
    pred_paths, gt_paths = [os.fspath(q) for q in pred_paths], [os.fspath(q) for q in gt_paths]
    if len(pred_paths) != len(gt_paths) or not pred_paths:
        raise ValueError(f"{len(pred_paths)} predictions and {len(gt_paths)} GT files: expected the same, non-zero number")
    _check_trajectory_args(protocol, delta)
    preds = [read_kitti_poses(q, project_so3=project_so3) for q in pred_paths]
    gts = [read_kitti_poses(q) for q in gt_paths]
    res = evaluate_trajectory(preds, gts, protocol=protocol, delta=delta, all_pairs=all_pairs, align_origin=align_origin, align=align,
                              correct_scale=correct_scale)
    if results_dir is not None:
        os.makedirs(results_dir, exist_ok=True)
        for i, q in enumerate(pred_paths):
            res.write_csv(os.path.join(results_dir, os.path.splitext(os.path.basename(q))[0] + ".csv"), i)
    return res


def _as_points(x, what: str) -> torch.Tensor:
    return AR.points(x, what, unwrap=False)


def similarity_fit_record(source, target) -> np.ndarray:
    """The 16 doubles of bs_similarity_fit (include/bodyslam_hip.h): R (9), s, t (3), sigma_x, singular values above eps, n."""
    a, b = _as_points(source, "source"), _as_points(target, "target")
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"source shape {tuple(a.shape)} and target shape {tuple(b.shape)} differ")
    if a.dtype != b.dtype:
        raise ValueError(f"source dtype {a.dtype} and target dtype {b.dtype} differ")
    dev = AR.device_for(a, b)
    with torch.cuda.device(dev):
        a, b = a.to(dev).contiguous(), b.to(dev).contiguous()
        ws = torch.empty(L.SIMILARITY_FIT_WORKSPACE_BYTES, dtype=torch.uint8, device=dev)
        out = torch.empty(16, dtype=torch.float64, device=dev)
        L.similarity_fit(a, b, ws, out)
        return out.cpu().numpy()


def similarity_transform(source, target) -> Tuple[np.ndarray, float, np.ndarray]:
    """The similarity (R [3, 3], s, t [3]) with target ~ s R source + t in the least-squares sense (Umeyama), over [n, 3] point sets:
    device or host, fp32 or fp64, arithmetic in fp64 on the device.  What the reference's estimate_similarity_transformation computes
    (3DM/slam_utils.py:138-169; bodyslam_amd.slam_utils carries its [3, n] signature).  Like the reference it raises nothing for a
    degenerate point set; similarity_fit_record returns the rank next to the fit."""
    r = similarity_fit_record(source, target)
    return r[:9].reshape(3, 3).copy(), float(r[9]), r[10:13].copy()


# ---- reconstruction ---------------------------------------------------------------------------------------------------------------------
DISTANCE_STAT_NAMES = ("mean", "median", "rmse", "max")


@dataclass
class DistanceStats:
    """mean, median, rmse and max of the matched (finite) nearest-neighbour distances of one direction, in the units of the clouds; NaN
    when nothing was matched"""
    mean: float
    median: float
    rmse: float
    max: float


@dataclass
class ReconstructionMetrics:
    """accuracy: pred -> gt; completeness: gt -> pred; chamfer: the mean of the two means.  Per threshold tau (thresholds, as fp32 values):
    precision = the fraction of pred points with distance < tau, recall = that of gt points, fscore = 2 P R / (P + R), 0 when both are 0.
    The fractions are over the points with finite coordinates; a point without a neighbour within max_distance (n_unmatched_*) is a
    miss for every tau and enters neither mean, median, rmse nor max.  alignment: with align="icp" the registration.RegistrationResult whose
    transformation (pred -> gt, after `transform`) was applied to pred before the distances; None otherwise."""
    accuracy: DistanceStats
    completeness: DistanceStats
    chamfer: float
    thresholds: Tuple[float, ...]
    precision: np.ndarray
    recall: np.ndarray
    fscore: np.ndarray
    n_pred: int
    n_gt: int
    n_unmatched_pred: int
    n_unmatched_gt: int
    alignment: Optional["RegistrationResult"] = None       # align="icp": the registration applied to pred (not in as_dict() or the CSV)

    def as_dict(self) -> Dict[str, float]:
        out: Dict[str, float] = {}
        for side, st in (("accuracy", self.accuracy), ("completeness", self.completeness)):
            for k in DISTANCE_STAT_NAMES:
                out[f"{side}_{k}"] = float(getattr(st, k))
        out["chamfer"] = float(self.chamfer)
        for i, tau in enumerate(self.thresholds):
            for k in ("precision", "recall", "fscore"):
                out[f"{k}@{tau!r}"] = float(getattr(self, k)[i])
        for k in ("n_pred", "n_gt", "n_unmatched_pred", "n_unmatched_gt"):
            out[k] = int(getattr(self, k))
        return out

    def write_csv(self, path: str) -> str:
        """A Metric,Value file, one row per entry of as_dict(), csv.DictWriter as TrajectoryMetrics.write_csv writes its file."""
        with open(path, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=["Metric", "Value"])
            w.writeheader()
            for k, v in self.as_dict().items():
                w.writerow({"Metric": k, "Value": v})
        return path


def _check_thresholds(thresholds) -> Tuple[float, ...]:
    try:
        taus = tuple(float(np.float32(v)) for v in thresholds)
    except (TypeError, ValueError):
        raise ValueError(f"thresholds {thresholds!r}: expected a sequence of numbers") from None
    if len(taus) > L.PC_MAX_THRESHOLDS or any(not (v > 0.0 and math.isfinite(v)) for v in taus):
        raise ValueError(f"thresholds {thresholds!r}: expected at most {L.PC_MAX_THRESHOLDS} positive numbers")
    return taus


def distance_stats_record(dist: torch.Tensor, thresholds: Sequence[float] = ()) -> np.ndarray:
    """The PC_STATS_FIELDS doubles of bs_pc_stats (include/bodyslam_hip.h) over a fp32 [n] device tensor of distances: n, finite, infinite
    and NaN entries, sum, sum of squares, max, exact median, the count of d < tau per threshold.  The same bits in every run."""
    taus = _check_thresholds(thresholds)
    if not isinstance(dist, torch.Tensor) or dist.dtype != torch.float32 or dist.dim() != 1 or dist.numel() < 1:
        raise ValueError("dist: expected a non-empty fp32 torch tensor [n]")
    dev = AR.device_for(dist)
    with torch.cuda.device(dev):
        ws = torch.empty(L.PC_STATS_WORKSPACE_BYTES, dtype=torch.uint8, device=dev)
        out = torch.empty(L.PC_STATS_FIELDS, dtype=torch.float64, device=dev)
        L.pc_stats(dist.to(dev).contiguous(), taus, ws, out)
        return out.cpu().numpy()


def _distance_stats(rec: np.ndarray) -> DistanceStats:
    n = rec[1]
    if n == 0:
        return DistanceStats(math.nan, math.nan, math.nan, math.nan)
    return DistanceStats(float(rec[4] / n), float(rec[7]), float(math.sqrt(rec[5] / n)), float(rec[6]))


_ICP_KEYS = ("max_correspondence_distance", "init", "estimation", "target_normals", "max_iteration", "relative_fitness", "relative_rmse", "cell_size",
             "device", "voxel_size")       # (voxel_size is the evaluation's own: _align_icp takes it out before registration_icp is called)
_ALIGNS = ("icp", "global")


def _check_align(align, icp) -> Optional[dict]:
    if align is None:
        if icp is not None:
            raise ValueError('icp given without align="icp"')
        return None
    if align not in _ALIGNS:
        raise ValueError(f'unknown align {align!r}: None, "icp" or "global"')
    if not isinstance(icp, dict) or "max_correspondence_distance" not in icp:
        raise ValueError(f'align="{align}" needs icp, a dict of registration_icp keywords with max_correspondence_distance')
    from . import registration as REG
    kw = dict(icp)
    ransac = kw.pop("ransac", None) if align == "global" else None                      # (the one key align="global" adds)
    unknown = sorted(set(kw) - set(_ICP_KEYS))
    if unknown:
        raise ValueError(f"icp: unknown keys {unknown}; registration_icp takes {_ICP_KEYS}")
    if align == "global":
        if kw.get("voxel_size") is None:
            raise ValueError('align="global" needs icp["voxel_size"]: registration_global thins both clouds by it')
        if "init" in kw:
            raise ValueError('align="global" takes no icp["init"]: the global registration supplies it')
        if ransac is not None and not isinstance(ransac, dict):
            raise ValueError('icp["ransac"]: expected a dict of registration_global keywords')
        ransac = dict(ransac or {})
        REG._check_ransac_keys(ransac, REG.GLOBAL_KEYS, 'icp["ransac"]')
        if ransac.get("normal_sign", "either") not in REG.NORMAL_SIGNS:
            raise ValueError(f"unknown normal_sign {ransac['normal_sign']!r}: one of {REG.NORMAL_SIGNS}")
        from .pointcloud import _check_search_radius
        if ransac.get("feature_radius") is not None:
            _check_search_radius(ransac["feature_radius"], "feature_radius")
        if ransac.get("max_correspondence_distance") is not None:
            REG._check_radius(ransac["max_correspondence_distance"])
    REG._check_radius(kw["max_correspondence_distance"])
    kw["init"] = REG._check_init(kw.get("init"))
    kw.setdefault("estimation", "auto")
    if kw["estimation"] not in REG.ESTIMATIONS:
        raise ValueError(f"unknown estimation {kw['estimation']!r}: one of {REG.ESTIMATIONS}")
    REG._check_criteria(kw.get("max_iteration", 30), kw.get("relative_fitness", 1e-6), kw.get("relative_rmse", 1e-6))
    if kw.get("voxel_size") is not None:
        from .pointcloud import _check_voxel_size
        kw["voxel_size"] = _check_voxel_size(kw["voxel_size"])
    if align == "global":
        kw["ransac"] = ransac
    return kw


def _align_icp(p, g, p_normals, g_normals, A, kw, dev):
    """registers the fp32 device clouds p (pred, `transform` applied) -> g (gt); -> (p moved, the RegistrationResult of pred -> gt)"""
    import dataclasses

    from . import registration as REG
    from . import pointcloud as PC
    kw = dict(kw)
    radius, est, init = kw.pop("max_correspondence_distance"), kw.pop("estimation"), kw.pop("init")
    h = kw.pop("voxel_size", None)                                 # (not a keyword of registration_icp, whose signature is pinned)
    normals = kw.pop("target_normals", None)
    if normals is None:
        normals = g_normals
    ransac = kw.pop("ransac", None)
    if ransac is not None:
        # align="global": registration_global of pred -> gt gives the init; the ICP below runs exactly as with align="icp".  pred's own
        # normals are used only when no `transform` turned the points (otherwise they are estimated on the thinned cloud)
        init = REG.registration_global(p, g, h, source_normals=p_normals if A is None else None, target_normals=normals, **ransac).transformation

    def thinned(cloud, n):
        """the registration's (cloud, normals): as they are, or with voxel_size one point and one unit normal per voxel"""
        if h is None:
            return cloud, n
        if n is not None:
            n = REG._as_normals(n, int(cloud.shape[0])).to(dev)
        r = PC.voxel_down_sample(cloud, h, normals=n, unit_normals=True)
        return r.points, r.normals
    if est == "auto" and normals is None and p_normals is not None:
        # the map has normals and the scan has none: gt -> pred by point-to-plane, inverted.  Normals follow `transform` by the inverse
        # transpose of its linear part (R / s for a similarity); their length does not matter to the normal equations' solution
        n = REG._as_normals(p_normals, int(p.shape[0])).to(dev).contiguous()
        if A is not None:
            N = np.concatenate([np.linalg.inv(A[:, :3]).T, np.zeros((3, 1))], 1)
            if h is not None:                                      # (the thinning averages normals of |a| <= 2: take the scale out)
                N *= abs(np.linalg.det(A[:, :3])) ** (1.0 / 3.0)
            turned = torch.empty(n.shape[0], 3, dtype=torch.float32, device=dev)
            L.pc_transform(n, N, turned)
            n = turned
        (src, _), (tgt, n) = thinned(g, None), thinned(p, n)
        back = REG.registration_icp(src, tgt, radius, init=np.linalg.inv(init), estimation="point_to_plane", target_normals=n, **kw)
        res = dataclasses.replace(back, transformation=np.linalg.inv(back.transformation))
    else:
        (src, _), (tgt, normals) = thinned(p, None), thinned(g, normals)
        res = REG.registration_icp(src, tgt, radius, init=init, estimation=est, target_normals=normals, **kw)
    moved = torch.empty(p.shape[0], 3, dtype=torch.float32, device=dev)
    L.pc_transform(p, res.transformation[:3], moved)
    return moved, res


def evaluate_reconstruction(pred, gt, thresholds: Sequence[float] = (0.001, 0.002, 0.005), transform=None,
                            max_distance: Optional[float] = None) -> ReconstructionMetrics:
    """The reconstruction `pred` against the ground-truth geometry `gt`, by nearest-neighbour distances both ways.

    pred, gt: numpy arrays or torch tensors [n, 3] (fp32, or fp64, which is rounded to fp32 once), host or device; a tsdf.PointCloud; a
    tsdf.TriangleMesh (its vertices).  pred may also be a tsdf.TSDF or tsdf.MAP: its extract_pcd(host=False) is evaluated where it lies.
    transform: a 4 x 4, or (R, s, t) as similarity_transform returns it, applied to pred on the device as s R p + t in fp64 and rounded
    once to fp32 -- how a monocular map is put into the ground truth's frame, by the similarity of its trajectory (evaluate_trajectory,
    similarity_transform).  No alignment is searched for here: evaluate_reconstruction_aligned refines `transform` by ICP first.
    thresholds: at most 8, compared as fp32 values.
    max_distance: a point without a neighbour within it is unmatched (ReconstructionMetrics).  Two runs on the same arrays return the
    same bits.  A TSDF or MAP hands over its points in the order its extraction's atomics gave, which differs from call to call: counts,
    max, median, precision and recall are then still exact, the means and rmse agree to the rounding of an fp64 sum (n 2^-53 relative)."""
    return _evaluate_reconstruction(pred, gt, thresholds, transform, max_distance, None, None)


def evaluate_reconstruction_aligned(pred, gt, thresholds: Sequence[float] = (0.001, 0.002, 0.005), transform=None,
                                    max_distance: Optional[float] = None, align: Optional[str] = "icp",
                                    icp: Optional[dict] = None) -> ReconstructionMetrics:
    """evaluate_reconstruction after an alignment search.  align="icp": after `transform`, pred is registered onto gt by
    registration.registration_icp with the keywords of the dict `icp` (max_correspondence_distance is required; rigid, no scale: the
    scale is `transform`'s), and the result is applied on the device before the two distance queries; it is returned as
    ReconstructionMetrics.alignment.  Normals for point-to-plane come from icp["target_normals"] or a PointCloud gt; when gt has none and
    pred has them (a TSDF, MAP or PointCloud), estimation "auto" registers gt -> pred by point-to-plane and inverts the result (fitness and
    rmse are then those of that direction).  icp["voxel_size"] = h: the usual recipe -- both clouds are thinned by
    pointcloud.voxel_down_sample(h, unit_normals=True), the target's normals averaged along (they must then be finite with |a| <= 2), the
    registration runs on the thinned clouds in the same direction, and its transform is applied to the full pred: the two distance queries
    see the full clouds as before; fitness and rmse are those of the thinned pair.  align="global": for clouds that share no frame --
    registration.registration_global(pred, gt, icp["voxel_size"], **icp.get("ransac", {})) (FPFH features, matching, RANSAC) gives the init
    of the same ICP; icp must carry voxel_size, must not carry init, and may carry "ransac", a dict of registration_global's keywords; the
    global result stays in registration.last_global, `alignment` is the ICP's as before.  align=None: evaluate_reconstruction itself.
    (A function of its own: evaluate_reconstruction's parameter list is pinned by tests/test_pointcloud_cpu.py.)"""
    return _evaluate_reconstruction(pred, gt, thresholds, transform, max_distance, align, icp)


GT_MESH = ("vertices", "surface")


def evaluate_reconstruction_surface(pred, gt, thresholds: Sequence[float] = (0.001, 0.002, 0.005), transform=None,
                                    max_distance: Optional[float] = None, align: Optional[str] = None, icp: Optional[dict] = None,
                                    gt_mesh: str = "surface", n_gt_samples: Optional[int] = None) -> ReconstructionMetrics:
    """evaluate_reconstruction against the SURFACE of a ground-truth mesh rather than its vertices (against a coarse scan, accuracy measured
    to vertices is wrong by up to half an edge length).  gt_mesh="surface": gt must be a tsdf.TriangleMesh (else ValueError); accuracy is
    pred -> surface by raycasting.RaycastingScene.compute_distance; completeness is surface samples -> pred by the nearest-neighbour query,
    the samples being gt.sample_points_uniformly(n_gt_samples or the number of pred points, seed=0); n_gt in the result counts the
    samples.  With align="icp" the samples and their face normals are the registration's target, so point-to-plane needs no normal
    estimation.  The statistics are bs_pc_stats' as before.  gt_mesh="vertices" is evaluate_reconstruction_aligned(..., align, icp) itself,
    the same bits.  (A function of its own: the parameter lists of evaluate_reconstruction and evaluate_reconstruction_aligned are pinned
    by tests/test_pointcloud_cpu.py and tests/test_icp_cpu.py.)"""
    return _evaluate_reconstruction(pred, gt, thresholds, transform, max_distance, align, icp, gt_mesh, n_gt_samples)


@dataclass
class SignedReconstructionMetrics:
    """surface: evaluate_reconstruction_surface's result, the same bits.  The pred points with a finite distance to the surface (the ones
    its accuracy counts) are split by compute_occupancy of the ground-truth mesh: n_inside, n_outside, fraction_inside = n_inside / their
    sum (NaN for none); inside, outside: the DistanceStats of the two subsets' distances; signed_mean = (the sum of the outside distances -
    the sum of the inside distances) / their number -- negative for a map that lies inside the organ, as one with too small a depth scale
    does, positive for one outside.  An unsigned distance cannot tell the two apart."""
    surface: ReconstructionMetrics
    n_inside: int
    n_outside: int
    fraction_inside: float
    inside: DistanceStats
    outside: DistanceStats
    signed_mean: float

    def as_dict(self) -> Dict[str, float]:
        out = self.surface.as_dict()
        for side, st in (("inside", self.inside), ("outside", self.outside)):
            for k in DISTANCE_STAT_NAMES:
                out[f"{side}_{k}"] = float(getattr(st, k))
        out["fraction_inside"], out["signed_mean"] = float(self.fraction_inside), float(self.signed_mean)
        out["n_inside"], out["n_outside"] = int(self.n_inside), int(self.n_outside)
        return out


def evaluate_reconstruction_signed(pred, gt, thresholds: Sequence[float] = (0.001, 0.002, 0.005), transform=None,
                                   max_distance: Optional[float] = None, align: Optional[str] = None, icp: Optional[dict] = None,
                                   n_gt_samples: Optional[int] = None, nsamples: int = 1) -> SignedReconstructionMetrics:
    """evaluate_reconstruction_surface(pred, gt, ..., gt_mesh="surface") and on which SIDE of the ground-truth surface the reconstruction
    lies (SignedReconstructionMetrics).  gt: a tsdf.TriangleMesh that is_closed(), else ValueError -- the sign of a distance is defined
    only for a closed mesh; it is undefined for a point at distance ~ 0.  The side is RaycastingScene.compute_occupancy(points, nsamples)
    of the very points the accuracy side measures: after `transform` and the optional alignment.  nsamples: odd, 1 .. 15; more than one
    outvotes a sample whose ray meets a triangle edge-on.  (A function of its own: evaluate_reconstruction_surface's parameter list is
    pinned by tests/test_mesh_scene_cpu.py.)"""
    from .raycasting import _check_nsamples
    from .tsdf import TriangleMesh
    n = _check_nsamples(nsamples)
    if not isinstance(gt, TriangleMesh):
        raise ValueError(f"evaluate_reconstruction_signed needs a tsdf.TriangleMesh as gt, got {type(gt).__name__}")
    _check_gt_mesh("surface", gt, n_gt_samples)
    _check_thresholds(thresholds)
    _check_align(align, icp)
    AR.device_for()
    if not gt.is_closed():
        raise ValueError("gt: the mesh is not closed (an edge without exactly two triangles): the side of its surface is not defined")
    side: dict = {"nsamples": n}
    surface = _evaluate_reconstruction(pred, gt, thresholds, transform, max_distance, align, icp, "surface", n_gt_samples, side)
    d, occ = side["distance"], side["occupancy"]
    matched = torch.isfinite(d)
    d_in, d_out = d[matched & (occ == 1.0)].contiguous(), d[matched & (occ != 1.0)].contiguous()
    none = np.zeros(L.PC_STATS_FIELDS)                                # (bs_pc_stats takes no empty tensor: the record of no distances)
    r_in = distance_stats_record(d_in) if d_in.numel() else none
    r_out = distance_stats_record(d_out) if d_out.numel() else none
    n_in, n_out = int(d_in.numel()), int(d_out.numel())
    total = n_in + n_out
    return SignedReconstructionMetrics(surface=surface, n_inside=n_in, n_outside=n_out, fraction_inside=n_in / total if total else math.nan,
                                       inside=_distance_stats(r_in), outside=_distance_stats(r_out),
                                       signed_mean=float(r_out[4] - r_in[4]) / total if total else math.nan)


def _check_gt_mesh(gt_mesh, gt, n_gt_samples) -> bool:
    from .tsdf import TriangleMesh
    if gt_mesh not in GT_MESH:
        raise ValueError(f"unknown gt_mesh {gt_mesh!r}: one of {GT_MESH}")
    if n_gt_samples is not None:
        AR.integer(n_gt_samples, "n_gt_samples", 1, 2 ** 31 - 1, "None or an integer in [1, 2^31)")
    if gt_mesh == "vertices":
        if n_gt_samples is not None:
            raise ValueError('n_gt_samples given without gt_mesh="surface"')
        return False
    if not isinstance(gt, TriangleMesh):
        raise ValueError(f'gt_mesh="surface" needs a tsdf.TriangleMesh as gt, got {type(gt).__name__}')
    from .raycasting import as_triangles
    _, t = as_triangles(gt)
    if t.shape[0] < 1 or t.shape[0] > L.MESH_MAX_SAMPLED_TRIANGLES:
        raise ValueError(f"gt: a mesh of {t.shape[0]} triangles, expected 1 .. 2^22")
    return True


def _evaluate_reconstruction(pred, gt, thresholds, transform, max_distance, align, icp, gt_mesh="vertices",
                             n_gt_samples=None, side: Optional[dict] = None) -> ReconstructionMetrics:
    """side (evaluate_reconstruction_signed): a dict with "nsamples"; it receives "distance", the accuracy side's distances, and
    "occupancy" of the same points in the same scene"""
    from . import pointcloud as PC
    from .tsdf import MAP, TSDF
    surface = _check_gt_mesh(gt_mesh, gt, n_gt_samples)
    taus = _check_thresholds(thresholds)
    PC._check_max_distance(max_distance)
    A = None if transform is None else PC.affine_rows(transform)
    kw = _check_align(align, icp)
    p_normals = g_normals = None
    if kw is not None:
        from .tsdf import PointCloud
        p_normals = pred.normals if isinstance(pred, PointCloud) else None
        g_normals = gt.normals if isinstance(gt, PointCloud) else None
        if kw["estimation"] == "point_to_plane" and kw.get("target_normals") is None and g_normals is None and not surface:
            raise ValueError('icp: estimation "point_to_plane" needs target_normals (or a PointCloud gt with normals)')
    if not isinstance(pred, (TSDF, MAP)):
        p = PC.as_points(pred, "pred")
    g = PC.as_points(gt, "gt")
    AR.device_for()                            # (no GPU: the error comes before a map is asked for its points)
    if isinstance(pred, (TSDF, MAP)):
        cloud = pred.extract_pcd(host=False)
        pts = cloud.points
        if pts.shape[0] == 0:
            raise ValueError("pred: the map has no surface points")
        p = PC.as_points(pts, "pred")
        if kw is not None:
            p_normals = cloud.normals
    dev = AR.device_for(p, g)
    alignment = None
    with torch.cuda.device(dev):
        p, g = p.to(dev).contiguous(), g.to(dev).to(torch.float32).contiguous()
        if A is not None:
            moved = torch.empty(p.shape[0], 3, dtype=torch.float32, device=dev)
            L.pc_transform(p, A, moved)
            p = moved
        p = p.to(torch.float32)
        if surface:                                        # g: samples of the surface, with their face normals
            g, _, g_normals, _ = PC.sample_mesh(gt.vertices, gt.triangles, n_gt_samples or int(p.shape[0]), seed=0, device=dev.index)
            if g.shape[0] == 0:
                raise ValueError("gt: the mesh has no triangle of positive area")
            g, g_normals = g.to(dev), g_normals.to(dev)
        if kw is not None:
            p, alignment = _align_icp(p, g, p_normals, g_normals, A, kw, dev)
        if surface:
            from .raycasting import RaycastingScene
            scene = RaycastingScene(device=dev.index)
            scene.add_triangles(gt)
            d_pg = scene.compute_distance(p, max_distance=max_distance)
            if side is not None:
                side["distance"], side["occupancy"] = d_pg, scene.compute_occupancy(p, nsamples=side["nsamples"])
        else:
            d_pg, _ = PC.NearestNeighbours(g).query(p, max_distance=max_distance)
        d_gp, _ = PC.NearestNeighbours(p).query(g, max_distance=max_distance)
        ra, rc = distance_stats_record(d_pg, taus), distance_stats_record(d_gp, taus)
    acc, comp = _distance_stats(ra), _distance_stats(rc)
    k = len(taus)
    with np.errstate(invalid="ignore", divide="ignore"):
        prec = ra[8:8 + k] / (ra[1] + ra[2])
        rec = rc[8:8 + k] / (rc[1] + rc[2])
        f = np.where(prec + rec > 0.0, 2.0 * prec * rec / (prec + rec), 0.0)
    f = np.where(np.isnan(prec) | np.isnan(rec), math.nan, f)
    return ReconstructionMetrics(accuracy=acc, completeness=comp, chamfer=(acc.mean + comp.mean) / 2.0, thresholds=taus, precision=prec, recall=rec,
                                 fscore=f, n_pred=int(ra[0]), n_gt=int(rc[0]), n_unmatched_pred=int(ra[2]), n_unmatched_gt=int(rc[2]),
                                 alignment=alignment)
