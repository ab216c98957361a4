"""Rigid registration on the device: ICP, what everyone runs before comparing a reconstruction with a scan, and the global registration
that gives ICP its start when the two clouds share no frame (compute_fpfh_feature, match_features, registration_ransac_based_on_*,
registration_global: the second half of this file).

``registration_icp`` is the role of Open3D's ``pipelines.registration.registration_icp`` with ``TransformationEstimationPointToPlane`` or
``TransformationEstimationPointToPoint`` (no scale) and ``ICPConvergenceCriteria``; ``evaluate_registration`` is Open3D's function of that
name.  Open3D is not vendored: the meaning is restated from its published interface and parity with Open3D is unpinned.  The contract is
fixed (include/bodyslam_hip.h, tests/_icp_ref.py): the correspondences are the exact nearest neighbours of bodyslam_amd/pointcloud.py under
its fp32 arithmetic, within a mandatory radius; everything after them is fp64, summed in a fixed order relative to the midpoint of the
target's box.  So a run does not depend on the cell size of the index, and two runs return the same bits.

One iteration is two launches (csrc/icp.hip: bs_icp_step, one thread per source row, and bs_icp_finish, one block that adds, tests the
stopping rule, solves and updates the transform in device memory).  The host enqueues CHUNK iterations at a time and reads the small
state -- status, iteration count, transform, log -- once per chunk: once a status is set the remaining launches of a chunk return at their
first instruction.  There is no CPU fallback: without a GPU the calls raise BodySlamHipError.

Not built: scale estimation (point-to-point with Umeyama scale recovers a true 1.03 as 1.006 on the test surface: the scale comes from the
trajectory, evaluation.similarity_transform, and ICP refines rigidly), robust kernels, coloured and generalised ICP, multi-scale schedules.
(Global registration -- FPFH features, matching, RANSAC: the second half of this file.)  (Normals for a cloud that has none: pointcloud.estimate_normals / PointCloud.estimate_normals, then
target_normals= or a PointCloud target.)
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _args as AR
from . import _lib as L
from . import pointcloud as PC

CHUNK = 8                   # iterations enqueued between two reads of the state (a starting point, not tuned)
ESTIMATIONS = ("auto", "point_to_plane", "point_to_point")
STATUS = {L.ICP_RUNNING: "running", L.ICP_CONVERGED: "converged", L.ICP_MAX_ITERATION: "max_iteration", L.ICP_DEGENERATE: "degenerate"}


@dataclass
class RegistrationResult:
    """transformation: 4 x 4 float64, source -> target.  fitness = the fraction of source rows with a target point within the radius,
    inlier_rmse = the rms of those distances: both of the RETURNED transformation.  iterations: the passes logged; status: "converged",
    "max_iteration", "degenerate" (too few pairs or a singular system: the transformation is the last one before it), or "evaluated"
    (evaluate_registration).  log: one (fitness, rmse, count) per iteration, at the transformation that iteration started from."""
    transformation: np.ndarray
    fitness: float
    inlier_rmse: float
    iterations: int = 0
    status: str = "evaluated"
    log: List[Tuple[float, float, int]] = field(default_factory=list)


def _check_radius(r) -> float:
    return AR.number(r, "max_correspondence_distance", "a positive number (finite and non-zero in fp32)", AR.positive, fp32=True)


def _check_init(init, what: str = "init") -> np.ndarray:
    if init is None:
        return np.eye(4)
    try:
        T = np.asarray(PC._np(init), dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: expected a 4 x 4") from None
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise ValueError(f"{what}: expected a finite 4 x 4, got shape {T.shape}")
    return T.copy()


def _check_criteria(max_iteration, relative_fitness, relative_rmse) -> Tuple[int, float, float]:
    n = AR.integer(max_iteration, "max_iteration", 1, L.ICP_MAX_ITERATIONS)
    fitness, rmse = (AR.number(v, name, "a number", lambda v: not math.isnan(v))
                     for name, v in (("relative_fitness", relative_fitness), ("relative_rmse", relative_rmse)))
    return n, fitness, rmse


def _as_normals(normals, n: int) -> torch.Tensor:
    t = PC.as_points(normals, "target_normals")
    if t.shape[0] != n:
        raise ValueError(f"target_normals: shape {tuple(t.shape)}, expected [{n}, 3] like the target")
    return t


def _resolve(source, target, max_correspondence_distance, estimation, target_normals, cell_size):
    """the host-side checks of both entries -> (source tensor, target points tensor or None for a prebuilt index, normals tensor or None,
    radius, estimation constant); nothing here touches the device"""
    from .tsdf import PointCloud
    radius = _check_radius(max_correspondence_distance)
    if estimation not in ESTIMATIONS:
        raise ValueError(f"unknown estimation {estimation!r}: one of {ESTIMATIONS}")
    PC._check_cell_size(cell_size)
    s = PC.as_points(source, "source")
    if isinstance(target, PC.NearestNeighbours):
        t, n_target = None, len(target)
    else:
        t = PC.as_points(target, "target")
        n_target = int(t.shape[0])
    normals = target_normals
    if normals is None and isinstance(target, PointCloud):
        normals = target.normals
    nt = None if normals is None else _as_normals(normals, n_target)
    if estimation == "point_to_plane" and nt is None:
        raise ValueError('estimation "point_to_plane" needs target_normals (or a PointCloud target with normals)')
    plane = estimation == "point_to_plane" or (estimation == "auto" and nt is not None)
    return s, t, (nt if plane else None), radius, (L.ICP_POINT_TO_PLANE if plane else L.ICP_POINT_TO_POINT)


class _Run:
    """the device side of one registration: the index, the buffers and the two launches"""

    def __init__(self, s, t, target, nt, radius, est, cell_size, device, T0, max_iteration, relative_fitness, relative_rmse):
        self.nn = target if t is None else PC.NearestNeighbours(t, cell_size=cell_size, device=device)
        self.dev = AR.device_for(device=self.nn.dev.index)
        self.radius, self.est, self.crit = radius, est, (max_iteration, relative_fitness, relative_rmse)
        with torch.cuda.device(self.dev):
            self.src = s.to(self.dev).contiguous()
            self.normals = None if nt is None else nt.to(self.dev).to(torch.float32).contiguous()
            self.m = int(self.src.shape[0])
            host = np.zeros(L.ICP_STATE_FIELDS + L.ICP_LOG_FIELDS * max_iteration, np.float64)
            host[2:14] = T0[:3].reshape(-1)
            self.state = torch.from_numpy(host).to(self.dev)
            self.partial = torch.empty(-(-self.m // L.ICP_BLOCK), L.ICP_PARTIAL_FIELDS, dtype=torch.float64, device=self.dev)

    def launch(self, mode):
        nn = self.nn
        L.icp_step(nn.records, nn.n_finite, nn.cell_start, nn.lo, nn.hi, nn.cell_size, nn.dims, nn.target, self.normals, self.src, self.radius,
                   self.est, mode, self.state, self.partial)
        L.icp_finish(self.partial, self.m, nn.lo, nn.hi, self.est, mode, *self.crit, self.state)

    def read(self) -> np.ndarray:
        return self.state.cpu().numpy()

    @staticmethod
    def transformation(host) -> np.ndarray:
        T = np.eye(4)
        T[:3] = host[2:14].reshape(3, 4)
        return T


def registration_icp(source, target, max_correspondence_distance, init=None, estimation: str = "auto", target_normals=None,
                     max_iteration: int = 30, relative_fitness: float = 1e-6, relative_rmse: float = 1e-6, cell_size: Optional[float] = None,
                     device: int = 0) -> RegistrationResult:
    """Rigid ICP of `source` onto `target` from `init` (a 4 x 4, None = identity) -> RegistrationResult.

    source, target: anything pointcloud.as_points takes (numpy or torch [n, 3], fp32 or fp64, host or device; a tsdf.PointCloud; a
    tsdf.TriangleMesh); target may also be an existing pointcloud.NearestNeighbours (cell_size and device are then its own).  fp64 target
    points are rounded to fp32 once; an fp64 source is transformed in fp64 and rounded after it.  max_correspondence_distance: the radius,
    mandatory, a positive finite fp32 number.  estimation: "point_to_plane" (needs target_normals [n, 3], or a PointCloud target's
    normals; numpy or device tensors; a zero or non-finite normal leaves its pairs out of the sums), "point_to_point" (no scale), or
    "auto": point-to-plane when normals are there.  Stops "converged" when fitness and rmse both change by less than relative_fitness /
    relative_rmse between two iterations, "max_iteration" after max_iteration updates, "degenerate" when there are too few pairs or the
    system is singular.  Raises ValueError on bad arguments before the GPU is touched."""
    s, t, nt, radius, est = _resolve(source, target, max_correspondence_distance, estimation, target_normals, cell_size)
    T0 = _check_init(init)
    crit = _check_criteria(max_iteration, relative_fitness, relative_rmse)
    run = _Run(s, t, target, nt, radius, est, cell_size, device, T0, *crit)
    with torch.cuda.device(run.dev):
        enqueued = 0
        while True:
            k = min(CHUNK, crit[0] - enqueued)
            for _ in range(k):
                run.launch(L.ICP_ITERATE)
            enqueued += k
            host = run.read()
            if host[0] != L.ICP_RUNNING:
                break
            if enqueued >= crit[0]:
                raise L.BodySlamHipError("bs_icp_finish: no status after max_iteration iterations")
        run.launch(L.ICP_EVALUATE)
        host = run.read()
    its = int(host[1])
    log = host[L.ICP_STATE_FIELDS:L.ICP_STATE_FIELDS + L.ICP_LOG_FIELDS * its].reshape(its, L.ICP_LOG_FIELDS)
    return RegistrationResult(transformation=_Run.transformation(host), fitness=float(host[16]), inlier_rmse=float(host[17]), iterations=its,
                              status=STATUS[int(host[0])], log=[(float(r[0]), float(r[1]), int(r[2])) for r in log])


def evaluate_registration(source, target, max_correspondence_distance, transformation=None) -> RegistrationResult:
    """Open3D's evaluate_registration: fitness and inlier_rmse of `transformation` (a 4 x 4, None = identity), the correspondence pass of
    registration_icp on its own -> RegistrationResult(status="evaluated")."""
    s, t, _, radius, est = _resolve(source, target, max_correspondence_distance, "point_to_point", None, None)
    T0 = _check_init(transformation, "transformation")
    run = _Run(s, t, target, None, radius, est, None, 0, T0, 1, 0.0, 0.0)
    with torch.cuda.device(run.dev):
        run.launch(L.ICP_EVALUATE)
        host = run.read()
    return RegistrationResult(transformation=T0, fitness=float(host[16]), inlier_rmse=float(host[17]))


def _step_sums(source, target, max_correspondence_distance, init=None, estimation="auto", target_normals=None, cell_size=None, device=0):
    """One correspondence pass at `init` without an update, for the tests and tools: (the block partials fp64 [blocks,
    ICP_PARTIAL_FIELDS], the summed row fp64 [ICP_PARTIAL_FIELDS]) as numpy -- count, usable count, sum d^2, then the 27 or 15 sums."""
    s, t, nt, radius, est = _resolve(source, target, max_correspondence_distance, estimation, target_normals, cell_size)
    run = _Run(s, t, target, nt, radius, est, cell_size, device, _check_init(init), 1, 0.0, 0.0)
    with torch.cuda.device(run.dev):
        run.launch(L.ICP_EVALUATE)
        host = run.read()
        return run.partial.cpu().numpy(), host[32:32 + L.ICP_PARTIAL_FIELDS].copy()


# ---- global registration: FPFH features, matching, RANSAC (csrc/global_registration.hip) -------------------------------
# The roles of Open3D's compute_fpfh_feature and registration_ransac_based_on_feature_matching / _on_correspondence: a pose between two clouds
# that share no frame, the `init` of registration_icp.  The reference only calls Open3D.  Restated from Rusu, Blodow & Beetz 2009 (FPFH),
# Fischler & Bolles 1981 (RANSAC), Kabsch 1976 / Arun, Huang & Blostein 1987 (the fit, csrc/rigid3.h) and Open3D's documented meaning; parity
# with Open3D is unpinned.  The statement is tests/_global_registration_ref.py.  No floating-point atomics: the same input gives the same bits
# in every call and at every cell size.  There is no CPU fallback.
# Not built: normal and correspondence checkers beyond the edge-length and distance checkers, ransac_n != 3, scale, fast global registration
# (FGR), a k-d tree in feature space (the match is exhaustive).
RANSAC_CHUNK = 4096         # hypotheses between two reads of the best score: a constant, so that the result does not depend on timing
LIST_BUDGET = 1 << 26       # neighbour-list entries held at a time by compute_fpfh_feature: larger clouds are queried in source chunks
NORMAL_SIGNS = ("either", "given")
RANSAC_KEYS = ("edge_length_threshold", "max_iteration", "confidence", "n_refit", "seed")
GLOBAL_KEYS = ("feature_radius", "max_correspondence_distance", "normal_sign") + RANSAC_KEYS
RANSAC_MAX_ITERATION = 2 ** 31 - 1 - RANSAC_CHUNK

last_global = None          # the GlobalRegistrationResult of the last registration_global (align="global" leaves it here)
keep_tables = False         # tests: registration_ransac_based_on_correspondence keeps every chunk's (valid, score) in last_tables
last_tables: List[Tuple[np.ndarray, np.ndarray]] = []


@dataclass
class GlobalRegistrationResult(RegistrationResult):
    """RegistrationResult of a RANSAC over correspondences: fitness = inliers / correspondences (Open3D's correspondence-based evaluation),
    inlier_rmse over the inliers, iterations = the refit rounds run, status "converged" (the confidence stop was met), "max_iteration" or
    "degenerate" (identity, zero mask, h = -1).  correspondences: int32 [c, 2] (source row, target row), inlier_mask: bool [c], device
    tensors (registration_global: rows of the thinned clouds); hypotheses: the number tried; h: the winner."""
    correspondences: Optional[torch.Tensor] = None
    inlier_mask: Optional[torch.Tensor] = None
    hypotheses: int = 0
    h: int = -1

    @property
    def inliers(self) -> int:
        return 0 if self.inlier_mask is None else int(self.inlier_mask.sum())


def _check_max_nn(max_nn) -> Optional[int]:
    return None if max_nn is None else AR.integer(max_nn, "max_nn", 1, None, "None or an integer >= 1")


def _check_features(f, what: str, rows: Optional[int] = None) -> torch.Tensor:
    t = AR.floating(f, what)
    if t.dim() != 2 or t.shape[1] != L.FPFH_DIM or (rows is not None and t.shape[0] != rows):
        raise ValueError(f"{what}: shape {tuple(t.shape)}, expected [{'n' if rows is None else rows}, {L.FPFH_DIM}]")
    return t


def _check_ransac(edge_length_threshold=0.9, max_iteration=100000, confidence=0.999, n_refit=2, seed=0) -> dict:
    return dict(edge_length_threshold=AR.number(edge_length_threshold, "edge_length_threshold", "a number in (0, 1]", lambda v: 0.0 < v <= 1.0),
                max_iteration=AR.integer(max_iteration, "max_iteration", 1, RANSAC_MAX_ITERATION),
                confidence=AR.number(confidence, "confidence", "a number in (0, 1), both excluded", lambda v: 0.0 < v < 1.0),
                n_refit=AR.integer(n_refit, "n_refit", 0, 64), seed=AR.integer(seed, "seed", 0, 2 ** 64 - 1))


def _check_ransac_keys(kw: dict, allowed=RANSAC_KEYS, what: str = "ransac") -> dict:
    unknown = sorted(set(kw) - set(allowed))
    if unknown:
        raise ValueError(f"{what}: unknown keys {unknown}; the keywords are {allowed}")
    return _check_ransac(**{k: v for k, v in kw.items() if k in RANSAC_KEYS})


def _check_corres(corres, n_source: int, n_target: int) -> torch.Tensor:
    if isinstance(corres, np.ndarray):
        if corres.dtype.kind not in "iu":
            raise ValueError(f"corres: dtype {corres.dtype}, expected integers")
        corres = torch.from_numpy(np.ascontiguousarray(corres.astype(np.int64)))
    if not isinstance(corres, torch.Tensor) or corres.dtype.is_floating_point or corres.dtype == torch.bool:
        raise ValueError("corres: expected an integer numpy array or torch tensor [c, 2]")
    c = corres.detach()
    if c.dim() != 2 or c.shape[1] != 2:
        raise ValueError(f"corres: shape {tuple(c.shape)}, expected [c, 2]")
    if c.shape[0] >= 2 ** 31:
        raise ValueError(f"corres: {c.shape[0]} rows: the indices are int32")
    if c.shape[0]:
        lo, hi0, hi1 = int(c.min()), int(c[:, 0].max()), int(c[:, 1].max())
        if lo < 0 or hi0 >= n_source or hi1 >= n_target:
            raise ValueError(f"corres: indices out of range (source rows 0 .. {n_source - 1}, target rows 0 .. {n_target - 1})")
    return c.to(torch.int64)


def _fpfh(points, normals, radius, max_nn, cell_size, device):
    """-> (features fp32 [n, 33], spfh int32 [n, FPFH_ROW]: 33 counts, k, 0, 0), device tensors"""
    r = PC._check_search_radius(radius)
    k = _check_max_nn(max_nn)
    PC._check_cell_size(cell_size)
    t = PC.as_points(points, "points")
    n = int(t.shape[0])
    nr = PC.as_points(normals, "normals", unwrap=False) if normals is not None else None
    if nr is None or nr.shape[0] != n:
        raise ValueError(f"normals: expected [{n}, 3] like the points")
    nn = PC.NearestNeighbours.for_radius(t, r, cell_size=cell_size, device=device)
    dev = nn.dev
    with torch.cuda.device(dev):
        table = torch.zeros(n, 8, dtype=torch.float32, device=dev)                     # (x, y, z, ., nx, ny, nz, .): two 16-byte records a point
        table[:, 0:3] = nn.target
        table[:, 4:7] = nr.to(dev).to(torch.float32)
        spfh = torch.zeros(n, L.FPFH_ROW, dtype=torch.int32, device=dev)
        features = torch.zeros(n, L.FPFH_DIM, dtype=torch.float32, device=dev)
        count = nn.count_radius(nn.target, r).to(torch.int64)
        if k is not None:
            count = count.clamp(max=k)
        ends = torch.cumsum(count, 0).cpu().numpy()                                    # source chunks whose lists stay below LIST_BUDGET entries
        bounds, first = [0], 0
        while first < n:
            base = int(ends[first - 1]) if first else 0
            last = int(np.searchsorted(ends, base + LIST_BUDGET, side="right"))
            first = max(last, first + 1)
            bounds.append(min(first, n))
        chunks = list(zip(bounds[:-1], bounds[1:]))
        held = None
        for a, b in chunks:
            held = nn.query_radius(nn.target[a:b], r, max_nn=k)
            if held[1].numel():                                                         # (no list at all: every row of the chunk stays zero)
                L.fpfh_spfh(table, *held, a, spfh)
        for a, b in chunks:
            lists = held if len(chunks) == 1 else nn.query_radius(nn.target[a:b], r, max_nn=k)
            if lists[1].numel():
                L.fpfh_features(spfh, *lists, a, features)
    return features, spfh


def compute_fpfh_feature(points, normals, radius, max_nn: Optional[int] = 100, cell_size: Optional[float] = None, device: int = 0) -> torch.Tensor:
    """Fast point feature histograms -> fp32 [n, 33] device tensor, one row per point: Open3D's compute_fpfh_feature with
    KDTreeSearchParamHybrid(radius, max_nn) (Rusu, Blodow & Beetz 2009; restated, parity with Open3D unpinned; the statement is
    tests/_global_registration_ref.py).

    The neighbours of point i are the row of NearestNeighbours.query_radius(cloud on itself, radius, max_nn) without its entries of d2 == 0
    (the point itself, coincident points); max_nn=None takes everything within the radius.  Per pair, in fp64: the three Darboux-frame
    features, eleven bins each (33 integer counts and the number k of counted pairs per point: the SPFH, independent of the order of the
    row); a pair with a zero or non-finite normal at either end is skipped.  FPFH(i) = the blocks of sum_j SPFH(j) / d2_ij, each scaled to
    sum 100, + SPFH(i), summed in fp64 in a fixed order and rounded to fp32 once.  A non-finite point, or a point without counted pairs, has
    a zero row.  The cell size changes the time, never the bits.  Raises ValueError on bad arguments before the GPU is touched."""
    return _fpfh(points, normals, radius, max_nn, cell_size, device)[0]


def mirror_fpfh(features):
    """The features a cloud would have with every normal negated: blocks 1 and 3 (f1, f3) reversed, block 2 unchanged -- a bin permutation, bit
    for bit.  estimate_normals without direction or camera_location orients by the largest component, which is deterministic, consistent
    only on a nearly flat cloud (on a tube both signs appear) and flips with the cloud's pose.
    pointcloud.orient_normals_consistent_tangent_plane gives one sign per surface, but which of the two remains arbitrary between two
    clouds: registration_global(normal_sign="either") therefore tries both.  numpy in, numpy out; torch in, torch out."""
    perm = list(range(10, -1, -1)) + list(range(11, 22)) + list(range(32, 21, -1))
    if isinstance(features, np.ndarray):
        _check_features(features, "features")
        return np.ascontiguousarray(features[:, perm])
    f = _check_features(features, "features")
    return f[:, torch.tensor(perm, device=f.device)].contiguous()


def _nearest_feature(s: torch.Tensor, t: torch.Tensor, splits: Optional[int] = None) -> torch.Tensor:
    """s fp32 [m, 33], t fp32 [n, 33] on the device, m, n >= 1 -> int64 [m]: the target row of the minimum (distance, index), -1 for none"""
    m, n = int(s.shape[0]), int(t.shape[0])
    if splits is None:                                                                 # enough blocks for the device, a tile of 64 rows at least
        splits = max(1, min(-(-n // 64), -(-1024 // -(-m // 256)), 65535))
    best = torch.full((m,), -1, dtype=torch.int64, device=s.device)
    L.feature_match(s, t, splits, best)
    return torch.where(best == -1, best, best & 0xffffffff)


def match_features(source_features, target_features, mutual_filter: bool = False, _splits: Optional[int] = None) -> torch.Tensor:
    """Nearest neighbours in feature space -> correspondences int32 [c, 2] = (source row, target row), a device tensor, ascending by source
    row: the matching step of Open3D's registration_ransac_based_on_feature_matching (restated, parity unpinned).

    distance = sum_k (a_k - b_k)^2 in fp32, added in order; the match of a source row is the minimum of (distance, target index): ties go to
    the lower index.  A row that contains a non-finite value neither matches nor is matched.  mutual_filter: a pair is kept when the target
    row's match, by the same rule with the roles exchanged, is that source row.  Exhaustive (no index in feature space)."""
    s, t = _check_features(source_features, "source_features"), _check_features(target_features, "target_features")
    if not isinstance(mutual_filter, (bool, np.bool_)):
        raise ValueError(f"mutual_filter {mutual_filter!r}: expected a bool")
    dev = AR.device_for(s, t)
    with torch.cuda.device(dev):
        s, t = s.to(dev).to(torch.float32).contiguous(), t.to(dev).to(torch.float32).contiguous()
        m = int(s.shape[0])
        if m == 0 or t.shape[0] == 0:
            return torch.zeros(0, 2, dtype=torch.int32, device=dev)
        fwd = _nearest_feature(s, t, _splits)
        keep = fwd >= 0
        if mutual_filter:
            back = _nearest_feature(t, s, _splits)
            keep &= back[fwd.clamp(min=0)] == torch.arange(m, device=dev)
        rows = torch.nonzero(keep).reshape(-1)                                          # (the compaction is plumbing)
        return torch.stack([rows, fwd[rows]], 1).to(torch.int32).contiguous()


def _stop_need(best: int, c: int, confidence: float) -> float:
    """Open3D's stop rule: the hypotheses that `confidence` asks for when the best hypothesis holds `best` of c correspondences"""
    ratio = best / c
    if ratio >= 1.0:
        return 0.0
    return math.log(1.0 - confidence) / math.log(1.0 - ratio ** 3)


def _degenerate(corres, dev, tried: int) -> GlobalRegistrationResult:
    return GlobalRegistrationResult(transformation=np.eye(4), fitness=0.0, inlier_rmse=0.0, iterations=0, status="degenerate", correspondences=corres,
                                    inlier_mask=torch.zeros(int(corres.shape[0]), dtype=torch.bool, device=dev), hypotheses=tried, h=-1)


def registration_ransac_based_on_correspondence(source, target, corres, max_correspondence_distance, edge_length_threshold: float = 0.9,
                                                max_iteration: int = 100000, confidence: float = 0.999, n_refit: int = 2, seed: int = 0,
                                                device: int = 0) -> GlobalRegistrationResult:
    """RANSAC over any number of correspondences -> GlobalRegistrationResult: Open3D's registration_ransac_based_on_correspondence with
    ransac_n = 3, CorrespondenceCheckerBasedOnEdgeLength(edge_length_threshold), CorrespondenceCheckerBasedOnDistance(
    max_correspondence_distance) and RANSACConvergenceCriteria(max_iteration, confidence) (Fischler & Bolles 1981; restated, parity unpinned).

    corres: integers [c, 2] = (source row, target row).  Hypothesis h draws three distinct correspondences from loop closure's counter-based
    hash of (seed, h, draw); it is rejected before any fit unless every pair of the three has |ps| >= s |pt| and |pt| >= s |ps|; the fit is
    Kabsch with its rank test; the three samples must lie within the distance after the fit; the score is the number of correspondences
    with squared residual below the squared distance.  Hypotheses run in chunks of RANSAC_CHUNK; after a chunk the run stops "converged"
    when log(1 - confidence) / log(1 - (best / c)^3) <= the hypotheses tried.  The winner is the highest score, then the lowest h; a best
    score below 3 is "degenerate".  Then n_refit rounds of Kabsch over the inliers with a recount after each.  Everything is fp64, summed
    in a fixed order.  Raises ValueError on bad arguments before the GPU is touched."""
    global last_tables
    tau = _check_radius(max_correspondence_distance)
    rk = _check_ransac(edge_length_threshold, max_iteration, confidence, n_refit, seed)
    s, t = PC.as_points(source, "source"), PC.as_points(target, "target")
    cr = _check_corres(corres, int(s.shape[0]), int(t.shape[0]))
    dev = AR.device_for(s, t, cr, device=device)
    c = int(cr.shape[0])
    with torch.cuda.device(dev):
        cr = cr.to(dev)
        out_corres = cr.to(torch.int32).contiguous()
        last_tables = []
        if c < 3:
            return _degenerate(out_corres, dev, 0)
        corr = torch.cat([s.to(dev).to(torch.float64)[cr[:, 0]], t.to(dev).to(torch.float64)[cr[:, 1]]], 1).contiguous()      # [c, 6]
        fits = torch.empty(RANSAC_CHUNK * 12, dtype=torch.float64, device=dev)
        valid = torch.empty(RANSAC_CHUNK, dtype=torch.int32, device=dev)
        score = torch.empty(RANSAC_CHUNK, dtype=torch.int32, device=dev)
        best = torch.zeros(1, dtype=torch.int64, device=dev)
        tried, key, status = 0, 0, "max_iteration"
        while tried < rk["max_iteration"]:
            cnt = min(RANSAC_CHUNK, rk["max_iteration"] - tried)
            L.gr_hypotheses(corr, rk["seed"], tried, cnt, rk["edge_length_threshold"], tau, fits, valid)
            score.zero_()
            lst = torch.nonzero(valid[:cnt]).reshape(-1).to(torch.int32)                # (the compaction is plumbing)
            if lst.numel():
                splits = max(1, min(-(-c // L.GR_BLOCK), -(-512 // -(-int(lst.numel()) // L.GR_BLOCK)), 65535))
                L.gr_score(corr, fits, lst, cnt, splits, tau, score)
                L.gr_winner(score, cnt, tried, best)
            if keep_tables:
                last_tables.append((valid[:cnt].cpu().numpy().astype(bool), score[:cnt].cpu().numpy().astype(np.int64)))
            tried += cnt
            key = int(best.cpu())
            if (key >> 32) > 0 and _stop_need(key >> 32, c, rk["confidence"]) <= tried:
                status = "converged"
                break
        if (key >> 32) < 3:
            return _degenerate(out_corres, dev, tried)
        h = (~key) & 0xffffffff
        state = torch.zeros(L.GR_STATE_FIELDS, dtype=torch.float64, device=dev)
        mask = torch.zeros(c, dtype=torch.int32, device=dev)
        partial = torch.zeros(-(-c // L.GR_BLOCK), L.GR_PARTIAL_FIELDS, dtype=torch.float64, device=dev)
        L.gr_winner_fit(corr, rk["seed"], h, rk["edge_length_threshold"], tau, state)
        for rnd in range(rk["n_refit"] + 1):
            L.gr_refit_step(corr, state, tau, mask, partial)
            L.gr_refit_finish(partial, c, rnd == rk["n_refit"], state)
        host = state.cpu().numpy()
        if host[12] != 1.0:
            return _degenerate(out_corres, dev, tried)
        T = np.eye(4)
        T[:3] = host[:12].reshape(3, 4)
        return GlobalRegistrationResult(transformation=T, fitness=float(host[13]) / c, inlier_rmse=float(host[14]), iterations=int(host[15]), status=status,
                                        correspondences=out_corres, inlier_mask=mask != 0, hypotheses=tried, h=int(h))


def registration_ransac_based_on_feature_matching(source, target, source_feature, target_feature, mutual_filter, max_correspondence_distance,
                                                  edge_length_threshold: float = 0.9, max_iteration: int = 100000, confidence: float = 0.999,
                                                  n_refit: int = 2, seed: int = 0, device: int = 0) -> GlobalRegistrationResult:
    """match_features(source_feature, target_feature, mutual_filter), then registration_ransac_based_on_correspondence over the matches ->
    GlobalRegistrationResult: Open3D's registration_ransac_based_on_feature_matching (restated, parity unpinned).  The features are [n, 33],
    one row per point of their cloud."""
    _check_radius(max_correspondence_distance)
    _check_ransac(edge_length_threshold, max_iteration, confidence, n_refit, seed)
    s, t = PC.as_points(source, "source"), PC.as_points(target, "target")
    _check_features(source_feature, "source_feature", int(s.shape[0]))
    _check_features(target_feature, "target_feature", int(t.shape[0]))
    corres = match_features(source_feature, target_feature, mutual_filter)
    return registration_ransac_based_on_correspondence(s, t, corres, max_correspondence_distance, edge_length_threshold, max_iteration, confidence,
                                                       n_refit, seed, device)


def _cloud_normals(cloud, normals, what: str):
    from .tsdf import PointCloud
    if normals is None and isinstance(cloud, PointCloud):
        normals = cloud.normals
    pts = PC.as_points(cloud, what)
    if normals is None:
        return pts, None
    nr = PC.as_points(normals, f"{what}_normals", unwrap=False)
    if nr.shape[0] != pts.shape[0]:
        raise ValueError(f"{what}_normals: shape {tuple(nr.shape)}, expected [{int(pts.shape[0])}, 3] like the {what}")
    return pts, nr


def registration_global(source, target, voxel_size, source_normals=None, target_normals=None, feature_radius: Optional[float] = None,
                        max_correspondence_distance: Optional[float] = None, normal_sign: str = "either", **ransac) -> GlobalRegistrationResult:
    """The usual recipe before ICP -> GlobalRegistrationResult, source -> target, also left in ``last_global``.

    Both clouds are thinned with pointcloud.voxel_down_sample(voxel_size, normals=..., unit_normals=True); a cloud without normals (no
    argument, no PointCloud normals) gets pointcloud.estimate_normals(k=30) of its thinned points; the features are
    compute_fpfh_feature(feature_radius = 5 voxel_size); then registration_ransac_based_on_feature_matching with the mutual filter at
    max_correspondence_distance = 1.5 voxel_size -- Open3D's tutorial values.  normal_sign="either": matching and RANSAC run a second time
    on mirror_fpfh of the source features (estimated normals flip with a cloud's pose) and the run with more inliers is returned, a tie
    going to the unmirrored run; "given": one run.  ransac: edge_length_threshold, max_iteration, confidence, n_refit, seed.  The
    correspondences of the result are rows of the thinned clouds; the transformation applies to `source` as given."""
    global last_global
    h = PC._check_voxel_size(voxel_size)
    fr = PC._check_search_radius(5.0 * h if feature_radius is None else feature_radius, "feature_radius")
    tau = _check_radius(1.5 * h if max_correspondence_distance is None else max_correspondence_distance)
    if normal_sign not in NORMAL_SIGNS:
        raise ValueError(f"unknown normal_sign {normal_sign!r}: one of {NORMAL_SIGNS}")
    rk = _check_ransac_keys(ransac)
    (s, sn), (t, tn) = _cloud_normals(source, source_normals, "source"), _cloud_normals(target, target_normals, "target")
    dev = AR.device_for(s, t)
    with torch.cuda.device(dev):
        def thinned(cloud, normals):
            r = PC.voxel_down_sample(cloud.to(dev), h, normals=None if normals is None else normals.to(dev), unit_normals=True, device=dev.index)
            return r.points, (PC.estimate_normals(r.points, k=30, device=dev.index) if normals is None else r.normals)
        (ps, ns), (pt, nt) = thinned(s, sn), thinned(t, tn)
        fs = compute_fpfh_feature(ps, ns, fr, device=dev.index)
        ft = compute_fpfh_feature(pt, nt, fr, device=dev.index)
        res = registration_ransac_based_on_feature_matching(ps, pt, fs, ft, True, tau, device=dev.index, **rk)
        if normal_sign == "either":
            other = registration_ransac_based_on_feature_matching(ps, pt, mirror_fpfh(fs), ft, True, tau, device=dev.index, **rk)
            if other.inliers > res.inliers:
                res = other
    last_global = res
    return res
