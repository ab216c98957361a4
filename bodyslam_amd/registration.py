"""Rigid ICP registration on the device: what everyone runs before comparing a reconstruction with a scan.

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
trajectory, evaluation.similarity_transform, and ICP refines rigidly), robust kernels, global registration, coloured and generalised ICP,
multi-scale schedules.  (Normals for a cloud that has none: pointcloud.estimate_normals / PointCloud.estimate_normals, then
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
