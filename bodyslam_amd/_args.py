"""Argument checks shared by the geometry modules (pointcloud, mesh, registration, raycasting, evaluation): one copy of what a number, an
integer, an [n, 3] array of points and a (vertices, triangles) pair are, and of how a call picks its device.  Everything here raises
ValueError before the GPU is touched, except ``device_for``, which is the step that touches it.  Internal: the modules re-export what
their callers know by name."""
from __future__ import annotations

import math
from typing import Callable, List, Optional, Tuple

import numpy as np
import torch

from . import _lib as L


def number(x, what: str, expected: str, ok: Callable[[float], bool] = math.isfinite, fp32: bool = False) -> float:
    """x as a float.  ValueError(f"{what} {x!r}: expected {expected}") unless x is a real number (a bool is not one) and ok(value) holds.
    fp32: the value is rounded to fp32 first (an overflow gives inf), so `ok` judges what a kernel will see."""
    if not isinstance(x, bool) and isinstance(x, (int, float, np.integer, np.floating)):
        if fp32:
            with np.errstate(over="ignore"):
                v = float(np.float32(x))
        else:
            v = float(x)
        if ok(v):
            return v
    raise ValueError(f"{what} {x!r}: expected {expected}")


def positive(v: float) -> bool:
    return v > 0.0 and math.isfinite(v)


def integer(x, what: str, lo: int, hi: Optional[int] = None, expected: Optional[str] = None) -> int:
    """x as an int.  ValueError unless x is an integer (a bool is not one) with lo <= x <= hi (hi None: no upper limit)."""
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < lo or (hi is not None and x > hi):
        raise ValueError(f"{what} {x!r}: expected {expected or (f'an integer >= {lo}' if hi is None else f'an integer in {lo} .. {hi}')}")
    return int(x)


def floating(x, what: str, kinds: str = "a numpy array or a torch tensor") -> torch.Tensor:
    """a numpy array or torch tensor of fp32 or fp64 -> a torch tensor where the data lies"""
    if isinstance(x, np.ndarray):
        if x.dtype not in (np.float32, np.float64):
            raise ValueError(f"{what}: dtype {x.dtype}, expected float32 or float64")
        return torch.from_numpy(np.ascontiguousarray(x))
    if isinstance(x, torch.Tensor):
        if x.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"{what}: dtype {x.dtype}, expected torch.float32 or torch.float64")
        return x.detach()
    raise ValueError(f"{what}: expected {kinds}, got {type(x).__name__}")


def points(x, what: str, allow_empty: bool = False, unwrap: bool = True) -> torch.Tensor:
    """-> fp32 or fp64 torch tensor [n, 3] on whatever device x is on.  x: a numpy array or torch tensor [n, 3], fp32 or fp64; with
    `unwrap` also a tsdf.PointCloud (its points) or a tsdf.TriangleMesh (its vertices).  n = 0 only with allow_empty."""
    kinds = "a numpy array or a torch tensor"
    if unwrap:
        from .tsdf import PointCloud, TriangleMesh
        kinds = "a numpy array, a torch tensor, a PointCloud or a TriangleMesh"
        if isinstance(x, PointCloud):
            x = x.points
        elif isinstance(x, TriangleMesh):
            x = x.vertices
    t = floating(x, what, kinds)
    if t.dim() != 2 or t.shape[1] != 3 or (t.shape[0] < 1 and not allow_empty):
        raise ValueError(f"{what}: shape {tuple(t.shape)}, expected {'' if allow_empty else 'a non-empty '}[n, 3]")
    if t.shape[0] >= 2 ** 31:
        raise ValueError(f"{what}: {t.shape[0]} points: the indices are int32")
    return t


def triangles(vertices, triangles=None, allow_empty_vertices: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (vertices fp32 or fp64 torch [V, 3], triangles integer torch [T, 3]) where they lie.  (vertices, triangles): numpy arrays or torch
    tensors, or a tsdf.TriangleMesh alone.  T may be 0, V only with allow_empty_vertices.  The index range is not checked here: that is
    decided where the data is."""
    from .tsdf import TriangleMesh
    if isinstance(vertices, TriangleMesh):
        if triangles is not None:
            raise ValueError("a TriangleMesh brings its own triangles")
        vertices, triangles = vertices.vertices, vertices.triangles
    v = points(vertices, "vertices", allow_empty=allow_empty_vertices)
    if isinstance(triangles, np.ndarray):
        if triangles.dtype.kind not in "iu":
            raise ValueError(f"triangles: dtype {triangles.dtype}, expected integers")
        if triangles.dtype == np.uint64 and triangles.size and int(triangles.max()) >= 2 ** 63:
            raise ValueError("triangles: an index of 2^63 or more")
        t = torch.from_numpy(np.ascontiguousarray(triangles if triangles.dtype == np.int32 else triangles.astype(np.int64)))
    elif isinstance(triangles, torch.Tensor):
        if triangles.dtype.is_floating_point or triangles.dtype in (torch.bool, torch.complex64, torch.complex128):
            raise ValueError(f"triangles: dtype {triangles.dtype}, expected integers")
        t = triangles.detach()
    else:
        raise ValueError(f"triangles: expected a numpy array or a torch tensor, got {type(triangles).__name__}")
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"triangles: shape {tuple(t.shape)}, expected [T, 3]")
    if t.shape[0] > L.MESH_MAX_TRIANGLES:
        raise ValueError(f"triangles: {t.shape[0]} rows, at most 2^29")
    return v, t


def device_for(*tensors: Optional[torch.Tensor], device: Optional[int] = None) -> torch.device:
    """The device a call runs on: that of the first tensor already on a GPU, else cuda:`device`, else (device None) the current one; the
    library is initialised for it.  Without a GPU this raises BodySlamHipError: there is no CPU fallback."""
    if not torch.cuda.is_available():
        L.init(0)
    for t in tensors:
        if t is not None and t.is_cuda:
            dev = t.device
            break
    else:
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    L.init(dev.index)
    return dev


def first_ranks(flags: Callable, slot_of: torch.Tensor, first: torch.Tensor, status: Optional[torch.Tensor] = None):
    """The rank of every slot's first appearance, for the voxel table and the edge table alike -> (leader int32 [n], rank int32 [n], the
    words of `status` followed by the number of groups rank[-1], as ints from ONE read-back).  flags: L.pc_voxel_flags or
    L.mesh_edge_flags; the inclusive scan between the launches is plumbing: integer, exact.  The group led by item j has row rank[j] - 1."""
    leader, is_first = torch.empty_like(slot_of), torch.empty_like(slot_of)
    flags(slot_of, first, leader, is_first)
    rank = torch.cumsum(is_first, 0).to(torch.int32)
    words: List[int] = [int(x) for x in (rank[-1:] if status is None else torch.cat([status, rank[-1:]])).cpu()]
    return leader, rank, words
