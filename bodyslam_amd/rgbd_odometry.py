"""Dense RGB-D odometry of the VO step: what ``VO._compute_vo_o3d`` gets from Open3D's
``rgbd_odometry_multi_scale(curr, prev, intrinsic, init, 1000.0, depth_max, [20, 10, 5], Method.Hybrid)``
(BodySLAM_not_refactored/3DM/visual_odometry.py:97-120): the relative pose between two RGB-D frames.

Open3D is not vendored and not installable offline; the algorithm is restated in oracle/rgbd_odometry_ref.py from the published
structure of its tensor hybrid odometry (parity with Open3D unpinned): intensity = grey / 255, depth = raw / depth_scale with values
<= 0 or > depth_max invalid, a 3-level pyramid ([1 4 6 4 1]^2 / 256; depth: the weights over the neighbours within 2 * 0.07 m of the
centre), target Sobel gradients / 8, coarse to fine with 20 / 10 / 5 Gauss-Newton iterations on the photometric + geometric
residuals, 0.07 m depth outlier gate, Huber deltas 0.1 / 0.05.

``association="nearest"`` (the default, the faithful mode): the target images and gradients are read at the NEAREST pixel of the
projected source point, and the robust step has Open3D's form (J^T J unweighted, J^T applied to the Huber-clipped residual).
``association="bilinear"`` (round 2's variant, kept as an option): the target is sampled bilinearly and the step is IRLS-weighted --
a smooth cost, which on sub-pixel motions converges to the micrometre where the nearest-pixel cost is piecewise constant.

Everything runs in the kernels of csrc/odometry.hip.  Three ways to call it:
  * ``RGBDOdometry()(curr_rgbd, prev_rgbd)`` -- what ``_compute_vo_o3d`` returns (the inverse of source -> target), one pair at a time;
  * ``track(color, depth)`` -- a stream of consecutive frames: each frame's pyramid and gradients are built ONCE (it is the source of
    one pair and the target of the next), the 11 + 70 launches of a frame are captured in a HIP graph and replayed, and the pose
    stays on the device, so a sequence is tracked without a host round trip per pair;
  * ``track_block(colors, depths)`` -- a block of consecutive frames at once.  The pairs of a sequence do not depend on each other
    (the reference starts every pair from the identity, visual_odometry.py:100), so n frames are n simultaneous pairs: every stage is
    ONE launch over the whole block (~100 launches per block instead of 81 per frame) and the work is HBM streaming instead of a
    chain of 10-microsecond launches.  Pair for pair the same sums in the same order as the other two: bit-equal results.
All three go through one pyramid build and one step loop: a pair is a batch of one.

``PointToPlaneOdometry`` (below) is the other registration of the reference's Open3D models: a depth frame against the map's
ray-cast depth, point-to-plane, what ``MAP.track_frame_to_model`` runs."""
from __future__ import annotations

import ctypes as C
import functools
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

DEPTH_OUTLIER_TRUNC, DEPTH_HUBER, INTENSITY_HUBER = 0.07, 0.05, 0.1      # o3d.t.pipelines.odometry.OdometryLossParams defaults
ITERATIONS = (20, 10, 5)                                                   # visual_odometry.py:103-107, coarse -> fine
FLAG_NEAREST, FLAG_O3D_LOSS = 1, 2


def se3_exp(delta: np.ndarray) -> np.ndarray:
    w, v = np.asarray(delta[:3], dtype=np.float64), np.asarray(delta[3:], dtype=np.float64)
    th = float(np.linalg.norm(w))
    Wx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        R, V = np.eye(3) + Wx, np.eye(3) + 0.5 * Wx
    else:
        a, b, c = np.sin(th) / th, (1.0 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
        R = np.eye(3) + a * Wx + b * (Wx @ Wx)
        V = np.eye(3) + b * Wx + c * (Wx @ Wx)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, V @ v
    return T


# ---- what both odometries share: level shapes, the schedule, scratch, the host-walked loop ----------------------------------------
def _level_shapes(H: int, W: int, K: Sequence[float], n_levels: int) -> List[Tuple[int, int, np.ndarray]]:
    """(h, w, intrinsics as 4 host doubles) of every pyramid level, fine to coarse: sizes halve rounding up, intrinsics halve"""
    shapes, k = [], tuple(K)
    for _ in range(n_levels):
        shapes.append((H, W, np.array(k, dtype=np.float64)))
        H, W, k = (H + 1) // 2, (W + 1) // 2, tuple(v / 2.0 for v in k)
    return shapes


def _schedule(iterations: Sequence[int]) -> List[Tuple[int, int]]:
    """(level, iterations) coarse to fine"""
    return list(zip(range(len(iterations) - 1, -1, -1), iterations))


@functools.lru_cache(maxsize=None)
def _identity12(dev: torch.device) -> torch.Tensor:
    """rows 0..2 of the identity on the device: uploaded once, only ever read"""
    return torch.tensor([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=torch.float64, device=dev)


def _scratch(n: int, H: int, W: int, dev: torch.device) -> dict:
    """for n simultaneous pairs: the identity pose T0 [12], the poses T [n, 12], the Gauss-Newton step's block partials and sums"""
    blocks = min((H * W + 255) // 256, 256)          # the grid of the accumulate kernels (csrc/odometry.hip odo_grid)
    return dict(T0=_identity12(dev),
                T=torch.empty(n, 12, dtype=torch.float64, device=dev),
                partial=torch.empty(n, blocks, 29, dtype=torch.float64, device=dev),
                out=torch.zeros(n, 29, dtype=torch.float64, device=dev))


def _pyrdown(src: int, n: int, H: int, W: int, dst: int, depth_threshold: Optional[float], st: int) -> None:
    """n images at address src -> their next level at dst, on stream st; depth_threshold None: an intensity image"""
    is_depth = depth_threshold is not None
    L.check(L.load_library().bs_odo_pyrdown(src, n, H, W, dst, int(is_depth), depth_threshold if is_depth else 0.0, st), "bs_odo_pyrdown")


def _host_walk(T: np.ndarray, schedule: Sequence[Tuple[int, int]], sums: Callable[[int, np.ndarray], np.ndarray], starved_leaves_level: bool):
    """The Gauss-Newton loop walked from the host (trace=True: tests, diagnostics).  sums(level, T12) returns the 29 sums of that level
    at the host pose T12 (12 doubles).  Every step is logged as (level, A, b, cost, inliers); a step with fewer than 6 inliers leaves
    the pose alone and, with starved_leaves_level, ends its level's iterations.  Returns (T, log)."""
    iu = np.triu_indices(6)
    log = []
    for level, iters in schedule:
        for _ in range(iters):
            r = sums(level, np.ascontiguousarray(T[:3].reshape(12)))
            A = np.zeros((6, 6))
            A[iu] = r[:21]
            A = A + np.triu(A, 1).T
            b, cost, n = r[21:27], float(r[27]), int(round(r[28]))
            log.append((level, A.copy(), b.copy(), cost, n))
            if n >= 6:
                T = se3_exp(np.linalg.solve(A + 1e-12 * np.eye(6), -b)) @ T
            elif starved_leaves_level:
                break
    return T, log


class _Level:
    __slots__ = ("H", "W", "Kc", "I", "D", "gIx", "gIy", "gDx", "gDy")     # maps: [slots, H, W]

    def at(self, slot: int) -> List[int]:
        """the addresses of image `slot` of the six maps (I, D, gIx, gIy, gDx, gDy)"""
        o = 4 * slot * self.H * self.W
        return [m.data_ptr() + o for m in (self.I, self.D, self.gIx, self.gIy, self.gDx, self.gDy)]


class RGBDOdometry:
    def __init__(self, K: Sequence[float], device: int = 0, iterations: Sequence[int] = ITERATIONS, association: str = "nearest",
                 loss: Optional[str] = None):
        """K = (fx, fy, cx, cy) of the full-resolution frames.  association: "nearest" (Open3D's, default) | "bilinear";
        loss: "o3d" | "irls" (default: "o3d" with nearest, "irls" with bilinear)"""
        assert association in ("nearest", "bilinear")
        loss = loss or ("o3d" if association == "nearest" else "irls")
        assert loss in ("o3d", "irls")
        self.K = tuple(float(v) for v in K)
        self.dev = torch.device("cuda", device)
        self.iterations = tuple(int(i) for i in iterations)
        self.association, self.loss = association, loss
        self.flags = (FLAG_NEAREST if association == "nearest" else 0) | (FLAG_O3D_LOSS if loss == "o3d" else 0)
        L.init(device)
        self.last_trace = None
        self._trk = None
        self._blk = None

    # ---- device-side image preparation ---------------------------------------------------------------
    def _alloc_levels(self, H: int, W: int, slots: int = 1):
        """(levels, flat): the six [slots, h, w] maps of every pyramid level as views of ONE flat buffer (with one slot, a frame's
        whole state moves with one copy)"""
        shapes = _level_shapes(H, W, self.K, len(self.iterations))
        flat = torch.empty(sum(6 * slots * h * w for h, w, _ in shapes), device=self.dev, dtype=torch.float32)
        levels, off = [], 0
        for (h, w, kc) in shapes:
            lv = _Level()
            lv.H, lv.W, lv.Kc = h, w, kc
            maps = []
            for _ in range(6):
                maps.append(flat[off:off + slots * h * w].view(slots, h, w))
                off += slots * h * w
            lv.I, lv.D, lv.gIx, lv.gIy, lv.gDx, lv.gDy = maps
            levels.append(lv)
        return levels, flat

    def _build(self, levels: List[_Level], color: torch.Tensor, depth: torch.Tensor, depth_max: float, n: int = 1, slot: int = 0,
               gradients: bool = True):
        """the pyramids (and gradients) of n frames into slots slot .. slot + n - 1: one launch per stage, 1 + 4 + 6 on three levels"""
        lib, st = L.load_library(), L.stream_ptr()
        at = [lv.at(slot) for lv in levels]
        l0 = levels[0]
        L.check(lib.bs_odo_prepare(L.p(color), L.p(depth), n, l0.H, l0.W, float(depth_max), at[0][0], at[0][1], st), "bs_odo_prepare")
        for p, a, b in zip(levels[:-1], at[:-1], at[1:]):
            _pyrdown(a[0], n, p.H, p.W, b[0], None, st)
            _pyrdown(a[1], n, p.H, p.W, b[1], 2.0 * DEPTH_OUTLIER_TRUNC, st)
        if gradients:
            for lv, (I, D, gIx, gIy, gDx, gDy) in zip(levels, at):
                for img, gx, gy in ((I, gIx, gIy), (D, gDx, gDy)):
                    L.check(lib.bs_odo_sobel(img, n, lv.H, lv.W, gx, gy, st), "bs_odo_sobel")

    def _pyramid(self, color_u8, depth_m, depth_max: float, gradients: bool):
        color, depth = self._dev(color_u8, torch.uint8), self._dev(depth_m, torch.float32)      # numpy, host or device tensors
        levels, _ = self._alloc_levels(*depth.shape)
        self._build(levels, color, depth, depth_max, gradients=gradients)
        return levels

    def _steps(self, src: List[_Level], s: int, tgt: List[_Level], t: int, pairs: int, T: torch.Tensor, partial: torch.Tensor, out: torch.Tensor):
        """the coarse-to-fine loop on the device, sum(iterations) x (sums kernel, fixed-order reduction + 6x6 solve + pose update):
        pair p = image s + p of the source levels against image t + p of the target levels, at pose T[p]"""
        lib, st = L.load_library(), L.stream_ptr()
        for level, iters in _schedule(self.iterations):
            lv = src[level]
            L.check(lib.bs_odo_step(*lv.at(s)[:2], *tgt[level].at(t), pairs, lv.H, lv.W, lv.Kc.ctypes.data_as(C.c_void_p), L.p(T), iters,
                                    DEPTH_OUTLIER_TRUNC, DEPTH_HUBER, INTENSITY_HUBER, L.p(partial), L.p(out), self.flags, st), "bs_odo_step")

    # ---- the estimate ----------------------------------------------------------------------------------
    def estimate(self, src_color, src_depth, tgt_color, tgt_depth, depth_max: float, init: Optional[np.ndarray] = None, trace: bool = False):
        """T (4x4 float64): source points -> target frame"""
        ps = self._pyramid(src_color, src_depth, depth_max, gradients=False)
        pt = self._pyramid(tgt_color, tgt_depth, depth_max, gradients=True)
        T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
        k = _scratch(1, ps[0].H, ps[0].W, self.dev)
        if not trace:
            # no host round trip until the pose is read back; trace=True below walks the same steps from the host (tests, diagnostics)
            k["T"].copy_(k["T0"] if init is None else torch.from_numpy(np.ascontiguousarray(T[:3].reshape(1, 12))))
            self._steps(ps, 0, pt, 0, 1, k["T"], k["partial"], k["out"])
            T[:3] = k["T"].cpu().numpy().reshape(3, 4)
            self.last_trace = None
            return T
        lib, st = L.load_library(), L.stream_ptr()

        def sums(level, T12):
            s = ps[level]
            L.check(lib.bs_odo_accumulate(*s.at(0)[:2], *pt[level].at(0), s.H, s.W, s.Kc.ctypes.data_as(C.c_void_p), T12.ctypes.data_as(C.c_void_p),
                                          DEPTH_OUTLIER_TRUNC, DEPTH_HUBER, INTENSITY_HUBER, L.p(k["partial"]), L.p(k["out"]), self.flags, st),
                    "bs_odo_accumulate")
            return k["out"][0].cpu().numpy()                    # (synchronises: T12 / Kc outlive the launch)

        T, self.last_trace = _host_walk(T, _schedule(self.iterations), sums, starved_leaves_level=True)
        return T

    def __call__(self, curr_rgbd, prev_rgbd) -> np.ndarray:
        """what VO._compute_vo_o3d returns (visual_odometry.py:97-120): source = the current frame, target = the previous one,
        depth_max = the larger of the two frames' maxima, the estimated transform inverted"""
        dmax = max(self._depth_max(curr_rgbd), self._depth_max(prev_rgbd))
        T = self.estimate(curr_rgbd.color, curr_rgbd.depth, prev_rgbd.color, prev_rgbd.depth, dmax)
        return np.linalg.inv(T)

    # ---- a stream of consecutive frames --------------------------------------------------------------
    def reset(self):
        """forget the previous frame of track()"""
        for k in (self._trk, self._blk):
            if k is not None:
                k["have_prev"] = False

    def track(self, color_u8: torch.Tensor, depth_m: torch.Tensor, graph: bool = True) -> Optional[torch.Tensor]:
        """The next frame of a sequence (device tensors: color uint8 [H, W, 3], depth fp32 metres [H, W]).  Returns None for the first
        frame, then a fresh device tensor: the 12 doubles (rows 0..2) of T(current -> previous), as ``estimate(current, previous)``
        gives them -- nothing is read back to the host here.  depth_max of the pair is max(depth of either frame)
        (visual_odometry.py:99), which invalidates nothing, so the frames are prepared once and the previous frame's pyramid is
        reused as the target."""
        assert color_u8.is_cuda and depth_m.is_cuda and color_u8.dtype == torch.uint8 and depth_m.dtype == torch.float32
        H, W = depth_m.shape
        k = self._trk
        if k is None or k["hw"] != (H, W):
            prev, prev_flat = self._alloc_levels(H, W)
            cur, cur_flat = self._alloc_levels(H, W)
            k = self._trk = dict(hw=(H, W), prev=prev, cur=cur, prev_flat=prev_flat, cur_flat=cur_flat, have_prev=False, graph=None, warm=False,
                                 color=torch.empty(H, W, 3, dtype=torch.uint8, device=self.dev), depth=torch.empty(H, W, device=self.dev),
                                 **_scratch(1, H, W, self.dev))
        k["color"].copy_(color_u8)
        k["depth"].copy_(depth_m)
        if not k["have_prev"]:
            self._build(k["prev"], k["color"], k["depth"], 3.0e38)
            k["have_prev"] = True
            return None

        def pair():
            k["T"].copy_(k["T0"])
            self._build(k["cur"], k["color"], k["depth"], 3.0e38)
            self._steps(k["cur"], 0, k["prev"], 0, 1, k["T"], k["partial"], k["out"])
            k["prev_flat"].copy_(k["cur_flat"])                 # the current frame becomes the next pair's target

        if not graph:
            pair()
        elif k["graph"] is None and not k["warm"]:
            pair()                                              # first pair eagerly (lazy one-off initialisations), the second is captured
            k["warm"] = True
        elif k["graph"] is None:
            torch.cuda.synchronize(self.dev)
            g = torch.cuda.CUDAGraph()
            cap = torch.cuda.Stream(device=self.dev)
            cap.wait_stream(torch.cuda.current_stream(self.dev))
            with torch.cuda.stream(cap):
                with torch.cuda.graph(g, stream=cap, capture_error_mode="thread_local"):
                    pair()
            torch.cuda.current_stream(self.dev).wait_stream(cap)
            k["graph"] = g
            g.replay()
        else:
            k["graph"].replay()
        return k["T"][0].clone()

    # ---- a block of consecutive frames at once ---------------------------------------------------------
    def track_block(self, colors_u8: torch.Tensor, depths_m: torch.Tensor, max_block: int = 64) -> torch.Tensor:
        """The next n frames of a sequence (device tensors: colors uint8 [n, H, W, 3], depths fp32 metres [n, H, W]).  Returns a device
        tensor [pairs, 12] (float64): rows 0..2 of T(frame -> the frame before it) for every frame that has a predecessor -- n - 1 pairs
        for the first block after ``reset()`` / construction, n afterwards (the last frame of a block is kept as the next block's
        first target).  Nothing is read back to the host.  Pair for pair bit-equal to ``estimate(current, previous)``."""
        assert colors_u8.is_cuda and depths_m.is_cuda and colors_u8.dtype == torch.uint8 and depths_m.dtype == torch.float32
        n, H, W = depths_m.shape
        if n > max_block:                        # bounded scratch: long inputs go through in pieces
            return torch.cat([self.track_block(colors_u8[a:a + max_block], depths_m[a:a + max_block], max_block) for a in range(0, n, max_block)])
        k = self._blk
        if k is None or k["hw"] != (H, W) or k["slots"] < n + 1:
            old = k if (k is not None and k["hw"] == (H, W) and k["have_prev"]) else None      # a larger block than before: keep the previous frame
            slots = max(n, max_block if n > 1 else 1) + 1
            levels, _ = self._alloc_levels(H, W, slots)
            k = self._blk = dict(hw=(H, W), slots=slots, levels=levels, have_prev=False, **_scratch(slots - 1, H, W, self.dev))
            if old is not None:      # (a first call with one frame allocates two slots; the next, larger block must still pair with that frame)
                for l_new, l_old in zip(levels, old["levels"]):
                    for name in ("I", "D", "gIx", "gIy", "gDx", "gDy"):
                        getattr(l_new, name)[0].copy_(getattr(l_old, name)[0])
                k["have_prev"] = True
        if n == 0:
            return torch.empty(0, 12, dtype=torch.float64, device=self.dev)
        lv = k["levels"]
        # slot 0 holds the previous block's last frame; the n new frames go to slots 1..n.  Every new frame gets its gradients: it is a
        # target, in this block or (the last one) in the next
        self._build(lv, colors_u8.contiguous(), depths_m.contiguous(), 3.0e38, n, 1)
        first = 0 if k["have_prev"] else 1       # the first pair's target slot
        pairs = n - first
        T = k["T"][:max(pairs, 0)]
        if pairs > 0:
            T.copy_(k["T0"].expand(pairs, 12))
            self._steps(lv, first + 1, lv, first, pairs, T, k["partial"], k["out"])
        for l_ in lv:                           # the block's last frame is the next block's first target
            for m in (l_.I, l_.D, l_.gIx, l_.gIy, l_.gDx, l_.gDy):
                m[0].copy_(m[n])
        k["have_prev"] = True
        return T.clone()

    def _dev(self, x, dtype) -> torch.Tensor:
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
        return t.to(device=self.dev, dtype=dtype).contiguous()

    @staticmethod
    def _depth_max(rgbd) -> float:
        m = getattr(rgbd, "depth_max", None)
        if m is not None:
            return float(m)
        d = rgbd.depth
        return float(d.max()) if isinstance(d, torch.Tensor) else float(np.nanmax(np.asarray(d)))


P2P_ITERATIONS, P2P_DEPTH_DIFF = (6, 3, 1), 0.07      # o3d.t.pipelines.slam.Model.track_frame_to_model defaults, restated (parity unpinned)


class PointToPlaneOdometry:
    """Frame-to-model tracking: where a depth frame sits relative to a model depth image, by point-to-plane Gauss-Newton on a
    3-level pyramid -- the role of Open3D's ``Model.track_frame_to_model(input_frame, raycast_frame, depth_scale=1000,
    depth_max=3.0, depth_diff=0.07)`` (point-to-plane, criteria 6 / 3 / 1) behind the reference's MAP (3DM/tsdf.py:56-107).
    Open3D is not available: those defaults restate its published interface, the algorithm is the statement in
    tests/_point_to_plane_ref.py (and include/bodyslam_hip.h, bs_odo_p2p_*), and parity with Open3D itself is unpinned.

    The source is the input frame's depth (metres; <= 0 or > depth_max invalid), the target the model's ray-cast depth (0 = no
    surface).  Both get the hybrid odometry's depth pyramid; every target level becomes one (normal, depth) record per pixel, and
    the 10 steps run on the device through the hybrid path's reduction, solve and pose update."""

    def __init__(self, K: Sequence[float], device: int = 0, iterations: Sequence[int] = P2P_ITERATIONS, depth_diff: float = P2P_DEPTH_DIFF,
                 depth_huber: float = DEPTH_HUBER):
        self.K = tuple(float(v) for v in K)
        self.dev = torch.device("cuda", device)
        self.iterations = tuple(int(i) for i in iterations)
        self.depth_diff, self.depth_huber = float(depth_diff), float(depth_huber)
        L.init(device)
        self.last_trace = None
        self.last_sums = None        # [n, 29] float64 on the device: the sums of the last step of the last call (27 = cost, 28 = inliers)
        self._buf = None

    def _buffers(self, n: int, H: int, W: int) -> dict:
        """per (H, W): the depth levels of both sides as one [2, n, h, w] stack each (0 = source, 1 = target: a pyramid stage is one
        launch over both), the target records, poses and reduction scratch; grown when a larger batch arrives"""
        k = self._buf
        if k is not None and k["hw"] == (H, W) and k["n"] >= n:
            return k
        levels = [dict(H=h, W=w, Kc=kc, D=torch.empty(2, n, h, w, device=self.dev, dtype=torch.float32),
                       rec=torch.empty(n, h, w, 4, device=self.dev, dtype=torch.float32))
                  for h, w, kc in _level_shapes(H, W, self.K, len(self.iterations))]
        k = self._buf = dict(hw=(H, W), n=n, levels=levels, **_scratch(n, H, W, self.dev))
        return k

    def _build(self, k: dict, src: torch.Tensor, tgt: torch.Tensor, depth_max: float) -> None:
        """pyramids of both sides and the target records of every level: 2 + (levels - 1) + levels launches"""
        lib, st = L.load_library(), L.stream_ptr()
        n, m = src.shape[0], k["n"]
        lv = k["levels"]
        l0 = lv[0]
        for side, (depth, dmax) in enumerate(((src, float(depth_max)), (tgt, 3.0e38))):
            L.check(lib.bs_odo_p2p_prepare(L.p(depth), n, l0["H"], l0["W"], dmax, L.p(l0["D"][side]), st), "bs_odo_p2p_prepare")
        for p_, n_ in zip(lv[:-1], lv[1:]):
            if n == m:           # the stack is full: source and target images are contiguous, one launch
                _pyrdown(L.p(p_["D"]), 2 * n, p_["H"], p_["W"], L.p(n_["D"]), 2.0 * self.depth_diff, st)
            else:
                for side in (0, 1):
                    _pyrdown(L.p(p_["D"][side]), n, p_["H"], p_["W"], L.p(n_["D"][side]), 2.0 * self.depth_diff, st)
        for l_ in lv:
            L.check(lib.bs_odo_p2p_target(L.p(l_["D"][1]), n, l_["H"], l_["W"], l_["Kc"].ctypes.data_as(C.c_void_p), L.p(l_["rec"]), st), "bs_odo_p2p_target")

    @staticmethod
    def _init12(init, n: int) -> Optional[np.ndarray]:
        if init is None:
            return None
        a = init.detach().cpu().numpy() if isinstance(init, torch.Tensor) else np.asarray(init)
        a = np.asarray(a, dtype=np.float64)
        a = np.broadcast_to(a, (n, 4, 4)) if a.ndim == 2 else a
        assert a.shape == (n, 4, 4), "init: one 4x4 or [n, 4, 4]"
        return np.array(a[:, :3], dtype=np.float64).reshape(n, 12)       # (a fresh, writable copy: torch.from_numpy takes it)

    def estimate_batch(self, src_depths: torch.Tensor, tgt_depths: torch.Tensor, init=None, depth_max: float = 3.0) -> torch.Tensor:
        """n independent pairs at once (device tensors fp32 [n, H, W], metres): every stage is one launch over the batch.  Returns a
        fresh device tensor [n, 12] (float64): rows 0..2 of T(source -> target) per pair; nothing is read back (``last_sums`` keeps
        the last step's sums on the device).  Pair for pair bit-equal to ``estimate``.  init: None (identity), one 4x4 or [n, 4, 4]."""
        assert src_depths.is_cuda and tgt_depths.is_cuda and src_depths.dtype == torch.float32 and tgt_depths.dtype == torch.float32
        assert src_depths.dim() == 3 and src_depths.shape == tgt_depths.shape
        n, H, W = src_depths.shape
        if n == 0:
            return torch.empty(0, 12, dtype=torch.float64, device=self.dev)
        k = self._buffers(n, H, W)
        self._build(k, src_depths.contiguous(), tgt_depths.contiguous(), depth_max)
        T = k["T"][:n]
        i12 = self._init12(init, n)
        T.copy_(k["T0"].expand(n, 12) if i12 is None else torch.from_numpy(i12).to(self.dev))
        lib, st = L.load_library(), L.stream_ptr()
        for level, iters in _schedule(self.iterations):
            l_ = k["levels"][level]
            L.check(lib.bs_odo_p2p_step(L.p(l_["D"][0]), L.p(l_["rec"]), n, l_["H"], l_["W"], l_["Kc"].ctypes.data_as(C.c_void_p), L.p(T), iters,
                                        self.depth_diff, self.depth_huber, L.p(k["partial"]), L.p(k["out"]), st), "bs_odo_p2p_step")
        self.last_sums = k["out"][:n].clone()
        self.last_trace = None
        return T.clone()

    def estimate(self, src_depth, tgt_depth, depth_max: float = 3.0, init: Optional[np.ndarray] = None, trace: bool = False) -> np.ndarray:
        """T (4x4 float64): source points -> target frame.  Depths: numpy, host or device tensors, metres.  trace=True walks the same
        steps from the host through bs_odo_p2p_accumulate and keeps (level, A, b, cost, inliers) per step in ``last_trace``."""
        src, tgt = self._dev(src_depth)[None], self._dev(tgt_depth)[None]
        T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
        if not trace:
            T[:3] = self.estimate_batch(src, tgt, init=init, depth_max=depth_max).cpu().numpy().reshape(3, 4)
            return T
        lib, st = L.load_library(), L.stream_ptr()
        k = self._buffers(1, *src.shape[1:])
        self._build(k, src, tgt, depth_max)

        def sums(level, T12):
            l_ = k["levels"][level]
            L.check(lib.bs_odo_p2p_accumulate(L.p(l_["D"][0]), L.p(l_["rec"]), l_["H"], l_["W"], l_["Kc"].ctypes.data_as(C.c_void_p),
                                              T12.ctypes.data_as(C.c_void_p), self.depth_diff, self.depth_huber, L.p(k["partial"]), L.p(k["out"]),
                                              st), "bs_odo_p2p_accumulate")
            return k["out"][0].cpu().numpy()

        # (fewer than 6 inliers: the pose stays, the schedule goes on -- as the device loop does)
        T, self.last_trace = _host_walk(T, _schedule(self.iterations), sums, starved_leaves_level=False)
        self.last_sums = k["out"][:1].clone()
        return T

    def _dev(self, x) -> torch.Tensor:
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
        return t.to(device=self.dev, dtype=torch.float32).contiguous()
