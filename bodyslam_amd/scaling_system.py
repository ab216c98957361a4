"""Sparse-feature scale path of the VO step: drop-in for BodySLAM_not_refactored/3DM/scaling_system.py, what
``VO.estimate_relative_pose_between(..., rgbd_odo=False)`` feeds its filter with (3DM/visual_odometry.py:70-79): ORB keypoints on both
frames, a brute-force Hamming match with cross-check, depth looked up at the keypoints, the mean 3-D displacement of the matched points.

The reference gets ORB and the matcher from OpenCV, which is not vendored and not installable offline.  ORB (Rublee et al. 2011), FAST-9/16
(Rosten & Drummond 2006), the Harris measure and BRIEF's Gaussian test pairs (Calonder et al. 2010) are restated from their publications
with ``cv2.ORB_create()``'s default parameters; the statement is tests/_orb_ref.py and the kernels (csrc/sparse_features.hip) reproduce it
bit for bit.  Parity with OpenCV itself is UNPINNED, and in four places this is knowingly not OpenCV:

  * the 256 test pairs are BRIEF's isotropic Gaussian pairs from a fixed seed (``orb_tables.brief_pattern``), not OpenCV's learnt table,
    which is OpenCV's own: descriptors do not equal OpenCV's;
  * the pyramid's bilinear resize uses 11-bit fixed-point weights of its own, and the 7 x 7 smoothing is binomial;
  * the orientation is quantised to 30 bins of 12 degrees, as the ORB paper does, not OpenCV's continuous angle;
  * ties have a stated rule everywhere: (response descending, row-major pixel index ascending) in the selection, the lowest index among
    equal Hamming distances in the match.

What follows the match is the reference's own Python and is restated with its quirks (pinned by tests/golden/sparse_scale.npz):
``associate_depth`` reads depth at ``(int(y), int(x))``; ``compute_scaling_factor``'s second call passes the keypoint lists swapped but
the same matches, so ``queryIdx`` indexes the CURRENT frame's keypoints for that lookup; the two filtered lists are zipped after independent
filtering and misalign once either drops an entry.  ``association="reference"`` is that; ``association="matched"`` looks the current
frame's depth up at the matched keypoint itself and keeps the pairs aligned -- the evident intention, offered as an option.

ONE behavioural departure from the reference: with no usable pair its ``np.mean`` of an empty list is NaN (with a warning) and the NaN
then poisons the filter for the rest of the sequence.  Here ``compute_scaling_factor`` and ``SparseScale`` return three NaNs, and ``VO``
raises a ``RuntimeError`` naming the frame and leaves the filter untouched.

SIFT (``feature_type="sift"``) is not built and raises ``NotImplementedError``.  Depth maps are read as fp32.
Time not measured yet: tools/sparse_scale_time.py."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import numpy as np
import torch

from . import _lib as L
from . import orb_tables as T
from .geom3d import pixel_to_3d  # noqa: F401  (the reference module's name, re-exported)

MAX_FEATURES, MAX_LEVELS, OUT_FIELDS = 500, 8, 9
ASSOCIATIONS = {"reference": 0, "matched": 1}
COUNT_NAMES = ("keypoints_prev", "keypoints_curr", "matches", "associations_prev", "associations_curr", "pairs")


class KeyPoint:
    """the attributes of cv2.KeyPoint that the reference and ORB fill: pt (x, y) at full resolution, size, angle (the centre of the
    12-degree bin), response (Harris), octave"""
    __slots__ = ("pt", "size", "angle", "response", "octave", "class_id")

    def __init__(self, x: float, y: float, size: float = float(T.PATCH_SIZE), angle: float = -1.0, response: float = 0.0, octave: int = 0):
        self.pt, self.size, self.angle, self.response, self.octave, self.class_id = (float(x), float(y)), size, angle, response, octave, -1


class DMatch:
    """cv2.DMatch's attributes"""
    __slots__ = ("queryIdx", "trainIdx", "distance", "imgIdx")

    def __init__(self, queryIdx: int, trainIdx: int, distance: float):
        self.queryIdx, self.trainIdx, self.distance, self.imgIdx = int(queryIdx), int(trainIdx), float(distance), 0


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


class SparseScale:
    """The mean 3-D displacement of ORB matches between two RGB-D frames, on the device (see the module header for what is restated from
    publications, where it knowingly differs from OpenCV -- test pairs, fixed-point resize, quantised orientation, tie rules -- and for the
    NaN departure from the reference).

    ``SparseScale(K)(curr_rgbd, prev_rgbd) -> (3,) float64``: one pair, what ``compute_scaling_factor`` returns (NaN without a usable
    pair).  ``displacements_block(colors[n], depths[n]) -> [n - 1, 3]``: n consecutive frames; every frame's features are extracted once
    (a frame is the current frame of one pair and the previous frame of the next), every stage is one launch over the block, and the
    only readback is the result.  Pair for pair the block form is bit-equal to the pair form.  ``last_counts``: int [pairs, 6] =
    COUNT_NAMES.  ``last_stages``: the stage outputs of the last call as device tensors (tests read them)."""

    def __init__(self, K: Sequence[float], device: int = 0, association: str = "reference"):
        if association not in ASSOCIATIONS:
            raise ValueError(f"association {association!r}: one of {sorted(ASSOCIATIONS)}")
        if len(tuple(K)) != 4:
            raise ValueError("K = (fx, fy, cx, cy)")
        self.K = np.array([float(v) for v in K], dtype=np.float64)
        self.association = association
        L.init(device)
        self.dev = torch.device("cuda", device)
        self._nfeat = T.features_per_level()
        self._scales = T.level_scales()
        self._cos_sin = torch.tensor(list(T.COS) + list(T.SIN), dtype=torch.float64, device=self.dev)
        self._pattern = torch.from_numpy(T.rotated_pattern()).to(self.dev).contiguous()
        self.last_counts = None
        self.last_stages = None

    def _dev(self, x, dtype) -> torch.Tensor:
        if isinstance(x, (list, tuple)):
            x = torch.stack([self._dev(v, dtype) for v in x])
        if not isinstance(x, torch.Tensor):          # (numpy converts first: torch has no arithmetic for uint16 depth payloads)
            x = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.uint8 if dtype == torch.uint8 else np.float32))
        return x.to(device=self.dev, dtype=dtype).contiguous()

    # ---- the stages ------------------------------------------------------------------------------------------------------------------
    def features(self, colors, bgr: bool = False) -> dict:
        """ORB of n frames (uint8 [n, H, W, 3]): the stage outputs as device tensors, nothing read back"""
        color = self._dev(colors, torch.uint8)
        if color.dim() != 4 or color.shape[-1] != 3:
            raise ValueError(f"colour of shape {tuple(color.shape)}: [n, H, W, 3] expected")
        n, H, W = color.shape[:3]
        levels, stride = T.level_layout(H, W)
        lib, st, lp, nl = L.load_library(), L.stream_ptr(), _ptr(levels), len(levels)
        u8 = lambda *s: torch.empty(*s, dtype=torch.uint8, device=self.dev)
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=self.dev)
        s = dict(n=n, H=H, W=W, levels=levels, stride=stride, grey=u8(n, stride), smooth=u8(n, stride), score=u8(n, stride),
                 hist=torch.empty(n, MAX_LEVELS, 256, dtype=torch.int32, device=self.dev), kp=i32(n, MAX_FEATURES, 8), resp=torch.zeros(n, MAX_FEATURES, dtype=torch.float64, device=self.dev),
                 counts=i32(n, MAX_LEVELS + 1), pt=torch.zeros(n, MAX_FEATURES, 2, dtype=torch.float32, device=self.dev),
                 desc=i32(n, MAX_FEATURES, 8))
        L.check(lib.bs_orb_pyramid(L.p(color), n, H, W, int(bgr), lp, nl, stride, L.p(s["grey"]), L.p(s["smooth"]), st), "bs_orb_pyramid")
        L.check(lib.bs_orb_fast(L.p(s["grey"]), n, H, W, lp, nl, stride, L.p(s["score"]), L.p(s["hist"]), st), "bs_orb_fast")
        L.check(lib.bs_orb_select(L.p(s["grey"]), L.p(s["score"]), L.p(s["hist"]), n, H, W, lp, nl, stride, _ptr(self._nfeat), L.p(s["kp"]),
                                  L.p(s["resp"]), L.p(s["counts"]), st), "bs_orb_select")
        L.check(lib.bs_orb_describe(L.p(s["grey"]), L.p(s["smooth"]), n, H, W, lp, nl, stride, _ptr(self._scales), L.p(self._cos_sin),
                                    L.p(self._pattern), L.p(s["kp"]), L.p(s["counts"]), L.p(s["pt"]), L.p(s["desc"]), st), "bs_orb_describe")
        return s

    def match(self, s: dict) -> dict:
        """pair p = (frame p, frame p + 1) of the frames in `s`: adds matches [n - 1, 500, 4] and match_counts [n - 1]"""
        n = s["n"]
        s["matches"] = torch.zeros(n - 1, MAX_FEATURES, 4, dtype=torch.int32, device=self.dev)
        s["match_counts"] = torch.zeros(n - 1, dtype=torch.int32, device=self.dev)
        L.check(L.load_library().bs_orb_match(L.p(s["desc"]), L.p(s["counts"]), n, L.p(s["matches"]), L.p(s["match_counts"]), L.stream_ptr()),
                "bs_orb_match")
        return s

    def _displacement(self, s: dict, depth: torch.Tensor) -> torch.Tensor:
        n, H, W = s["n"], s["H"], s["W"]
        if tuple(depth.shape) != (n, H, W):
            raise ValueError(f"depth of shape {tuple(depth.shape)} for colour frames [{n}, {H}, {W}, 3]")
        out = torch.zeros(n - 1, OUT_FIELDS, dtype=torch.float64, device=self.dev)
        L.check(L.load_library().bs_orb_displacement(L.p(s["pt"]), L.p(s["counts"]), L.p(s["matches"]), L.p(s["match_counts"]), L.p(depth), n, H, W,
                                                     _ptr(self.K), ASSOCIATIONS[self.association], L.p(out), L.stream_ptr()), "bs_orb_displacement")
        s["out"] = out
        return out

    # ---- the public forms ------------------------------------------------------------------------------------------------------------
    def displacements_block(self, colors, depths, bgr: bool = False) -> np.ndarray:
        """colors uint8 [n, H, W, 3] (RGB as RGBDImage.color; bgr=True: BGR), depths [n, H, W] (numpy, host or device tensors, or lists
        of frames), n >= 2 -> float64 [n - 1, 3]: row p = the mean displacement of pair (previous = frame p, current = frame p + 1),
        NaN where the pair has no usable match"""
        depth = self._dev(depths, torch.float32)
        if depth.dim() != 3 or depth.shape[0] < 2:
            raise ValueError(f"depth of shape {tuple(depth.shape)}: a block is [n, H, W] with at least two frames")
        s = self.match(self.features(colors, bgr))
        out = self._displacement(s, depth).cpu().numpy()              # the one readback
        self.last_counts = out[:, 3:].astype(np.int64)
        self.last_stages = s
        return out[:, :3].copy()

    def __call__(self, curr_rgbd, prev_rgbd) -> np.ndarray:
        color = [_frame_attr(prev_rgbd, "color"), _frame_attr(curr_rgbd, "color")]
        depth = [_frame_attr(prev_rgbd, "depth"), _frame_attr(curr_rgbd, "depth")]
        return self.displacements_block(color, depth)[0]


def _frame_attr(rgbd, name: str):
    """.color / .depth of an RGBDImage (colour RGB), or .cv2_color / .cv2_depth where an object has those (visual_odometry.py:76; colour BGR
    as cv2.imread gives it: flipped to RGB here)"""
    v = getattr(rgbd, "cv2_" + name, None)
    if v is None:
        return getattr(rgbd, name)
    if name == "color":
        return torch.flip(v, dims=(-1,)) if isinstance(v, torch.Tensor) else np.ascontiguousarray(np.asarray(v)[..., ::-1])
    return v


# ---- the reference module's names --------------------------------------------------------------------------------------------------------
_engines = {}


def _engine(K=(1.0, 1.0, 0.0, 0.0), association: str = "reference") -> SparseScale:
    key = (tuple(float(v) for v in K), association)
    if key not in _engines:
        _engines[key] = SparseScale(key[0], association=association)
    return _engines[key]


def _as_color(image) -> np.ndarray:
    a = image.cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
    if a.dtype != np.uint8:
        raise ValueError(f"image of dtype {a.dtype}: uint8 expected")
    if a.ndim == 2:
        a = np.repeat(a[..., None], 3, axis=2)        # (a grey image: the luminance of three equal channels is the value itself)
    return a


def extract_features_orb(image):
    """scaling_system.py:5-10: (keypoints, descriptors uint8 [n, 32]) of a BGR (cv2.imread) or grey uint8 image; descriptors is None
    without keypoints, as cv2 returns it"""
    e = _engine()
    s = e.features(_as_color(image)[None], bgr=True)
    n = int(s["counts"][0, MAX_LEVELS])
    kp, resp, pt = s["kp"][0, :n].cpu().numpy(), s["resp"][0, :n].cpu().numpy(), s["pt"][0, :n].cpu().numpy()
    scales = T.level_scales()
    keypoints = [KeyPoint(pt[i, 0], pt[i, 1], float(T.PATCH_SIZE * scales[kp[i, 0]]), 12.0 * kp[i, 6], float(resp[i]), int(kp[i, 0])) for i in range(n)]
    if n == 0:
        return keypoints, None
    return keypoints, s["desc"][0, :n].cpu().numpy().view(np.uint8).reshape(n, 32).copy()


def extract_features_sift(image):
    raise NotImplementedError("SIFT is not built; the sparse-feature path here is ORB (feature_type='orb')")


def match_features_orb(descriptors1, descriptors2) -> List[DMatch]:
    """scaling_system.py:25-32: cross-checked brute-force Hamming matches, sorted by distance"""
    e = _engine()
    sets = [np.zeros((0, 32), np.uint8) if d is None else np.ascontiguousarray(np.asarray(d, dtype=np.uint8)) for d in (descriptors1, descriptors2)]
    if any(d.ndim != 2 or d.shape[1] != 32 or len(d) > MAX_FEATURES for d in sets):
        raise ValueError(f"descriptors: uint8 [n, 32] with n <= {MAX_FEATURES}")
    desc = np.zeros((2, MAX_FEATURES, 32), dtype=np.uint8)
    counts = np.zeros((2, MAX_LEVELS + 1), dtype=np.int32)
    for i, d in enumerate(sets):
        desc[i, :len(d)] = d
        counts[i, MAX_LEVELS] = len(d)
    s = dict(n=2, desc=torch.from_numpy(desc.view(np.int32).reshape(2, MAX_FEATURES, 8)).to(e.dev), counts=torch.from_numpy(counts).to(e.dev))
    e.match(s)
    m = s["matches"][0, :int(s["match_counts"][0])].cpu().numpy()
    return [DMatch(q, t, d) for (q, t, d, _) in m]


def match_features_sift(descriptors1, descriptors2):
    raise NotImplementedError("SIFT is not built; the sparse-feature path here is ORB (feature_type='orb')")


def associate_depth(keypoints1, keypoints2, matches, depth_image):
    """scaling_system.py:46-69, list bookkeeping on the host as in the reference"""
    depth_associations = []
    for match in matches:
        if match.queryIdx >= len(keypoints1) or match.trainIdx >= len(keypoints2):
            continue
        x1, y1 = keypoints1[match.queryIdx].pt
        if not (0 <= int(x1) < depth_image.shape[1] and 0 <= int(y1) < depth_image.shape[0]):
            continue
        depth1 = depth_image[int(y1), int(x1)]
        if depth1 != 0:
            depth_associations.append((match, depth1))
    return depth_associations


def calculate_displacements(keypoints1, keypoints2, depth_associations1, depth_associations2, fx, fy, cx, cy):
    """scaling_system.py:80-100; the back-projections of all pairs are one bs_pixel_to_3d call"""
    rows = []
    for (match1, depth1), (match2, depth2) in zip(depth_associations1, depth_associations2):
        u1, v1 = keypoints1[match1.queryIdx].pt
        u2, v2 = keypoints2[match2.trainIdx].pt
        rows.append((u1, v1, float(depth1)))
        rows.append((u2, v2, float(depth2)))
    if not rows:
        return []
    L.init(0)
    uvd = torch.tensor(rows, dtype=torch.float64, device="cuda:0")
    out = torch.empty(len(rows), 3, dtype=torch.float64, device="cuda:0")
    L.pixel_to_3d(uvd, (fx, fy, cx, cy), out, len(rows))
    pos = out.cpu().numpy()
    return [pos[2 * i + 1] - pos[2 * i] for i in range(len(rows) // 2)]


def compute_scaling_factor(curr_rgb, prev_rgb, curr_dp, prev_dp, intrinsics, feature_type="orb"):
    """scaling_system.py:107-137: the mean displacement (3,) float64 of the ORB matches between two frames; colour is BGR as cv2.imread
    gives it.  Three NaNs where no pair is usable (the reference's np.mean of an empty list, without the warning)."""
    if feature_type == "sift":
        raise NotImplementedError("SIFT is not built; the sparse-feature path here is ORB (feature_type='orb')")
    if feature_type != "orb":
        raise ValueError(f"feature_type {feature_type!r}")         # (the reference runs into a NameError here)
    e = _engine(tuple(intrinsics)[:4])
    return e.displacements_block([_as_color(prev_rgb), _as_color(curr_rgb)], [np.asarray(prev_dp), np.asarray(curr_dp)], bgr=True)[0]
