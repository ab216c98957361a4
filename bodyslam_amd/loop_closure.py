"""Loop closure on the device: one frame's ORB features against every stored keyframe, and a RANSAC rigid registration of the matched 3-D
points that yields a pose-graph edge ``(source, target, T, information)`` -- or nothing, when there is no closure.

The reference declares this step and never wrote it: ``3DM/slam.py`` has ``perform_loop_closure`` (:30), ``num_closure`` (:41),
``global_key_frame_indices`` (:42) and calls an undefined ``self._loop_closure()`` every ``num_closure`` frames (:79-80).  So nothing here
is the reference's code.  The features are the sparse-feature path's (``scaling_system.SparseScale``: ORB restated from its publications,
parity with OpenCV unpinned).  The registration is RANSAC (Fischler & Bolles 1981) over three-point Kabsch fits (Kabsch 1976; Arun, Huang
& Blostein 1987), and the information matrix has the form of Open3D's ``get_information_matrix_from_point_clouds``, restated from its
documentation: ``sum G^T G`` with ``G = [-[q]x | I3]`` over the inlier points of the target frame, rotation parameters first.  Parity with
Open3D is UNPINNED.  The numpy statement is tests/_loop_closure_ref.py; the kernels are csrc/loop_closure.hip.

Descriptor counts do not tell a revisit from a different place with similar corners; the geometric check does (see ``MIN_INLIERS``).
Time not measured yet: tools/loop_closure_time.py."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .scaling_system import MAX_FEATURES, MAX_LEVELS, SparseScale, _ptr

FIELDS = 64                     # BS_LOOP_FIELDS
TAU = 0.005                     # PoseGraph's max_correspondence_distance
# The numpy statement on rendered 200 x 152 frames of the height field (tests/test_loop_closure_cpu.py::MEASURED, CPU, 2026-10-17): a revisit
# of the keyframe's place keeps 190 of 192 correspondences as inliers at 5 mm (164 of 167 from a pose about twice as far), views of a
# different place with the same corner geometry keep 0 to 5 of 54 to 83.  The default lies six times above the one and below a fifth of
# the other.
MIN_INLIERS = 30
CHUNK = 64                      # keyframes the store grows by


def _records(rec: np.ndarray) -> dict:
    """the per-pair table of bs_loop_register as named columns"""
    return dict(T=rec[:, :16].reshape(-1, 4, 4).copy(), inliers=rec[:, 16].astype(np.int64), correspondences=rec[:, 17].astype(np.int64),
                h=rec[:, 18].astype(np.int64), rmse=rec[:, 19].copy(), status=rec[:, 20].astype(np.int64), matches=rec[:, 21].astype(np.int64),
                information=rec[:, 22:58].reshape(-1, 6, 6).copy())


def _register(xyz: torch.Tensor, pairs: torch.Tensor, matches: torch.Tensor, match_counts: torch.Tensor, max_hamming: int, tau: float, n_hyp: int,
              n_refit: int, min_matches: int, seed: int) -> Tuple[torch.Tensor, torch.Tensor]:
    P = pairs.shape[0]
    rec = torch.zeros(P, FIELDS, dtype=torch.float64, device=xyz.device)
    mask = torch.zeros(P, MAX_FEATURES, dtype=torch.int32, device=xyz.device)
    L.check(L.load_library().bs_loop_register(L.p(xyz), xyz.shape[0], L.p(pairs), P, L.p(matches), L.p(match_counts), int(max_hamming), float(tau),
                                              int(n_hyp), int(n_refit), int(min_matches), int(seed) & 0xFFFFFFFFFFFFFFFF, L.p(rec), L.p(mask),
                                              L.stream_ptr()), "bs_loop_register")
    return rec, mask


def register_points(src_xyz, dst_xyz, tau: float, n_hyp: int = 256, n_refit: int = 2, seed: int = 0, device: int = 0):
    """RANSAC rigid registration of given correspondences ``src_xyz[i] -> dst_xyz[i]`` ([C, 3], C <= 500, numpy or tensors), one launch:
    ``(T fp64 [4, 4] with dst ~ T src, mask bool [C], information fp64 [6, 6], rmse, h)`` as device tensors -- ``h`` the winning hypothesis,
    -1 where the registration is rejected (fewer than three points, or collinear / coincident ones): then T is the identity, the mask
    and the information matrix are zero.  The same input gives the same bits in every call."""
    L.init(device)
    dev = torch.device("cuda", device)
    src = torch.as_tensor(src_xyz, dtype=torch.float64).reshape(-1, 3).to(dev)
    dst = torch.as_tensor(dst_xyz, dtype=torch.float64).reshape(-1, 3).to(dev)
    n = src.shape[0]
    if dst.shape[0] != n or n > MAX_FEATURES:
        raise ValueError(f"{n} source and {dst.shape[0]} target points: equal counts of at most {MAX_FEATURES}")
    xyz = torch.zeros(2, MAX_FEATURES, 4, dtype=torch.float64, device=dev)
    xyz[0, :n, :3], xyz[1, :n, :3] = src, dst
    xyz[:, :n, 3] = 1.0
    matches = torch.zeros(1, MAX_FEATURES, 4, dtype=torch.int32, device=dev)
    matches[0, :, 0] = matches[0, :, 1] = torch.arange(MAX_FEATURES, dtype=torch.int32, device=dev)
    pairs = torch.tensor([[0, 1]], dtype=torch.int32, device=dev)
    rec, mask = _register(xyz, pairs, matches, torch.tensor([n], dtype=torch.int32, device=dev), 0, tau, n_hyp, n_refit, 0, seed)
    return rec[0, :16].reshape(4, 4).clone(), mask[0, :n] != 0, rec[0, 22:58].reshape(6, 6).clone(), rec[0, 19].clone(), rec[0, 18].to(torch.int64)


class LoopCloser:
    """Keyframes on the device and the search of a closure against them.

    ``add_keyframe(index, color, depth)`` stores a frame's ORB descriptors and the 3-D points of its keypoints (colour uint8 [H, W, 3]
    RGB, depth [H, W] in metres; numpy or tensors).  ``detect(index, color, depth)`` returns the closures of a frame as
    ``[(source = index, target = keyframe index, T fp64 [4, 4], information fp64 [6, 6])]``: exactly what ``pipe.loop_closures`` and
    ``PoseGraph.add_edge(T, source, target, True, information)`` take.  **Convention:** ``T = pose_target^-1 . pose_source`` for
    camera -> world poses, i.e. ``X_target = T . X_source`` -- what oracle/posegraph_ref.py:79 measures an edge against, and what the
    odometry edge ``add_edge(T_rel, i, i - 1)`` uses.

    ``detect`` extracts the frame's features once, runs ONE ``bs_orb_match_pairs`` over all keyframes at least ``min_gap`` frames older and
    ONE ``bs_loop_register`` over the same pairs (a pair with fewer than ``min_matches`` usable matches returns at once), and makes ONE
    readback of the per-pair records.  On the host it keeps the pairs with at least ``min_inliers`` inliers and returns the best
    ``top_k`` by inlier count, ties to the older keyframe.  ``last_records``: the whole per-pair table of the last call (``_records``'
    columns + ``keyframe`` indices + ``mask``, the device tensor of inlier flags by match row).

    ``tau`` (inlier distance, metres) defaults to ``PoseGraph``'s ``max_correspondence_distance``; ``information[5, 5]`` is the inlier
    count, which ``PoseGraph``'s line-process weight reads."""

    def __init__(self, K: Sequence[float], device: int = 0, min_gap: int = 30, max_hamming: int = 64, min_matches: int = 30, tau: float = TAU,
                 min_inliers: int = MIN_INLIERS, n_hyp: int = 256, top_k: int = 1, seed: int = 0, n_refit: int = 2):
        self.features = SparseScale(K, device=device, association="matched")
        self.dev = self.features.dev
        self.min_gap, self.max_hamming, self.min_matches, self.tau = int(min_gap), int(max_hamming), int(min_matches), float(tau)
        self.min_inliers, self.n_hyp, self.top_k, self.seed, self.n_refit = int(min_inliers), int(n_hyp), int(top_k), int(seed), int(n_refit)
        self.n = 0
        self.indices: List[int] = []
        self._grow(CHUNK)
        self.last_records = None
        self._query_index = None

    # ---- the store ---------------------------------------------------------------------------------------------------------------------
    def _grow(self, cap: int) -> None:
        """slot `cap` of the store is the frame a detect call is looking at"""
        z = lambda *s, dt: torch.zeros(*s, dtype=dt, device=self.dev)
        desc, counts, xyz = z(cap + 1, MAX_FEATURES, 8, dt=torch.int32), z(cap + 1, MAX_LEVELS + 1, dt=torch.int32), z(cap + 1, MAX_FEATURES, 4, dt=torch.float64)
        if self.n:
            desc[:self.n], counts[:self.n], xyz[:self.n] = self.desc[:self.n], self.counts[:self.n], self.xyz[:self.n]
        self.cap, self.desc, self.counts, self.xyz = cap, desc, counts, xyz

    def _extract_into(self, slot: int, color, depth) -> None:
        f = self.features
        s = f.features(f._dev(color, torch.uint8)[None])
        d = f._dev(depth, torch.float32)
        if tuple(d.shape) != (s["H"], s["W"]):
            raise ValueError(f"depth of shape {tuple(d.shape)} for a colour frame [{s['H']}, {s['W']}, 3]")
        self.desc[slot].copy_(s["desc"][0])
        self.counts[slot].copy_(s["counts"][0])
        L.check(L.load_library().bs_orb_lift(L.p(s["pt"]), L.p(s["counts"]), L.p(d), 1, s["H"], s["W"], _ptr(f.K), L.p(self.xyz[slot]), L.stream_ptr()),
                "bs_orb_lift")

    def add_keyframe(self, index: int, color=None, depth=None) -> None:
        """color None: the frame the last ``detect`` call looked at, which must have had this index (its features are kept, not
        extracted again)"""
        reuse = None
        if color is None:
            if self._query_index != int(index):
                raise ValueError(f"add_keyframe({index}) without a frame: the last detect call extracted frame {self._query_index}")
            reuse = (self.desc[self.cap].clone(), self.counts[self.cap].clone(), self.xyz[self.cap].clone())
        if self.n == self.cap:
            self._grow(self.cap + CHUNK)
        if reuse is None:
            self._extract_into(self.n, color, depth)
        else:
            self.desc[self.n], self.counts[self.n], self.xyz[self.n] = reuse
        self.indices.append(int(index))
        self.n += 1

    # ---- the search --------------------------------------------------------------------------------------------------------------------
    def detect(self, index: int, color, depth) -> list:
        slots = [k for k in range(self.n) if index - self.indices[k] >= self.min_gap]
        if not slots:
            self.last_records, self._query_index = None, None
            return []
        q = self.cap                                                      # the query frame's slot, behind the keyframes
        self._extract_into(q, color, depth)
        self._query_index = int(index)
        P = len(slots)
        pairs = torch.tensor([[q, k] for k in slots], dtype=torch.int32, device=self.dev)
        matches = torch.zeros(P, MAX_FEATURES, 4, dtype=torch.int32, device=self.dev)
        mcount = torch.zeros(P, dtype=torch.int32, device=self.dev)
        L.check(L.load_library().bs_orb_match_pairs(L.p(self.desc), L.p(self.counts), self.cap + 1, L.p(pairs), P, L.p(matches), L.p(mcount),
                                                    L.stream_ptr()), "bs_orb_match_pairs")
        rec, mask = _register(self.xyz, pairs, matches, mcount, self.max_hamming, self.tau, self.n_hyp, self.n_refit, self.min_matches, self.seed)
        r = _records(rec.cpu().numpy())                                   # the one readback
        r["keyframe"] = np.array([self.indices[k] for k in slots], dtype=np.int64)
        r["mask"], r["matches_dev"], r["match_counts_dev"] = mask, matches, mcount
        self.last_records = r
        keep = [p for p in range(P) if r["status"][p] == 1 and r["inliers"][p] >= self.min_inliers]
        keep.sort(key=lambda p: (-int(r["inliers"][p]), int(r["keyframe"][p])))
        return [(int(index), int(r["keyframe"][p]), r["T"][p].copy(), r["information"][p].copy()) for p in keep[:self.top_k]]
