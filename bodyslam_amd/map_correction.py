"""Which frames a pose-graph update makes the TSDF map take out and put back -- host planning, pure numpy.

After an optimisation moved poses the reference throws the volume away and integrates frames 0..i again (3DM/slam.py:159-175,
slam_utils.py:124-135 update_map_after_pg).  The map's running means are invertible (``TSDF.apply_batch``), so it can be corrected in
place instead: a frame whose pose moved is removed with the pose it went in with and added with its new one.  This module only decides
and orders; the ledger -- the extrinsic every frame is in the map with, ``None`` for a frame that is not in it -- belongs to the caller
(``BodySlamPipeline.run_slam_loop``).  Nothing here comes from Open3D, whose ScalableTSDFVolume has no de-integration, and nothing from
the reference, whose mapping_module.py was an unfinished attempt at selective updates.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

GROUP_FRAMES = 32           # frames per group: at most 32 removals + 32 additions = one 64-record pass (BS_TSDF_BATCH_MAX)


def pose_change(E_old, E_new) -> Tuple[float, float]:
    """(translation in metres, rotation in radians) of ``E_new @ inv(E_old)``"""
    D = np.asarray(E_new, dtype=np.float64) @ np.linalg.inv(np.asarray(E_old, dtype=np.float64))
    R = D[:3, :3]
    # the angle from both the skew part (exact near 0) and the trace (exact near pi)
    s = 0.5 * np.sqrt((R[2, 1] - R[1, 2]) ** 2 + (R[0, 2] - R[2, 0]) ** 2 + (R[1, 0] - R[0, 1]) ** 2)
    c = 0.5 * (np.trace(R) - 1.0)
    return float(np.linalg.norm(D[:3, 3])), float(np.arctan2(s, c))


class MapCorrection(NamedTuple):
    decision: str                                   # "correct" or "rebuild"
    added: List[int]                                # frames that are not in the map yet (ledger None): added only
    moved: List[int]                                # frames taken out with their ledger pose and put back with the new one
    records: List[Tuple[int, np.ndarray, bool]]     # (frame, extrinsic, remove) in the order TSDF.apply_batch takes them
    groups: List[Tuple[int, int]]                   # [start, end) of every group in `records`: one pass each


def plan_map_correction(ledger: Sequence[Optional[np.ndarray]], new_poses: Sequence[np.ndarray], upto: int, tol: Tuple[float, float] = (0.0, 0.0),
                        mode: str = "incremental") -> MapCorrection:
    """What brings a map that holds frame j with ``ledger[j]`` to one that holds frames 0..upto with ``new_poses``, up to ``tol``.

    A frame is moved when its ``pose_change`` exceeds the translation tolerance (metres) or the rotation tolerance (radians); with
    ``tol = (0, 0)`` any bit that differs moves it.  A frame that is left alone keeps its ledger pose -- the caller must not overwrite
    it -- so the next correction measures its change against what the map really holds and small changes cannot pile up unseen.
    Records: the frames concerned in ascending order, in groups of at most 32; every group gives its removals in ascending order, then
    its additions in ascending order.  ``mode="auto"`` decides "rebuild" when ``2 * moved + added >= upto + 1`` (a fresh volume costs
    upto + 1 integrations, the correction two per moved frame and one per added); ``mode="incremental"`` never does."""
    if mode not in ("incremental", "auto"):
        raise ValueError(f"plan_map_correction: mode {mode!r} is neither 'incremental' nor 'auto'")
    tol_t, tol_r = float(tol[0]), float(tol[1])
    added, moved = [], []
    for j in range(upto + 1):
        old = ledger[j] if j < len(ledger) else None
        if old is None:
            added.append(j)
            continue
        if np.array_equal(np.asarray(old), np.asarray(new_poses[j])):
            continue
        dt, dr = pose_change(old, new_poses[j])
        if (tol_t == 0.0 and tol_r == 0.0) or dt > tol_t or dr > tol_r:
            moved.append(j)
    decision = "rebuild" if mode == "auto" and 2 * len(moved) + len(added) >= upto + 1 else "correct"
    concerned = sorted(added + moved)
    is_moved = set(moved)
    records, groups = [], []
    for g0 in range(0, len(concerned), GROUP_FRAMES):
        group = concerned[g0:g0 + GROUP_FRAMES]
        start = len(records)
        records += [(j, np.array(ledger[j], dtype=np.float64), True) for j in group if j in is_moved]
        records += [(j, np.array(new_poses[j], dtype=np.float64), False) for j in group]
        groups.append((start, len(records)))
    return MapCorrection(decision, added, moved, records, groups)
