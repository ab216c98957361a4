"""The reference's 3DM helper names, importable as ``from bodyslam_amd.slam_utils import ...``
(BodySLAM_not_refactored/3DM/slam_utils.py:71-122,138-169, scaling_system.py:72-77)."""
import numpy as np

from .posegraph import PoseGraph, update_global_extrinsic  # noqa: F401
from .geom3d import (REF_DEPTH_SCALE, REF_DEPTH_TRUNC, REF_INTRINSICS, add_pose_to_list,  # noqa: F401
                     compute_curr_estimate_global_pose, ensure_so3_v2, pixel_to_3d)


def save_poses_as_kitti(poses_list, output_path) -> None:
    """Drop-in for TXTIO.save_poses_as_kitti (BodySLAM_not_refactored/UTILS/io_utils.py:264-278): one line per 4x4 pose, its
    first three rows flattened (12 numbers) and formatted with ``str`` -- byte-identical to the reference's file for equal
    inputs.  (The reference copies each pose and leaves the SO(3) correction commented out; nothing is corrected here either.)"""
    with open(output_path, "w") as f:
        for pose in poses_list:
            flat = np.asarray(pose).flatten()[:-4]
            f.write(" ".join(map(str, flat)) + "\n")


def estimate_similarity_transformation(source: np.ndarray, target: np.ndarray):
    """Drop-in for estimate_similarity_transformation (BodySLAM_not_refactored/3DM/slam_utils.py:138-169): [3, n] numpy point sets in,
    (R [3, 3], s, t [3]) out with target ~ s R source + t.  Runs on the device (bs_similarity_fit); no CPU fallback."""
    from .evaluation import similarity_transform
    source, target = np.asarray(source), np.asarray(target)
    if source.ndim != 2 or source.shape[0] != 3 or source.shape != target.shape:
        raise ValueError(f"source shape {source.shape}, target shape {target.shape}: expected two [3, n] arrays")
    dt = np.float32 if source.dtype == np.float32 and target.dtype == np.float32 else np.float64
    return similarity_transform(np.ascontiguousarray(source.T, dtype=dt), np.ascontiguousarray(target.T, dtype=dt))
