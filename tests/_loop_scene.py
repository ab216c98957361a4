"""Views for the loop-closure tests on tests/_corner_scene.py's surfaces: a revisit (the same tiles from a nearby pose) and "a different
place" -- the same surface and tile grid, every tile's grey value and tint taken from the hash of shifted tile coordinates, so the corners
sit where they sat and look different.  _corner_scene itself is unchanged; place 0 is its own render."""
import numpy as np

import _corner_scene as S
from _render import small_pose

H, W, K = S.H, S.W, S.K
SURFACE = "field"                     # _render.g's height field: the lifted points are not coplanar

# the poses of the tests (camera -> world)
ORIGIN = np.eye(4)
REVISIT = small_pose(0.02, -0.03, 0.05, 0.010, -0.006, 0.008)
REVISIT_FAR = small_pose(0.05, -0.06, 0.15, 0.020, -0.012, 0.015)
ELSEWHERE = small_pose(-0.01, 0.02, -0.03, -0.004, 0.005, 0.003)          # a second view of another place


def texture(X, Y, place):
    """_corner_scene.texture with the tile hash taken at (i + 1009 place, j - 757 place)"""
    i, j = np.floor(X / S.TILE).astype(np.int64), np.floor(Y / S.TILE).astype(np.int64)
    inside = (np.abs(X) < S.REGION[0]) & (np.abs(Y) < S.REGION[1])
    hi, hj = i + 1009 * place, j - 757 * place
    base = np.where(inside, 30 + (S._hash(hi, hj, 0) % 180), 120) + np.rint(S.RIPPLE * np.sin(700.0 * X + 0.4) * np.cos(640.0 * Y - 1.1)).astype(np.int64)
    return np.stack([np.clip(base + (S._hash(hi, hj, c) % 31) - 15, 0, 255) for c in (1, 2, 3)], -1).astype(np.uint8)


def render(pose, place=0, surface=SURFACE):
    """(colour u8 [H, W, 3] RGB, depth fp32 [H, W]); place 0 is _corner_scene.render"""
    color, depth = S.render(pose, surface)
    if place == 0:
        return color, depth
    fx, fy, cx, cy = K
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u, dtype=np.float64)], -1) @ pose[:3, :3].T
    P = pose[:3, 3] + depth.astype(np.float64)[..., None] * d
    return texture(P[..., 0], P[..., 1], place), depth


def motion(pose_source, pose_target=ORIGIN):
    """the edge of a closure source -> target: T = pose_target^-1 pose_source (X_target = T X_source for camera -> world poses)"""
    return np.linalg.inv(pose_target) @ pose_source
