"""A corner-rich RGB-D scene for the sparse-feature tests, rendered through tests/_render.py's camera model (pinhole, pose = camera ->
world, depth = camera-frame z).  _render's sinusoid texture has no FAST corner at threshold 20; this texture is piecewise constant: square
tiles of TILE metres in the world's (X, Y), each with a grey value (and a slight tint) from an integer hash of its tile coordinates, so
every junction of four tiles is a corner of high contrast.  On exactly constant tiles the pixels around a junction share one FAST score
and the strict 3 x 3 non-maximum suppression drops them all, so a smooth ripple of a few grey levels lies on top.  Two surfaces: the fronto-parallel plane Z = PLANE_Z (depth is constant under
a translation in X, Y) and _render.g's height field."""
import numpy as np

from _render import g

H, W = 152, 200                       # no multiple of any tile; level 7 of the ORB pyramid is 56 x 42 and has no interior
K = (200.0, 200.0, 100.0, 76.0)
PLANE_Z = 0.30
TILE = 0.0105                         # 7 pixels at PLANE_Z
REGION = (0.084, 0.0525)              # the tiles cover |X|, |Y| below this (whole tiles); around them the surface is plain, so that two
                                      # views a few millimetres apart see the same corners well inside the frame
RIPPLE = 8.0                          # grey levels of a smooth ripple on top of the tiles (below the FAST threshold: it makes no corner)


def _hash(i, j, c):
    h = (i.astype(np.int64) * 73856093) ^ (j.astype(np.int64) * 19349663) ^ (c * 83492791)
    h = (h ^ (h >> 13)) * 1274126177
    return (h ^ (h >> 16)) & 0xFFFF


def texture(X, Y):
    """uint8 [..., 3]"""
    i, j = np.floor(X / TILE).astype(np.int64), np.floor(Y / TILE).astype(np.int64)
    inside = (np.abs(X) < REGION[0]) & (np.abs(Y) < REGION[1])
    base = np.where(inside, 30 + (_hash(i, j, 0) % 180), 120) + np.rint(RIPPLE * np.sin(700.0 * X + 0.4) * np.cos(640.0 * Y - 1.1)).astype(np.int64)
    return np.stack([np.clip(base + (_hash(i, j, c) % 31) - 15, 0, 255) for c in (1, 2, 3)], -1).astype(np.uint8)


def render(pose, surface="plane", K=K, H=H, W=W):
    """(colour u8 [H, W, 3] RGB, depth fp32 [H, W])"""
    fx, fy, cx, cy = K
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u, dtype=np.float64)], -1) @ pose[:3, :3].T
    o = pose[:3, 3]
    if surface == "plane":
        s = (PLANE_Z - o[2]) / d[..., 2]
    else:
        s, eps = np.full((H, W), 0.3), 1e-6
        for _ in range(30):                                      # Newton on (o + s d).z = g((o + s d).x, (o + s d).y), as _render.render
            P = o + s[..., None] * d
            F = P[..., 2] - g(P[..., 0], P[..., 1])
            gx = (g(P[..., 0] + eps, P[..., 1]) - g(P[..., 0] - eps, P[..., 1])) / (2 * eps)
            gy = (g(P[..., 0], P[..., 1] + eps) - g(P[..., 0], P[..., 1] - eps)) / (2 * eps)
            s = s - F / (d[..., 2] - gx * d[..., 0] - gy * d[..., 1])
    P = o + s[..., None] * d
    return texture(P[..., 0], P[..., 1]), s.astype(np.float32)


def translation_pose(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


def blank(value=128):
    """a textureless frame: no keypoint"""
    return np.full((H, W, 3), value, dtype=np.uint8), np.full((H, W), PLANE_Z, dtype=np.float32)


# the two rendered pairs of the tests: camera 0 at the origin, camera 1 translated by T (camera -> world), so a static point moves by -T
# in the camera frame.  Chosen at least ten times the numpy statement's measured error (tests/test_sparse_scale_gpu.py).
PLANE_T = np.array([0.0125, -0.0067, 0.0])
FIELD_T = np.array([0.0185, -0.0097, 0.004])


def pair(surface):
    """((colour, depth) of the previous frame, (colour, depth) of the current frame, the camera-frame motion of a static point)"""
    t = PLANE_T if surface == "plane" else FIELD_T
    return render(translation_pose(np.zeros(3)), surface), render(translation_pose(t), surface), -t
