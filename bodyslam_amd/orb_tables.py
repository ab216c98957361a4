"""The constant tables of the ORB path (bodyslam_amd/scaling_system.py, csrc/sparse_features.hip): numpy only, no device.

They are DATA for both the kernels and the numpy statement of the algorithm (tests/_orb_ref.py):

  * ``COS`` / ``SIN``: cos and sin of the 30 orientation bins (12 degrees each, Rublee et al. 2011 section 4.2), committed as fp64
    literals so that no libm enters the bin decision or the rotation of the pattern;
  * ``brief_pattern()``: 256 test pairs drawn from an isotropic Gaussian with sigma = patch / 5 (Calonder et al. 2010, "BRIEF", the
    G II arrangement), clipped to the 31 x 31 patch.  OpenCV's ORB uses a LEARNT pair table instead, which is OpenCV's own and not
    reproduced here: descriptors therefore differ from OpenCV's and parity with it is unpinned.  The draw is integer-only (a 64-bit
    linear congruential generator, a sum of twelve uniforms for the Gaussian) so the table is the same on every machine;
  * ``rotated_pattern()``: the pattern rotated once per bin and rounded to pixels, int8 [30, 256, 4] = (x1, y1, x2, y2);
  * ``level_sizes`` / ``level_layout`` / ``features_per_level``: the pyramid geometry and cv2.ORB_create()'s split of the 500 features.
"""
from __future__ import annotations

import numpy as np

N_FEATURES, SCALE_FACTOR, N_LEVELS, EDGE_THRESHOLD, PATCH_SIZE, FAST_THRESHOLD = 500, 1.2, 8, 31, 31, 20
HARRIS_BLOCK, HARRIS_K = 7, 0.04
HALF_PATCH = PATCH_SIZE // 2
N_BINS = 30
PATTERN_SEED = 0x0B51AB
RESIZE_BITS = 11                                   # weight bits of the fixed-point bilinear resize
SMOOTH_TAPS = (1, 6, 15, 20, 15, 6, 1)             # binomial, sum 64: the 7 x 7 kernel sums to 4096

COS = (1.0, 0.9781476007338057, 0.9135454576426009, 0.8090169943749475, 0.6691306063588582, 0.5000000000000001, 0.30901699437494745,
       0.10452846326765346, -0.10452846326765355, -0.30901699437494734, -0.4999999999999998, -0.6691306063588582, -0.8090169943749473,
       -0.9135454576426008, -0.9781476007338057, -1.0, -0.9781476007338056, -0.9135454576426009, -0.8090169943749476,
       -0.6691306063588581, -0.5000000000000004, -0.30901699437494756, -0.10452846326765336, 0.10452846326765299, 0.30901699437494723,
       0.5000000000000001, 0.6691306063588578, 0.8090169943749473, 0.913545457642601, 0.9781476007338056)
SIN = (0.0, 0.20791169081775934, 0.4067366430758002, 0.5877852522924731, 0.7431448254773942, 0.8660254037844386, 0.9510565162951535,
       0.9945218953682733, 0.9945218953682733, 0.9510565162951536, 0.8660254037844387, 0.7431448254773942, 0.5877852522924732,
       0.40673664307580043, 0.20791169081775931, 1.2246467991473532e-16, -0.2079116908177595, -0.4067366430758002, -0.587785252292473,
       -0.7431448254773944, -0.8660254037844384, -0.9510565162951535, -0.9945218953682734, -0.9945218953682734, -0.9510565162951536,
       -0.8660254037844386, -0.7431448254773946, -0.5877852522924734, -0.40673664307580015, -0.20791169081775987)


def brief_pattern(seed: int = PATTERN_SEED) -> np.ndarray:
    """int32 [256, 4] = (x1, y1, x2, y2), every coordinate in [-15, 15]"""
    state = seed & 0xFFFFFFFFFFFFFFFF

    def gauss() -> int:
        nonlocal state
        total = 0
        for _ in range(12):                        # twelve uniforms in [0, 2^16): their sum has sigma = 2^16
            state = (state * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
            total += state >> 48
        v = (total - 6 * 65535) * (PATCH_SIZE * 2)             # sigma = patch / 5 = 2 patch / 10
        c = (v + 5 * 65536) // (10 * 65536)                    # round to the nearest pixel (floor of v / 655360 + 1/2)
        return max(-HALF_PATCH, min(HALF_PATCH, c))

    return np.array([[gauss() for _ in range(4)] for _ in range(256)], dtype=np.int32)


def rotated_pattern(seed: int = PATTERN_SEED) -> np.ndarray:
    """int8 [30, 256, 4]: bin k holds (rint(x c_k - y s_k), rint(x s_k + y c_k)) of both points of every pair (IEEE multiply, subtract /
    add and round-half-even only); |coordinate| <= 22"""
    p = brief_pattern(seed).astype(np.float64)
    out = np.empty((N_BINS, 256, 4), dtype=np.int8)
    for k in range(N_BINS):
        c, s = COS[k], SIN[k]
        for j in (0, 2):
            x, y = p[:, j], p[:, j + 1]
            out[k, :, j] = np.rint(x * c - y * s)
            out[k, :, j + 1] = np.rint(x * s + y * c)
    return out


def level_scales(n_levels: int = N_LEVELS) -> np.ndarray:
    return np.array([SCALE_FACTOR ** l for l in range(n_levels)], dtype=np.float64)


def level_sizes(H: int, W: int, n_levels: int = N_LEVELS):
    """[(W_l, H_l)]: round(W / 1.2^l) x round(H / 1.2^l), round half to even"""
    return [(int(np.rint(W / s)), int(np.rint(H / s))) for s in level_scales(n_levels)]


def level_layout(H: int, W: int, n_levels: int = N_LEVELS):
    """int32 [n_levels, 3] = (W_l, H_l, offset_l) and the stride of one frame in the flat pyramid buffer: the levels of a frame lie one
    behind the other, each offset a multiple of 16 bytes with 16 bytes of slack behind the last pixel (the selector reads 16 at a time)"""
    rows, off = [], 0
    for (w, h) in level_sizes(H, W, n_levels):
        rows.append((w, h, off))
        off += (w * h + 15) // 16 * 16 + 16
    return np.array(rows, dtype=np.int32), off


def features_per_level(n_features: int = N_FEATURES, n_levels: int = N_LEVELS) -> np.ndarray:
    """cv2.ORB's geometric split: n_0 = N (1 - f) / (1 - f^L) with f = 1 / 1.2, n_l = round(n_0 f^l), the last level takes the rest"""
    f = 1.0 / SCALE_FACTOR
    want = n_features * (1.0 - f) / (1.0 - f ** n_levels)
    out, total = [], 0
    for _ in range(n_levels - 1):
        out.append(int(np.rint(want)))
        total += out[-1]
        want *= f
    out.append(max(n_features - total, 0))
    return np.array(out, dtype=np.int32)
