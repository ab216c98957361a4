"""Inputs and plain numpy statements for the 3DM geometry stage tests (tests/test_geom3d_cases_cpu.py, tests/test_geom3d_stages_gpu.py):
numpy only, every draw seeded; the only file read is tests/golden/geom3d_chain.npz (its 16 `so3_in` matrices).

tests/test_ops_gpu.py drives csrc/geom3d.hip with one golden chain, one golden frame and random 480 x 640 frames.  The builders here put
the inputs ON the edges of the kernels instead; what each one reaches is asserted on the oracle (oracle/geom3d_ref.py) in
tests/test_geom3d_cases_cpu.py.

  chain_case(name)          every pose-chain case by name -> dict(t_rel float32 [N, 4, 4], g0 float64 [4, 4] or None, ...):
                            "len<N>-<none|rot|general>"  the lengths on the wave (64) and round (256) borders of pose_scan_kernel
                            "so3-<i>"                    golden so3_in[i] as the g0 block, one identity step (geom3d.ensure_so3_v2)
                            "nonaffine-<variant>"        N = 300 with one bottom row that is not [0 0 0 1] (pose_chain_sequential)
                            "rank-<variant>"             a rank-deficient g0 block, one identity step
                            "nan"                        N = 257 with a NaN in the step that makes pose 100
  prefix_product(case)      the chain as the product of independently projected elements (what the scan path computes), LAPACK SVD
  CHAIN_GAPS / chain_bar()  the measured oracle-against-prefix-product gaps and the device bar they define
  bp_statement(...)         back-projection in the kernel's order of operations, fp64 with one rounding to fp32
  z32_rule / z64_rule       the fp32 validity rule of the reference's image path, and the rule with the division left in fp64
  the depth builders        scan_round_depth, border_depth, load_path_depth, every_code_depth
"""
import functools
import os

import numpy as np

from oracle import geom3d_ref as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- A. pose chain ---------------------------------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 512, 513)
G0_KINDS = ("none", "rot", "general")
FROM_STEPS = (64, 64, 128, 1, 256)                      # the N = 513 chain cut for bs_pose_chain_from
NONAFFINE_N = 300
NONAFFINE_VARIANTS = ("row0", "row70", "row299", "w2", "g0")
NAN_N, NAN_POSE = 257, 100
RANK_VARIANTS = ("diag110", "middle_zero", "zero", "product", "one_column")
RANK2 = ("diag110", "middle_zero", "product")          # the closest rotation is unique: compared with the oracle


def _orth(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.diag(r))


def _rotation(rng):
    q = _orth(rng)
    return q * np.linalg.det(q)                         # det +1 (a 3 x 3: -q has the other sign)


def relative_poses(N, seed):
    """float32 [N, 4, 4]: R_i = Q1 diag(1 + uniform(-0.2, 0.2)) Q2 rounded to fp32 (no rotation: the projection does real work), every
    seventh element (i % 7 == 6) the reflection Q1 diag(1.2, 1.0, -0.7) Q2; translations normal(0, 0.05); bottom row [0 0 0 1]"""
    rng = np.random.default_rng(seed)
    t = np.zeros((N, 4, 4), np.float32)
    for i in range(N):
        q1, q2 = _rotation(rng), _rotation(rng)
        d = 1.0 + rng.uniform(-0.2, 0.2, size=3)
        if i % 7 == 6:
            d = np.array([1.2, 1.0, -0.7])
        t[i, :3, :3] = (q1 @ np.diag(d) @ q2).astype(np.float32)
        t[i, :3, 3] = rng.normal(0.0, 0.05, size=3).astype(np.float32)
        t[i, 3, 3] = 1.0
    return t


def g0_of(kind, seed=100):
    """None; a rotation with a translation; a general full-rank block (singular values 0.9 .. 1.5, det > 0) with a translation"""
    if kind == "none":
        return None
    rng = np.random.default_rng(seed)
    g = np.eye(4)
    if kind == "rot":
        g[:3, :3] = _rotation(rng)
    else:
        g[:3, :3] = _rotation(rng) @ np.diag([1.5, 1.2, 0.9]) @ _rotation(rng)
    g[:3, 3] = rng.normal(0.0, 1.0, size=3)
    return g


@functools.lru_cache(maxsize=None)
def so3_golden():
    g = np.load(os.path.join(GOLDEN, "geom3d_chain.npz"))
    return np.array(g["so3_in"], dtype=np.float64), np.array(g["so3_out"], dtype=np.float64)


def rank_block(variant):
    """the rank-deficient 3 x 3 blocks: exact zero columns (the Jacobi leaves a zero column in U there) and one product A[3x2] B[2x3] with no
    zero entry whose smallest singular value is rounding noise"""
    rng = np.random.default_rng(7)
    if variant == "diag110":
        return np.diag([1.0, 1.0, 0.0])
    if variant == "middle_zero":
        m = _rotation(rng) @ np.diag([1.3, 0.8, 0.6])
        m[:, 1] = 0.0
        return m
    if variant == "zero":
        return np.zeros((3, 3))
    if variant == "product":
        return rng.normal(size=(3, 2)) @ rng.normal(size=(2, 3))
    if variant == "one_column":                         # rank 1 with two exactly zero columns
        m = np.zeros((3, 3))
        m[:, 2] = [0.3, -1.1, 0.7]
        return m
    raise KeyError(variant)


def assert_proper_completion(R, M, tol=1e-12):
    """what every answer to a rank-deficient block M must satisfy, unique or not: R is a proper rotation, it maps the dominant right singular
    vector onto the dominant left one (when there is one), and R^T M is symmetric positive semi-definite (R is a polar factor of M)"""
    R = np.asarray(R, dtype=np.float64)
    assert np.isfinite(R).all(), R
    assert np.abs(R.T @ R - np.eye(3)).max() < tol, R
    assert abs(np.linalg.det(R) - 1.0) < tol, R
    U, s, Vt = np.linalg.svd(M)
    if s[0] > 0:
        assert np.abs(R @ Vt[0] - U[:, 0]).max() < tol, (R @ Vt[0], U[:, 0])
    S = R.T @ M
    scale = max(1.0, s[0])
    if np.linalg.matrix_rank(M) == 2:                   # with rank 2 and det R = +1 the polar factor is the closest rotation, and unique
        assert np.abs(S - S.T).max() < tol * scale and np.linalg.eigvalsh(0.5 * (S + S.T)).min() > -tol * scale, S


def chain_names():
    names = [f"len{N}-{k}" for N in LENGTHS for k in G0_KINDS]
    names += [f"so3-{i}" for i in range(16)]
    names += [f"nonaffine-{v}" for v in NONAFFINE_VARIANTS] + [f"affine-twin-{v}" for v in NONAFFINE_VARIANTS]
    names += [f"rank-{v}" for v in RANK_VARIANTS]
    return names


@functools.lru_cache(maxsize=None)
def chain_case(name):
    """-> dict(name, t_rel, g0, affine: the scan path is taken, ref: the oracle's chain [N + 1, 4, 4] or None where it has none)"""
    kind, _, arg = name.partition("-")
    affine = True
    if kind.startswith("len"):
        N = int(kind[3:])
        t, g0 = relative_poses(N, seed=1000 + N), g0_of(arg)
    elif kind == "so3":
        t, g0 = np.eye(4, dtype=np.float32)[None], np.eye(4)
        g0[:3, :3] = so3_golden()[0][int(arg)]
    elif kind == "rank":
        t, g0 = np.eye(4, dtype=np.float32)[None], np.eye(4)
        g0[:3, :3] = rank_block(arg)
        g0[:3, 3] = [0.25, -0.5, 2.0]
    elif kind in ("nonaffine", "affine"):
        if kind == "affine":
            arg = arg[len("twin-"):]
        t, g0 = relative_poses(NONAFFINE_N, seed=2000), g0_of("rot", seed=101)
        if kind == "nonaffine":
            affine = False
            if arg.startswith("row"):
                t[int(arg[3:]), 3, :] = [0.1, 0.0, 0.0, 1.0]
            elif arg == "w2":
                t[150, 3, :] = [0.0, 0.0, 0.0, 2.0]
            elif arg == "g0":
                g0[3, :] = [0.05, -0.02, 0.0, 1.0]
            else:
                raise KeyError(name)
    elif name == "nan":
        t, g0 = relative_poses(NAN_N, seed=3000), None
        t[NAN_POSE - 1, 0, 1] = np.nan                  # pose k = proj(pose k-1 @ t_rel[k - 1])
        return dict(name=name, t_rel=t, g0=g0, affine=True, ref=None)
    else:
        raise KeyError(name)
    t.setflags(write=False)
    ref = G.pose_chain(t, g0)
    ref.setflags(write=False)
    return dict(name=name, t_rel=t, g0=g0, affine=affine, ref=ref)


def nan_twin():
    """the "nan" case without its NaN"""
    return relative_poses(NAN_N, seed=3000)


def projected_blocks(case):
    """the 3 x 3 blocks the oracle hands to ensure_so3_v2 along the chain, [N, 3, 3]"""
    ref, t = case["ref"], case["t_rel"]
    return np.stack([np.dot(ref[i], t[i])[:3, :3] for i in range(len(t))])


def prefix_product(case):
    """The chain as the scan path states it: element 0 is formed from g0 as the reference does, every other element is (proj(R_i), t_i)
    projected on its own, and pose i is the running product (Ra, ta) o (Rb, tb) = (Ra Rb, Ra tb + ta).  Both sides use LAPACK, so the gap
    to the oracle's chain is what the reassociation alone moves.  Affine inputs only."""
    g = np.eye(4) if case["g0"] is None else np.array(case["g0"], dtype=np.float64)
    out = [g.copy()]
    R = t = None
    for i, T in enumerate(case["t_rel"].astype(np.float64)):
        if i == 0:
            C = g @ T
            R, t = G.ensure_so3_v2(C[:3, :3]), C[:3, 3].copy()
        else:
            t = R @ T[:3, 3] + t
            R = R @ G.ensure_so3_v2(T[:3, :3])
        P = np.eye(4)
        P[:3, :3], P[:3, 3] = R, t
        out.append(P)
    return np.stack(out)


def gap_name(name):
    """the case whose measured gap sets the bar of `name`: a non-affine chain takes the strict recurrence, where no reassociation happens; its
    bar is that of the same chain with the row restored (same length, same magnitudes)"""
    return name.replace("nonaffine-", "affine-twin-")


# Gaps between oracle.geom3d_ref.pose_chain and prefix_product(), max |difference| over the whole [N + 1, 4, 4] result, as printed by
# tests/test_geom3d_cases_cpu.py::test_chain_gaps.  Measured on an x86-64 host (numpy 2.x on OpenBLAS / LAPACK gesdd).  The device bar of a
# case is max(1e-12, 8 x its gap), never above the 1e-9 of tests/test_ops_gpu.py::test_pose_chain; nothing here comes from a device.
CHAIN_GAPS = {
    "len1-none": 0.0, "len1-rot": 0.0, "len1-general": 0.0,
    "len2-none": 5.6e-16, "len2-rot": 8.9e-16, "len2-general": 4.4e-16,
    "len63-none": 7.0e-15, "len63-rot": 4.3e-15, "len63-general": 6.0e-15,
    "len64-none": 1.0e-14, "len64-rot": 1.2e-14, "len64-general": 9.4e-15,
    "len65-none": 6.4e-15, "len65-rot": 7.2e-15, "len65-general": 6.6e-15,
    "len255-none": 2.3e-14, "len255-rot": 2.0e-14, "len255-general": 2.2e-14,
    "len256-none": 1.3e-14, "len256-rot": 2.2e-14, "len256-general": 1.5e-14,
    "len257-none": 1.6e-14, "len257-rot": 2.7e-14, "len257-general": 2.1e-14,
    "len512-none": 2.4e-14, "len512-rot": 2.4e-14, "len512-general": 2.8e-14,
    "len513-none": 4.2e-14, "len513-rot": 2.3e-14, "len513-general": 2.3e-14,
    "affine-twin-row0": 1.8e-14, "affine-twin-row70": 1.8e-14, "affine-twin-row299": 1.8e-14, "affine-twin-w2": 1.8e-14,
    "affine-twin-g0": 1.8e-14,
}
SINGLE_STEP_GAP = 0.0      # "so3-*", "rank-*": one element, formed from g0 as the reference forms it: there is nothing to reassociate
BAR_FLOOR, BAR_CAP = 1e-12, 1e-9


def chain_gap(name):
    name = gap_name(name)
    return SINGLE_STEP_GAP if name.startswith(("so3-", "rank-")) else CHAIN_GAPS[name]


def chain_bar(name):
    return min(BAR_CAP, max(BAR_FLOOR, 8.0 * chain_gap(name)))


# ---- B. back-projection ------------------------------------------------------------------------------------------------------------------------
def z32_rule(depth_u16, scale, trunc):
    """the reference's float32 image path: z = fl32(d / scale), z >= fl32(trunc) -> 0; a pixel is valid iff z > 0"""
    z = depth_u16.astype(np.float32) / np.float32(scale)
    return np.where(z >= np.float32(trunc), np.float32(0), z)


def z64_rule(depth_u16, scale, trunc):
    """the same rule with the quotient left in fp64 (the two float32 arguments as the kernel receives them): what a kernel that divides in
    double would decide"""
    z = depth_u16.astype(np.float64) / np.float64(np.float32(scale))
    return np.where(z >= np.float64(np.float32(trunc)), 0.0, z)


def bp_statement(depth_u16, K, scale, trunc, pose=None, rounded=True):
    """[H, W] uint16 -> (xyz [M, 3], idx int32 [M]) of the valid pixels in row-major order, in the kernel's order of operations (the library
    is built with -ffp-contract=off): x = ((u - cx) z) / fx, y = ((v - cy) z) / fy, w = ((P0 x + P1 y) + P2 z) + P3 per row of the pose, all
    fp64, one rounding to fp32 at the end (rounded=False: the fp64 values before it)"""
    fx, fy, cx, cy = (np.float64(k) for k in K)
    H, W = depth_u16.shape
    z32 = z32_rule(depth_u16, scale, trunc).ravel()
    idx = np.flatnonzero(z32 > 0)
    v, u = np.divmod(idx, W)
    z = z32[idx].astype(np.float64)
    x = ((u.astype(np.float64) - cx) * z) / fx
    y = ((v.astype(np.float64) - cy) * z) / fy
    if pose is not None:
        P = np.asarray(pose, dtype=np.float64)
        x, y, z = (((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3] for r in range(3))
    pts = np.stack([x, y, z], axis=1)
    return (pts.astype(np.float32) if rounded else pts), idx.astype(np.int32)


def pixel_statement(uvd, K):
    """bs_pixel_to_3d's order: ((u - cx) d) / fx, ((v - cy) d) / fy, d"""
    fx, fy, cx, cy = (np.float64(k) for k in K)
    u, v, d = uvd[:, 0], uvd[:, 1], uvd[:, 2]
    return np.stack([((u - cx) * d) / fx, ((v - cy) * d) / fy, d], axis=1)


def bp_poses(B, seed=50):
    """camera -> world poses float64 [B, 4, 4]: rotations with translations of a few metres"""
    rng = np.random.default_rng(seed)
    P = np.tile(np.eye(4), (B, 1, 1))
    for b in range(B):
        P[b, :3, :3] = _rotation(rng)
        P[b, :3, 3] = rng.normal(0.0, 2.0, size=3)
    return P


def half_valid(rng, shape):
    """about half the pixels valid at (1000, 3.0): codes 1 .. 2999 valid; 0, 3000 (the first invalid code) and larger ones invalid"""
    d = rng.integers(1, 3000, size=shape).astype(np.uint16)
    kind = rng.integers(0, 6, size=shape)
    d[kind == 0] = 0
    d[kind == 1] = 3000
    d[kind == 2] = rng.integers(3000, 65536, size=shape).astype(np.uint16)[kind == 2]
    return d


SCAN_SHAPES = ((1, 526339), (513, 1027), (512, 1024))   # 258, 258 and 256 chunks of 2048: two scan rounds, and the last shape of one


@functools.lru_cache(maxsize=None)
def scan_round_depth(shape):
    """uint16 [2, H, W]: image 0 about half valid, image 1 all valid (every chunk count 2048, the last one the remainder)"""
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    d = np.empty((2,) + tuple(shape), np.uint16)
    d[0] = half_valid(rng, shape)
    d[1] = rng.integers(1, 3000, size=shape).astype(np.uint16)
    d.setflags(write=False)
    return d


BORDER_SHAPE = (3, 2048)                                # three chunks; thread t of a chunk holds pixels 8 t .. 8 t + 7, a wave 512 pixels
BORDER_PATTERNS = ("borders", "first", "last", "alternate", "all", "none")


def border_depth(pattern):
    """uint16 [1, 3, 2048] whose valid pixels sit on the thread, wave and chunk borders of the compaction"""
    H, W = BORDER_SHAPE
    n = H * W
    valid = np.zeros(n, bool)
    if pattern == "borders":
        valid[[7, 8, 511, 512, 2047, 2048, 4095, 4096, n - 1]] = True
    elif pattern == "first":
        valid[0] = True
    elif pattern == "last":
        valid[n - 1] = True
    elif pattern == "alternate":
        valid[::2] = True
    elif pattern == "all":
        valid[:] = True
    elif pattern != "none":
        raise KeyError(pattern)
    rng = np.random.default_rng(11)
    d = np.where(valid, rng.integers(1, 3000, size=n), rng.choice([0, 3000, 65535], size=n)).astype(np.uint16)
    return d.reshape(1, H, W)


LOAD_SHAPES = ((37, 61), (5, 8), (1, 1), (1, 7))        # npix odd: the second image of a batch is misaligned and takes the element path


def load_path_depth(shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    d = half_valid(rng, (3,) + tuple(shape))
    d[:, -1, -1] = 1234                                 # the last pixel of every image is valid: the ragged tail of the last load is read
    return d


RULES = ((1000.0, 3.0), (1000.0, 0.3), (5000.0, 3.0), (256.0, 3.0), (1000.0, 3.0e38))


@functools.lru_cache(maxsize=None)
def every_code_depth():
    """uint16 [1, 256, 256]: every code 0 .. 65535 once, in a seeded order (so a pixel's index says nothing about its code)"""
    d = np.random.default_rng(21).permutation(65536).astype(np.uint16).reshape(1, 256, 256)
    d.setflags(write=False)
    return d


ODD_INTRINSICS = ((525.3, 310.9, -13.7, 1000.25), (201.125, 417.6, 700.5, -8.125))   # fx != fy; cx, cy negative and far outside a 37 x 61 frame
PIXEL_SIZES = (1, 255, 256, 257, 1000)


def pixel_points(n, seed=31):
    """float64 [n, 3] of (u, v, d): random, with d = 0, d = -0.0 and negative d among them"""
    rng = np.random.default_rng(seed + n)
    uvd = np.stack([rng.uniform(-50, 700, n), rng.uniform(-50, 500, n), rng.uniform(-1.0, 4.0, n)], axis=1)
    uvd[::5, 2] = 0.0
    uvd[3::50, 2] = -0.0
    uvd[n - 1, 2] = -1.75 if n > 1 else 0.0
    return uvd
