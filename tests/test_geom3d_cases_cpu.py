"""The cases of tests/_geom3d_cases.py are fair and reach what they are built for -- checked on the oracle (oracle/geom3d_ref.py) alone, without
a GPU.  tests/test_geom3d_stages_gpu.py runs the same cases through csrc/geom3d.hip.  The fairness quantities and the gaps that define the
device bars are printed (pytest -s shows them)."""
import numpy as np
import pytest

import _geom3d_cases as C
from oracle import geom3d_ref as G

BP_CHUNK = 2048          # pixels per block of the compaction (csrc/geom3d.hip)
SCAN_ROUND = 256         # chunk counts per round of bp_scan_kernel, poses per round of pose_scan_kernel


# ---- A. pose chain ---------------------------------------------------------------------------------------------------------------------------
def _fairness(blocks):
    """-> (smallest sigma_3 over the blocks with det > 0, smallest sigma_2 - sigma_3 over those with det < 0, number of reflections)"""
    s = np.linalg.svd(blocks, compute_uv=False)
    neg = np.linalg.det(blocks) < 0
    s3 = float(s[~neg, 2].min()) if (~neg).any() else np.inf
    split = float((s[neg, 1] - s[neg, 2]).min()) if neg.any() else np.inf
    return s3, split, int(neg.sum())


@pytest.mark.parametrize("name", [n for n in C.chain_names() if n.startswith(("len", "nonaffine", "affine"))])
def test_generated_chains_are_fair(name):
    """A reflection is decided by the smallest singular value, so Jacobi and LAPACK agree only where it is well separated: sigma_2 - sigma_3
    >= 0.1 wherever det < 0, sigma_3 >= 0.5 elsewhere -- on the inputs and on every block the oracle projects along the chain (a general
    g0 and a bottom row other than [0 0 0 1] both change the first of those).  The reflections diag(1.2, 1.0, -0.7) have singular values
    1.2, 1.0, 0.7: sigma_2 - sigma_3 = 0.3 up to the fp32 rounding."""
    case = C.chain_case(name)
    t = case["t_rel"]
    N = len(t)
    for what, blocks in (("inputs", t[:, :3, :3].astype(np.float64)), ("projected", C.projected_blocks(case))):
        s3, split, nrefl = _fairness(blocks)
        print(f"{name} {what}: min sigma_3 (det > 0) {s3:.4f}, min sigma_2 - sigma_3 (det < 0) {split:.4f}, {nrefl} reflections of {N}")
        assert s3 >= 0.5 and split >= 0.1
        assert nrefl == N // 7                                           # every seventh element, and no other
    # the projection does real work: no input block is a rotation already
    R = t[:, :3, :3].astype(np.float64)
    assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max(axis=(1, 2)).min() > 1e-3
    rows_affine = bool(np.all(t[:, 3, :] == np.array([0, 0, 0, 1], np.float32)))
    g0_affine = case["g0"] is None or np.array_equal(case["g0"][3], [0, 0, 0, 1])
    assert (rows_affine and g0_affine) == case["affine"]
    if name == "nonaffine-g0":
        assert rows_affine and not g0_affine
    elif name.startswith("nonaffine"):
        assert g0_affine and (~np.all(t[:, 3, :] == np.array([0, 0, 0, 1], np.float32), axis=1)).sum() == 1


def test_lengths_sit_on_the_wave_and_round_borders():
    assert set(C.LENGTHS) >= {63, 64, 65, 255, 256, 257, 512, 513, 1, 2}
    assert sum(C.FROM_STEPS) == 513 and set(C.FROM_STEPS) >= {1, 64, 256} and C.NONAFFINE_N > SCAN_ROUND
    assert C.NAN_POSE < C.NAN_N and C.NAN_N > SCAN_ROUND


def test_general_g0_is_no_rotation_and_rot_is_one():
    g = C.g0_of("general")[:3, :3]
    s = np.linalg.svd(g, compute_uv=False)
    print("general g0 singular values", s)
    assert s[2] >= 0.85 and s[0] - s[2] > 0.5 and np.linalg.det(g) > 0
    r = C.g0_of("rot")[:3, :3]
    assert np.abs(r.T @ r - np.eye(3)).max() < 1e-14 and np.linalg.det(r) > 0


def test_golden_so3_inputs_are_what_the_oracle_is_pinned_on():
    """All 16: the oracle reproduces so3_out bit for bit (tests/test_oracle_geom3d.py pins the same).  Their conditioning: sigma_2 + sigma_3
    where det > 0, sigma_2 - sigma_3 where det < 0.  Matrix 0 is diag(1, 1, -1), an exact tie of all three singular values: its answer is a
    convention (the last index is flipped), pinned by the reference's own output."""
    so3_in, so3_out = C.so3_golden()
    assert so3_in.shape == (16, 3, 3)
    for i, m in enumerate(so3_in):
        assert np.array_equal(G.ensure_so3_v2(m), so3_out[i])
        assert np.array_equal(C.chain_case(f"so3-{i}")["ref"][1, :3, :3], so3_out[i])      # the chain form adds exact zeros only
        s = np.linalg.svd(m, compute_uv=False)
        det = np.linalg.det(m)
        cond = s[1] + s[2] if det > 0 else s[1] - s[2]
        print(f"so3-{i}: det {det:+.3f} sigma {s.round(4)} conditioning {cond:.4f}")
        if i == 0:
            assert np.array_equal(m, np.diag([1.0, 1.0, -1.0]))
        else:
            assert cond >= 0.3
    assert (np.linalg.det(so3_in) < 0).sum() >= 4 and (np.linalg.det(so3_in) > 0).sum() >= 8


@pytest.mark.parametrize("name", [n for n in C.chain_names() if C.chain_case(n)["affine"]])
def test_chain_gaps(name):
    """The gap between the oracle's recurrence and the prefix product of independently projected elements (LAPACK on both sides) is what the
    reassociation alone moves; 8 x it (at least 1e-12, at most 1e-9) is the device bar.  The bars are held in _geom3d_cases.py; here they
    must cover what this host measures."""
    case = C.chain_case(name)
    gap = float(np.abs(C.prefix_product(case) - case["ref"]).max())
    tmax = float(np.abs(case["ref"][:, :3, 3]).max())
    print(f"{name}: N {len(case['t_rel'])} max|t| {tmax:.2f} gap {gap:.1e} held {C.chain_gap(name):.1e} bar {C.chain_bar(name):.1e}")
    assert gap <= C.chain_bar(name)
    assert C.BAR_FLOOR <= C.chain_bar(name) <= C.BAR_CAP
    assert np.array_equal(C.prefix_product(case)[0], case["ref"][0])


@pytest.mark.parametrize("variant", C.NONAFFINE_VARIANTS)
def test_nonaffine_cases_differ_from_their_affine_twins(variant):
    """the bottom row matters: from the element that carries it the oracle's chain leaves the affine twin's by far more than the bar, in the
    bottom rows and (through the full 4 x 4 product) in the top rows; before it the two are bit-equal"""
    bad, twin = C.chain_case(f"nonaffine-{variant}"), C.chain_case(f"affine-twin-{variant}")
    first = {"row0": 0, "row70": 70, "row299": 299, "w2": 150, "g0": -1}[variant] + 1
    assert np.array_equal(bad["ref"][:first], twin["ref"][:first])
    assert np.all(twin["ref"][:, 3, :] == [0, 0, 0, 1])
    rows = np.abs(bad["ref"][first:, 3, :] - [0, 0, 0, 1]).max(axis=1)
    top = np.abs(bad["ref"][first:, :3, :] - twin["ref"][first:, :3, :]).max(axis=(1, 2))
    print(f"nonaffine-{variant}: bottom rows off [0 0 0 1] by {rows.min():.2e} .. {rows.max():.2e}, top rows off the twin by up to {top.max():.2e}")
    assert rows.min() > 1e-3
    if variant == "g0":      # the top rows of G T never read G's bottom row: only the bottom rows tell this chain from its twin
        assert top.max() == 0.0
    else:
        assert top.max() > 1e-3
    assert C.gap_name(bad["name"]) == twin["name"]


@pytest.mark.parametrize("variant", C.RANK_VARIANTS)
def test_rank_deficient_blocks(variant):
    """what each block is, and that the oracle's answer is a proper rotation; with rank 2 it is the unique closest one"""
    M = C.rank_block(variant)
    s = np.linalg.svd(M, compute_uv=False)
    rank = {"diag110": 2, "middle_zero": 2, "zero": 0, "product": 2, "one_column": 1}[variant]
    print(f"rank-{variant}: sigma {s}")
    assert np.linalg.matrix_rank(M) == rank and (variant in C.RANK2) == (rank == 2)
    if variant == "product":
        assert np.all(M != 0) and 0 < s[2] < 1e-14 * s[0] and s[1] > 0.1
    elif rank == 2:
        assert s[2] < 1e-15 and s[1] > 0.5 and np.any(np.all(M == 0, axis=0))
    ref = C.chain_case(f"rank-{variant}")["ref"][1]
    C.assert_proper_completion(ref[:3, :3], M)
    assert np.array_equal(ref[:3, 3], [0.25, -0.5, 2.0])
    if variant in ("diag110", "zero"):
        assert np.array_equal(ref[:3, :3], np.eye(3))                    # LAPACK completes the basis


def test_nan_case():
    t, twin = C.chain_case("nan")["t_rel"], C.nan_twin()
    k = C.NAN_POSE - 1
    assert np.isnan(t[k]).sum() == 1 and np.isnan(t[k, 0, 1])
    assert np.array_equal(np.delete(t, k, axis=0), np.delete(twin, k, axis=0))
    assert np.all(t[:, 3, :] == np.array([0, 0, 0, 1], np.float32))     # the scan path, not the fallback


# ---- B. back-projection ------------------------------------------------------------------------------------------------------------------------
def _half_ulp_ok(stmt64, ref32):
    return np.all(np.abs(stmt64 - ref32.astype(np.float64)) <= 0.5 * np.spacing(np.abs(ref32)).astype(np.float64) + 1e-12)


@pytest.mark.parametrize("shape", C.LOAD_SHAPES + ((48, 64),))
def test_statement_against_the_oracle(shape):
    """bp_statement is oracle.geom3d_ref.backproject with the order of operations written out: equal bit for bit without a pose; with one
    the oracle multiplies through BLAS, and the statement's fp64 value lies within half an fp32 ulp (plus 1e-12) of the oracle's fp32"""
    depth = C.load_path_depth(shape)
    poses = C.bp_poses(3)
    worst = 0
    for K in (G.REF_INTRINSICS,) + C.ODD_INTRINSICS:
        for b in range(3):
            rx, ri = G.backproject(depth[b], K)
            sx, si = C.bp_statement(depth[b], K, 1000.0, 3.0)
            assert np.array_equal(si, ri) and si.dtype == np.int32 and np.array_equal(sx, rx) and sx.dtype == np.float32
            rx, ri = G.backproject(depth[b], K, pose=poses[b])
            s64, si = C.bp_statement(depth[b], K, 1000.0, 3.0, pose=poses[b], rounded=False)
            assert np.array_equal(si, ri) and _half_ulp_ok(s64, rx)
            worst += int((C.bp_statement(depth[b], K, 1000.0, 3.0, pose=poses[b])[0] != rx).sum())
    print(f"{shape}: {worst} coordinates where the statement and the BLAS product round to different floats")


@pytest.mark.parametrize("shape", C.SCAN_SHAPES)
def test_scan_round_shapes(shape):
    """two rounds of bp_scan_kernel need more than 256 chunks; (512, 1024) is the last shape of one round.  Image 1 of an npix % 8 == 3
    batch starts 6 bytes off a 16-byte boundary"""
    npix = shape[0] * shape[1]
    chunks = -(-npix // BP_CHUNK)
    depth = C.scan_round_depth(shape)
    valid = (C.z32_rule(depth, 1000.0, 3.0) > 0).reshape(2, -1)
    print(f"{shape}: {npix} pixels, {chunks} chunks, npix % 8 = {npix % 8}, valid {valid.sum(axis=1).tolist()}")
    if shape == (512, 1024):
        assert chunks == SCAN_ROUND and npix % 8 == 0
    else:
        assert chunks == 258 and npix % 8 == 3 and (npix * 2) % 16 != 0
        # the carry of the second round is not zero, and the chunks of that round hold valid pixels
        assert valid[0, :SCAN_ROUND * BP_CHUNK].sum() > 0 and valid[0, SCAN_ROUND * BP_CHUNK:].sum() > 0
    assert valid[1].all() and 0.45 < valid[0].mean() < 0.55
    assert npix < 2 ** 31


def test_border_patterns():
    H, W = C.BORDER_SHAPE
    n = H * W
    assert n == 3 * BP_CHUNK
    want = {"borders": [7, 8, 511, 512, 2047, 2048, 4095, 4096, n - 1], "first": [0], "last": [n - 1], "alternate": list(range(0, n, 2)),
            "all": list(range(n)), "none": []}
    for pattern in C.BORDER_PATTERNS:
        idx = C.bp_statement(C.border_depth(pattern)[0], G.REF_INTRINSICS, 1000.0, 3.0)[1]
        assert idx.tolist() == want[pattern]


def test_load_path_shapes():
    """(37, 61): 2257 pixels, odd, so images 1 and 2 of a batch start 2 and 4 bytes off a 16-byte boundary and their last load is ragged;
    (5, 8): whole 16-byte loads; (1, 1) and (1, 7): less than one load"""
    assert [(h * w) % 8 for h, w in C.LOAD_SHAPES] == [1, 0, 1, 7]
    for shape in C.LOAD_SHAPES:
        d = C.load_path_depth(shape)
        assert d.shape == (3,) + shape and np.all(C.z32_rule(d, 1000.0, 3.0)[:, -1, -1] > 0)


def test_validity_rule_cases_tell_the_fp32_rule_from_fp64():
    """every code once; at (1000, 0.3) the fp32 rule (z = fl32(d / scale) against fl32(trunc)) has 299 valid codes and the rule with the
    quotient left in fp64 has 300: they differ at exactly d = 300 (fl32(0.3) > 0.3 = 300 / 1000).  With both the quotient and the threshold
    in fp64 the two rules agree again, so it is the rounding of z that the case pins."""
    d = C.every_code_depth()[0]
    assert np.array_equal(np.sort(d.ravel()), np.arange(65536))
    counts = {}
    for scale, trunc in C.RULES:
        v32 = C.z32_rule(d, scale, trunc) > 0
        v64 = C.z64_rule(d, scale, trunc) > 0
        counts[(scale, trunc)] = int(v32.sum())
        diff = sorted(d[v32 != v64].tolist())
        print(f"scale {scale} trunc {trunc}: {v32.sum()} valid codes under the fp32 rule, {v64.sum()} with the quotient in fp64, differ at {diff}")
        assert diff == ([300] if (scale, trunc) == (1000.0, 0.3) else [])
        assert np.array_equal(G.backproject(d, depth_scale=scale, depth_trunc=trunc)[1], np.flatnonzero(v32.ravel()))
        assert np.array_equal(v32, (d > 0) & (d.astype(np.float32) / np.float32(scale) < np.float32(trunc)))
    assert counts == {(1000.0, 3.0): 2999, (1000.0, 0.3): 299, (5000.0, 3.0): 14999, (256.0, 3.0): 767, (1000.0, 3.0e38): 65535}
    assert not (np.float64(300) / 1000.0 < 0.3) and np.float32(300) / np.float32(1000) >= np.float32(0.3)
    assert np.isfinite(np.float32(3.0e38))


def test_odd_intrinsics():
    for fx, fy, cx, cy in C.ODD_INTRINSICS:
        assert fx != fy and (cx < 0 or cx > 61) and (cy < 0 or cy > 37)
    assert any(k[2] < 0 for k in C.ODD_INTRINSICS) and any(k[3] < 0 for k in C.ODD_INTRINSICS)


# ---- C. bs_pixel_to_3d -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.PIXEL_SIZES)
def test_pixel_points(n):
    uvd = C.pixel_points(n)
    assert uvd.shape == (n, 3) and uvd.dtype == np.float64
    assert (uvd[:, 2] == 0).any() and (n == 1 or (uvd[:, 2] < 0).any())
    if n >= 4:
        assert np.signbit(uvd[3, 2]) and uvd[3, 2] == 0
    K = C.ODD_INTRINSICS[0]
    want = np.stack([G.pixel_to_3d(u, v, d, *K) for u, v, d in uvd])
    assert np.array_equal(C.pixel_statement(uvd, K).view(np.int64), want.view(np.int64))
