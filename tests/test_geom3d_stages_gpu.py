"""The four entry points of csrc/geom3d.hip -- bs_pose_chain, bs_pose_chain_from, bs_backproject, bs_pixel_to_3d -- on the inputs of
tests/_geom3d_cases.py: the wave and round borders of the pose scan, the one-lane fallback for a bottom row other than [0 0 0 1], a chain
continued on the device (separate buffers and in place), g0 blocks that are no rotations (all 16 golden ones, and rank-deficient ones),
a NaN; back-projection over two rounds of the chunk scan, on the thread / wave / chunk borders of the compaction, through both load paths
with a pose, under the fp32 validity rule for every depth code, with the tails of the outputs watched.  tests/test_geom3d_cases_cpu.py
shows on the CPU that every case is fair and reaches what it is built for.

References: the oracle's chain (oracle/geom3d_ref.py) within the bars held in _geom3d_cases.py (8 x the measured reassociation gap, at
least 1e-12); for back-projection and bs_pixel_to_3d the explicit-order numpy statements, bit for bit.  Every call runs twice and must
give the same bits."""
import numpy as np
import pytest
import torch

import _geom3d_cases as C
from oracle import geom3d_ref as G

pytestmark = pytest.mark.gpu

EYE_ROW = np.array([0.0, 0.0, 0.0, 1.0])


@pytest.fixture(scope="module")
def L():
    from bodyslam_amd import _lib
    _lib.init(0)
    return _lib


def dev():
    return torch.device("cuda:0")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def report(msg):
    print(msg)


# ---- A. pose chain ---------------------------------------------------------------------------------------------------------------------------
def run_chain(L, t_rel, g0):
    """bs_pose_chain twice into NaN-filled buffers -> float64 [N + 1, 4, 4]; the two runs must agree bit for bit"""
    N = len(t_rel)
    t = torch.from_numpy(np.array(t_rel, dtype=np.float32).reshape(N, 16)).to(dev())     # (a copy: the cases are read-only)
    runs = []
    for _ in range(2):
        out = torch.full((N + 1, 16), float("nan"), dtype=torch.float64, device=dev())
        L.pose_chain(t, N, None if g0 is None else np.asarray(g0, dtype=np.float64).reshape(16), out)
        runs.append(out.cpu().numpy().reshape(N + 1, 4, 4))
    assert same_bits(runs[0], runs[1]), "bs_pose_chain: two runs differ"
    return runs[0]


def check_chain(name, got):
    case = C.chain_case(name)
    g0 = np.eye(4) if case["g0"] is None else case["g0"]
    assert same_bits(got[0], g0), "pose 0 is not g0"
    err = float(np.abs(got - case["ref"]).max())
    report(f"{name}: max|err| vs the oracle {err:.2e} (bar {C.chain_bar(name):.1e})")
    assert np.isfinite(got).all() and err < C.chain_bar(name), (name, err)
    return err


@pytest.mark.parametrize("name", [f"len{N}-{k}" for N in C.LENGTHS for k in C.G0_KINDS])
def test_chain_lengths(L, name):
    """N on the wave (63 / 64 / 65) and round (255 / 256 / 257, 512 / 513) borders of pose_scan_kernel, elements that need their projection
    and reflections among them; g0 absent, a rotation, a general full-rank block.  The scan path writes every bottom row as [0 0 0 1]."""
    case = C.chain_case(name)
    got = run_chain(L, case["t_rel"], case["g0"])
    check_chain(name, got)
    assert np.all(got[1:, 3, :] == EYE_ROW)


@pytest.mark.parametrize("i", range(16))
def test_ensure_so3_v2_on_every_golden_matrix(L, i):
    """geom3d.ensure_so3_v2 (a g0 that is no rotation, one identity step) on all 16 matrices the oracle is pinned on"""
    from bodyslam_amd import geom3d
    so3_in, so3_out = C.so3_golden()
    R = geom3d.ensure_so3_v2(so3_in[i])
    assert same_bits(R, geom3d.ensure_so3_v2(so3_in[i]))
    err = float(np.abs(R - so3_out[i]).max())
    report(f"so3-{i}: max|err| {err:.2e}")
    assert err < C.chain_bar(f"so3-{i}")
    check_chain(f"so3-{i}", run_chain(L, C.chain_case(f"so3-{i}")["t_rel"], C.chain_case(f"so3-{i}")["g0"]))


FROM_CASE = "len513-rot"


def _steps():
    s = 0
    for n in C.FROM_STEPS:
        yield s, n
        s += n


def _from_separate(L, t, g0):
    g = torch.from_numpy(g0.reshape(16).copy()).to(dev())
    pieces = [g0.reshape(1, 16)]
    for s, n in _steps():
        out = torch.full((n + 1, 16), float("nan"), dtype=torch.float64, device=dev())
        assert g.data_ptr() != out.data_ptr()
        L.pose_chain_from(t[s:s + n], n, g, out)
        o = out.cpu().numpy()
        assert same_bits(o[0], g.cpu().numpy()), f"step at {s}: pose 0 of the step is not its g0"
        pieces.append(o[1:])
        g = out[n].clone()                                   # the next step's g0, in a buffer of its own
    return np.concatenate(pieces).reshape(-1, 4, 4)


def _from_in_place(L, t, g0):
    N = t.shape[0]
    buf = torch.full((N + 1, 16), float("nan"), dtype=torch.float64, device=dev())
    buf[0] = torch.from_numpy(g0.reshape(16).copy()).to(dev())
    for s, n in _steps():
        before = buf[s].cpu().numpy()
        assert buf[s].data_ptr() == buf[s:].data_ptr()       # g0_dev == g_abs: the branch without the copy
        L.pose_chain_from(t[s:s + n], n, buf[s], buf[s:])
        assert same_bits(buf[s].cpu().numpy(), before), f"step at {s}: its g0 slot was rewritten"
        assert torch.isnan(buf[s + n + 1:]).all(), f"step at {s}: poses behind the step were written"
    return buf.cpu().numpy().reshape(N + 1, 4, 4)


@pytest.mark.parametrize("form", ["separate", "in_place"])
def test_chain_continued_on_the_device(L, form):
    """bs_pose_chain_from: the N = 513 chain in steps of 64, 64, 128, 1 and 256 poses, the last pose of a step being the next step's g0 on
    the device -- handed over in a separate buffer, or in place, each step writing behind the previous one in a single [N + 1, 16] buffer
    (g0_dev == g_abs).  The concatenation is the oracle's single chain; pose 0 is g0 bit for bit."""
    case = C.chain_case(FROM_CASE)
    t = torch.from_numpy(case["t_rel"].reshape(-1, 16).copy()).to(dev())
    run = _from_separate if form == "separate" else _from_in_place
    got = run(L, t, case["g0"])
    assert same_bits(got, run(L, t, case["g0"])), "two runs differ"
    check_chain(FROM_CASE, got)
    assert np.all(got[1:, 3, :] == EYE_ROW)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_chain_from_a_device_g0_through_the_python_surface(L, dtype):
    """geom3d.pose_chain(t, g0=<cuda tensor>) takes bs_pose_chain_from; an fp32 tensor is widened, and is then no rotation any more (the
    oracle starts from the same widened matrix)"""
    from bodyslam_amd import geom3d
    case = C.chain_case(FROM_CASE)
    g0_t = torch.from_numpy(case["g0"].copy()).to(dtype).to(dev())
    g0 = g0_t.to(torch.float64).cpu().numpy()
    ref = case["ref"] if dtype == torch.float64 else G.pose_chain(case["t_rel"], g0)
    assert (dtype == torch.float64) == same_bits(g0, case["g0"])
    t = torch.from_numpy(case["t_rel"].copy()).to(dev())

    def run():
        g, pieces = g0_t, [g0[None]]
        for s, n in _steps():
            out = geom3d.pose_chain(t[s:s + n], g0=g)
            assert out.shape == (n + 1, 4, 4) and out.dtype == torch.float64 and out.is_cuda
            assert same_bits(out[0].cpu().numpy(), g.to(torch.float64).cpu().numpy())
            pieces.append(out[1:].cpu().numpy())
            g = out[n]
        return np.concatenate(pieces)
    got = run()
    assert same_bits(got, run()), "two runs differ"
    assert same_bits(got[0], g0)
    err = float(np.abs(got - ref).max())
    report(f"{FROM_CASE} from a {dtype} device g0: max|err| {err:.2e}")
    assert err < C.chain_bar(FROM_CASE)


@pytest.mark.parametrize("variant", C.NONAFFINE_VARIANTS)
def test_nonaffine_input_takes_the_strict_recurrence(L, variant):
    """N = 300 with one bottom row [0.1 0 0 1] (element 0, 70 or 299) or [0 0 0 2], or an affine t_rel behind a non-affine g0: the full
    4 x 4 product of the reference, bottom rows included.  (The scan path would write [0 0 0 1] into every bottom row.)"""
    name = f"nonaffine-{variant}"
    case = C.chain_case(name)
    got = run_chain(L, case["t_rel"], case["g0"])
    check_chain(name, got)
    first = {"row0": 0, "row70": 70, "row299": 299, "w2": 150, "g0": -1}[variant] + 1
    assert np.all(got[1:first, 3, :] == EYE_ROW)
    assert np.abs(got[max(first, 1):, 3, :] - EYE_ROW).max(axis=1).min() > 1e-3
    assert float(np.abs(got[:, 3, :] - case["ref"][:, 3, :]).max()) < C.chain_bar(name)


def test_affine_twin_takes_the_scan(L):
    """the same t_rel with the row restored: within the bar of the oracle, every bottom row exactly [0 0 0 1]"""
    name = f"affine-twin-{C.NONAFFINE_VARIANTS[0]}"
    case = C.chain_case(name)
    got = run_chain(L, case["t_rel"], case["g0"])
    check_chain(name, got)
    assert np.all(got[:, 3, :] == EYE_ROW)


@pytest.mark.parametrize("variant", C.RANK_VARIANTS)
def test_rank_deficient_g0_block(L, variant):
    """A block with an exactly zero singular value still yields a proper rotation (the Jacobi leaves a zero column in U; the projection
    completes the basis as LAPACK does).  Rank 2: the closest rotation is unique and is the oracle's.  Rank <= 1: any proper rotation that
    maps the dominant right singular vector onto the left one."""
    from bodyslam_amd import geom3d
    name = f"rank-{variant}"
    case = C.chain_case(name)
    M = C.rank_block(variant)
    got = run_chain(L, case["t_rel"], case["g0"])
    R = got[1, :3, :3]
    report(f"{name}: R =\n{R}")
    C.assert_proper_completion(R, M)
    assert same_bits(got[1, :3, 3], case["g0"][:3, 3]) and np.all(got[1, 3, :] == EYE_ROW) and same_bits(got[0], case["g0"])
    if variant in C.RANK2:
        check_chain(name, got)
    assert np.array_equal(geom3d.ensure_so3_v2(M), R)


def test_nan_stays_behind_its_pose(L):
    """a NaN in the step that makes pose 100 of 257: the call returns, poses 0 .. 99 are those of the chain without it bit for bit, and
    every later rotation block is non-finite"""
    k = C.NAN_POSE
    got = run_chain(L, C.chain_case("nan")["t_rel"], None)
    twin = run_chain(L, C.nan_twin(), None)
    assert same_bits(got[:k], twin[:k])
    assert not np.isfinite(got[k:, :3, :3]).any()
    assert np.isfinite(twin).all()


# ---- B. back-projection ------------------------------------------------------------------------------------------------------------------------
def to_dev_u16(depth):
    return torch.from_numpy(np.array(depth, dtype=np.uint16).view(np.int16)).to(dev())


def run_bp(L, d, K, scale, trunc, poses):
    """bs_backproject twice on the int16-stored device tensor d [B, H, W] (possibly a slice of a larger one): xyz pre-filled with NaN, idx
    with -1, the scratch sized as geom3d.backproject sizes it -> (xyz, idx, count) as numpy; the two runs must agree bit for bit"""
    assert d.is_contiguous() and d.dtype == torch.int16
    B, H, W = d.shape
    n = H * W
    pz = None if poses is None else torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64).reshape(B, 16)).to(dev())
    runs = []
    for _ in range(2):
        xyz = torch.full((B, n, 3), float("nan"), device=dev())
        idx = torch.full((B, n), -1, dtype=torch.int32, device=dev())
        cnt = torch.full((B,), -7, dtype=torch.int32, device=dev())
        scratch = torch.full((max(1, B * (n // 256 + 2)),), -3, dtype=torch.int32, device=dev())
        L.backproject(d, K, scale, trunc, pz, xyz, idx, cnt, scratch, B, H, W)
        runs.append((xyz.cpu().numpy(), idx.cpu().numpy(), cnt.cpu().numpy()))
    for a, b in zip(*runs):
        assert same_bits(a, b), "bs_backproject: two runs differ"
    return runs[0]


def check_bp(got, depth, K, scale, trunc, poses):
    """against the explicit-order statement, bit for bit; entries [count[b]:] of every image untouched"""
    xyz, idx, cnt = got
    assert cnt.dtype == np.int32 and idx.dtype == np.int32 and xyz.dtype == np.float32
    for b in range(depth.shape[0]):
        sx, si = C.bp_statement(depth[b], K, scale, trunc, None if poses is None else poses[b])
        m = len(si)
        assert int(cnt[b]) == m, (b, int(cnt[b]), m)
        assert np.array_equal(idx[b, :m], si), f"image {b}: indices"
        bad = np.flatnonzero((xyz[b, :m].view(np.int32) != sx.view(np.int32)).any(axis=1))
        assert bad.size == 0, f"image {b}: {bad.size} points differ from the statement, first at {bad[:3]}: {xyz[b, bad[:3]]} vs {sx[bad[:3]]}"
        assert np.all(idx[b, m:] == -1) and np.isnan(xyz[b, m:]).all(), f"image {b}: entries after count were written"
    return cnt


def bp_both(L, depth, K, scale=1000.0, trunc=3.0, poses=None):
    """with the poses and without"""
    d = to_dev_u16(depth)
    cnt = check_bp(run_bp(L, d, K, scale, trunc, None), depth, K, scale, trunc, None)
    if poses is not None:
        check_bp(run_bp(L, d, K, scale, trunc, poses), depth, K, scale, trunc, poses)
    return cnt


@pytest.mark.parametrize("shape", C.SCAN_SHAPES)
def test_backproject_over_two_scan_rounds(L, shape):
    """258 chunks per image (two rounds of bp_scan_kernel, the carry between them), and 256 chunks, the last shape of one round; image 0
    half valid, image 1 all valid; with poses.  526 339 and 526 851 pixels leave image 1 off the 16-byte boundary."""
    depth = C.scan_round_depth(shape)
    poses = C.bp_poses(2)
    d = to_dev_u16(depth)
    cnt = check_bp(run_bp(L, d, G.REF_INTRINSICS, 1000.0, 3.0, poses), depth, G.REF_INTRINSICS, 1000.0, 3.0, poses)
    assert int(cnt[1]) == shape[0] * shape[1]
    if shape == C.SCAN_SHAPES[0]:
        check_bp(run_bp(L, d, G.REF_INTRINSICS, 1000.0, 3.0, None), depth, G.REF_INTRINSICS, 1000.0, 3.0, None)


@pytest.mark.parametrize("pattern", C.BORDER_PATTERNS)
def test_backproject_compaction_borders(L, pattern):
    """one 3 x 2048 image per pattern: valid pixels only on the thread, wave and chunk borders; the first alone; the last alone; every
    second; all; none"""
    cnt = bp_both(L, C.border_depth(pattern), G.REF_INTRINSICS, poses=C.bp_poses(1))
    H, W = C.BORDER_SHAPE
    assert int(cnt[0]) == {"borders": 9, "first": 1, "last": 1, "alternate": H * W // 2, "all": H * W, "none": 0}[pattern]


def test_backproject_compaction_borders_as_one_batch(L):
    """the six patterns as one batch: every image has its own row of chunk offsets"""
    depth = np.concatenate([C.border_depth(p) for p in C.BORDER_PATTERNS])
    bp_both(L, depth, G.REF_INTRINSICS, poses=C.bp_poses(len(C.BORDER_PATTERNS)))


@pytest.mark.parametrize("shape", C.LOAD_SHAPES)
def test_backproject_load_paths_with_a_pose(L, shape):
    """B = 3 at (37, 61), (5, 8), (1, 1), (1, 7): with an odd pixel count the later images of a batch take the element path, and the last
    load of an image is ragged.  Once on the whole tensor, once on the slice [1:3] of it (the pipeline passes slices), whose base pointer is
    off the boundary that image 1 had in the whole batch only by the slice's offset: the same bits."""
    depth = C.load_path_depth(shape)
    poses = C.bp_poses(3)
    K = G.REF_INTRINSICS
    d = to_dev_u16(depth)
    whole = run_bp(L, d, K, 1000.0, 3.0, poses)
    check_bp(whole, depth, K, 1000.0, 3.0, poses)
    part = d[1:3]
    assert part.data_ptr() == d.data_ptr() + 2 * shape[0] * shape[1]
    sliced = run_bp(L, part, K, 1000.0, 3.0, poses[1:3])
    check_bp(sliced, depth[1:3], K, 1000.0, 3.0, poses[1:3])
    for a, b in zip(whole, sliced):
        assert same_bits(a[1:3], b)
    check_bp(run_bp(L, d, K, 1000.0, 3.0, None), depth, K, 1000.0, 3.0, None)


@pytest.mark.parametrize("scale,trunc", C.RULES)
def test_validity_rule_on_every_code(L, scale, trunc):
    """every code 0 .. 65535 in one frame: the valid set is the fp32 rule's exactly (at (1000, 0.3) code 300 is invalid; with the quotient in
    fp64 it would be valid).  bs_depth_u16_to_m restates the rule: bit-equal to the fp32 statement, and > 0 exactly where back-projection
    counted a pixel."""
    depth = C.every_code_depth()
    d = to_dev_u16(depth)
    got = run_bp(L, d, G.REF_INTRINSICS, scale, trunc, None)
    check_bp(got, depth, G.REF_INTRINSICS, scale, trunc, None)
    xyz, idx, cnt = got
    z32 = C.z32_rule(depth[0], scale, trunc)
    m = int(cnt[0])
    assert np.array_equal(idx[0, :m], np.flatnonzero(z32.ravel() > 0))
    assert m == {(1000.0, 3.0): 2999, (1000.0, 0.3): 299, (5000.0, 3.0): 14999, (256.0, 3.0): 767, (1000.0, 3.0e38): 65535}[(scale, trunc)]
    if (scale, trunc) == (1000.0, 0.3):
        assert 300 not in set(depth[0].ravel()[idx[0, :m]].tolist()) and 299 in set(depth[0].ravel()[idx[0, :m]].tolist())
    zm = L.depth_u16_to_m(d, scale, trunc).cpu().numpy()
    assert same_bits(zm, L.depth_u16_to_m(d, scale, trunc).cpu().numpy())
    assert zm.dtype == np.float32 and same_bits(zm[0], z32)
    assert np.array_equal(np.flatnonzero(zm[0].ravel() > 0), idx[0, :m])
    assert same_bits(xyz[0, :m, 2], z32.ravel()[idx[0, :m]])             # without a pose the third coordinate is z itself


@pytest.mark.parametrize("K", C.ODD_INTRINSICS)
def test_backproject_intrinsics(L, K):
    """fx != fy; the principal point outside the image, negative on one axis"""
    bp_both(L, C.load_path_depth((37, 61)), K, poses=C.bp_poses(3, seed=51))


# ---- C. bs_pixel_to_3d -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.PIXEL_SIZES)
def test_pixel_to_3d_across_the_block_border(L, n):
    """n on both sides of the 256-thread block; d = 0, -0.0 and negative among the points; bit-equal to ((u - cx) d) / fx, ((v - cy) d) / fy, d;
    rows behind n untouched"""
    uvd = C.pixel_points(n)
    u = torch.from_numpy(uvd).to(dev())
    for K in (G.REF_INTRINSICS, C.ODD_INTRINSICS[0]):
        runs = []
        for _ in range(2):
            out = torch.full((n + 3, 3), float("nan"), dtype=torch.float64, device=dev())
            L.pixel_to_3d(u, K, out, n)
            runs.append(out.cpu().numpy())
        assert same_bits(runs[0], runs[1])
        assert same_bits(runs[0][:n], C.pixel_statement(uvd, K))
        assert np.isnan(runs[0][n:]).all()
