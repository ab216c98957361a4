"""Every stage of csrc/odometry.hip in isolation against the fp64 statements (oracle/rgbd_odometry_ref.py,
tests/_point_to_plane_ref.py), and all four modes of the hybrid step.

A stage's reference is computed in fp64 from the device's OWN fp32 input to that stage (downloaded and upcast): nothing compounds,
so the bounds are those of one stage -- 1 fp32 ulp for the image stages, and for the 28 sums of a Gauss-Newton step 1e-9 of their
Cauchy-Schwarz scales (fp64 rounding and summation order, about N 2^-52 = 1.5e-11 at N = 66049, with 60x headroom), with EQUAL
inlier counts.  The inputs (tests/_odometry_inputs.py) populate every branch and keep every decision at least 1e-9 from its
boundary; tests/test_odometry_inputs_cpu.py asserts that from the statements alone, and the step tests re-assert the margin on the
maps the device actually built.  The measured worst ratios go to odometry_stages.txt in the suite's report directory."""
import ctypes as C
import os

import numpy as np
import pytest

import _odometry_inputs as X
import _point_to_plane_ref as P2P
from conftest import TWO_PROC
from oracle import rgbd_odometry_ref as R

pytestmark = pytest.mark.gpu

OUT = os.path.dirname(TWO_PROC["dir"])       # the suite's report directory (tests/conftest.py keeps the two-process run's files under it)
GATE, HUBER_D, HUBER_I = R.DEPTH_OUTLIER_TRUNC, R.DEPTH_HUBER, R.INTENSITY_HUBER
P2P_DIFF, P2P_HUBER = P2P.DEPTH_DIFF, P2P.DEPTH_HUBER
SUM_BOUND = 1e-9
CASES = [(hw, 1) for hw in X.STAGE_SIZES] + [((45, 61), 3)]
ident = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)
case_id = lambda c: f"{c[0][0]}x{c[0][1]}-batch{c[1]}"


def record(line):
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "odometry_stages.txt"), "a") as f:
        f.write(line + "\n")
    print(line)


# ---- plumbing: numpy <-> device, the C entry points ---------------------------------------------------------------------------------
def gpu():
    import torch
    from bodyslam_amd import _lib as L
    L.init(0)
    return torch, L, L.load_library(), torch.device("cuda:0")


def up(a):
    torch, _, _, dev = gpu()
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def down(t):
    return t.cpu().numpy()


def hp(a):
    return a.ctypes.data_as(C.c_void_p)


def k4(K):
    return np.array(K, dtype=np.float64)


def t12(T):
    return np.ascontiguousarray(np.asarray(T, dtype=np.float64)[:3].reshape(12))


def t44(v12):
    T = np.eye(4)
    T[:3] = np.asarray(v12).reshape(3, 4)
    return T


def scenes(hw, batch):
    """[batch] different (source colour, source depth, target colour, target depth)"""
    p = [X.pair(*hw, seed) for seed in range(batch)]
    return tuple(np.stack([q[i] for q in p]) for i in range(4))


def dev_prepare(colour, depth, depth_max):
    torch, L, lib, dev = gpu()
    n, H, W = depth.shape
    inten, d = torch.full((n, H, W), 7.0, device=dev), torch.full((n, H, W), 7.0, device=dev)
    c_in, d_in = up(colour), up(depth)                  # (named: both inputs stay allocated until the launch has run)
    L.check(lib.bs_odo_prepare(L.p(c_in), L.p(d_in), n, H, W, float(depth_max), L.p(inten), L.p(d), L.stream_ptr()), "bs_odo_prepare")
    torch.cuda.synchronize()
    return inten, d


def dev_p2p_prepare(depth, depth_max):
    torch, L, lib, dev = gpu()
    n, H, W = depth.shape
    d = torch.full((n, H, W), 7.0, device=dev)
    d_in = up(depth)
    L.check(lib.bs_odo_p2p_prepare(L.p(d_in), n, H, W, float(depth_max), L.p(d), L.stream_ptr()), "bs_odo_p2p_prepare")
    torch.cuda.synchronize()
    return d


def dev_pyrdown(img, is_depth, thr):
    torch, L, lib, dev = gpu()
    n, H, W = img.shape
    out = torch.full((n, (H + 1) // 2, (W + 1) // 2), 7.0, device=dev)
    L.check(lib.bs_odo_pyrdown(L.p(img), n, H, W, L.p(out), int(is_depth), float(thr), L.stream_ptr()), "bs_odo_pyrdown")
    return out


def dev_sobel(img):
    torch, L, lib, dev = gpu()
    n, H, W = img.shape
    gx, gy = torch.full((n, H, W), 7.0, device=dev), torch.full((n, H, W), 7.0, device=dev)
    L.check(lib.bs_odo_sobel(L.p(img), n, H, W, L.p(gx), L.p(gy), L.stream_ptr()), "bs_odo_sobel")
    return gx, gy


def dev_target(depth, K):
    torch, L, lib, dev = gpu()
    n, H, W = depth.shape
    rec = torch.full((n, H, W, 4), 7.0, device=dev)
    Kc = k4(K)
    L.check(lib.bs_odo_p2p_target(L.p(depth), n, H, W, hp(Kc), L.p(rec), L.stream_ptr()), "bs_odo_p2p_target")
    torch.cuda.synchronize()
    return rec


def sum_buffers(batch):
    """(partial, out29) filled with NaN: an entry a kernel forgets to write shows"""
    torch, _, _, dev = gpu()
    return (torch.full((batch, 256, 29), float("nan"), dtype=torch.float64, device=dev),
            torch.full((batch, 29), float("nan"), dtype=torch.float64, device=dev))


def assert_ulp(got, ref64, what, ulps=1):
    """NaN masks equal; elsewhere got within `ulps` fp32 ulp of float32(ref64)"""
    assert got.dtype == np.float32 and got.shape == ref64.shape, what
    nan = np.isnan(ref64)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN mask differs at {np.argwhere(np.isnan(got) != nan)[:5].tolist()}"
    ref = ref64.astype(np.float32)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))[~nan]
    tol = ulps * np.spacing(np.abs(ref[~nan])).astype(np.float64)
    assert (err <= tol).all(), f"{what}: {int((err > tol).sum())} values beyond {ulps} ulp, worst {float((err / tol).max()):.1f}"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the image stages ---------------------------------------------------------------------------------------------------------------
def edge_depths(depth):
    """d == depth_max (valid) and the next fp32 above it (invalid), in every image"""
    depth = depth.copy()
    depth[:, 0, 0] = np.float32(X.DEPTH_MAX)
    depth[:, 0, 1] = np.nextafter(np.float32(X.DEPTH_MAX), np.float32(np.inf))
    return depth


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_prepare(case):
    hw, batch = case
    colour, depth, _, _ = scenes(hw, batch)
    depth = edge_depths(depth)
    assert np.float64(np.float32(X.DEPTH_MAX)) == X.DEPTH_MAX
    inten, d = (down(t) for t in dev_prepare(colour, depth, X.DEPTH_MAX))
    d2 = down(dev_p2p_prepare(depth, X.DEPTH_MAX))
    d3 = down(dev_p2p_prepare(depth, 3.0e38))
    for i in range(batch):
        ri, rd = R.prepare(colour[i], depth[i], X.DEPTH_MAX)
        assert_ulp(inten[i], ri, f"intensity of image {i}")
        assert_ulp(d[i], rd, f"depth of image {i}")
        assert not np.isnan(d[i][0, 0]) and np.isnan(d[i][0, 1])
        assert_ulp(d2[i], P2P.prepare_source(depth[i], X.DEPTH_MAX), f"point-to-plane source depth of image {i}")
        assert_ulp(d3[i], P2P.prepare_target(depth[i]), f"point-to-plane target depth of image {i}")
        valid = ~np.isnan(rd)
        assert np.array_equal(bits(d[i])[valid], bits(depth[i])[valid])          # a valid depth passes through untouched


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_pyrdown_both_modes(case):
    """two pyramid steps where the size allows; every step's reference from the device's own input to it"""
    hw, batch = case
    colour, depth, _, _ = scenes(hw, batch)
    inten, d = dev_prepare(colour, depth, X.DEPTH_MAX)
    thresholds = sorted({2 * GATE, 2 * P2P_DIFF, 0.05})          # the product's (both paths pass 2 * 0.07), and one that is not the default
    for step in range(2):
        n, H, W = d.shape
        if H < 2 or W < 2:
            break
        i_in, d_in = down(inten).astype(np.float64), down(d).astype(np.float64)
        i_out = dev_pyrdown(inten, False, 0.0)
        d_outs = [dev_pyrdown(d, True, thr) for thr in thresholds]
        assert tuple(i_out.shape) == (n, (H + 1) // 2, (W + 1) // 2) == tuple(d_outs[0].shape)
        for i in range(batch):
            assert_ulp(down(i_out)[i], R.pyr_down(i_in[i]), f"intensity level {step + 1} of image {i}")
            for thr, got in zip(thresholds, d_outs):
                assert_ulp(down(got)[i], R.pyr_down_depth(d_in[i], thr), f"depth level {step + 1} (thr {thr}) of image {i}")
        inten, d = i_out, d_outs[thresholds.index(2 * GATE)]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_sobel(case):
    hw, batch = case
    colour, depth, _, _ = scenes(hw, batch)
    inten, d = dev_prepare(colour, depth, X.DEPTH_MAX)
    for name, img in (("intensity", inten), ("depth", d)):
        gx, gy = (down(t) for t in dev_sobel(img))
        src = down(img).astype(np.float64)
        for i in range(batch):
            rx, ry = R.sobel(src[i])
            assert_ulp(gx[i], rx, f"d/dx of {name}, image {i}")
            assert_ulp(gy[i], ry, f"d/dy of {name}, image {i}")
    if min(hw) >= 8:
        assert np.isnan(down(d)).any()


def check_target(rec, depth, K, what):
    """one image's records [H, W, 4] against vertex_map / normal_map of the fp32 depth [H, W] they were built from"""
    assert np.array_equal(bits(rec[..., 3]), bits(depth)), f"{what}: w is not the input depth"
    N = P2P.normal_map(P2P.vertex_map(depth.astype(np.float64), K))
    nan = np.isnan(N)
    assert nan[-1].all() and nan[:, -1].all()
    assert np.array_equal(np.isnan(rec[..., :3]), nan), f"{what}: the normal's NaN mask differs"
    assert (nan.all(-1) | ~nan.any(-1)).all()
    err = np.abs(rec[..., :3].astype(np.float64) - N)[~nan]
    assert err.size == 0 or err.max() <= 2.4e-7, f"{what}: normal off by {err.max():.2e}"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_p2p_target(case):
    hw, batch = case
    _, _, _, depth = scenes(hw, batch)
    K = X.intrinsics(*hw)
    d = dev_p2p_prepare(depth, 3.0e38)
    rec, d_in = down(dev_target(d, K)), down(d)
    for i in range(batch):
        check_target(rec[i], d_in[i], K, f"image {i}")
    if min(hw) >= 8:        # valid pixels whose right or lower neighbour is not
        valid = ~np.isnan(d_in[0])
        assert (valid[:-1, :-1] & (~valid[:-1, 1:] | ~valid[1:, :-1])).sum() >= 5


def test_depth_u16_to_m():
    torch, L, lib, dev = gpu()
    u16 = np.arange(65536, dtype=np.uint16)
    t = up(u16.view(np.int16))
    z = u16.astype(np.float32) / np.float32(1000.0)
    for trunc in (3.0, 3.0e38):
        want = np.where(z >= np.float32(trunc), np.float32(0.0), z)
        assert np.array_equal(bits(down(L.depth_u16_to_m(t, 1000.0, trunc))), bits(want)), trunc
    assert (want > 0).sum() == 65535
    # an empty call: no launch, nothing written; an empty tensor (null pointers) is fine
    out = torch.full((8,), 7.0, device=dev)
    L.check(lib.bs_depth_u16_to_m(L.p(t), 0, 1000.0, 3.0, L.p(out), L.stream_ptr()), "bs_depth_u16_to_m")
    assert (down(out) == 7.0).all()
    empty = L.depth_u16_to_m(torch.empty((0, 4, 5), dtype=torch.int16, device=dev), 1000.0, 3.0)
    assert tuple(empty.shape) == (0, 4, 5) and empty.dtype == torch.float32


# ---- one Gauss-Newton step's sums -----------------------------------------------------------------------------------------------------
_maps = {}


def step_maps(hw, batch=1):
    """built ONCE per size on the device, through the stages tested above: the source's (I, D), the target's six maps, the
    point-to-plane source depth and target records -- device tensors [batch, H, W(, 4)] and their downloads"""
    key = (hw, batch)
    if key not in _maps:
        cs, ds, ct, dt = scenes(hw, batch)
        K = X.intrinsics(*hw)
        Is, Ds = dev_prepare(cs, ds, X.DEPTH_MAX)
        It, Dt = dev_prepare(ct, dt, X.DEPTH_MAX)
        dev = dict(Is=Is, Ds=Ds, It=It, Dt=Dt, p2p_src=dev_p2p_prepare(ds, X.DEPTH_MAX))
        dev["gIx"], dev["gIy"] = dev_sobel(It)
        dev["gDx"], dev["gDy"] = dev_sobel(Dt)
        dev["p2p_tgt"] = dev_p2p_prepare(dt, 3.0e38)
        dev["rec"] = dev_target(dev["p2p_tgt"], K)
        host = {k: down(v) for k, v in dev.items()}
        for v in host.values():
            v.setflags(write=False)
        _maps[key] = (K, dev, host)
    return _maps[key]


def hybrid_inputs(host, K, i=0):
    return dict(K=K, src=(host["Is"][i], host["Ds"][i]), tgt=tuple(host[k][i] for k in ("It", "Dt", "gIx", "gIy", "gDx", "gDy")))


def dev_accumulate(dev, i, hw, K, T, flags):
    torch, L, lib, _ = gpu()
    partial, out = sum_buffers(1)
    Kc, Tc = k4(K), t12(T)
    L.check(lib.bs_odo_accumulate(*(L.p(dev[k][i]) for k in ("Is", "Ds", "It", "Dt", "gIx", "gIy", "gDx", "gDy")), hw[0], hw[1], hp(Kc), hp(Tc),
                                  GATE, HUBER_D, HUBER_I, L.p(partial), L.p(out), flags, L.stream_ptr()), "bs_odo_accumulate")
    return down(out)[0]


def dev_p2p_accumulate(dev, i, hw, K, T):
    torch, L, lib, _ = gpu()
    partial, out = sum_buffers(1)
    Kc, Tc = k4(K), t12(T)
    L.check(lib.bs_odo_p2p_accumulate(L.p(dev["p2p_src"][i]), L.p(dev["rec"][i]), hw[0], hw[1], hp(Kc), hp(Tc), P2P_DIFF, P2P_HUBER, L.p(partial),
                                      L.p(out), L.stream_ptr()), "bs_odo_p2p_accumulate")
    return down(out)[0]


def sums_ratio(got29, ref):
    """(worst |difference| / Cauchy-Schwarz scale over the 28 sums, device inlier count, reference inlier count)"""
    A, b, cost, n = ref
    sA, sb, sc = X.sum_bounds(A, cost)
    assert np.isfinite(got29).all()
    ratio = max((np.abs(got29[:21] - X.upper(A)) / sA).max(), (np.abs(got29[21:27] - b) / sb).max(), abs(got29[27] - cost) / sc)
    return float(ratio), int(round(got29[28])), n


@pytest.mark.parametrize("flags", range(4), ids=lambda f: "-".join(X.MODES[f]))
@pytest.mark.parametrize("hw", X.SIZES, ids=ident)
def test_accumulate_all_four_modes(hw, flags):
    association, loss = X.MODES[flags]
    K, dev, host = step_maps(hw)
    inp = hybrid_inputs(host, K)
    worst = 0.0
    for name in X.POSES:
        T = X.pose(name)
        cs = X.census(*inp["src"], inp["tgt"][0], inp["tgt"][1], inp["tgt"][2:], K, T, association)
        assert cs["margin"] >= 1e-9, (name, cs["margins"])              # on the device's own maps, as on the statement's (the CPU file)
        ref = X.hybrid_reference(inp, T, association, loss)
        ratio, n_dev, n_ref = sums_ratio(dev_accumulate(dev, 0, hw, K, T, flags), ref)
        print(f"{hw} flags {flags} {name}: inliers {n_dev} / {n_ref} (second trip {cs['counts']['inlier_second_trip']}), worst ratio {ratio:.2e}")
        assert n_dev == n_ref == cs["counts"]["inlier"] and n_ref >= 20
        assert ratio <= SUM_BOUND, (name, ratio)
        worst = max(worst, ratio)
    record(f"bs_odo_accumulate flags {flags} ({association} + {loss}) {hw[0]}x{hw[1]}: worst |difference| / Cauchy-Schwarz scale over "
           f"{len(X.POSES)} poses = {worst:.2e} (bound {SUM_BOUND:.0e})")


@pytest.mark.parametrize("hw", X.SIZES, ids=ident)
def test_p2p_accumulate(hw):
    K, dev, host = step_maps(hw)
    check_target(host["rec"][0], host["p2p_tgt"][0], K, "the step's target records")
    Ds, Dt, Nt = host["p2p_src"][0], host["rec"][0][..., 3], host["rec"][0][..., :3]
    worst = 0.0
    for name in X.POSES:
        T = X.pose(name)
        cs = X.census_p2p(Ds, Dt, Nt, K, T, P2P_DIFF, P2P_HUBER)
        assert cs["margin"] >= 1e-9, (name, cs["margins"])
        ref = X.p2p_reference(Ds, Dt, Nt, K, T)
        ratio, n_dev, n_ref = sums_ratio(dev_p2p_accumulate(dev, 0, hw, K, T), ref)
        print(f"{hw} point-to-plane {name}: inliers {n_dev} / {n_ref} (second trip {cs['counts']['inlier_second_trip']}), worst ratio {ratio:.2e}")
        assert n_dev == n_ref == cs["counts"]["inlier"] and n_ref >= 20
        assert ratio <= SUM_BOUND, (name, ratio)
        worst = max(worst, ratio)
    record(f"bs_odo_p2p_accumulate {hw[0]}x{hw[1]}: worst |difference| / Cauchy-Schwarz scale over {len(X.POSES)} poses = {worst:.2e} "
           f"(bound {SUM_BOUND:.0e})")


# ---- the device loop against the host loop ------------------------------------------------------------------------------------------------
LOOP_HW, LOOP_BATCH, LOOP_ITERS = (45, 61), 3, 2


def loop_starts():
    return [R.se3_exp(np.array(X.HAIR)), X.pose("small"), X.pose("sideways")]


def solve_update(got29, T):
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = got29[:21]
    A = A + np.triu(A, 1).T
    return R.se3_exp(np.linalg.solve(A + 1e-12 * np.eye(6), -got29[21:27])) @ T


def sparse_stack(dev, key, hw):
    """a two-pair stack: pair 0 = a source with exactly 5 valid pixels, pair 1 = pair 0 of the batch of three"""
    torch, _, _, _ = gpu()
    _, d = X.sparse_source(*hw, 0)
    sparse = dev_p2p_prepare(d[None], X.DEPTH_MAX)          # (the same rule as bs_odo_prepare's depth: tested above)
    assert int((~np.isnan(down(sparse))).sum()) == 5
    return torch.cat([sparse, dev[key][:1]]).contiguous()


@pytest.mark.parametrize("flags", range(4), ids=lambda f: "-".join(X.MODES[f]))
def test_device_loop_equals_host_loop(flags):
    torch, L, lib, _ = gpu()
    hw = LOOP_HW
    K, dev, host = step_maps(hw, LOOP_BATCH)
    Kc, starts = k4(K), loop_starts()
    names = ("Is", "Ds", "It", "Dt", "gIx", "gIy", "gDx", "gDy")

    def device_loop(maps, start, iters=LOOP_ITERS):
        n = len(start)
        partial, out = sum_buffers(n)
        T = up(np.stack([t12(s) for s in start]))
        L.check(lib.bs_odo_step(*(L.p(maps[k]) for k in names), n, hw[0], hw[1], hp(Kc), L.p(T), iters, GATE, HUBER_D, HUBER_I, L.p(partial),
                                L.p(out), flags, L.stream_ptr()), "bs_odo_step")
        return down(T), down(out)

    T_dev, out_dev = device_loop(dev, starts)
    for i in range(LOOP_BATCH):
        T = starts[i]
        for _ in range(LOOP_ITERS):
            s = dev_accumulate(dev, i, hw, K, T, flags)
            assert s[28] >= 6, (i, s[28])
            T = solve_update(s, T)
        d = np.abs(t44(T_dev[i]) - T).max()
        print(f"flags {flags} pair {i}: |T_device - T_host| = {d:.2e}, inliers of the last step {int(out_dev[i][28])}")
        assert d < 1e-9, (i, d)
        assert out_dev[i][28] == s[28]
    T_again, out_again = device_loop(dev, starts)
    assert np.array_equal(T_again, T_dev) and np.array_equal(out_again, out_dev)
    # one step's sums are the accumulate entry's at the same pose, bit for bit: both entries reduce the partials with one kernel
    out_one = device_loop(dev, starts, iters=1)[1]
    for i in range(LOOP_BATCH):
        assert np.array_equal(out_one[i], dev_accumulate(dev, i, hw, K, starts[i], flags)), i
    # a source with 5 valid pixels: no solve, the pose comes back bit for bit; its neighbour in the batch is untouched by that
    two = {k: torch.cat([dev[k][:1], dev[k][:1]]).contiguous() for k in names}
    two["Ds"] = sparse_stack(dev, "Ds", hw)
    T2, out2 = device_loop(two, [starts[0], starts[0]])
    assert np.array_equal(T2[0], t12(starts[0])), "the pose of a pair with fewer than 6 inliers moved"
    inp = hybrid_inputs(host, K)
    inp["src"] = (inp["src"][0], down(two["Ds"])[0])
    n_ref = X.hybrid_reference(inp, starts[0], *X.MODES[flags])[3]
    print(f"flags {flags}: 5 valid source pixels, inliers {int(out2[0][28])} / {n_ref}")
    assert out2[0][28] == n_ref and 1 <= n_ref < 6
    assert np.array_equal(T2[1], T_dev[0]) and np.array_equal(out2[1], out_dev[0])


def test_p2p_device_loop_equals_host_loop():
    torch, L, lib, _ = gpu()
    hw = LOOP_HW
    K, dev, host = step_maps(hw, LOOP_BATCH)
    Kc, starts = k4(K), loop_starts()

    def device_loop(src, rec, start, iters=LOOP_ITERS):
        n = len(start)
        partial, out = sum_buffers(n)
        T = up(np.stack([t12(s) for s in start]))
        L.check(lib.bs_odo_p2p_step(L.p(src), L.p(rec), n, hw[0], hw[1], hp(Kc), L.p(T), iters, P2P_DIFF, P2P_HUBER, L.p(partial), L.p(out),
                                    L.stream_ptr()), "bs_odo_p2p_step")
        return down(T), down(out)

    T_dev, out_dev = device_loop(dev["p2p_src"], dev["rec"], starts)
    for i in range(LOOP_BATCH):
        check_target(host["rec"][i], host["p2p_tgt"][i], K, f"target records of pair {i}")
        T = starts[i]
        for _ in range(LOOP_ITERS):
            s = dev_p2p_accumulate(dev, i, hw, K, T)
            assert s[28] >= 6, (i, s[28])
            T = solve_update(s, T)
        d = np.abs(t44(T_dev[i]) - T).max()
        print(f"point-to-plane pair {i}: |T_device - T_host| = {d:.2e}, inliers of the last step {int(out_dev[i][28])}")
        assert d < 1e-9, (i, d)
        assert out_dev[i][28] == s[28]
    T_again, out_again = device_loop(dev["p2p_src"], dev["rec"], starts)
    assert np.array_equal(T_again, T_dev) and np.array_equal(out_again, out_dev)
    out_one = device_loop(dev["p2p_src"], dev["rec"], starts, iters=1)[1]          # as in the hybrid test: one step's sums, bit for bit
    for i in range(LOOP_BATCH):
        assert np.array_equal(out_one[i], dev_p2p_accumulate(dev, i, hw, K, starts[i])), i
    src2 = sparse_stack(dev, "p2p_src", hw)
    rec2 = torch.cat([dev["rec"][:1], dev["rec"][:1]]).contiguous()
    T2, out2 = device_loop(src2, rec2, [starts[0], starts[0]])
    assert np.array_equal(T2[0], t12(starts[0])), "the pose of a pair with fewer than 6 inliers moved"
    n_ref = X.p2p_reference(down(src2)[0], host["rec"][0][..., 3], host["rec"][0][..., :3], K, starts[0])[3]
    print(f"point-to-plane: 5 valid source pixels, inliers {int(out2[0][28])} / {n_ref}")
    assert out2[0][28] == n_ref and 1 <= n_ref < 6
    assert np.array_equal(T2[1], T_dev[0]) and np.array_equal(out2[1], out_dev[0])


# ---- the public loss= argument, end to end -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["full", "short"])
@pytest.mark.parametrize("association,loss", [("nearest", "irls"), ("bilinear", "o3d")])
def test_public_loss_argument(association, loss, schedule):
    """the two modes no caller of the suite ever asked for, through RGBDOdometry itself, on a pair whose robust terms are live.  The
    bound on T is the association's (test_matches_oracle_and_truth).  Under the full schedule both losses reach the same fixed point
    (they share their right-hand side); the short schedule stops where the statement's poses for the two losses are more than ten
    bounds apart (tests/test_odometry_inputs_cpu.py), so the loss that ran is the one that was asked for.
    Measured |T - T_oracle|: nearest + irls 2.0e-8 (full) and 8.4e-9 (short) against 5e-5; bilinear + o3d 6.0e-10 (full) and 1.8e-6
    (short) against 2e-6 -- the short run stops two steps after the coarsest level, where the fp32 rounding of the pyramid has not
    been iterated away yet."""
    from bodyslam_amd.rgbd_odometry import FLAG_NEAREST, FLAG_O3D_LOSS, RGBDOdometry
    cs, ds, ct, dt = X.loss_pair(association)
    odo = RGBDOdometry(X.LOSS_K, association=association, loss=loss, iterations=X.LOSS_SCHEDULES[schedule])
    assert odo.flags == (FLAG_NEAREST if association == "nearest" else 0) | (FLAG_O3D_LOSS if loss == "o3d" else 0) == X.MODES.index((association, loss))
    T_ref, trace = X.loss_reference(association, loss, schedule)
    T = odo.estimate(cs, ds, ct, dt, X.LOSS_DEPTH_MAX, trace=True)
    assert len(odo.last_trace) == len(trace) == sum(X.LOSS_SCHEDULES[schedule])
    assert [s[0] for s in odo.last_trace] == [s[0] for s in trace]
    T_loop = odo.estimate(cs, ds, ct, dt, X.LOSS_DEPTH_MAX)                 # the product path: the loop on the device
    d, d_loop = np.abs(T - T_ref).max(), np.abs(T_loop - T_ref).max()
    other = X.loss_reference(association, "irls" if loss == "o3d" else "o3d", schedule)[0]
    print(f"{association} + {loss}, {schedule} schedule: |T - T_oracle| = {d:.2e} (device loop {d_loop:.2e}), bound {X.LOSS_BOUND[association]:.0e}; "
          f"from the other loss's pose: {np.abs(T - other).max():.2e}")
    assert d < X.LOSS_BOUND[association] and d_loop < X.LOSS_BOUND[association]
