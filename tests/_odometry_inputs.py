"""Adversarial inputs for the odometry kernels (csrc/odometry.hip) and a census of the decisions the fp64 statements
(oracle/rgbd_odometry_ref.py, tests/_point_to_plane_ref.py) take on them -- TEST INFRASTRUCTURE ONLY, numpy only.

The rendered scene of tests/_render.py is smooth: it never rejects a valid pyramid tap, never reaches a Huber delta and leaves
the outlier gate, the ``pz <= 0`` branch and three image borders almost empty.  ``scene`` is built to populate all of them;
``census`` counts, per outcome, the source pixels of one Gauss-Newton step and measures how far the nearest deciding quantity sits
from its boundary, so that tests/test_odometry_inputs_cpu.py can assert -- from the statements alone -- that every branch is
populated and that no decision hangs on the last bits of a double (where device and numpy arithmetic may differ).
tests/test_odometry_stages_gpu.py then requires EQUAL inlier counts and sums within fp64 summation error."""
import numpy as np

import _point_to_plane_ref as P2P
from oracle import rgbd_odometry_ref as R

HAIR = (3e-4, -2e-4, 1e-4, 2e-4, 1e-4, -1e-4)          # a start a hair off the identity: no projection exactly on a pixel or border
DEPTH_MAX = 1.25                      # exact in fp32; the scene's depths lie on both sides of it
SIZES = ((45, 61), (257, 257))        # odd by odd (23x31 and 12x16 below it); the smallest odd size with more than 65536 pixels
STAGE_SIZES = ((2, 2), (2, 3), (17, 16), (45, 61), (257, 257))
GRID_PIXELS = 256 * 256               # pixels of one trip of the accumulate kernels' grid-stride loop (ODO_GRID blocks of 256)
MODES = (("bilinear", "irls"), ("nearest", "irls"), ("bilinear", "o3d"), ("nearest", "o3d"))       # index = the kernels' `flags`

# source -> target poses (twists of R.se3_exp: omega, nu).  No single pose populates every outcome:
#   small     the issue's moderate motion: most inliers, both Huber deltas and the gate
#   backward  a moderate backward translation: the near part of the scene falls behind the camera, the rest spreads over all four
#             borders, and the far part still lands on the target
#   sideways  a turn that pushes a band of the image out on one side and brings the step edge across many pixels
POSES = {
    "small": (0.01, -0.02, 0.015, 0.03, -0.02, 0.01),
    "backward": (-0.02, 0.03, 0.01, -0.02, 0.02, -0.14),
    "sideways": (-0.06, 0.11, 0.04, -0.05, 0.04, 0.02),
}


def intrinsics(H, W):
    return (0.9 * W, 0.9 * W, W / 2 - 0.3, H / 2 + 0.2)


def pose(name):
    return R.se3_exp(np.array(POSES[name], dtype=np.float64))


def _blur121(a):
    p = np.pad(a, ((1, 1), (0, 0), (0, 0)), mode="edge")
    a = (p[:-2] + 2.0 * p[1:-1] + p[2:]) / 4.0
    p = np.pad(a, ((0, 0), (1, 1), (0, 0)), mode="edge")
    return (p[:, :-2] + 2.0 * p[:, 1:-1] + p[:, 2:]) / 4.0


def scene(H, W, seed):
    """(colour u8 [H, W, 3], depth fp32 [H, W] in metres, 0 / negative = no measurement)"""
    rng = np.random.default_rng(1000 + seed)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = 0.8 + 0.15 * np.sin(u / 7.0 + 0.9 * seed) + 0.1 * np.cos(v / 5.0 - 0.4 * seed)
    d[v >= int(0.6 * H)] += 0.3                                        # a step > 0.14 m across a row; beyond it depths pass DEPTH_MAX
    if W >= 8:
        c0 = int(0.8 * W)
        d[:, c0:c0 + 3] = 0.12 + 0.01 * np.sin(v[:, c0:c0 + 3] / 3.0)    # a near pole: steps across columns, and the pixels a backward motion puts behind the camera
    spikes = rng.random((H, W)) < 0.03                                 # isolated spikes that straddle 0.05 (Huber), 0.07 (gate), 0.14 (pyramid)
    d = d + spikes * rng.choice([-1.0, 1.0], (H, W)) * rng.uniform(0.03, 0.2, (H, W))
    holes = rng.random((H, W)) < 0.04
    if H >= 8 and W >= 8:
        d[2 * (H // 8), 2 * (W // 8)] -= 0.25                          # an even pixel more than 0.14 m from its whole 5x5 neighbourhood
        holes[2 * (H // 8) - 2:2 * (H // 8) + 3, 2 * (W // 8) - 2:2 * (W // 8) + 3] = False
        a, b = H // 3, W // 3
        holes[0:2, b:b + W // 6 + 1] = True                            # holes on all four borders ...
        holes[H - 2:, b:b + W // 6 + 1] = True
        holes[a:a + H // 6 + 1, 0:2] = True
        holes[a:a + H // 6 + 1, W - 2:] = True
        holes[H - 3:, W - 3:] = True                                   # ... and in the corner the odd sizes clamp at
    d[holes] = np.where(rng.random((H, W)) < 0.25, -1.0, 0.0)[holes]   # `<= 0` is invalid, not only `== 0`
    noise = _blur121(rng.integers(0, 256, (H, W, 3)).astype(np.float64))
    smooth = 40.0 * np.stack([np.sin(u / 9.0 + seed), np.cos(v / 6.0), np.sin((u + v) / 11.0)], -1)
    colour = np.clip(np.rint(0.8 * noise + 25.0 + smooth), 0, 255).astype(np.uint8)
    return colour, d.astype(np.float32)


def pair(H, W, seed):
    """(source colour, source depth, target colour, target depth): the target is the scene seen a little brighter and 0.4 % farther,
    with holes of its own -- source and target maps differ everywhere, so a kernel that confuses them shows"""
    cs, ds = scene(H, W, seed)
    rng = np.random.default_rng(2000 + seed)
    ct = np.clip(cs.astype(np.int32) + 6, 0, 255).astype(np.uint8)
    dt = (ds * np.float32(1.004)).astype(np.float32)
    dt[rng.random((H, W)) < 0.02] = 0.0
    return cs, ds, ct, dt


def sparse_source(H, W, seed, valid=5):
    """pair(H, W, seed)'s source with all but `valid` depths removed: fewer than 6 inliers, whatever the pose.  The survivors sit where
    the target is valid and smooth over the 5x5 pixels around them, so near the identity they ARE inliers in every mode"""
    colour, d, _, dt = pair(H, W, seed)
    ok = (dt > 0) & (dt <= DEPTH_MAX)
    t = np.where(ok, dt, np.nan).astype(np.float64)
    p = np.pad(t, 2, constant_values=np.nan)
    nb = np.stack([p[a:a + H, b:b + W] for a in range(5) for b in range(5)])
    calm = ~np.isnan(nb).any(0) & (np.nanmax(np.where(np.isnan(nb), 0.0, nb), 0) - np.nanmin(np.where(np.isnan(nb), 9.0, nb), 0) < 0.05)
    keep = np.flatnonzero(calm & (d > 0) & (d <= DEPTH_MAX) & (np.abs(d - dt) < 0.02))
    keep = keep[np.linspace(0, len(keep) - 1, valid).astype(int)]
    out = np.zeros_like(d)
    out.ravel()[keep] = d.ravel()[keep]
    return colour, out


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def level0(colour, depth, depth_max=DEPTH_MAX):
    """the six fp32 maps of one frame at full resolution as the statement gives them, every stage rounded to fp32 as the device
    stores it: (I, D, gIx, gIy, gDx, gDy)"""
    inten, d = R.prepare(colour, depth, depth_max)
    inten, d = f32(inten), f32(d)
    gix, giy = R.sobel(inten.astype(np.float64))
    gdx, gdy = R.sobel(d.astype(np.float64))
    return inten, d, f32(gix), f32(giy), f32(gdx), f32(gdy)


def _project(Ds, K, T):
    fx, fy, cx, cy = K
    H, W = Ds.shape
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    valid = ~np.isnan(Ds)
    z = np.where(valid, Ds, 1.0)
    X, Y = (u - cx) * z / fx, (v - cy) * z / fy
    px = T[0, 0] * X + T[0, 1] * Y + T[0, 2] * z + T[0, 3]
    py = T[1, 0] * X + T[1, 1] * Y + T[1, 2] * z + T[1, 3]
    pz = T[2, 0] * X + T[2, 1] * Y + T[2, 2] * z + T[2, 3]
    front = valid & (pz > 0)
    pzs = np.where(front, pz, 1.0)
    uf, vf = np.where(front, fx * px / pzs + cx, 0.0), np.where(front, fy * py / pzs + cy, 0.0)
    return valid, front, px, py, pz, uf, vf


def _round_half_away(a):
    return np.sign(a) * np.floor(np.abs(a) + 0.5)


def _min(a, mask):
    return float(np.min(a[mask])) if mask.any() else np.inf


def _association(front, uf, vf, H, W, nearest, margins):
    """(inside, out-left, out-right, out-top, out-bottom, sampler) and the margins of the decisions taken here"""
    if nearest:
        ur, vr = _round_half_away(uf), _round_half_away(vf)
        left, right, top, bottom = front & (ur < 0), front & (ur > W - 1), front & (vr < 0), front & (vr > H - 1)
        inside = front & ~(left | right | top | bottom)
        # a point whose OTHER coordinate is more than a pixel outside is out whichever way this one rounds
        near = front & (uf >= -1.0) & (uf <= W) & (vf >= -1.0) & (vf <= H)
        half = lambda a: np.abs(a - np.floor(a) - 0.5)
        margins["half_pixel"] = min(_min(half(uf), near), _min(half(vf), near))
        ui, vi = np.where(inside, ur, 0).astype(int), np.where(inside, vr, 0).astype(int)
        return inside, (left, right, top, bottom), lambda img: img[vi, ui]
    left, right, top, bottom = front & (uf < 0), front & (uf > W - 1), front & (vf < 0), front & (vf > H - 1)
    inside = front & ~(left | right | top | bottom)
    margins["border"] = min(_min(np.abs(uf), front), _min(np.abs(uf - (W - 1)), front), _min(np.abs(vf), front), _min(np.abs(vf - (H - 1)), front))
    # at an integer coordinate the floor picks the cell: the value is continuous across it, a NaN neighbour of weight 0 is not
    whole = lambda a: np.abs(a - np.rint(a))
    margins["cell"] = min(_min(whole(uf), inside), _min(whole(vf), inside))
    us, vs = np.where(inside, uf, 0.0), np.where(inside, vf, 0.0)
    u0, v0 = np.minimum(np.floor(us).astype(int), W - 2), np.minimum(np.floor(vs).astype(int), H - 2)
    au, av = us - u0, vs - v0
    return inside, (left, right, top, bottom), lambda img: ((1 - av) * ((1 - au) * img[v0, u0] + au * img[v0, u0 + 1]) +
                                                             av * ((1 - au) * img[v0 + 1, u0] + au * img[v0 + 1, u0 + 1]))


def _finish(counts, margins, valid, front, sides, pz, inlier):
    counts.update(invalid_source=int((~valid).sum()), behind=int((valid & ~front).sum()), out_left=int(sides[0].sum()), out_right=int(sides[1].sum()),
                  out_top=int(sides[2].sum()), out_bottom=int(sides[3].sum()), inlier=int(inlier.sum()),
                  inlier_second_trip=int(inlier.ravel()[GRID_PIXELS:].sum()))
    margins["pz"] = _min(np.abs(pz), valid)
    return dict(counts=counts, margins=margins, margin=min(margins.values()))


def census(Is, Ds, It, Dt, grads, K, T, association):
    """the outcome of every source pixel of one hybrid step (R.accumulate) at pose T, in fp64.  Returns
    counts:  invalid_source, behind (pz <= 0), out_left / out_right / out_top / out_bottom (a pixel out on two sides counts on
             both), invalid_target (target depth or depth gradient NaN where it is read), gated (|r_D| > 0.07), inlier, and among the
             inliers intensity_clipped (|r_I| > 0.1), depth_clipped (|r_D| > 0.05), inlier_second_trip (linear index >= 65536);
    margins: the smallest distance of a deciding quantity from its boundary, per kind; margin: the smallest of them."""
    Is, Ds, It, Dt = (np.asarray(a, dtype=np.float64) for a in (Is, Ds, It, Dt))
    dDx, dDy = (np.asarray(a, dtype=np.float64) for a in grads[2:])
    H, W = Ds.shape
    margins, counts = {}, {}
    valid, front, px, py, pz, uf, vf = _project(Ds, K, T)
    inside, sides, sample = _association(front, uf, vf, H, W, association == "nearest", margins)
    with np.errstate(invalid="ignore"):
        dt, hx, hy = sample(Dt), sample(dDx), sample(dDy)
        finite = inside & ~np.isnan(dt) & ~np.isnan(hx) & ~np.isnan(hy)
        rD = np.where(finite, dt - pz, 0.0)
        inlier = finite & (np.abs(rD) <= R.DEPTH_OUTLIER_TRUNC)
        rI = np.where(inlier, sample(It) - Is, 0.0)
    counts.update(invalid_target=int((inside & ~finite).sum()), gated=int((finite & ~inlier).sum()),
                  intensity_clipped=int((inlier & (np.abs(rI) > R.INTENSITY_HUBER)).sum()), depth_clipped=int((inlier & (np.abs(rD) > R.DEPTH_HUBER)).sum()))
    margins["gate"] = _min(np.abs(np.abs(rD) - R.DEPTH_OUTLIER_TRUNC), finite)
    margins["huber_depth"] = _min(np.abs(np.abs(rD) - R.DEPTH_HUBER), inlier)
    margins["huber_intensity"] = _min(np.abs(np.abs(rI) - R.INTENSITY_HUBER), inlier)
    return _finish(counts, margins, valid, front, sides, pz, inlier)


def census_p2p(Ds, Dt, Nt, K, T, depth_diff=0.07, huber=0.05):
    """the same for one point-to-plane step (tests/_point_to_plane_ref.accumulate): Dt [H, W] and Nt [H, W, 3] are the target's depth
    and normals; invalid_target = depth or normal NaN at the nearest pixel, gated = |r| > depth_diff, depth_clipped = |r| > huber"""
    Ds, Dt, Nt = (np.asarray(a, dtype=np.float64) for a in (Ds, Dt, Nt))
    fx, fy, cx, cy = K
    H, W = Ds.shape
    margins, counts = {}, {}
    valid, front, px, py, pz, uf, vf = _project(Ds, K, T)
    inside, sides, sample = _association(front, uf, vf, H, W, True, margins)
    zt, n = sample(Dt), np.stack([sample(Nt[..., i]) for i in range(3)], -1)
    finite = inside & ~np.isnan(zt) & ~np.isnan(n).any(-1)
    ur, vr = _round_half_away(uf), _round_half_away(vf)
    with np.errstate(invalid="ignore"):
        r = (px - (ur - cx) * zt / fx) * n[..., 0] + (py - (vr - cy) * zt / fy) * n[..., 1] + (pz - zt) * n[..., 2]
    r = np.where(finite, r, 0.0)
    inlier = finite & (np.abs(r) <= depth_diff)
    counts.update(invalid_target=int((inside & ~finite).sum()), gated=int((finite & ~inlier).sum()), depth_clipped=int((inlier & (np.abs(r) > huber)).sum()))
    margins["gate"] = _min(np.abs(np.abs(r) - depth_diff), finite)
    margins["huber_depth"] = _min(np.abs(np.abs(r) - huber), inlier)
    return _finish(counts, margins, valid, front, sides, pz, inlier)


def pyramid_census(d, thr):
    """of one depth-pyramid step (R.pyr_down_depth) on d (NaN = invalid): the number of output pixels that reject at least one VALID
    tap, the number that keep a single tap (the centre's), and the smallest distance of |tap - centre| from thr"""
    t = R._taps(np.asarray(d, dtype=np.float64), np.nan)
    centre = t[2, 2]
    with np.errstate(invalid="ignore"):
        diff = np.abs(t - centre[None, None])
        live = ~np.isnan(diff)
        kept = live & (diff <= thr)
    rejecting = ((live & ~kept).sum((0, 1)) > 0)
    single = (kept.sum((0, 1)) == 1)
    return dict(rejecting=int(rejecting.sum()), single=int(single.sum()), rejected_taps=int((live & ~kept).sum()),
                margin=_min(np.abs(diff - thr), live))


_step_cache = {}


def step_inputs(H, W, seed=0):
    """what one Gauss-Newton step at (H, W) reads, from the statements alone and rounded to fp32 stage by stage (computed once per
    process, never modified): K, the source's (I, D), the target's six maps, and the point-to-plane target's depth and normals"""
    key = (H, W, seed)
    if key not in _step_cache:
        cs, ds, ct, dt = pair(H, W, seed)
        K = intrinsics(H, W)
        src, tgt = level0(cs, ds), level0(ct, dt)
        Dt = f32(P2P.prepare_target(dt))
        Nt = f32(P2P.normal_map(P2P.vertex_map(Dt.astype(np.float64), K)))
        _step_cache[key] = dict(K=K, src=src[:2], tgt=tgt, p2p_depth=Dt, p2p_normals=Nt)
    return _step_cache[key]


def hybrid_reference(inp, T, association, loss):
    """R.accumulate on fp32 maps (upcast): (A, b, cost, inliers)"""
    f = lambda a: np.asarray(a, dtype=np.float64)
    Is, Ds = inp["src"]
    It, Dt, gIx, gIy, gDx, gDy = inp["tgt"]
    return R.accumulate(f(Is), f(Ds), f(It), f(Dt), (f(gIx), f(gIy), f(gDx), f(gDy)), inp["K"], T, association, loss)


def p2p_reference(Ds, Dt, Nt, K, T):
    """tests/_point_to_plane_ref.accumulate on an fp32 source depth, target depth and target normals (upcast)"""
    f = lambda a: np.asarray(a, dtype=np.float64)
    return P2P.accumulate(f(Ds), P2P.vertex_map(f(Dt), K), f(Nt), K, T)


def upper(A):
    return A[np.triu_indices(6)]


def sum_bounds(A, cost):
    """the issue's Cauchy-Schwarz scales of the 28 sums: sqrt(A_aa A_bb) for the 21 of A (upper triangle, row-major),
    sqrt(2 A_aa cost) for b, cost itself"""
    dg = np.sqrt(np.diag(A))
    return upper(np.outer(dg, dg)), np.sqrt(2.0 * np.diag(A) * cost), cost


# ---- the public loss= argument, end to end: the rendered pair of tests/test_rgbd_odometry_gpu.py, made robust-active ---------------
LOSS_HW, LOSS_K, LOSS_DEPTH_MAX = (120, 160), (150.0, 150.0, 80.0, 60.0), 3.0
LOSS_MOTION = {"nearest": (0.01, -0.015, 0.008, 0.012, -0.009, 0.006), "bilinear": (0.004, -0.006, 0.003, 0.002, -0.0015, 0.001)}
LOSS_BOUND = {"nearest": 5e-5, "bilinear": 2e-6}          # |T - T_oracle| of test_matches_oracle_and_truth, per association
# Both losses have the same right-hand side (w r IS the clipped residual), hence the same fixed points: after the full 20 / 10 / 5
# schedule their poses agree (to 2e-12 bilinear, 3e-4 nearest on this pair) and a pose cannot tell them apart.  One coarse and one
# full-resolution step are far from converged: there the poses differ by 6e-3 (nearest) and 9e-5 (bilinear), and the end-to-end
# test runs both schedules.
LOSS_SCHEDULES = {"full": R.ITERATIONS, "short": (1, 0, 1)}
_loss_cache = {}


def loss_pair(association):
    """(source colour, source depth, target colour, target depth): that test's pair with holes=True, plus a saturated 12x12 block of
    source colour (intensity residuals far beyond 0.1) and +0.06 m on a 10x10 block of source depth (between the depth Huber delta
    and the gate)"""
    from _render import render, small_pose
    H, W = LOSS_HW
    ct, dt = render(np.eye(4), LOSS_K, H, W)
    cs, ds = render(small_pose(*LOSS_MOTION[association]), LOSS_K, H, W)
    rng = np.random.default_rng(3)
    ds[rng.random((H, W)) < 0.05] = 0.0
    dt[40:50, 70:90] = 0.0
    cs[30:42, 50:62] = 255
    ds[70:80, 100:110] += np.float32(0.06)
    return cs, ds, ct, dt


def loss_reference(association, loss, schedule):
    """(T, trace) of the statement on loss_pair(association), computed once per process"""
    key = (association, loss, schedule)
    if key not in _loss_cache:
        trace = []
        T = R.rgbd_odometry(*loss_pair(association), LOSS_K, LOSS_DEPTH_MAX, iterations=LOSS_SCHEDULES[schedule], trace=trace,
                            association=association, loss=loss)
        _loss_cache[key] = (T, trace)
    return _loss_cache[key]
