"""What tests/test_odometry_stages_gpu.py relies on, asserted from the fp64 statements alone (oracle/rgbd_odometry_ref.py,
tests/_point_to_plane_ref.py): the inputs of tests/_odometry_inputs.py populate every branch of the odometry kernels, no decision
of a compared step sits within 1e-9 of its boundary (so the device, whose last bits may differ from numpy's, must decide as numpy does and
inlier counts can be required EQUAL), the systems are well conditioned, and the two robust losses are distinguishable."""
import numpy as np
import pytest

import _odometry_inputs as X
from oracle import rgbd_odometry_ref as R

MARGIN = 1e-9
OUTCOMES = ("invalid_source", "behind", "out_left", "out_right", "out_top", "out_bottom", "invalid_target", "gated", "intensity_clipped",
            "depth_clipped", "inlier")
HYBRID = [(hw, name, flags) for hw in X.SIZES for name in X.POSES for flags in range(4)]
P2P = [(hw, name) for hw in X.SIZES for name in X.POSES]
ident = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def hybrid_census(hw, name, association):
    inp = X.step_inputs(*hw)
    return X.census(*inp["src"], inp["tgt"][0], inp["tgt"][1], inp["tgt"][2:], inp["K"], X.pose(name), association)


def p2p_census(hw, name):
    inp = X.step_inputs(*hw)
    return X.census_p2p(inp["src"][1], inp["p2p_depth"], inp["p2p_normals"], inp["K"], X.pose(name))


def test_scene_is_deterministic_and_has_what_it_promises():
    for (H, W) in X.SIZES:
        c, d = X.scene(H, W, 0)
        c2, d2 = X.scene(H, W, 0)
        assert c.dtype == np.uint8 and c.shape == (H, W, 3) and d.dtype == np.float32 and d.shape == (H, W)
        assert np.array_equal(c, c2) and np.array_equal(d, d2) and not np.array_equal(d, X.scene(H, W, 1)[1])
        hole = ~(d > 0)
        assert 0.03 <= hole.mean() <= 0.12 and (d < 0).any() and (d == 0).any()
        assert hole[0].any() and hole[-1].any() and hole[:, 0].any() and hole[:, -1].any() and hole[-1, -1]
        assert ((d > 0) & (d <= X.DEPTH_MAX)).sum() >= 0.5 * H * W and (d > X.DEPTH_MAX).sum() >= 20
        step = np.abs(np.diff(d.astype(np.float64), axis=0))[:, : W // 2]
        assert (step > 2 * R.DEPTH_OUTLIER_TRUNC).sum() >= W // 4
    for hw in X.STAGE_SIZES:                      # the builder serves the tiny sizes of the stage tests too
        assert X.scene(*hw, 0)[1].shape == hw


def test_sparse_source_has_inliers_but_too_few_to_solve():
    """5 valid source pixels: every mode finds some of them (the count the device must report) and none finds 6"""
    hw = (45, 61)
    _, d = X.sparse_source(*hw, 0)
    assert ((d > 0) & (d <= X.DEPTH_MAX)).sum() == 5
    inp = dict(X.step_inputs(*hw))
    Ds = X.f32(R.prepare(np.zeros(hw + (3,), np.uint8), d, X.DEPTH_MAX)[1])
    inp["src"] = (inp["src"][0], Ds)
    T = R.se3_exp(np.array(X.HAIR))
    counts = [X.hybrid_reference(inp, T, *mode)[3] for mode in X.MODES] + [X.p2p_reference(Ds, inp["p2p_depth"], inp["p2p_normals"], inp["K"], T)[3]]
    print(counts)
    assert all(1 <= n < 6 for n in counts), counts


@pytest.mark.parametrize("hw", X.SIZES, ids=ident)
def test_every_outcome_is_populated(hw):
    """over the poses of a size every outcome of a source pixel has at least 20 pixels, in both associations and in the
    point-to-plane step; at 257x257 some pose has 20 inliers in the second trip of the grid-stride loop"""
    for association in ("nearest", "bilinear"):
        cs = [hybrid_census(hw, name, association)["counts"] for name in X.POSES]
        best = {k: max(c[k] for c in cs) for k in OUTCOMES}
        print(hw, association, best)
        assert all(v >= 20 for v in best.values()), best
        if hw[0] * hw[1] > X.GRID_PIXELS:
            assert max(c["inlier_second_trip"] for c in cs) >= 20
    cs = [p2p_census(hw, name)["counts"] for name in X.POSES]
    best = {k: max(c[k] for c in cs) for k in OUTCOMES if k != "intensity_clipped"}
    print(hw, "point-to-plane", best)
    assert all(v >= 20 for v in best.values()), best
    if hw[0] * hw[1] > X.GRID_PIXELS:
        assert max(c["inlier_second_trip"] for c in cs) >= 20
    # the backward pose leaves both: pixels behind the camera AND a system to solve
    for association in ("nearest", "bilinear"):
        c = hybrid_census(hw, "backward", association)["counts"]
        assert c["behind"] >= 20 and c["inlier"] >= 20, c


@pytest.mark.parametrize("hw,name,flags", HYBRID, ids=ident)
def test_hybrid_step_is_decidable_conditioned_and_loss_sensitive(hw, name, flags):
    association, loss = X.MODES[flags]
    cs = hybrid_census(hw, name, association)
    print(hw, name, association, loss, cs["counts"], {k: f"{v:.1e}" for k, v in cs["margins"].items()})
    assert cs["margin"] >= MARGIN, cs["margins"]
    inp, T = X.step_inputs(*hw), X.pose(name)
    A, b, cost, n = X.hybrid_reference(inp, T, association, loss)
    assert n == cs["counts"]["inlier"] >= 20              # the census restates R.accumulate's decisions
    assert np.linalg.cond(A) < 1e6
    # the other loss on the same step.  b is the SAME for both (w r is the clipped residual: the two forms share their gradient),
    # so it is A and the cost that tell them apart
    A2, b2, cost2, n2 = X.hybrid_reference(inp, T, association, "irls" if loss == "o3d" else "o3d")
    assert n2 == n
    assert np.abs(A - A2).max() > 1e-3 * np.abs(A).max() and abs(cost - cost2) > 1e-3 * cost
    assert np.abs(b - b2).max() <= 1e-12 * np.abs(b).max()


@pytest.mark.parametrize("hw,name", P2P, ids=ident)
def test_point_to_plane_step_is_decidable_and_conditioned(hw, name):
    cs = p2p_census(hw, name)
    print(hw, name, cs["counts"], {k: f"{v:.1e}" for k, v in cs["margins"].items()})
    assert cs["margin"] >= MARGIN, cs["margins"]
    inp = X.step_inputs(*hw)
    A, b, cost, n = X.p2p_reference(inp["src"][1], inp["p2p_depth"], inp["p2p_normals"], inp["K"], X.pose(name))
    assert n == cs["counts"]["inlier"] >= 20
    assert np.linalg.cond(A) < 1e6


@pytest.mark.parametrize("hw,seed", [((45, 61), 0), ((45, 61), 1), ((45, 61), 2), ((257, 257), 0)], ids=ident)
def test_depth_pyramid_rejects_valid_taps(hw, seed):
    """the depth pyramid's |tap - centre| <= thr decides on these inputs: at least 100 output pixels drop a valid tap, at least one
    keeps nothing but its centre, and no difference sits within 1e-9 of the threshold"""
    _, d = X.scene(*hw, seed)
    d = X.f32(R.prepare(np.zeros(hw + (3,), np.uint8), d, X.DEPTH_MAX)[1]).astype(np.float64)
    for thr in (2 * R.DEPTH_OUTLIER_TRUNC,):
        c = X.pyramid_census(d, thr)
        print(hw, seed, c)
        assert c["rejecting"] >= 100 and c["single"] >= 1 and c["margin"] >= MARGIN
    # the next level down (what the device's second pyramid step reads, up to fp32 rounding) still rejects
    c = X.pyramid_census(X.f32(R.pyr_down_depth(d)).astype(np.float64), 2 * R.DEPTH_OUTLIER_TRUNC)
    assert c["rejecting"] >= 20


def test_intensity_residuals_pass_the_huber_delta():
    for hw in X.SIZES:
        c = hybrid_census(hw, "small", "nearest")["counts"]
        assert c["intensity_clipped"] >= 0.1 * c["inlier"] and c["intensity_clipped"] <= 0.9 * c["inlier"]


@pytest.mark.parametrize("association", ["nearest", "bilinear"])
def test_loss_pair_tells_the_losses_apart(association):
    """the end-to-end pair of the public loss= argument: under the short schedule the statement's poses for the two losses differ by
    more than ten times the bound the device is held to, so a device that ran the wrong loss could not pass.  (Under the full
    schedule they cannot: both losses share their right-hand side and so their fixed points.)"""
    To, tro = X.loss_reference(association, "o3d", "short")
    Ti, tri = X.loss_reference(association, "irls", "short")
    diff = np.abs(To - Ti).max()
    print(association, f"short schedule: |T_o3d - T_irls| = {diff:.2e}, bound {X.LOSS_BOUND[association]:.0e}")
    assert diff > 10 * X.LOSS_BOUND[association]
    assert len(tro) == len(tri) == sum(X.LOSS_SCHEDULES["short"])
    # the robust branches are live on the first step: the planted blocks clip
    assert abs(tro[0][3] - tri[0][3]) > 1e-3 * tri[0][3] and np.abs(tro[0][1] - tri[0][1]).max() > 1e-3 * np.abs(tri[0][1]).max()
