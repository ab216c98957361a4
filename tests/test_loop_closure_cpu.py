"""The numpy statement of the loop closure (tests/_loop_closure_ref.py) against ground truth, on the CPU: the registration recovers a known
SE(3), the sampler's indices, the information matrix of hand-computable points, and the rendered measurement that the defaults of
bodyslam_amd.loop_closure (MIN_INLIERS) and the GPU test's bounds rest on."""
import numpy as np
import pytest

import _loop_closure_ref as LR
import _loop_scene as LS
from _render import small_pose

TAU = 0.005


def test_registration_recovers_a_known_se3():
    rng = np.random.default_rng(3)
    T = small_pose(0.3, -0.2, 0.5, 0.05, -0.02, 0.08)
    P = rng.uniform(-0.2, 0.2, size=(120, 3)) + (0, 0, 0.5)
    Q = P @ T[:3, :3].T + T[:3, 3]
    planted = np.ones(120, dtype=bool)
    planted[::3] = False
    Q[~planted] += rng.choice([-1.0, 1.0], size=(40, 3)) * rng.uniform(0.05, 0.2, size=(40, 3))
    r = LR.register(P, Q, TAU, seed=1)
    assert r["status"] == 1 and r["margin"] >= 1e-10
    assert np.array_equal(r["mask"], planted) and r["inliers"] == 80 and r["C"] == 120
    assert np.abs(r["T"] - T).max() < 1e-12 and r["rmse"] < 1e-12
    assert np.allclose(r["info"], LR.information(Q[planted]), rtol=1e-12) and r["info"][5, 5] == 80
    # a reflection of the points is not a rigid motion: the fit stays a proper rotation
    r2 = LR.register(P, Q * (1, 1, -1), TAU, seed=1)
    assert abs(np.linalg.det(r2["T"][:3, :3]) - 1.0) < 1e-12


def test_rejections():
    rng = np.random.default_rng(4)
    P = rng.uniform(-0.2, 0.2, size=(50, 3))
    for C in (0, 1, 2):
        r = LR.register(P[:C], P[:C], TAU)
        assert r["status"] == 0 and r["h"] == -1 and np.array_equal(r["T"], np.eye(4)) and not r["info"].any() and r["mask"].shape == (C,)
    line = np.outer(np.linspace(0.0, 1.0, 50), (0.3, -0.2, 0.1)) + (0.1, 0.2, 0.3)
    same = np.tile((0.1, 0.2, 0.3), (50, 1))
    for pts in (line, same):
        r = LR.register(pts, pts, TAU)
        assert r["status"] == 0 and r["inliers"] == 0 and not r["scores"].any()
    assert LR.register(P, P, TAU, min_matches=51)["status"] == 0 and LR.register(P, P, TAU, min_matches=50)["status"] == 1


@pytest.mark.parametrize("C", [3, 4, 5, 500])
def test_sampler_indices_are_distinct_and_in_range(C):
    seen = set()
    for seed in (0, 1, 0xFFFFFFFFFFFFFFFF):
        for pair in (0, 7):
            for h in range(300):
                ids = LR.sample(seed, pair, h, C)
                assert len(set(ids)) == 3 and min(ids) >= 0 and max(ids) < C, (seed, pair, h, ids)
                seen.update(ids)
    assert len(seen) == min(C, len(seen)) and (C > 5 or seen == set(range(C)))          # every index is reachable
    assert LR.draw(0, 0, 0, 0) == 0xE220A839 and LR.sample(0, 0, 0, 500) != LR.sample(0, 1, 0, 500)


def test_information_matrix_by_hand():
    # one point on the z axis at distance 2: rotations about x and y move it by 2 per radian, about z not at all
    info = LR.information(np.array([[0.0, 0.0, 2.0]]))
    want = np.zeros((6, 6))
    want[0, 0] = want[1, 1] = 4.0
    want[3, 3] = want[4, 4] = want[5, 5] = 1.0
    want[0, 4] = want[4, 0] = -2.0
    want[1, 3] = want[3, 1] = 2.0
    assert np.array_equal(info, want)
    pts = np.array([[1.0, 2.0, 3.0], [-1.0, 0.5, 2.0]])
    info = LR.information(pts)
    assert np.array_equal(info, info.T) and info[5, 5] == 2.0
    x, y, z = pts.T
    assert np.allclose(np.diag(info)[:3], [(y * y + z * z).sum(), (x * x + z * z).sum(), (x * x + y * y).sum()])
    assert np.allclose(info[0, 1], -(x * y).sum()) and np.allclose(info[:3, 3:], [[0, -z.sum(), y.sum()], [z.sum(), 0, -x.sum()], [-y.sum(), x.sum(), 0]])


# ---- the rendered measurement -------------------------------------------------------------------------------------------------------------
# The statement on rendered 200 x 152 frames of the height field against the keyframe at the origin, max_hamming 64, tau 5 mm, 256
# hypotheses, seed 2, measured on the CPU (2026-10-17):
#   view                                       keypoints  matches  <= 64   C    inliers   |t - t_true|   max |R - R_true|
#   revisit (0.02, -0.03, 0.05 rad; 10, -6, 8 mm)    352      198    192  192      190     4.306e-04 m      3.648e-03
#   revisit, farther (0.05, -0.06, 0.15; 20, -12, 15)  335    176    167  167      164     9.499e-05 m      1.790e-03
#   another place, same pose as the keyframe         360      113     64   64   0 .. 3          --              --
#   another place, a second view                     354      125     60   60   3 .. 4          --              --
#   blank frame                                        0        0      0    0        0          --              --
# (the ranges: seeds 0, 1, 2.)  Descriptor counts do not separate a revisit from another place (60 against 192); the inliers do
# (at most 5 on any surface and seed against 164 and more).  The error of T is set by the integer keypoint positions.
MEASURED = {"revisit": dict(inliers=190, t=4.306e-04, R=3.648e-03), "far": dict(inliers=164, t=9.499e-05, R=1.790e-03), "elsewhere_max_inliers": 5}
SEED = 2


@pytest.fixture(scope="module")
def keyframe():
    return LR.frame(*LS.render(LS.ORIGIN), LS.K)


@pytest.mark.parametrize("view", ["revisit", "far"])
def test_rendered_revisit_is_registered(keyframe, view):
    pose = LS.REVISIT if view == "revisit" else LS.REVISIT_FAR
    f = LR.frame(*LS.render(pose), LS.K)
    m = LR.match_pairs([f["desc"], keyframe["desc"]], [(0, 1)])[0]
    r = LR.register_pair(f["xyz"], keyframe["xyz"], m, 64, TAU, seed=SEED)
    T = LS.motion(pose)
    et, eR = float(np.linalg.norm(r["T"][:3, 3] - T[:3, 3])), float(np.abs(r["T"][:3, :3] - T[:3, :3]).max())
    print(view, "keypoints", len(f["pt"]), "matches", len(m), "C", r["C"], "inliers", r["inliers"], "h", r["h"], "margin", r["margin"], "unique", r["unique"],
          "t error", et, "R error", eR, "rmse", r["rmse"])
    assert r["status"] == 1 and r["margin"] >= 1e-10
    assert r["inliers"] == MEASURED[view]["inliers"] and r["info"][5, 5] == r["inliers"]
    assert et <= 1.001 * MEASURED[view]["t"] and eR <= 1.001 * MEASURED[view]["R"]
    assert r["inliers"] >= 5 * 30                                    # LoopCloser's default min_inliers lies far below


@pytest.mark.parametrize("place,pose", [(1, "origin"), (2, "elsewhere"), (1, "revisit")])
def test_another_place_is_not_registered(keyframe, place, pose):
    P = dict(origin=LS.ORIGIN, elsewhere=LS.ELSEWHERE, revisit=LS.REVISIT)[pose]
    f = LR.frame(*LS.render(P, place), LS.K)
    m = LR.match_pairs([f["desc"], keyframe["desc"]], [(0, 1)])[0]
    assert (m[:, 2] <= 64).sum() >= 30                               # the descriptors alone would let it through (min_matches = 30)
    for seed in (0, 1, 2):
        r = LR.register_pair(f["xyz"], keyframe["xyz"], m, 64, TAU, seed=seed)
        print("place", place, pose, "seed", seed, "matches", len(m), "C", r["C"], "inliers", r["inliers"])
        assert r["inliers"] <= MEASURED["elsewhere_max_inliers"] < 30


def test_blank_frame_has_nothing_to_register(keyframe):
    import _corner_scene as S
    f = LR.frame(*S.blank(), LS.K)
    m = LR.match_pairs([f["desc"], keyframe["desc"]], [(0, 1)])[0]
    r = LR.register_pair(f["xyz"], keyframe["xyz"], m, 64, TAU, min_matches=30)
    assert len(f["pt"]) == 0 and len(m) == 0 and r["status"] == 0 and r["C"] == 0 and not r["mask_rows"].any()


def test_lift_rules():
    pt = np.array([[3.7, 2.2], [0.0, 0.0], [-0.5, 1.0], [9.99, 4.99], [10.0, 1.0], [5.0, 3.0], [6.0, 3.0]], dtype=np.float32)
    depth = np.full((5, 10), 0.5, dtype=np.float32)
    depth[3, 5], depth[3, 6] = 0.0, np.nan
    K = (20.0, 25.0, 5.0, 2.5)
    xyz = LR.lift(pt, depth, K)
    assert list(xyz[:, 3]) == [1, 1, 1, 1, 0, 0, 0]                     # (-0.5 truncates to column 0, as associate_depth's int() does)
    assert np.array_equal(xyz[0, :3], [(np.float64(np.float32(3.7)) - 5.0) * 0.5 / 20.0, (np.float64(np.float32(2.2)) - 2.5) * 0.5 / 25.0, 0.5])
    assert not xyz[4:].any()
