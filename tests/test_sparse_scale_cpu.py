"""The sparse-feature scale path without a GPU: the numpy statement (tests/_orb_ref.py) against the reference's own association and
displacement code (tests/golden/sparse_scale.npz, tools/make_sparse_scale_golden.py), the conditions on the test scene that the GPU tests
rely on, and the drop-in surface."""
import inspect
import os

import numpy as np
import pytest

import _corner_scene as S
import _orb_ref as R
from bodyslam_amd import orb_tables as T

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_scale.npz"))
CASES = ("valid", "misaligned", "outside", "more_prev", "more_curr")


@pytest.mark.parametrize("name", CASES)
def test_statement_equals_the_reference_after_the_match(name):
    g = {k: GOLDEN[f"{name}/{k}"] for k in ("pts_prev", "pts_curr", "matches", "depth_prev", "depth_curr", "assoc_prev", "assoc_curr", "displacements", "mean")}
    a = R.associate_depth(g["pts_prev"], g["pts_curr"], g["matches"], g["depth_prev"])
    b = R.associate_depth(g["pts_curr"], g["pts_prev"], g["matches"], g["depth_curr"])
    assert [m for m, _ in a] == list(g["assoc_prev"]) and [m for m, _ in b] == list(g["assoc_curr"])
    mean, counts = R.displacement(g["pts_prev"], g["pts_curr"], g["matches"], g["depth_prev"], g["depth_curr"], GOLDEN["K"], "reference")
    assert counts == (len(g["pts_prev"]), len(g["pts_curr"]), len(g["matches"]), len(g["assoc_prev"]), len(g["assoc_curr"]), len(g["displacements"]))
    assert np.max(np.abs(mean - g["mean"])) <= 1e-12
    assert np.max(np.abs(mean - g["displacements"].mean(0))) <= 1e-12


def test_golden_cases_exercise_the_quirks():
    n = {c: (len(GOLDEN[f"{c}/matches"]), len(GOLDEN[f"{c}/assoc_prev"]), len(GOLDEN[f"{c}/assoc_curr"])) for c in CASES}
    assert n["valid"][0] == n["valid"][1] == n["valid"][2]
    m = GOLDEN["misaligned/matches"]
    a, b = GOLDEN["misaligned/assoc_prev"], GOLDEN["misaligned/assoc_curr"]
    k = min(len(a), len(b))
    assert len(a) < len(m) and len(b) < len(m) and np.any(a[:k] != b[:k])                       # the zip pairs different matches
    assert n["outside"][1] < n["outside"][0] and n["outside"][2] < n["outside"][0]
    for c, col, other in (("more_prev", 0, "pts_curr"), ("more_curr", 1, "pts_prev")):
        past = GOLDEN[f"{c}/matches"][:, col] >= len(GOLDEN[f"{c}/{other}"])
        assert past.any() and not np.isin(np.flatnonzero(past), GOLDEN[f"{c}/assoc_curr"]).any()  # the bounds check skipped them


def test_matched_association_keeps_pairs_aligned():
    g = {k: GOLDEN[f"misaligned/{k}"] for k in ("pts_prev", "pts_curr", "matches", "depth_prev", "depth_curr")}
    mean, counts = R.displacement(g["pts_prev"], g["pts_curr"], g["matches"], g["depth_prev"], g["depth_curr"], GOLDEN["K"], "matched")
    fx, fy, cx, cy = GOLDEN["K"]
    rows = []
    for (q, t, _) in g["matches"]:
        (u1, v1), (u2, v2) = g["pts_prev"][q].astype(np.float64), g["pts_curr"][t].astype(np.float64)
        d1, d2 = g["depth_prev"][int(v1), int(u1)], g["depth_curr"][int(v2), int(u2)]
        if d1 != 0 and d2 != 0:
            rows.append(R.pixel_to_3d(u2, v2, d2, fx, fy, cx, cy) - R.pixel_to_3d(u1, v1, d1, fx, fy, cx, cy))
    assert counts[5] == len(rows) and np.allclose(mean, np.mean(rows, axis=0), atol=1e-12)


def test_scene_meets_what_the_gpu_tests_rely_on():
    (c0, _), _, _ = S.pair("plane")
    levels = R.pyramid(R.grey(c0))
    sizes = T.level_sizes(S.H, S.W)
    assert [a.shape for a in levels] == [(h, w) for (w, h) in sizes] and sizes[7] == (56, 42)
    nf = T.features_per_level()
    assert int(nf.sum()) == 500 and list(nf) == [109, 90, 75, 63, 52, 44, 36, 31]
    cand = [int((R.fast_nms(a) > 0).sum()) for a in levels]
    assert cand[0] > 2 * nf[0], cand                   # the histogram cut and its tie rule run
    assert any(c == 0 for c in cand), cand             # the empty-level path runs
    assert cand[7] == 0 and min(sizes[7]) <= 2 * T.EDGE_THRESHOLD
    assert (S.H % 16, S.W % 16) != (0, 0)


def test_tables_are_reproducible_and_inside_the_margin():
    p = T.brief_pattern()
    assert p.shape == (256, 4) and np.abs(p).max() <= 15 and np.array_equal(p, T.brief_pattern())
    assert 5.0 < p.std() < 7.0                          # sigma = 31 / 5, clipped
    r = T.rotated_pattern()
    assert r.shape == (30, 256, 4) and np.array_equal(r[0], p) and np.abs(r.astype(int)).max() <= 22 < T.EDGE_THRESHOLD - 3
    assert np.allclose(T.COS, np.cos(np.radians(12.0 * np.arange(30))), atol=1e-15)
    assert np.allclose(T.SIN, np.sin(np.radians(12.0 * np.arange(30))), atol=1e-15)
    lv, stride = T.level_layout(S.H, S.W)
    assert np.all(lv[:, 2] % 16 == 0) and stride % 16 == 0 and np.all(lv[1:, 2] >= lv[:-1, 2] + lv[:-1, 0] * lv[:-1, 1])


def test_drop_in_surface():
    from bodyslam_amd import scaling_system as SS
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(SS.extract_features_orb) == ["image"] and sig(SS.extract_features_sift) == ["image"]
    assert sig(SS.match_features_orb) == ["descriptors1", "descriptors2"] and sig(SS.match_features_sift) == ["descriptors1", "descriptors2"]
    assert sig(SS.associate_depth) == ["keypoints1", "keypoints2", "matches", "depth_image"]
    assert sig(SS.calculate_displacements) == ["keypoints1", "keypoints2", "depth_associations1", "depth_associations2", "fx", "fy", "cx", "cy"]
    assert sig(SS.pixel_to_3d) == ["u", "v", "depth", "fx", "fy", "cx", "cy"]
    assert sig(SS.compute_scaling_factor) == ["curr_rgb", "prev_rgb", "curr_dp", "prev_dp", "intrinsics", "feature_type"]
    assert inspect.signature(SS.compute_scaling_factor).parameters["feature_type"].default == "orb"
    for call in (lambda: SS.extract_features_sift(None), lambda: SS.match_features_sift(None, None),
                 lambda: SS.compute_scaling_factor(None, None, None, None, (1, 1, 0, 0), feature_type="sift")):
        with pytest.raises(NotImplementedError):
            call()
    kp, m = SS.KeyPoint(1.5, 2.5), SS.DMatch(3, 4, 17)
    assert kp.pt == (1.5, 2.5) and (m.queryIdx, m.trainIdx, m.distance) == (3, 4, 17.0)
    # the host bookkeeping of associate_depth is the reference's: against the golden fixture
    g = {k: GOLDEN[f"outside/{k}"] for k in ("pts_prev", "pts_curr", "matches", "depth_prev", "assoc_prev")}
    k1, k2 = [SS.KeyPoint(x, y) for (x, y) in g["pts_prev"]], [SS.KeyPoint(x, y) for (x, y) in g["pts_curr"]]
    ms = [SS.DMatch(q, t, d) for (q, t, d) in g["matches"]]
    assert [ms.index(m) for m, _ in SS.associate_depth(k1, k2, ms, g["depth_prev"])] == list(g["assoc_prev"])


def test_vo_sparse_path_takes_a_callable_and_refuses_nan():
    from bodyslam_amd.visual_odometry import VO

    class MPEM:
        def infer_relative_pose_between(self, a, b):
            return np.eye(4, dtype=np.float32)

    vo = VO(MPEM(), sparse_scale=lambda curr, prev: np.array([0.01, 0.0, 0.02]))
    T4 = vo.estimate_relative_pose_between("a", "b", "p", "c", 1, rgbd_odo=False)
    assert np.all(np.isfinite(T4)) and 0 < T4[0, 3] < 0.01
    x, P = vo.ukf.x.copy(), vo.ukf.P.copy()
    vo.sparse_scale = lambda curr, prev: np.full(3, np.nan)
    with pytest.raises(RuntimeError, match="frame 7"):
        vo.estimate_relative_pose_between("a", "b", "p", "c", 7, rgbd_odo=False)
    assert np.array_equal(vo.ukf.x, x) and np.array_equal(vo.ukf.P, P)
