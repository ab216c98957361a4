"""Trajectory evaluation without a GPU: the numpy restatement tests/_trajectory_eval_ref.py against the reference's golden outputs
(tests/golden/trajectory_eval.npz, written by tools/make_trajectory_eval_golden.py from the reference's own functions) and against
hand-computed cases; the product's input validation, file formats and its refusal to run without a GPU."""
import csv
import os

import numpy as np
import pytest

import _trajectory_eval_ref as TR

# fp64 round-off: every compared number is a sum of fewer than 5 000 terms (or a 3x3 factorisation of such sums)
RTOL = 1e-12


def load_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "trajectory_eval.npz"))


def golden_poses(d, key):
    rows = d[key].astype(np.float64)
    T = np.tile(np.eye(4), (len(rows), 1, 1))
    T[:, :3, :] = rows
    return T


SIM_NAMES = ("n3", "n50", "n50_reflection", "n5000")
TRAJ_NAMES = ("len3", "kitti24", "len1000")


def test_golden_holds_the_cases(golden_dir):
    d = load_golden(golden_dir)
    assert tuple(d["sim_names"]) == SIM_NAMES and tuple(d["traj_names"]) == TRAJ_NAMES and tuple(d["deltas"]) == (1, 5)
    assert [d[f"sim_{n}_source"].shape[0] for n in SIM_NAMES] == [3, 50, 50, 5000]
    assert d["sim_n50_reflection_detSxy"] < 0 < d["sim_n50_detSxy"]
    assert [d[f"traj_{n}_gt"].shape[0] for n in TRAJ_NAMES] == [3, 24, 1000]
    assert os.path.getsize(os.path.join(golden_dir, "trajectory_eval.npz")) < 200 * 1024


@pytest.mark.parametrize("name", SIM_NAMES)
def test_restated_umeyama_equals_reference(golden_dir, name):
    d = load_golden(golden_dir)
    x, y = d[f"sim_{name}_source"].astype(np.float64), d[f"sim_{name}_target"].astype(np.float64)
    R, s, t, (sigma_x, rank) = TR.umeyama(x, y, rule="reference")
    print(name, "max |dR|", np.abs(R - d[f"sim_{name}_R"]).max(), "ds/s", abs(s / d[f"sim_{name}_s"] - 1), "max |dt|", np.abs(t - d[f"sim_{name}_t"]).max())
    np.testing.assert_allclose(s, d[f"sim_{name}_s"], rtol=RTOL)
    np.testing.assert_allclose(R, d[f"sim_{name}_R"], rtol=RTOL, atol=RTOL)          # (entries of a rotation: absolute on the scale 1)
    np.testing.assert_allclose(t, d[f"sim_{name}_t"], rtol=RTOL, atol=RTOL * np.abs(d[f"sim_{name}_t"]).max())
    assert rank == (2 if name == "n3" else 3)                                       # three points span a plane
    if name != "n3":
        # full rank: the evo rule is the same fit, a proper rotation also for the mirrored target
        R2, s2, t2, _ = TR.umeyama(x, y, rule="evo")
        assert np.array_equal(R2, R) and s2 == s and np.array_equal(t2, t)
        assert abs(np.linalg.det(R) - 1) < 1e-12


@pytest.mark.parametrize("name", TRAJ_NAMES)
def test_restated_training_protocol_equals_reference(golden_dir, name):
    d = load_golden(golden_dir)
    gt, pred = golden_poses(d, f"traj_{name}_gt"), golden_poses(d, f"traj_{name}_pred")
    pred0 = pred.copy()
    np.testing.assert_allclose(TR.training_scale(gt, pred), d[f"traj_{name}_scale"], rtol=RTOL)
    checked = 0
    for delta in (1, 5):
        if f"traj_{name}_rre_d{delta}" not in d.files:
            assert len(gt) <= delta                          # (the reference divides by zero there; the restatement reports it)
            with pytest.raises(TR.Degenerate):
                TR.evaluate_training(gt, pred, delta)
            continue
        r = TR.evaluate_training(gt, pred, delta)
        print(name, delta, {k: r[k]["mean"] for k in ("ate", "are", "rte", "rre")})
        np.testing.assert_allclose(r["scale"], d[f"traj_{name}_scale"], rtol=RTOL)
        np.testing.assert_allclose(r["ate"]["mean"], d[f"traj_{name}_ate"], rtol=RTOL)
        np.testing.assert_allclose(r["are"]["mean"], d[f"traj_{name}_are"], rtol=RTOL)
        np.testing.assert_allclose(r["rte"]["mean"], d[f"traj_{name}_rte_d{delta}"], rtol=RTOL)
        np.testing.assert_allclose(r["rre"]["mean"], d[f"traj_{name}_rre_d{delta}"], rtol=RTOL)
        assert r["n_pairs"] == len(gt) - delta
        checked += 1
    assert checked == (1 if name == "len3" else 2)
    assert np.array_equal(pred, pred0)                       # nothing is scaled in place


def similarity_of(gt, s, R, t):
    """pred with gt = [R|t] o scale_s(pred) pose by pose: pred_i = scale_{1/s}([R|t]^-1 gt_i)"""
    A = np.eye(4)
    A[:3, :3], A[:3, 3] = R, t
    P = np.array([TR.se3_inv(A) @ g for g in gt])
    P[:, :3, 3] /= s
    return P


def test_evo_protocol_recovers_a_similarity():
    rng = np.random.default_rng(1)
    gt = TR.random_walk(rng, 300)
    s, R, t = 2.5, TR.rot([0.2, 1.0, -0.4], 1.1), np.array([0.7, -0.3, 1.9])
    pred = similarity_of(gt, s, R, t)
    path = np.sum(np.linalg.norm(np.diff(gt[:, :3, 3], axis=0), axis=1))
    # without the origin alignment the fit is the similarity itself
    r = TR.evaluate_evo(gt, pred, align_origin=False)
    print("ATE rmse / path", r["ate"]["rmse"] / path, "scale", r["scale"])
    assert r["ate"]["rmse"] < 1e-12 * path
    np.testing.assert_allclose(r["scale"], s, rtol=1e-12)
    np.testing.assert_allclose(r["rotation"], R, atol=1e-12)
    np.testing.assert_allclose(r["translation"], t, atol=1e-12 * path)
    assert r["rte"]["max"] < 1e-12 * path and r["rre"]["max"] < 1e-5          # (arccos near 1: sqrt(eps) rad, in degrees)
    # with it (the reference's order) the origin alignment has already undone the rigid part; the scale remains
    r = TR.evaluate_evo(gt, pred)
    assert r["ate"]["rmse"] < 1e-12 * path
    np.testing.assert_allclose(r["scale"], s, rtol=1e-12)
    assert r["n_poses"] == 300 and r["n_pairs"] == 299
    assert TR.evaluate_evo(gt, pred, delta=7)["n_pairs"] == len(range(0, 300, 7)) - 1
    assert TR.evaluate_evo(gt, pred, delta=7, all_pairs=True)["n_pairs"] == 293


def test_one_injected_relative_error_is_read_back():
    """A prediction equal to gt except for one extra motion D between poses k - 1 and k: every relative pose across that step has the
    error E = inv(Q_rel) P_rel with |trans| and angle that can be written down by hand, every other pair has none."""
    rng = np.random.default_rng(2)
    n, k = 40, 17
    gt = TR.random_walk(rng, n)
    ang, shift = 0.05, np.array([0.003, -0.004, 0.012])
    D = np.eye(4)
    D[:3, :3], D[:3, 3] = TR.rot([1.0, 2.0, -1.0], ang), shift
    pred = gt.copy()
    rel = [np.linalg.inv(gt[i - 1]) @ gt[i] for i in range(1, n)]
    for i in range(1, n):
        pred[i] = pred[i - 1] @ (rel[i - 1] @ D if i == k else rel[i - 1])
    r = TR.evaluate_evo(gt, pred, delta=1, align_origin=False, align=False, correct_scale=False)
    # delta = 1: the pair (k - 1, k) has E = inv(rel) rel D = D, all others E = I
    assert r["n_pairs"] == n - 1
    np.testing.assert_allclose(r["rte"]["max"], np.linalg.norm(shift), rtol=1e-10)
    np.testing.assert_allclose(r["rre"]["max"], np.degrees(ang), rtol=1e-10)
    np.testing.assert_allclose(r["rte"]["mean"], np.linalg.norm(shift) / (n - 1), rtol=1e-9)
    np.testing.assert_allclose(r["rte"]["rmse"], np.linalg.norm(shift) / np.sqrt(n - 1), rtol=1e-9)
    np.testing.assert_allclose(r["rre"]["rmse"], np.degrees(ang) / np.sqrt(n - 1), rtol=1e-9)
    assert r["rte"]["min"] < 1e-14 and r["ate"]["min"] == 0.0
    # the training protocol: the same single pair, errors |t_q - t_p| and the angle of R_q R_p^T between rel and rel D
    tr = TR.evaluate_training(gt, pred, delta=1)
    a, b = rel[k - 1], rel[k - 1] @ D
    np.testing.assert_allclose(tr["rte"]["max"], np.linalg.norm(a[:3, 3] - b[:3, 3]), rtol=1e-10)
    np.testing.assert_allclose(tr["rre"]["max"], ang, rtol=1e-10)            # R_a (R_a R_D)^T = R_a R_D^T R_a^T: the angle of D
    # the error-free pairs: a trace off 3 by a few ulp, (tr - 1) / 2 = 1 - u with u <= 4 * 2^-53, gives arccos = sqrt(2 u) <= 3e-8 rad each
    np.testing.assert_allclose(tr["rre"]["mean"], ang / (n - 1), rtol=1e-9, atol=3e-8)


def test_straight_line_and_two_poses_are_degenerate():
    gt = np.tile(np.eye(4), (20, 1, 1))
    gt[:, :3, 3] = np.outer(np.arange(20), [0.1, 0.2, -0.05])
    pred = gt.copy()
    pred[:, :3, 3] *= 0.5
    with pytest.raises(TR.Degenerate):
        TR.evaluate_evo(gt, pred)
    rng = np.random.default_rng(3)
    two = TR.random_walk(rng, 2)
    with pytest.raises(TR.Degenerate):
        TR.evaluate_evo(two, TR.perturbed(rng, two))
    with pytest.raises(TR.Degenerate):                          # and too short for delta = 2
        TR.evaluate_evo(two, two, delta=2, align=False, correct_scale=False)
    still = np.tile(np.eye(4), (5, 1, 1))
    with pytest.raises(TR.Degenerate):                          # sigma_x = 0
        TR.evaluate_evo(gt[:5], still)


# ---- the product, as far as it goes without a GPU -----------------------------------------------------------------------------------------
def test_estimate_similarity_transformation_is_importable():
    from bodyslam_amd.slam_utils import estimate_similarity_transformation
    assert callable(estimate_similarity_transformation)
    with pytest.raises(ValueError):
        estimate_similarity_transformation(np.zeros((5, 3)), np.zeros((5, 3)))       # the reference's layout is [3, n]


def test_input_validation_comes_before_the_device():
    from bodyslam_amd import evaluation as E
    ok = np.tile(np.eye(4), (6, 1, 1))
    bad = [
        dict(pred=ok, gt=ok, protocol="kitti"),
        dict(pred=ok, gt=ok, delta=0),
        dict(pred=ok, gt=ok, delta=1.5),
        dict(pred=ok[:5], gt=ok),
        dict(pred=ok, gt=ok, delta=6),                           # fewer than delta + 1 poses
        dict(pred=np.zeros((6, 4, 3)), gt=ok),
        dict(pred=np.zeros((6, 11)), gt=ok),
        dict(pred=ok.astype(np.int64), gt=ok),
        dict(pred=[ok], gt=ok),
        dict(pred=[ok, ok], gt=[ok]),
        dict(pred=[], gt=[]),
        dict(pred="poses.txt", gt=ok),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            E.evaluate_trajectory(**kw)
    with pytest.raises(ValueError, match="sequence 1"):
        E.evaluate_trajectory([ok, ok[:1]], [ok, ok[:1]])
    for a, b in ((np.zeros((4, 2)), np.zeros((4, 2))), (np.zeros((4, 3)), np.zeros((5, 3))), (np.zeros((4, 3), np.float32), np.zeros((4, 3))),
                 (np.zeros((0, 3)), np.zeros((0, 3))), (np.zeros((4, 3), np.int32), np.zeros((4, 3), np.int32))):
        with pytest.raises(ValueError):
            E.similarity_transform(a, b)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from bodyslam_amd import _lib as L
    from bodyslam_amd import evaluation as E
    from bodyslam_amd.slam_utils import estimate_similarity_transformation
    rng = np.random.default_rng(4)
    gt = TR.random_walk(rng, 10)
    with pytest.raises(L.BodySlamHipError):
        E.evaluate_trajectory(TR.perturbed(rng, gt), gt)
    with pytest.raises(L.BodySlamHipError):
        E.evaluate_trajectory(TR.perturbed(rng, gt)[:, :3, :].reshape(-1, 12), gt, protocol="training")
    x = rng.normal(size=(10, 3))
    with pytest.raises(L.BodySlamHipError):
        E.similarity_transform(x, 2 * x)
    with pytest.raises(L.BodySlamHipError):
        estimate_similarity_transformation(x.T, 2 * x.T)


def test_csv_layout_and_reference_dict(tmp_path):
    from bodyslam_amd import evaluation as E
    rec = np.zeros((2, 40))
    rec[1, 16:21] = [0.5, 0.4, 0.3, 0.1, 0.9]                   # ATE
    rec[1, 26:31] = [0.05, 0.04, 0.03, 0.01, 0.09]              # RTE
    rec[1, 31:36] = [1.5, 1.25, 0.75, 0.25, 2.5]                # RRE
    m = E._metrics_from_records(rec, "evo")
    ref = m.as_reference_dict(1)
    assert list(ref) == ["ATE", "RTE", "RRE"]
    assert ref == {"ATE": (0.5, 0.3), "RTE": (0.05, 0.03), "RRE": (1.5, 0.75)}
    assert all(type(v) is tuple and len(v) == 2 and all(type(x) is float for x in v) for v in ref.values())
    assert m.ate.mean[1] == 0.4 and m.rre.max[1] == 2.5 and m.are.rmse[1] == 0.0 and len(m) == 2
    path = m.write_csv(str(tmp_path / "seq.csv"), 1)
    text = open(path, newline="").read()
    assert text == 'Metric,Value\r\nATE,"(0.5, 0.3)"\r\nRTE,"(0.05, 0.03)"\r\nRRE,"(1.5, 0.75)"\r\n'
    rows = list(csv.DictReader(open(path, newline="")))
    assert [r["Metric"] for r in rows] == ["ATE", "RTE", "RRE"] and "np.float64" not in text


def test_read_kitti_poses_round_trips_the_reference_file(golden_dir, tmp_path):
    from bodyslam_amd import evaluation as E
    from bodyslam_amd.slam_utils import save_poses_as_kitti
    src = os.path.join(golden_dir, "kitti_poses_24.txt")
    T = E.read_kitti_poses(src)
    assert T.shape == (24, 4, 4) and T.dtype == np.float64
    assert np.array_equal(T[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (24, 1)))
    out = tmp_path / "again.txt"
    save_poses_as_kitti(list(T), str(out))
    assert open(out, "rb").read() == open(src, "rb").read()
    bad = tmp_path / "bad.txt"
    bad.write_text("1 0 0 0 0 1 0 0 0 0 1\n")
    with pytest.raises(ValueError, match="11 numbers"):
        E.read_kitti_poses(str(bad))
    with pytest.raises(ValueError):
        E.evaluate_trajectory_files([src], [src, src])
