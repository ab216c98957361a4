"""Trajectory evaluation on the device (bs_similarity_fit, bs_trajectory_metrics through bodyslam_amd.evaluation): the reference's golden
outputs and the numpy restatement tests/_trajectory_eval_ref.py, bitwise reproducibility and batch invariance, device-resident poses of
the pipeline, a two-million-point fit, guard bands, and per-sequence status.

Tolerances: rtol 1e-9, the project's fp64 bar (test_pose_chain).  Angles get an absolute 1e-9 rad instead (arccos is ill-conditioned near
0); the inputs keep every rotation error above 1e-4 rad, which each test asserts of its reference values, so that the bar means nine
digits.  Translation errors are differences of positions: their absolute floor is 1e-9 of the largest position."""
import os

import numpy as np
import pytest

import _trajectory_eval_ref as TR
from test_trajectory_eval_cpu import SIM_NAMES, TRAJ_NAMES, golden_poses, load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from bodyslam_amd import _lib as L  # noqa: E402
from bodyslam_amd import evaluation as E  # noqa: E402

RTOL = 1e-9
ANGLE_ATOL_RAD = 1e-9
MIN_ANGLE_RAD = 1e-4


def assert_matches_restatement(m, i, ref, gt, protocol, what=""):
    """sequence i of the TrajectoryMetrics m against a dict of the restatement"""
    unit = 180.0 / np.pi if protocol == "evo" else 1.0
    scale = np.abs(np.asarray(gt)[:, :3, 3]).max()
    assert m.n_poses[i] == ref["n_poses"] and m.n_pairs[i] == ref["n_pairs"], what
    for name in ("ate", "rte", "are", "rre"):
        angle = name in ("are", "rre")
        if angle:
            assert ref[name]["min"] > MIN_ANGLE_RAD * unit, (what, name, ref[name]["min"])      # the inputs keep the bar meaningful
        for st in TR.STATS:
            got, want = getattr(getattr(m, name), st)[i], ref[name][st]
            print(f"{what} {name}.{st}: device {got:.17g} restatement {want:.17g} diff {abs(got - want):.3e}")
            if angle:
                assert abs(got - want) <= ANGLE_ATOL_RAD * unit, (what, name, st, got, want)
            else:
                assert abs(got - want) <= RTOL * abs(want) + RTOL * scale, (what, name, st, got, want)
    np.testing.assert_allclose(m.scale[i], ref["scale"], rtol=RTOL, err_msg=what)
    np.testing.assert_allclose(m.rotation[i], ref["rotation"], atol=RTOL, err_msg=what)
    np.testing.assert_allclose(m.translation[i], ref["translation"], rtol=RTOL, atol=RTOL * scale, err_msg=what)


# ---- bs_similarity_fit --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", SIM_NAMES)
def test_similarity_fit_matches_golden_and_restatement(golden_dir, name, dtype):
    d = load_golden(golden_dir)
    x, y = d[f"sim_{name}_source"].astype(dtype), d[f"sim_{name}_target"].astype(dtype)       # float16 values: exact in both
    rec = E.similarity_fit_record(x, y)
    R, s, t = rec[:9].reshape(3, 3), rec[9], rec[10:13]
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    Rr, sr, tr, (sigma_x, rank) = TR.umeyama(x64, y64, rule="evo")
    print(name, dtype.__name__, "ds/s", abs(s / sr - 1), "max|dR|", np.abs(R - Rr).max(), "max|dt|", np.abs(t - tr).max(), "rank", rec[14])
    assert rec[14] == rank and rec[15] == len(x)
    np.testing.assert_allclose(rec[13], sigma_x, rtol=RTOL)
    np.testing.assert_allclose(s, d[f"sim_{name}_s"], rtol=RTOL)
    np.testing.assert_allclose(s, sr, rtol=RTOL)
    tscale = np.abs(y64).max()
    if name == "n3":
        # Three points span a plane: Sxy has rank 2, det(Sxy) is round-off, and the reference's sign rule returned a reflection for this
        # input (det R = -1 in the golden).  The device returns the proper rotation (the evo rule); the two differ only along the plane's
        # normal, where the centred source has no component, so both map the source points alike: that, and s, is what is compared.
        assert np.linalg.det(d["sim_n3_R"]) < 0 < np.linalg.det(R)
        np.testing.assert_allclose(R, Rr, atol=RTOL)
        np.testing.assert_allclose(t, tr, rtol=RTOL, atol=RTOL * tscale)
        mapped = s * x64 @ R.T + t
        golden_mapped = d["sim_n3_s"] * x64 @ d["sim_n3_R"].T + d["sim_n3_t"]
        np.testing.assert_allclose(mapped, golden_mapped, rtol=RTOL, atol=RTOL * tscale)
    else:
        for Rw, tw in ((d[f"sim_{name}_R"], d[f"sim_{name}_t"]), (Rr, tr)):
            np.testing.assert_allclose(R, Rw, atol=RTOL)
            np.testing.assert_allclose(t, tw, rtol=RTOL, atol=RTOL * tscale)
        assert abs(np.linalg.det(R) - 1) < 1e-12


def test_slam_utils_drop_in_matches_golden(golden_dir):
    from bodyslam_amd.slam_utils import estimate_similarity_transformation
    d = load_golden(golden_dir)
    for name in ("n50", "n50_reflection", "n5000"):
        x, y = d[f"sim_{name}_source"].astype(np.float64), d[f"sim_{name}_target"].astype(np.float64)
        R, s, t = estimate_similarity_transformation(x.T, y.T)                        # the reference's [3, n]
        assert R.shape == (3, 3) and t.shape == (3,) and isinstance(s, float)
        np.testing.assert_allclose(s, d[f"sim_{name}_s"], rtol=RTOL)
        np.testing.assert_allclose(R, d[f"sim_{name}_R"], atol=RTOL)
        np.testing.assert_allclose(t, d[f"sim_{name}_t"], rtol=RTOL, atol=RTOL * np.abs(y).max())
    # n3: three points span a plane and the reference's det(Sxy) rule read round-off there -- the golden holds a reflection.  The drop-in
    # returns the proper rotation; both map the source points alike (test_similarity_fit_matches_golden_and_restatement says why), so the
    # scale and the mapped points are what the public name is held to
    x, y = d["sim_n3_source"].astype(np.float64), d["sim_n3_target"].astype(np.float64)
    R, s, t = estimate_similarity_transformation(x.T, y.T)
    assert np.linalg.det(d["sim_n3_R"]) < 0 < np.linalg.det(R)
    np.testing.assert_allclose(s, d["sim_n3_s"], rtol=RTOL)
    np.testing.assert_allclose(s * x @ R.T + t, d["sim_n3_s"] * x @ d["sim_n3_R"].T + d["sim_n3_t"], rtol=RTOL, atol=RTOL * np.abs(y).max())
    # device tensors, and an unaligned view (the element-wise load form) give the same bits as the aligned one
    x = torch.from_numpy(d["sim_n5000_source"].astype(np.float32)).cuda()
    y = torch.from_numpy(d["sim_n5000_target"].astype(np.float32)).cuda()
    a = E.similarity_fit_record(x, y)
    pad_x, pad_y = torch.zeros(5000 * 3 + 1, device="cuda"), torch.zeros(5000 * 3 + 1, device="cuda")
    pad_x[1:] = x.reshape(-1)
    pad_y[1:] = y.reshape(-1)
    b = E.similarity_fit_record(pad_x[1:].view(5000, 3), pad_y[1:].view(5000, 3))
    assert pad_x[1:].data_ptr() % 16 != 0 and a.tobytes() == b.tobytes()


def test_similarity_fit_two_million_points_fp32():
    """2 000 003 fp32 points (a tail of three points after the last group of four), against fp64 numpy."""
    rng = np.random.default_rng(6)
    n = 2_000_003
    x = rng.normal(size=(n, 3)) * [2.0, 1.0, 0.5] + [10.0, -4.0, 3.0]
    R0, s0, t0 = TR.rot([0.3, -1.0, 0.5], 0.8), 0.6, np.array([1.0, 2.0, -3.0])
    y = s0 * x @ R0.T + t0 + 1e-2 * rng.normal(size=(n, 3))
    x32, y32 = x.astype(np.float32), y.astype(np.float32)
    rec = E.similarity_fit_record(torch.from_numpy(x32).cuda(), torch.from_numpy(y32).cuda())
    R, s, t = rec[:9].reshape(3, 3), rec[9], rec[10:13]
    assert rec[15] == n and rec[14] == 3
    # the same fp32 values through the restatement: both sides run fp64 arithmetic on identical inputs
    Rr, sr, tr, _ = TR.umeyama(x32.astype(np.float64), y32.astype(np.float64), rule="evo")
    print(f"device vs restatement on the fp32 inputs: ds/s {abs(s / sr - 1):.3e} max|dR| {np.abs(R - Rr).max():.3e} max|dt| {np.abs(t - tr).max():.3e}")
    np.testing.assert_allclose(s, sr, rtol=RTOL)
    np.testing.assert_allclose(R, Rr, atol=RTOL)
    np.testing.assert_allclose(t, tr, rtol=RTOL, atol=RTOL * np.abs(y).max())
    # against the unrounded source: the tolerance is what rounding the inputs to fp32 does to the restatement itself (measured here)
    # plus the fp64 bar to the restatement above -- the triangle inequality, the bar counted twice for the second-order terms
    Rf, sf, tf, _ = TR.umeyama(x, y, rule="evo")
    ds, dR, dt_ = abs(sr / sf - 1), np.abs(Rr - Rf).max(), np.abs(tr - tf).max()
    print(f"restatement fp32-rounded vs fp64 inputs (sets the tolerance): ds/s {ds:.3e} max|dR| {dR:.3e} max|dt| {dt_:.3e}")
    print(f"device vs fp64 inputs: ds/s {abs(s / sf - 1):.3e} max|dR| {np.abs(R - Rf).max():.3e} max|dt| {np.abs(t - tf).max():.3e}")
    assert abs(s / sf - 1) <= ds + 2 * RTOL
    assert np.abs(R - Rf).max() <= dR + 2 * RTOL
    assert np.abs(t - tf).max() <= dt_ + 2 * RTOL * np.abs(y).max()
    assert ds < 1e-6 and dR < 1e-6                              # (fp32 rounding of two million points averages out far below 2^-24)


# ---- bs_trajectory_metrics ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TRAJ_NAMES)
def test_training_protocol_matches_golden_and_restatement(golden_dir, name):
    d = load_golden(golden_dir)
    gt, pred = golden_poses(d, f"traj_{name}_gt"), golden_poses(d, f"traj_{name}_pred")
    pred_dev = torch.from_numpy(pred).cuda()
    keep = pred_dev.clone()
    for delta in (1, 5):
        if len(gt) <= delta:
            with pytest.raises(ValueError, match="sequence 0"):
                E.evaluate_trajectory(pred_dev, gt, protocol="training", delta=delta)
            continue
        m = E.evaluate_trajectory(pred_dev, gt, protocol="training", delta=delta)
        assert_matches_restatement(m, 0, TR.evaluate_training(gt, pred, delta), gt, "training", f"{name} d{delta}")
        np.testing.assert_allclose(m.scale[0], d[f"traj_{name}_scale"], rtol=RTOL)
        np.testing.assert_allclose(m.ate.mean[0], d[f"traj_{name}_ate"], rtol=RTOL)
        assert abs(m.are.mean[0] - d[f"traj_{name}_are"]) <= ANGLE_ATOL_RAD
        np.testing.assert_allclose(m.rte.mean[0], d[f"traj_{name}_rte_d{delta}"], rtol=RTOL)
        assert abs(m.rre.mean[0] - d[f"traj_{name}_rre_d{delta}"]) <= ANGLE_ATOL_RAD
    assert torch.equal(pred_dev, keep)                           # the inputs are not scaled in place


EVO_CONFIGS = [dict(), dict(delta=5), dict(delta=5, all_pairs=True), dict(align_origin=False), dict(correct_scale=False),
               dict(align_origin=False, align=False, correct_scale=False, delta=3)]


@pytest.mark.parametrize("name", TRAJ_NAMES)
def test_evo_protocol_matches_restatement(golden_dir, name):
    d = load_golden(golden_dir)
    gt, pred = golden_poses(d, f"traj_{name}_gt"), golden_poses(d, f"traj_{name}_pred")
    for kw in EVO_CONFIGS:
        if len(gt) < kw.get("delta", 1) + 1:
            continue
        m = E.evaluate_trajectory(pred, gt, **kw)
        assert_matches_restatement(m, 0, TR.evaluate_evo(gt, pred, **kw), gt, "evo", f"{name} {kw}")
    m = E.evaluate_trajectory(pred[:, :3, :].reshape(-1, 12), gt[:, :3, :])              # KITTI rows and [N, 3, 4] are the same poses
    ref = E.evaluate_trajectory(pred, gt)
    assert m.ate.rmse.tobytes() == ref.ate.rmse.tobytes() and m.rre.std.tobytes() == ref.rre.std.tobytes()
    rd = ref.as_reference_dict(0)
    assert list(rd) == ["ATE", "RTE", "RRE"] and all(len(v) == 2 for v in rd.values())


def test_evo_protocol_recovers_a_similarity_on_device():
    from test_trajectory_eval_cpu import similarity_of
    rng = np.random.default_rng(1)
    gt = TR.random_walk(rng, 300)
    s, R, t = 2.5, TR.rot([0.2, 1.0, -0.4], 1.1), np.array([0.7, -0.3, 1.9])
    pred = similarity_of(gt, s, R, t)
    path = np.sum(np.linalg.norm(np.diff(gt[:, :3, 3], axis=0), axis=1))
    m = E.evaluate_trajectory(pred, gt, align_origin=False)
    print("ATE rmse / path", m.ate.rmse[0] / path)
    assert m.ate.rmse[0] < 1e-12 * path
    np.testing.assert_allclose(m.scale[0], s, rtol=1e-12)
    np.testing.assert_allclose(m.rotation[0], R, atol=1e-12)
    np.testing.assert_allclose(m.translation[0], t, atol=1e-12 * path)


def _records(pred, gt, **kw):
    m = E.evaluate_trajectory(pred, gt, **kw)
    return np.concatenate([np.stack([getattr(getattr(m, n), s) for n in ("ate", "are", "rte", "rre") for s in TR.STATS], axis=1),
                           m.scale[:, None], m.rotation.reshape(-1, 9), m.translation], axis=1)


def test_ragged_batch_is_bit_equal_to_its_pairs_and_to_a_rerun():
    rng = np.random.default_rng(8)
    gts = [TR.random_walk(rng, n) for n in (3, 24, 1000, 4000)]
    preds = [TR.perturbed(rng, g) for g in gts]
    for kw in (dict(), dict(protocol="training", delta=2)):
        a = _records(preds, gts, **kw)
        b = _records(preds, gts, **kw)
        assert a.tobytes() == b.tobytes(), kw
        assert np.all(np.isfinite(a))
        for i in range(4):
            assert _records(preds[i], gts[i], **kw).tobytes() == a[i:i + 1].tobytes(), (kw, i)
        rev = _records(preds[::-1], gts[::-1], **kw)                      # other positions in another batch
        assert rev[::-1].tobytes() == a.tobytes(), kw
    # S = 256 sequences of 1000 poses: one walk and its prediction under 256 different rigid motions and scales (device tensors)
    base_g, base_p = gts[2], preds[2]
    G, P = [], []
    for k in range(256):
        A = np.eye(4)
        A[:3, :3], A[:3, 3] = TR.rot(rng.normal(size=3), rng.uniform(0.1, 3.0)), rng.normal(size=3)
        g, p = A @ base_g, np.linalg.inv(A) @ base_p
        p[:, :3, 3] *= rng.uniform(0.2, 5.0)
        G.append(torch.from_numpy(g).cuda())
        P.append(torch.from_numpy(p).cuda())
    a = _records(P, G, delta=4)
    assert a.tobytes() == _records(P, G, delta=4).tobytes()
    assert np.all(np.isfinite(a)) and len(np.unique(a[:, 20])) == 256          # 256 different scales: no record is another's copy
    for k in range(256):
        assert _records(P[k], G[k], delta=4).tobytes() == a[k:k + 1].tobytes(), k


def test_device_poses_of_run_sequence_equal_their_host_copy():
    import dataclasses

    from bodyslam_amd.pipeline import BodySlamPipeline
    from bodyslam_amd.synthetic import make_sequence
    from bodyslam_amd.zoedepth import ZoeConfig
    from oracle import cyclepose_ref as CP
    from oracle import zoedepth_ref as Z
    cfg_o = Z.ZoeConfig(hidden=128, layers=4, heads=2, intermediate=256, taps=(1, 2, 3, 4), image_size=64)
    names = {f.name for f in dataclasses.fields(ZoeConfig)}
    cfg_p = ZoeConfig(**{k: v for k, v in dataclasses.asdict(cfg_o).items() if k in names})
    pipe = BodySlamPipeline(Z.synth_weights(cfg_o, seed=2), CP.synth_weights(seed=2), cfg_p, batch=2, target_hw=(64, 96))
    res = pipe.run_sequence(make_sequence(6, 160, 192, seed=5))
    assert res.g_abs.is_cuda and res.g_abs.dtype == torch.float64 and tuple(res.g_abs.shape) == (6, 4, 4)
    host = res.g_abs.cpu().numpy()
    gt = TR.perturbed(np.random.default_rng(12), host, scale=2.0)
    before = res.g_abs.clone()
    for kw in (dict(), dict(protocol="training"), dict(delta=2, all_pairs=True)):
        assert _records(res.g_abs, gt, **kw).tobytes() == _records(host, gt, **kw).tobytes(), kw
        assert _records(res.g_abs, torch.from_numpy(gt).cuda(), **kw).tobytes() == _records(host, gt, **kw).tobytes(), kw
    assert torch.equal(res.g_abs, before)
    m = E.evaluate_trajectory(res.g_abs, gt)
    assert_matches_restatement(m, 0, TR.evaluate_evo(gt, host), gt, "evo", "run_sequence")


def test_nothing_is_written_past_the_outputs():
    rng = np.random.default_rng(9)
    dev = torch.device("cuda")
    L.init(0)
    guard = 256
    # bs_trajectory_metrics: S records inside a larger buffer
    gts = [TR.random_walk(rng, n) for n in (3, 50, 700)]
    preds = [TR.perturbed(rng, g) for g in gts]
    g_all = torch.from_numpy(np.concatenate(gts)).to(dev).reshape(-1, 16)
    p_all = torch.from_numpy(np.concatenate(preds)).to(dev).reshape(-1, 16)
    offsets = torch.tensor([0, 3, 53, 753], dtype=torch.int32, device=dev)
    S, F = 3, L.TRAJ_FIELDS
    for protocol in (L.TRAJ_EVO, L.TRAJ_TRAINING):
        buf = torch.full((guard + S * F + guard,), -7.0, dtype=torch.float64, device=dev)
        L.trajectory_metrics(g_all, p_all, offsets, protocol, 1, L.TRAJ_ALIGN_ORIGIN | L.TRAJ_ALIGN | L.TRAJ_CORRECT_SCALE, buf[guard:guard + S * F].view(S, F))
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        assert np.all(h[:guard] == -7.0) and np.all(h[guard + S * F:] == -7.0)
        assert np.all(h[guard:guard + S * F] != -7.0)                # every field of every record is written
    # bs_similarity_fit: the workspace at its declared size and the 16 outputs, each inside a larger buffer
    W = L.SIMILARITY_FIT_WORKSPACE_BYTES
    for n, dt in ((7, torch.float32), (100_001, torch.float32), (600_000, torch.float64), (3_000_001, torch.float32)):
        x = torch.from_numpy(rng.normal(size=(n, 3))).to(dev, dt)
        y = (2.0 * x + 1.0).contiguous()
        ws = torch.full((guard + W + guard,), 0xAB, dtype=torch.uint8, device=dev)
        out = torch.full((guard + 16 + guard,), -7.0, dtype=torch.float64, device=dev)
        L.similarity_fit(x, y, ws[guard:guard + W], out[guard:guard + 16])
        torch.cuda.synchronize()
        hw, ho = ws.cpu().numpy(), out.cpu().numpy()
        assert np.all(hw[:guard] == 0xAB) and np.all(hw[guard + W:] == 0xAB), n
        assert np.all(ho[:guard] == -7.0) and np.all(ho[guard + 16:] == -7.0), n
        np.testing.assert_allclose(ho[guard + 9], 2.0, rtol=1e-6 if dt == torch.float32 else 1e-12)
    with pytest.raises(L.BodySlamHipError):                          # a workspace one byte short is refused, not overrun
        L.similarity_fit(x, y, ws[guard:guard + W - 1], out[guard:guard + 16])


def test_degenerate_and_short_sequences_set_only_their_own_status():
    rng = np.random.default_rng(10)
    dev = torch.device("cuda")
    L.init(0)
    good = TR.random_walk(rng, 60)
    good_p = TR.perturbed(rng, good)
    line = np.tile(np.eye(4), (20, 1, 1))
    # (millimetre steps: the criterion is evo's absolute one, singular values above eps = 2.2e-16, and the round-off that stands in for the
    # two vanishing singular values is about 1e-16 of the largest -- at this size it lies four orders below eps in any arithmetic)
    line[:, :3, 3] = np.outer(np.arange(20), [0.001, 0.002, -0.0005])
    line_p = line.copy()
    line_p[:, :3, 3] *= 0.5
    still_p = np.tile(np.eye(4), (20, 1, 1))                            # no motion at all: sigma_x = 0
    short = TR.random_walk(rng, 3)
    gts = [good, line, short, good, line, good[:2]]
    preds = [good_p, line_p, TR.perturbed(rng, short), good_p, still_p, good_p[:2]]
    lengths = [len(g) for g in gts]
    g_all = torch.from_numpy(np.concatenate(gts)).to(dev).reshape(-1, 16)
    p_all = torch.from_numpy(np.concatenate(preds)).to(dev).reshape(-1, 16)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32, device=dev)
    flags = L.TRAJ_ALIGN_ORIGIN | L.TRAJ_ALIGN | L.TRAJ_CORRECT_SCALE
    out = torch.empty(6, L.TRAJ_FIELDS, dtype=torch.float64, device=dev)
    L.trajectory_metrics(g_all, p_all, offsets, L.TRAJ_EVO, 4, flags, out)
    rec = out.cpu().numpy()
    assert list(rec[:, 2]) == [L.TRAJ_OK, L.TRAJ_DEGENERATE, L.TRAJ_TOO_SHORT, L.TRAJ_OK, L.TRAJ_DEGENERATE, L.TRAJ_TOO_SHORT]
    assert list(rec[:, 0]) == lengths
    for i in (1, 2, 4, 5):
        assert np.all(np.isnan(rec[i, 3:36])), i
    alone = torch.empty(1, L.TRAJ_FIELDS, dtype=torch.float64, device=dev)
    L.trajectory_metrics(g_all[:60], p_all[:60], offsets[:2], L.TRAJ_EVO, 4, flags, alone)
    assert rec[0].tobytes() == alone.cpu().numpy()[0].tobytes() and rec[3].tobytes() == rec[0].tobytes()
    assert np.all(np.isfinite(rec[0]))
    # offsets that leave the arrays are reported, and nothing of that pair is read
    bad = torch.tensor([0, 60, 10_000_000], dtype=torch.int32, device=dev)
    out2 = torch.empty(2, L.TRAJ_FIELDS, dtype=torch.float64, device=dev)
    L.trajectory_metrics(g_all, p_all, bad, L.TRAJ_EVO, 4, flags, out2)
    rec2 = out2.cpu().numpy()
    assert rec2[0].tobytes() == rec[0].tobytes() and rec2[1, 2] == L.TRAJ_BAD_OFFSETS
    # the Python surface names the sequence
    with pytest.raises(ValueError, match="sequence 1"):
        E.evaluate_trajectory([good_p, line_p], [good, line])
    with pytest.raises(ValueError, match="sequence 0"):
        E.evaluate_trajectory(good_p[:2], good[:2])                     # two poses: rank 1


def test_kitti_files_and_csv(golden_dir, tmp_path):
    from bodyslam_amd.slam_utils import save_poses_as_kitti
    src = os.path.join(golden_dir, "kitti_poses_24.txt")
    gt = E.read_kitti_poses(src)
    pred = TR.perturbed(np.random.default_rng(11), gt)
    pp = str(tmp_path / "seq_a.txt")
    save_poses_as_kitti(list(pred), pp)
    m = E.evaluate_trajectory_files([pp], [src], results_dir=str(tmp_path / "results"))
    ref = E.evaluate_trajectory(pred, gt)
    assert m.ate.rmse.tobytes() == ref.ate.rmse.tobytes() and m.rre.rmse.tobytes() == ref.rre.rmse.tobytes()
    text = open(tmp_path / "results" / "seq_a.csv", newline="").read().split("\r\n")
    assert text[0] == "Metric,Value" and text[1] == f'ATE,"{m.as_reference_dict(0)["ATE"]}"' and len(text) == 5
    # project_so3: the reference's correct_poses, through ensure_so3_v2
    skew = pred.copy()
    skew[:, :3, :3] *= 1.001
    ps = str(tmp_path / "skew.txt")
    save_poses_as_kitti(list(skew), ps)
    fixed = E.read_kitti_poses(ps, project_so3=True)
    np.testing.assert_allclose(fixed[:, :3, :3], pred[:, :3, :3], atol=1e-9)
    assert np.array_equal(fixed[:, :3, 3], skew[:, :3, 3])
