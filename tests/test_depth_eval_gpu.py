"""Depth evaluation on the device (bs_depth_metrics through bodyslam_amd.evaluation): the reference's golden metrics, the restatement
tests/_depth_eval_ref.py on random frames, bitwise reproducibility and batch invariance, a sequence of the pipeline, and PNG input."""
import os

import numpy as np
import pytest

import _depth_eval_ref as R
from test_depth_eval_cpu import assert_metrics_match, load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from bodyslam_amd import evaluation as E  # noqa: E402

LOG_ATOL_REST = 1e-12        # against the restatement both sides take the correctly rounded fp32 log g; log p is fp64 on both


def device_eval(pred, gt, protocol="hamlyn", gt_range=None, scale=None):
    return E.evaluate_depth(pred, gt, protocol=protocol, gt_range=gt_range, scale=scale).per_frame


def test_golden_on_device(golden_dir):
    d = load_golden(golden_dir)
    ref = {k: d[k] for k in R.PER_FRAME_NAMES}
    n = len(d["names"])
    got = {k: np.empty(n) for k in R.PER_FRAME_NAMES}
    for i in range(n):
        sc = None if np.isnan(d["scale_in"][i]) else float(d["scale_in"][i])
        r = device_eval(d["pred"][i], d["gt"][i], gt_range=(float(d["gt_lo"][i]), float(d["gt_hi"][i])), scale=sc)
        for k in R.PER_FRAME_NAMES:
            got[k][i] = r[k][0]
    assert_metrics_match(got, ref)


def smooth_frames(rng, B, H, W, lo, hi):
    y, x = np.mgrid[0:H, 0:W] / np.array([max(H, 1), max(W, 1)])[:, None, None]
    out = np.empty((B, H, W), np.uint16)
    for b in range(B):
        a = rng.uniform(0, 6.3, 3)
        z = 0.5 + 0.3 * np.sin(4 * x + a[0]) * np.cos(3 * y + a[1]) + 0.15 * np.sin(9 * x * y + a[2])
        out[b] = np.clip(lo + (hi - lo) * z + rng.normal(0, 0.02 * (hi - lo), (H, W)), lo, hi).astype(np.uint16)
    return out


CASES = [(1, 1, 1), (1, 37, 53), (1, 480, 640), (3, 1, 1), (3, 37, 53), (3, 480, 640), (64, 1, 1), (64, 37, 53), (64, 480, 640)]


@pytest.mark.parametrize("B,H,W", CASES)
def test_random_frames_match_restatement(B, H, W):
    rng = np.random.default_rng(B * 1000 + H)
    protocol = ("hamlyn", "scared", "endoslam")[(B + H) % 3]
    gt = smooth_frames(rng, B, H, W, 0, 400 if protocol == "hamlyn" else 5000)
    gt[rng.random(gt.shape) < 0.15] = 0
    pred = smooth_frames(rng, B, H, W, 0, 3000)
    pred[rng.random(pred.shape) < 0.05] = 0
    # host numpy input for the small shapes, device tensors (int16 storage) for the full-size one
    if H * W > 10000:
        got = device_eval(torch.from_numpy(pred.view(np.int16)).cuda(), torch.from_numpy(gt.view(np.int16)).cuda(), protocol)
    else:
        got = device_eval(pred, gt, protocol)
    lo, hi = R.PROTOCOLS[protocol]
    ref = R.evaluate(pred, gt, lo, hi)
    assert_metrics_match(got, ref, log_atol=LOG_ATOL_REST, frames=(B, H, W, protocol))


@pytest.mark.parametrize("protocol", ["hamlyn", "scared", "endoslam"])
def test_protocols_range_and_fixed_scale(protocol):
    rng = np.random.default_rng(7)
    gt = smooth_frames(rng, 5, 37, 53, 0, 2500)
    gt[rng.random(gt.shape) < 0.2] = 0
    pred = smooth_frames(rng, 5, 37, 53, 1, 900)
    lo, hi = R.PROTOCOLS[protocol]
    assert_metrics_match(device_eval(pred, gt, protocol), R.evaluate(pred, gt, lo, hi), log_atol=LOG_ATOL_REST)
    for rng_ in [(100.0, 2000.0), (0.5, 299.5), (-5.0, 1e9)]:
        assert_metrics_match(device_eval(pred, gt, protocol, gt_range=rng_), R.evaluate(pred, gt, *rng_), log_atol=LOG_ATOL_REST)
    for sc in (1000.0 / 256.0, 0.0, np.inf):
        assert_metrics_match(device_eval(pred, gt, protocol, scale=sc), R.evaluate(pred, gt, lo, hi, scale=sc), log_atol=LOG_ATOL_REST)


def test_extreme_values_and_one_high_byte():
    rng = np.random.default_rng(11)
    B, H, W = 4, 61, 67
    gt = rng.integers(0, 65536, (B, H, W)).astype(np.uint16)
    pred = rng.integers(0, 65536, (B, H, W)).astype(np.uint16)
    gt[:, ::3] = 65535
    gt[:, 1::5] = 0
    pred[:, ::4] = 65535
    pred[:, 2::7] = 0
    for protocol in ("endoslam", "scared"):
        lo, hi = R.PROTOCOLS[protocol]
        assert_metrics_match(device_eval(pred, gt, protocol), R.evaluate(pred, gt, lo, hi), log_atol=LOG_ATOL_REST)
    # every pixel of a map in one high-byte bucket: the whole median search happens in the low byte (both middle ranks in one bucket)
    gt1 = (0x1200 | rng.integers(0, 256, (B, 480, 640))).astype(np.uint16)
    pred1 = (0x0300 | rng.integers(0, 256, (B, 480, 640))).astype(np.uint16)
    assert_metrics_match(device_eval(pred1, gt1, "scared"), R.evaluate(pred1, gt1, 0.0, np.inf), log_atol=LOG_ATOL_REST)
    # the two middle ranks in two different buckets: n even, half the values at 0x00ff, half at 0x0100
    g2 = np.where(np.arange(480 * 640).reshape(480, 640) % 2 == 0, 0x00FF, 0x0100).astype(np.uint16)[None]
    p2 = np.where(np.arange(480 * 640).reshape(480, 640) % 3 == 0, 0x02FF, 0x0300).astype(np.uint16)[None]
    got = device_eval(p2, g2, "endoslam")
    assert got["median_gt"][0] == 255.5
    assert_metrics_match(got, R.evaluate(p2, g2, -np.inf, np.inf), log_atol=LOG_ATOL_REST)


def test_bitwise_reproducible_and_batch_invariant():
    rng = np.random.default_rng(5)
    for H, W in ((480, 640), (37, 53)):              # the 16-byte load form and the element form
        gt = smooth_frames(rng, 64, H, W, 0, 400)
        pred = smooth_frames(rng, 64, H, W, 0, 3000)
        pd_, gd = torch.from_numpy(pred.view(np.int16)).cuda(), torch.from_numpy(gt.view(np.int16)).cuda()
        a = device_eval(pd_, gd)
        b = device_eval(pd_, gd)
        for k in R.PER_FRAME_NAMES:
            assert a[k].tobytes() == b[k].tobytes(), k
        for j in (0, 17, 63):
            one = device_eval(pd_[j:j + 1], gd[j:j + 1])
            for k in R.PER_FRAME_NAMES:
                assert one[k].tobytes() == a[k][j:j + 1].tobytes(), (H, W, j, k)
        sub = device_eval(pd_[5:8], gd[5:8])                 # another position in another batch
        for k in R.PER_FRAME_NAMES:
            assert sub[k].tobytes() == a[k][5:8].tobytes(), (H, W, k)


def test_pipeline_sequence_depth_on_device():
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
    res = pipe.run_sequence(make_sequence(3, 160, 192, seed=5))
    assert res.depth_u16.dtype == torch.int16 and res.depth_u16.is_cuda
    host = res.depth_u16.cpu().numpy().view(np.uint16)
    rng = np.random.default_rng(3)
    # a GT in mm from the prediction (metres * 256): a smooth multiplicative error and SCARED-like holes
    gt = np.rint(host.astype(np.float64) * (1000.0 / 256.0) * rng.uniform(0.9, 1.1, host.shape)).clip(0, 65535).astype(np.uint16)
    gt[rng.random(gt.shape) < 0.1] = 0
    for protocol, scale in (("scared", None), ("scared", 1000.0 / 256.0), ("endoslam", None)):
        got = device_eval(res.depth_u16, torch.from_numpy(gt.view(np.int16)).cuda(), protocol, scale=scale)
        lo, hi = R.PROTOCOLS[protocol]
        assert_metrics_match(got, R.evaluate(host, gt, lo, hi, scale=scale), log_atol=LOG_ATOL_REST)
        assert np.all(np.isfinite(got["abs_rel_diff"]))


def test_png_files_match_arrays(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(9)
    gt = smooth_frames(rng, 5, 48, 64, 0, 400)
    pred = smooth_frames(rng, 5, 48, 64, 200, 2000)
    pp, gp = [], []
    for i in range(5):
        pp.append(str(tmp_path / f"pred_{i:04d}.png"))
        gp.append(str(tmp_path / f"gt_{i:04d}.png"))
        Image.fromarray(pred[i]).save(pp[-1])
        Image.fromarray(gt[i]).save(gp[-1])
    out = tmp_path / "results"
    m = E.evaluate_depth_files(pp, gp, protocol="hamlyn", results_dir=str(out), batch=2)
    a = device_eval(pred, gt, "hamlyn")
    for k in R.PER_FRAME_NAMES:
        assert m.per_frame[k].tobytes() == a[k].tobytes(), k
    assert os.path.exists(out / "results.csv") and os.path.exists(out / "avg.csv")
