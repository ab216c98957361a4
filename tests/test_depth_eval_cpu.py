"""Depth evaluation (bodyslam_amd.evaluation, bs_depth_metrics) without a GPU: the restatement tests/_depth_eval_ref.py against the
reference's own metrics (tests/golden/depth_eval.npz, tools/make_depth_eval_golden.py), the CSV layout, input validation, and the
missing CPU fallback."""
import csv
import io
import math
import os

import numpy as np
import pytest

import _depth_eval_ref as R
from bodyslam_amd import _lib as L
from bodyslam_amd import evaluation as E

EXACT = ("accuracy_1.25", "accuracy_(1.25)^2", "accuracy_(1.25)^3", "scale", "median_gt", "median_pred", "n_mask", "n_valid", "n_pos")
# rmse_log: log(gt) is an fp32 value and fp32 logs differ by up to 1 ulp between implementations (numpy's SIMD loops and the correctly
# rounded value here: 1988 of the 65535 uint16 inputs, |difference| <= 2^-20 for log g < 16).  By the triangle inequality of the RMS,
# rmse_log then moves by at most 2^-20 absolutely -- which is more than 1e-7 relative where rmse_log itself is small
LOG_ATOL = 2.0 ** -20


def load_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "depth_eval.npz"))


def assert_metrics_match(got, ref, log_atol=LOG_ATOL, rtol=1e-12, frames=None):
    """got / ref: name -> float64 [B].  Exact where the contract is exact; non-finite values must sit where the reference has them."""
    for k in R.PER_FRAME_NAMES:
        a, b = np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
        assert a.shape == b.shape, (k, a.shape, b.shape)
        where = f"{k}, frames {frames if frames is not None else ''}"
        assert np.array_equal(np.isnan(a), np.isnan(b)), (where, a, b)
        assert np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(np.isneginf(a), np.isneginf(b)), (where, a, b)
        fin = np.isfinite(b)
        if k in EXACT:
            assert np.array_equal(a[fin], b[fin]), (where, a, b)
        elif k == "rmse_log":
            err = np.abs(a[fin] - b[fin])
            assert np.all(err <= 1e-7 * np.abs(b[fin]) + log_atol), (where, a, b, err.max(initial=0.0))
        else:
            assert np.allclose(a[fin], b[fin], rtol=rtol, atol=0.0), (where, a, b)


def test_restatement_matches_reference_golden(golden_dir):
    d = load_golden(golden_dir)
    ref = {k: d[k] for k in R.PER_FRAME_NAMES}
    rows = []
    for i in range(len(d["names"])):
        sc = None if np.isnan(d["scale_in"][i]) else float(d["scale_in"][i])
        rows.append(R.frame_metrics(d["pred"][i], d["gt"][i], float(d["gt_lo"][i]), float(d["gt_hi"][i]), sc))
    got = {k: np.array([r[k] for r in rows]) for k in R.PER_FRAME_NAMES}
    assert_metrics_match(got, ref)
    names = list(d["names"])
    # the degenerate frames as the contract states them
    i = names.index("empty_mask")
    assert all(math.isnan(got[k][i]) for k in R.METRIC_NAMES + ("scale", "median_gt", "median_pred"))
    i = names.index("median_pred_zero")
    assert [got[k][i] for k in R.METRIC_NAMES] == [math.inf] * 4 + [0.0] * 3
    i = names.index("all_equal")
    assert got["accuracy_1.25"][i] == 1.0 and got["median_gt"][i] == 123.0 and got["median_pred"][i] == 77.0
    # odd / even masked counts, and EndoSlam's median over GT zeros
    assert int(d["n_mask"][names.index("hamlyn_odd")]) % 2 == 1 and int(d["n_mask"][names.index("hamlyn_even")]) % 2 == 0
    i = names.index("endoslam_zeros")
    assert d["n_mask"][i] == d["gt"][i].size and np.count_nonzero(d["gt"][i] == 0) > 0 and d["n_valid"][i] < d["n_mask"][i]


def test_protocol_masks():
    assert E.PROTOCOLS == R.PROTOCOLS
    assert E.METRIC_NAMES == R.METRIC_NAMES and E.PER_FRAME_NAMES == R.PER_FRAME_NAMES


def test_csv_layout_matches_reference_writers(tmp_path, golden_dir):
    pd = pytest.importorskip("pandas")
    d = load_golden(golden_dir)
    m = E.DepthMetrics({k: d[k].copy() for k in E.PER_FRAME_NAMES})
    results, avg = m.write_csv(str(tmp_path / "seq"))
    # results.csv: CSVIO.write_metrics_on_cvs (UTILS/io_utils.py:247-258) -- csv.DictWriter over the per-frame dicts of
    # MDEM_eval.py:220-228, numpy float64 values, file opened with newline=''
    buf = io.StringIO(newline="")
    w = csv.DictWriter(buf, fieldnames=list(E.METRIC_NAMES))
    w.writeheader()
    for i in range(len(d["names"])):
        w.writerow({k: np.float64(d[k][i]) for k in E.METRIC_NAMES})
    with open(results, newline="") as f:
        assert f.read() == buf.getvalue()
    # avg.csv: pd.read_csv(results).mean().to_csv(header=True) (MDEM_eval.py:247-254)
    want = pd.read_csv(results).mean().to_csv(header=True)
    with open(avg) as f:
        have = f.read()
    wl, hl = want.splitlines(), have.splitlines()
    assert len(wl) == len(hl) and wl[0] == hl[0] == ",0"
    for a, b in zip(wl[1:], hl[1:]):
        ka, va = a.split(",")
        kb, vb = b.split(",")
        assert ka == kb
        assert (va == vb == "") or math.isclose(float(va), float(vb), rel_tol=1e-14), (a, b)
    mean = m.mean()
    assert list(mean) == list(E.METRIC_NAMES)
    for k in E.METRIC_NAMES:
        v = d[k][~np.isnan(d[k])]
        assert math.isclose(mean[k], float(np.mean(v)), rel_tol=1e-14) or (math.isinf(mean[k]) and mean[k] == float(np.mean(v)))


def test_mean_skips_nan_frames():
    pf = {k: np.array([1.0, np.nan, 3.0]) for k in E.PER_FRAME_NAMES}
    pf["rmse"] = np.array([np.nan, np.nan, np.nan])
    m = E.DepthMetrics(pf).mean()
    assert m["abs_rel_diff"] == 2.0 and math.isnan(m["rmse"])


@pytest.mark.parametrize("bad", [
    dict(pred=np.zeros((2, 4, 4), np.float32)),
    dict(gt=np.zeros((2, 4, 4), np.uint8)),
    dict(gt=np.zeros((2, 4, 5), np.uint16)),
    dict(pred=np.zeros((1, 2, 4, 4), np.uint16), gt=np.zeros((1, 2, 4, 4), np.uint16)),
    dict(pred=np.zeros((0, 4, 4), np.uint16), gt=np.zeros((0, 4, 4), np.uint16)),
    dict(pred=[[1, 2]]),
    dict(protocol="kitti"),
    dict(gt_range=(1.0,)),
    dict(scale="median"),
])
def test_input_validation(bad):
    import torch
    kw = dict(pred=np.zeros((2, 4, 4), np.uint16), gt=np.zeros((2, 4, 4), np.uint16))
    kw.update(bad)
    if bad.get("gt") is not None and isinstance(bad["gt"], np.ndarray) and bad["gt"].dtype == np.uint8:
        kw["gt"] = torch.from_numpy(bad["gt"])       # (torch input, wrong dtype)
    with pytest.raises(ValueError):
        E.evaluate_depth(**kw)


def test_png_validation(tmp_path):
    from PIL import Image
    p16 = str(tmp_path / "p.png")
    Image.fromarray(np.full((4, 6), 300, np.uint16)).save(p16)
    p8 = str(tmp_path / "g8.png")
    Image.fromarray(np.full((4, 6), 30, np.uint8)).save(p8)
    prgb = str(tmp_path / "rgb.png")
    Image.fromarray(np.zeros((4, 6, 3), np.uint8)).save(prgb)
    for bad in (p8, prgb):
        with pytest.raises(ValueError, match=os.path.basename(bad)):
            E.evaluate_depth_files([p16], [bad])
    with pytest.raises(ValueError):
        E.evaluate_depth_files([p16, p16], [p16])
    with pytest.raises(ValueError):
        E.evaluate_depth_files([p16], [p16], protocol="nyu")


def test_no_cpu_fallback(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(L, "_inited_device", None)
    with pytest.raises(L.BodySlamHipError):
        E.evaluate_depth(np.ones((1, 8, 8), np.uint16), np.ones((1, 8, 8), np.uint16))
