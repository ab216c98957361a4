"""Full-size ZoeD_NK on the image-major backbone path against the fp32 oracle.

_ZoePlan runs the table attention (grouped token rows, bs_attention_table*, the cheap "wcls" / "wmean" / "wstat" corrections) only for
512-wide network inputs with at most 40 patch rows.  Every other frame geometry takes the image-major path: token rows image by image,
the generic bs_attention kernel with a host-built [heads, Sp, Sp] bias per layer, no split-precision attention, both FP8 corrections on
every row in accurate mode.  Frames of 320x320 (384x384 network input, S = 577), 720x1280 (16:9: 384x672, S = 1009) and 640 tall x
480 wide (672x512, S = 1345) run it here at the real configuration: hidden 1024, 16 heads, 24 layers.
Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import torch

from test_zoedepth_gpu import compare_taps, oracle_case, product_cfg, report, run_case

pytestmark = pytest.mark.gpu

SEED = 1        # one weight set for every geometry (the calibration cache then serves the batch test)


def assert_image_major(plan):
    """the plan runs the image-major backbone: a routing change must fail here, not quietly test the table path instead"""
    assert not plan.grouped, f"{plan.geom}: grouped token rows (the table path)"
    assert not plan.attn_corr, f"{plan.geom}: split-precision attention (the table path)"
    kinds = {getattr(fn, "__name__", fn) for fn, _ in plan.plan.calls}
    assert "bs_attention" in kinds, f"{plan.geom}: no bs_attention launch"
    assert not any(str(k).startswith("bs_attention_table") for k in kinds), f"{plan.geom}: table attention launches"


def depth_errors(r, tag):
    d = r["dm"] - r["ref"]
    l1, mx = d.abs().mean().item(), d.abs().max().item()
    lsb = np.abs(r["du"].astype(np.int32) - r["Z"].to_uint16(r["ref"]).astype(np.int32))
    report(f"[{tag}] depth L1={l1:.3e} m, max={mx:.3e} m (depth range {r['ref'].min():.3f}..{r['ref'].max():.3f} m); "
           f"u16: max |diff| = {lsb.max()} LSB, mean {lsb.mean():.3f} LSB; oracle forward {r['t_oracle']:.1f} s")
    return l1


# (frame H, W, dtype, precision), ordered so that consecutive cases share the oracle's forward (it is cached per case)
CASES = [(720, 1280, torch.float16, "fast"), (720, 1280, torch.float16, "accurate"), (720, 1280, torch.bfloat16, "fast"),
         (640, 480, torch.float16, "fast"), (640, 480, torch.float16, "accurate"),
         (320, 320, torch.float16, "fast"), (320, 320, torch.float16, "accurate")]


@pytest.mark.parametrize("H,W,dtype,precision", CASES, ids=[f"{h}x{w}-{str(d)[6:]}-{p}" for h, w, d, p in CASES])
def test_image_major_full_size(H, W, dtype, precision):
    """tap by tap to TAP_TOL, the oracle's route, and the depth map: fast fp16 < 1e-3 m, fast bf16 < 1e-2 m, accurate fp16 <= 1e-4 m (the
    north star) -- with the engine calibrated at this geometry, where the calibration's reference engine has no split attention either"""
    from oracle import zoedepth_ref as Z
    r = run_case(Z.ZOED_NK, dtype, B=1, H=H, W=W, target_hw=(384, 512), seed=SEED, precision=precision)
    plan = r["eng"].plan_for(1, H, W, True)
    assert_image_major(plan)
    tname = "f16" if dtype == torch.float16 else "bf16"
    tag = f"image-major {W}x{H} ({plan.geom['nw']}x{plan.geom['nh']}, S {plan.geom['S']}) {tname} {precision}"
    if r["calibration"] is not None:
        cal = r["calibration"]
        report(f"[{tag}] calibration: classes {cal['class_modes']}, attention {cal.get('attn_mode')}, "
               f"vs reference {cal.get('l1_abs_vs_reference_m')}, warning {cal.get('warning')}")
    compare_taps(r["taps_p"], r["taps_o"], None, tag, tol=(precision, tname))          # (TAP_TOL of test_zoedepth_gpu.py)
    assert torch.equal(torch.argmax(r["logits_o"], -1).int(), r["route_p"])
    l1 = depth_errors(r, tag)
    if precision == "accurate":
        assert l1 <= 1e-4
    else:
        assert l1 < (1e-3 if dtype == torch.float16 else 1e-2)


def test_calibration_made_on_the_table_path_holds_on_the_image_major_path():
    """plan_for() calibrates once, at the first plan's geometry.  An accurate engine whose first frames are 480x640 (table path: its
    calibration decides with the split-precision attention at hand) then serves 320x320 frames (image-major: no split attention) on
    that same calibration; the 320x320 depth must still meet 1e-4 m against the oracle."""
    from bodyslam_amd.synthetic import make_sequence
    from bodyslam_amd.zoedepth import ZoeDepthEngine
    from oracle import zoedepth_ref as Z
    w, frames, taps_o, logits_o, ref, t_or = oracle_case(Z.ZOED_NK, 1, 320, 320, (384, 512), SEED, 0.0, True)
    eng = ZoeDepthEngine(w, product_cfg(Z.ZOED_NK), dtype=torch.float16, target_hw=(384, 512), precision="accurate")
    eng.infer(torch.from_numpy(make_sequence(2, 480, 640, seed=5)).cuda())
    cal = eng.calibration
    assert cal is not None and eng.plan_for(2, 480, 640, True).grouped
    dm, _ = eng.infer(frames.cuda())
    torch.cuda.synchronize()
    plan = eng.plan_for(1, 320, 320, True)
    assert_image_major(plan)
    assert eng.calibration is cal, "the 320x320 plan was built on another calibration than the 480x640 one"
    assert torch.equal(torch.argmax(logits_o, -1).int(), plan.route.cpu())
    d = dm.cpu() - ref
    l1 = d.abs().mean().item()
    report(f"[320x320 on the 480x640 calibration: classes {cal['class_modes']}, attention {cal.get('attn_mode')}] depth L1={l1:.3e} m, "
           f"max={d.abs().max().item():.3e} m")
    assert l1 <= 1e-4


def test_image_major_batch_equals_single_frame_plan():
    """test_bench_batch_equals_single_frame_plan on the image-major path: 720x1280 frames, accurate fp16, B = 64 (128 network inputs of
    384x672): frames 0, 17 and 63 give exactly the bits and the routes of the B = 1 plan."""
    from bodyslam_amd.synthetic import make_sequence
    from bodyslam_amd.zoedepth import ZoeDepthEngine
    from oracle import zoedepth_ref as Z
    B, H, W = 64, 720, 1280
    eng = ZoeDepthEngine(Z.synth_weights(Z.ZOED_NK, seed=SEED), product_cfg(Z.ZOED_NK), dtype=torch.float16, target_hw=(384, 512),
                         precision="accurate")
    frames = torch.from_numpy(make_sequence(B, H, W, seed=0)).cuda()
    dm, du = eng.infer(frames)
    dm, du = dm.clone(), du.clone()
    plan = eng.plan_for(B, H, W, True)
    assert_image_major(plan)
    route = plan.route.clone()
    assert torch.isfinite(dm).all() and (dm > 0).all()
    sample = (0, 17, B - 1)
    for i in sample:
        d1, u1 = eng.infer(frames[i:i + 1])
        assert torch.equal(d1[0], dm[i]), f"frame {i}: B={B} plan differs from the B=1 plan (max {(d1[0] - dm[i]).abs().max().item():.3e})"
        assert torch.equal(u1[0], du[i])
        assert torch.equal(eng.plan_for(1, H, W, True).route, route[[i, B + i]])       # frame i and its flipped copy
    report(f"image-major {W}x{H}: B={B} plan == B=1 plan on frames {sample} [f16 accurate]")
    del eng, plan
    torch.cuda.empty_cache()
