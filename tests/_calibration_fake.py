"""A fake measurement model for ZoeDepthEngine.calibrate, pure torch on the CPU and deterministic: what tests/test_calibration_cpu.py
replays and tools/make_calibration_traces.py records tests/golden/calibration_traces.json with.

depth = per-frame truth field + sum over the active cheap choices of amplitude x a fixed seeded unit-normal field (so a choice of
amplitude a reads an L1 of ~0.8 a, and independent choices add in quadrature), amplitudes per scenario, with an optional extra gain on the
held-out frames.  The neck is a dozen invented products with fixed FLOPs.  `installed(zd)` puts the fake in place of the launch plan, the
reference engine and the device synchronisation of the zoedepth module it is given -- this tree's, or a checkout of the parent commit's."""
import contextlib
import hashlib
import os
import warnings

import torch

# neck / head weight key -> FLOPs per network input: a per-image readout bias (w_cls) and the bins head's bottleneck conv (mh.), which are
# never candidates, the fused up-convolution (rh.conv2.w: never one-pass) and two products below AUTO_NECK_SITE_MIN_SHARE (a group)
SITES = {"rh.conv1.w": 40e9, "rh.projection.w": 20e9, "rh.conv2.w": 15e9, "fu3.r1.c1.w": 10e9, "fu2.proj.w": 5e9, "nc2.w": 2e9,
         "ra3.down.w": 1e9, "ro2.w": 0.05e9, "pj3.c1.w": 0.04e9, "ro2.w_cls": 0.5e9, "mh.conv.w": 0.3e9}
BACKBONE_KEY = "l0.qkv.w"        # the one backbone product whose channel means the fake reports (BS_AUTO_WSTAT=1)
SHRINK = 8                       # the fake's depth maps are [n, H/8, W/8]: calibrate() only takes per-frame means of them
TRACE = []                       # one entry per measurement: (class modes, neck mode, attention mode, frame ids, means requested, live site_bias_corr keys)
STATE = {"amp": {}, "cal_ids": [], "ulp_call": None}


def field(name, h, w):
    g = torch.Generator().manual_seed(int(hashlib.blake2b(name.encode(), digest_size=4).hexdigest(), 16))
    return torch.randn(h, w, generator=g)


def frame_id(fr):
    return [int(v) for v in fr.reshape(fr.shape[0], -1)[:, :64].long().sum(1)]


def truth(fr):
    return torch.stack([field(f"truth{i}", fr.shape[1] // SHRINK, fr.shape[2] // SHRINK) for i in frame_id(fr)])


class FakePlan:
    """stands in for zoedepth._ZoePlan: the engine's modes at run() time decide the error fields that are added"""

    def __init__(self, eng, B, H, W, flip):
        self.eng, self.h, self.w = eng, H // SHRINK, W // SHRINK
        self.frames = torch.zeros(B, H, W, 3, dtype=torch.uint8)
        self.site_flops = {k: v * 2 * B for k, v in SITES.items()}

    def run(self, taps):
        e, A = self.eng, STATE["amp"]
        ids = frame_id(self.frames)
        STATE["cal_ids"] = STATE["cal_ids"] or ids           # the first measurement is of the calibration frames
        TRACE.append((dict(e.class_modes), e.neck_mode, e.attn_mode, ids, taps is not None, sorted(e.site_bias_corr)))
        d = torch.stack([field(f"truth{i}", self.h, self.w) for i in ids])

        def add(name, a):
            gain = lambda i: 1.0 if i in STATE["cal_ids"] else A.get("hold_gain:" + name.split(":")[0], A.get("hold_gain", 1.0))
            d.add_(a * torch.stack([gain(i) * field(f"{name}/{i}", self.h, self.w) for i in ids]))
        add("floor", A["floor"])
        for k, m in e.class_modes.items():
            if m != "full":
                add(f"{k}:{m}", A[f"{k}:{m}"])
        if e.attn_mode == "single":
            add("attn", A["attn"])
        for k in SITES:
            if e.neck_site_plain(k):
                add(f"plain:{k}", A.get(f"plain:{k}", 0.4e-5) * (0.5 if k in e.site_bias_corr else 1.0))
            elif e.neck_site_wonly(k):
                add(f"wonly:{k}", A.get(f"wonly:{k}", 0.5e-5))
        if len(TRACE) - 1 == STATE["ulp_call"]:               # a run that does not reproduce: one ulp off
            d = torch.nextafter(d, torch.full_like(d, float("inf")))
        self.depth_m = d
        if taps is not None:
            for k in (*SITES, BACKBONE_KEY):
                taps["__site_means__"]["in:" + k] = torch.ones(8)


def make_engine(zd):
    """an accurate-mode engine with everything on "auto", without weights or a device"""
    e = zd.ZoeDepthEngine.__new__(zd.ZoeDepthEngine)
    e.acc, e._sd, e.cfg, e.dtype, e.target_hw = True, {"a": torch.ones(3)}, zd.ZoeConfig(), torch.float16, (384, 512)
    e.auto_classes = e.auto_attn = e.auto_modes = True
    e.class_modes = {k: "full" for k in zd.BACKBONE_CLASSES}
    e.attn_mode, e.neck_mode = "corr", "full"
    e.fuse_mlp, e.add_projection, e.neck_f8, e.dev = 2, True, True, torch.device("cpu")
    e.site_bias_corr, e._bias_corr_cache, e.backbone_bias_corr, e._plans, e.calibration = {}, {}, {}, {}, None
    e.w = {BACKBONE_KEY + ".lo": torch.ones(4, 8)}
    e.dw_sum = {k: torch.ones(4, 8) for k in SITES}
    e.reference_depth = truth
    return e


@contextlib.contextmanager
def installed(zd):
    saved = zd._ZoePlan, torch.cuda.synchronize, torch.cuda.empty_cache
    zd._ZoePlan, torch.cuda.synchronize, torch.cuda.empty_cache = FakePlan, (lambda *a, **k: None), (lambda *a, **k: None)
    try:
        yield
    finally:
        zd._ZoePlan, torch.cuda.synchronize, torch.cuda.empty_cache = saved


_B = {"floor": 1.5e-5, "qkv:wmean": 1.5e-5, "qkv:wcls": 1e-5, "o:wmean": 1.2e-5, "o:wcls": 1e-5, "fc1:wmean": 1.5e-5, "fc1:wcls": 1e-5,
      "fc2:wmean": 1.4e-5, "fc2:wcls": 1e-5, "attn": 0.3e-5, "wonly:nc2.w": 4e-5, "plain:ra3.down.w": 6e-5}
_GROUPS = ("ro,ra,nc,fu,pj,mh", "full")
# name -> (amplitudes, calibrate() arguments, options: env = switches set for the run, twice = a second default call, ulp_call = index of the
# measurement that comes back one ulp off).  Between them they take the parent's calibrate() through every branch it can reach.
SCENARIOS = {
    "benign": (_B, {}, {}),
    "outlier": ({**_B, "floor": 6.6e-5, "qkv:wmean": 9e-5, "qkv:wcls": 7e-5, "o:wmean": 8e-5, "o:wcls": 6e-5, "fc1:wmean": 9e-5, "fc1:wcls": 6e-5,
                 "fc2:wmean": 7e-5, "fc2:wcls": 3e-5, "attn": 30e-5}, {}, {}),                                  # margin_note; the neck gets no budget
    "over_tolerance": ({**_B, "floor": 14e-5}, {}, {}),                                                        # warning
    "stepup": ({**_B, "qkv:wmean": 4.5e-5, "o:wmean": 4.5e-5, "fc1:wmean": 4.5e-5, "fc2:wmean": 4.5e-5, "attn": 4e-5}, {}, {}),
    "class_fallthrough": ({**_B, "qkv:wmean": 6e-5, "qkv:wcls": 5.5e-5, "o:wmean": 6e-5, "o:wcls": 4e-5}, {}, {}),      # qkv -> full, o -> wcls
    "holdout_plain": ({**_B, "hold_gain:plain": 6.0}, {}, {}),
    "holdout_all": ({**_B, "hold_gain": 2.6}, {}, {}),
    "holdout_deep": ({**_B, "hold_gain": 4.0}, {}, {}),
    "bisect": ({**_B, "wonly:nc2.w": 6e-5, "wonly:ra3.down.w": 5e-5, "plain:fu2.proj.w": 5e-5}, {}, {}),
    "no_reference": (_B, {"reference": False}, {}),
    "group_candidates": (_B, {"neck_candidates": _GROUPS}, {}),
    "image_major": (_B, {"H": 320, "W": 320}, {}),                                                             # attn_note
    "cache_hit": (_B, {}, {"twice": True}),
    "cache_hit_warning": ({**_B, "floor": 14e-5}, {}, {"twice": True}),
    "rerun_differs": (_B, {}, {"ulp_call": 1}),
    "rerun_first_differs": (_B, {}, {"ulp_call": 0}),
    "stepup_neck": ({**_B, "qkv:wmean": 3.5e-5, "fc1:wmean": 3.5e-5, "fc2:wmean": 3.5e-5, "wonly:rh.conv1.w": 4.8e-5}, {"neck_candidates": _GROUPS}, {}),
    "stepup_attn": ({**_B, "qkv:wmean": 2.5e-5, "o:wmean": 1e-5, "fc1:wmean": 4e-5, "fc2:wmean": 4e-5, "attn": 4.9e-5}, {}, {}),
    "neck_plain_off": (_B, {}, {"env": {"BS_NECK_PLAIN": "0"}}),
    "wstat": ({**_B, "qkv:wstat": 1.5e-5, "o:wstat": 6e-5, "fc1:wstat": 1.5e-5, "fc2:wstat": 1.4e-5}, {}, {"env": {"BS_AUTO_WSTAT": "1"}}),
    "caller_tolerances": (_B, {"tol_class": 1.1e-5, "tol_total": 3e-5, "tol_abs": 3.5e-5}, {}),
    "fixed_class": ({**_B, "floor": 14e-5}, {}, {"fixed": {"fc2": "w"}}),                                     # the warning names the mode the caller fixed
}


def run_scenario(zd, name):
    """-> {"calls": the measurements in order, "warnings": the messages warned, "report": the report without calibrate_s}"""
    amp, kw, opt = SCENARIOS[name]
    kw = dict(kw)
    H, W = kw.pop("H", 480), kw.pop("W", 640)
    STATE.update(amp={"fc2:w": 0.0, **amp}, cal_ids=[], ulp_call=opt.get("ulp_call"))
    TRACE.clear()
    zd._CALIBRATION_CACHE.clear()
    env = opt.get("env", {})
    saved_env = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        with installed(zd), warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            for _ in range(2 if opt.get("twice") else 1):
                e = make_engine(zd)
                e.class_modes.update(opt.get("fixed", {}))
                rep = dict(e.calibrate(H, W, **kw))
    finally:
        for k, v in saved_env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        zd._CALIBRATION_CACHE.clear()
    rep.pop("calibrate_s")
    cal = STATE["cal_ids"]
    calls = [[",".join(m[k] for k in zd.BACKBONE_CLASSES), neck, attn, "cal" if ids == cal else "hold", means, corr]
             for m, neck, attn, ids, means, corr in TRACE]
    return {"calls": calls, "warnings": [str(w.message) for w in caught], "report": rep}
