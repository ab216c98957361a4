"""ZoeDepthEngine.calibrate off the device.

(1) Characterisation: tests/golden/calibration_traces.json holds, for every scenario of tests/_calibration_fake.py, what calibrate() did
BEFORE it was split into calibration.py's stages (recorded from that commit by tools/make_calibration_traces.py): the measurements in order,
the warnings and the report.  The replay must match call by call, and the report key by key and bit by bit -- the fake is deterministic, so
any difference is a changed decision or a reordered measurement.
(2) One direct test per stage on hand-made inputs."""
import dataclasses
import json
import math
import os

import pytest
import torch

from bodyslam_amd import calibration as C

import _calibration_fake as fake

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "calibration_traces.json")))


def test_golden_covers_the_scenarios():
    assert set(GOLDEN["scenarios"]) == set(fake.SCENARIOS)


# Quirks of the recorded behaviour that these scenarios pin, and that a follow-up which changes them on purpose may re-record:
#   holdout_deep      after a "backbone step" the hold-out loop sets the neck back to the mode it started from, whatever step_up() did to it
#   holdout_*         the withdrawal pops the weight-only list that report["neck_sites"]["weight_only"] aliases
#   cache_hit_warning a cache hit warns again with the stored warning, but not with a stored margin_note
#   rerun_*           a yardstick that differs from its rerun is replaced by the rerun only when a third run agrees with the second
@pytest.mark.parametrize("name", list(fake.SCENARIOS))
def test_replay_matches_the_recorded_behaviour(name):
    import bodyslam_amd.zoedepth as ZD
    want = GOLDEN["scenarios"][name]
    got = fake.run_scenario(ZD, name)
    want_calls = [[c[0], GOLDEN["neck_modes"][c[1]], *c[2:]] for c in want["calls"]]
    for i, (g, w) in enumerate(zip(got["calls"], want_calls)):
        assert g == w, f"measurement {i}"
    assert len(got["calls"]) == len(want_calls)
    assert got["warnings"] == want["warnings"]
    assert json.dumps(got["report"]) == json.dumps(want["report"])


# ---- the stages alone -------------------------------------------------------------------------------------------------------------

class Device:
    """a measurement whose depth "map" is one number per frame: truth 0, the yardstick `floor`, plus `cost(modes, neck, attn, holdout)`"""

    def __init__(self, cost, floor=1e-5, site_flops=None, hold=True):
        self.cost, self.ncal, self.site_flops, self.calls, self.corr = cost, 2, dict(site_flops or {}), [], None
        self.ref, self.truth = torch.full((2, 1, 1), floor), torch.zeros(2, 1, 1)
        self.truth_hold = torch.zeros(2, 1, 1) if hold else None

    def depth(self, modes, neck, attn, holdout=False, means=None):
        self.calls.append((dict(modes), neck, attn, holdout))
        if means is not None:
            means["in:x"] = 1.0
        return self.ref + self.cost(modes, neck, attn, holdout)

    def set_site_bias_corr(self, means):
        self.corr = sorted(k[3:] for k in means)
        return self.corr


def scope(**kw):
    base = dict(switchable=("qkv", "o", "fc1", "fc2"), class_cands=("wmean", "wcls", "full"), fixed_modes={k: "full" for k in ("qkv", "o", "fc1", "fc2")},
                auto_attn=True, attn_best="corr", neck_full="full", neck_cands=("full",), explicit_neck=False, per_site=True, neck_plain=True,
                saving={"qkv": 100.0, "o": 40.0, "fc1": 150.0, "fc2": 150.0, "attn": 170.0})
    return C.Scope(**{**base, **kw})


P = C.DEFAULT_POLICY
SITES = {n: [n] for n in "abcdefg"}
wonly = lambda neck: [s for s in neck.split(";")[0][6:].split(",") if s] if neck.startswith("wonly:") else []
plain = lambda neck: neck.split(";plain:")[1].split(",") if ";plain:" in neck else []


def test_scan_takes_the_cheapest_candidate_within_tol_class():
    err = {"qkv:wmean": 5e-5, "qkv:wcls": 3e-5, "o:wmean": 1e-5, "fc1:wmean": 5e-5, "fc1:wcls": 5e-5, "fc2:wmean": 4e-5}
    dev = Device(lambda m, neck, attn, h: sum(err.get(f"{k}:{v}", 0.0) for k, v in m.items()) + (4.1e-5 if attn == "single" else 0.0))
    seen = {}
    c = C.scan_candidates(P, scope(), dev, seen)
    assert c.modes == {"qkv": "wcls", "o": "wmean", "fc1": "full", "fc2": "wmean"} and c.attn == "corr" and c.neck == "full"
    assert {k: round(v, 9) for k, v in c.cost.items()} == {"qkv": 3e-5, "o": 1e-5, "fc1": 0.0, "fc2": 4e-5}
    assert list(seen) == ["qkv:wmean", "qkv:wcls", "o:wmean", "fc1:wmean", "fc1:wcls", "fc2:wmean", "attn:single"]     # "full" is never measured
    assert all(sum(v != "full" for v in m.values()) <= 1 for m, *_ in dev.calls)                                        # each candidate alone


def test_step_up_raises_the_worst_error_per_gflop_saved():
    dev = Device(None, site_flops={"a": 4 * 80e9})
    c = C.Choice(modes={"qkv": "wmean", "o": "wmean", "fc1": "wcls", "fc2": "full"}, neck="ro", attn="single",
                 cost={"qkv": 2e-5, "o": 1e-5, "fc1": 3e-5, "fc2": 0.0, "attn": 1e-5, "neck": 0.9e-5})
    alone = {"o:wcls": 0.3e-5, "qkv:wcls": 1e-5}
    # error per GFLOP saved: qkv 2e-7, o 2.5e-7, fc1 3e-5 / (150 x 0.5) = 4e-7, attn 0.6e-7, neck 0.9e-5 / (0.5 x 80) = 2.25e-7; fc2 is not live
    order = []
    while C.step_up(P, scope(), dev, c, alone):
        order.append((dict(c.modes), c.neck, c.attn))
    steps = [next(k for k in ("qkv", "o", "fc1", "fc2") if a[0][k] != b[0][k]) if a[0] != b[0] else ("neck" if a[1] != b[1] else "attn")
             for a, b in zip([({"qkv": "wmean", "o": "wmean", "fc1": "wcls", "fc2": "full"}, "ro", "single")] + order, order)]
    # a class comes back one candidate up with the error the scan recorded for it there: o at "wcls" 0.3e-5 / 20 = 1.5e-7, qkv 1e-5 / 50 = 2e-7
    assert steps == ["fc1", "o", "neck", "qkv", "qkv", "o", "attn"]
    assert c.modes == {k: "full" for k in c.modes} and c.neck == "full" and c.attn == "corr" and not any(c.cost.values())


def test_settle_steps_up_until_total_and_absolute_hold():
    err = {"wmean": 2.5e-5, "wcls": 1.5e-5, "full": 0.0}
    dev = Device(lambda m, neck, attn, h: sum(err[v] for v in m.values()), floor=1e-5)
    c = C.Choice(modes={k: "wmean" for k in ("qkv", "o", "fc1", "fc2")}, cost={k: 2.5e-5 for k in ("qkv", "o", "fc1", "fc2")}, neck="full", attn="corr")
    alone = {f"{k}:wcls": 1.5e-5 for k in c.modes}
    C.settle(P, scope(), dev, c, alone)
    # 10e-5 -> "o" (the smallest saving) to wcls 9e-5 -> qkv 8e-5 -> o to full 6.5e-5 -> fc1 / fc2 ... until <= tol_total 6e-5
    assert c.total <= P.tol_total and c.l1_abs <= P.tol_abs and abs(c.l1_abs - c.total - 1e-5) < 1e-9
    assert c.modes["o"] == "full" and len(dev.calls) == 5
    quiet = C.Choice(modes={"qkv": "full"}, neck="full", attn="corr")
    n = len(dev.calls)
    C.settle(P, scope(), dev, quiet, {})
    assert len(dev.calls) == n and quiet.total == 0.0 and abs(quiet.l1_abs - 1e-5) < 1e-12           # nothing cheap: the yardstick itself


def test_candidate_sites_group_the_small_and_skip_cls_and_bins_head():
    sites = C.neck_candidate_sites(P, {"rh.conv1.w": 900.0, "fu1.w": 99.0, "ro2.w": 0.5, "pj3.w": 0.3, "zz.w": 0.2, "ro2.w_cls": 50.0, "mh.conv.w": 50.0})
    assert sites == {"rh.conv1.w": ["rh.conv1.w"], "fu1.w": ["fu1.w"], "group:tiny": ["ro2.w", "pj3.w"]}     # zz: small and in no group


@pytest.mark.parametrize("n,longest", [(7, 5), (7, 0), (7, 7), (1, 1), (20, 13)])
def test_bisection_finds_the_longest_passing_prefix_in_log_steps(n, longest):
    asked = []
    k, kept = C.longest_passing_prefix(n, lambda k: (asked.append(k), ("ok", k) if k <= longest else None)[1])
    assert k == longest and kept == (("ok", longest) if longest else None)
    assert len(asked) <= math.ceil(math.log2(n + 1)) and len(set(asked)) == len(asked)


def test_neck_stage_1_orders_by_error_per_flop_and_keeps_the_longest_prefix():
    flops = {n: f * 4e9 for n, f in zip("abcdefg", (10, 20, 30, 40, 50, 60, 70))}
    e1 = dict(zip("abcdefg", (7e-6, 1e-6, 6e-6, 2e-6, 5e-6, 3e-6, 4e-6)))         # error per FLOP order: b d f g e c a
    dev = Device(lambda m, neck, attn, h: sum(e1[s] for s in wonly(neck)), floor=3e-5, site_flops=flops)
    c = C.Choice(modes={"qkv": "wmean"}, neck="full", attn="single", l1_abs=3e-5, total=1e-5)
    rep = C.neck_weight_only(P, dev, c, dev.ref)
    # budget max(5e-5, 3e-5 + 0.5e-5) against a floor of 3e-5: 2e-5 to spend: b d f g e = 1.5e-5 fits, + c does not
    assert c.wsites == list("bdfge") and c.neck == "wonly:b,d,e,f,g" and rep["weight_only"] == c.wsites
    assert list(rep["l1_alone_vs_chosen_m"]) == list("bdfgeca") and abs(c.l1_abs - 4.5e-5) < 1e-9 and abs(c.total - 1.5e-5) < 1e-9
    assert len(dev.calls) == 7 + 3                                                 # each candidate alone, then a bisection: not 7 + 7
    tight = C.Choice(modes={"qkv": "wmean"}, neck="full", attn="single", l1_abs=P.tol_neck_cap, total=1e-5)
    assert C.neck_weight_only(P, dev, tight, dev.ref) is None and tight.wsites == [] and len(dev.calls) == 10     # no budget: nothing measured


def test_neck_stage_2_walks_largest_first_and_never_proposes_the_fused_upconv():
    flops = {"rh.conv2.w": 90 * 4e9, "a": 50 * 4e9, "b": 30 * 4e9, "c": 10 * 4e9, "d": 0.01 * 4e9}
    e2 = {"a": 0.5e-5, "b": 4e-5, "c": 0.5e-5, "d": 0.1e-5, "rh.conv2.w": 0.0}
    dev = Device(lambda m, neck, attn, h: sum(e2[s] for s in plain(neck)), floor=2e-5, site_flops=flops)
    c = C.Choice(modes={}, neck="wonly:a,b,c,d,rh.conv2.w", attn="corr", sites={k: [k] for k in flops}, wsites=["d", "c", "b", "a", "rh.conv2.w"], l1_abs=2e-5)
    rep = {}
    C.neck_one_pass(P, dev, c, rep)
    tried = [plain(neck) for _, neck, _, _ in dev.calls[2:]]
    assert tried == [["a"], ["a", "b"], ["a", "c"]]                    # largest first; b refused and left out of the next; d below the share; never rh.conv2.w
    assert c.plain == ["a", "c"] and c.neck == "wonly:a,b,c,d,rh.conv2.w;plain:a,c" and abs(c.l1_abs - 3e-5) < 1e-9
    assert dev.corr == ["x"] and rep["static_bias_correction"] == ["x"] and rep["plain"] == ["a", "c"]      # the means run came first
    assert list(rep["l1_with_candidate_plain_m"]) == ["a", "b", "c"]


def test_holdout_withdraws_one_pass_then_weight_only_then_backbone():
    def cost(m, neck, attn, holdout):
        return (3e-5 * len(plain(neck)) + 2e-5 * len(wonly(neck)) + 3e-5 * sum(v != "full" for v in m.values())) if holdout else 0.0
    dev = Device(cost, floor=0.0)
    c = C.Choice(modes={"qkv": "wmean", "o": "wcls"}, cost={"qkv": 1e-5, "o": 1e-5}, neck="wonly:a,b;plain:a", attn="corr", sites=SITES,
                 wsites=["a", "b"], plain=["a"], l1_abs=1e-5, total=1e-5)
    report = {"l1_vs_full_m": {"qkv:wcls": 0.5e-5}, "neck_sites": {}}
    C.validate_holdout(P, scope(), dev, c, report)
    # 13e-5 -> plain a 10e-5 -> wonly b 8e-5 -> wonly a 6e-5: under tol_holdout 7e-5, the backbone is not touched
    assert report["holdout"]["withdrawn"] == ["plain:a", "wonly:b", "wonly:a"] and c.neck == "full" and c.modes == {"qkv": "wmean", "o": "wcls"}
    assert report["neck_sites"] == {"weight_only": [], "plain": []} and report["holdout"]["l1_max_m"] == 6e-5
    c2 = C.Choice(modes={"qkv": "wmean", "o": "wcls", "fc1": "wcls"}, cost={"qkv": 1e-5, "o": 1e-5, "fc1": 1e-5}, neck="full", attn="corr")
    rep2 = {"l1_vs_full_m": {}}
    C.validate_holdout(P, scope(), dev, c2, rep2)
    assert rep2["holdout"]["withdrawn"] == ["backbone step"] and sum(v != "full" for v in c2.modes.values()) == 2


def test_finish_report_warns_above_the_tolerance_and_notes_the_margin():
    c = C.Choice(modes={"qkv": "wmean"}, neck="full", attn="single", l1_abs=1.2e-4, total=1e-5)
    sc = scope(switchable=("qkv",), fixed_modes={"qkv": "full", "o": "w", "fc1": "full", "fc2": "full"})
    rep = {"l1_best_vs_reference_m": 9e-5}
    msgs = C.finish_report(P, sc, c, rep, "320x320", {}, {}, True)
    assert msgs == [rep["warning"]] and "margin_note" not in rep and "'o': 'w'" in rep["warning"]
    assert rep["attn_mode"] == "corr" and c.attn == "corr" and "320x320" in rep["attn_note"]
    assert rep["class_modes"] == {"qkv": "wmean", "o": "w", "fc1": "full", "fc2": "full"}
    c.l1_abs, rep = 6e-5, {"l1_best_vs_reference_m": 5.5e-5}
    assert C.finish_report(P, sc, c, rep, None, {}, {}, True) == [rep["margin_note"]] and "warning" not in rep
    c.l1_abs, rep = None, {}
    assert C.finish_report(P, sc, c, rep, None, {}, {}, False) == [] and "note" in rep


def test_every_policy_field_reaches_the_cache_key():
    def changed(v):
        if isinstance(v, tuple):
            return v + v[-1:]
        return v + 1 if isinstance(v, int) else v * 1.5
    keys = {repr(P)}                                        # what ZoeDepthEngine.calibrate keys its cache with
    for f in dataclasses.fields(P):
        other = dataclasses.replace(P, **{f.name: changed(getattr(P, f.name))})
        assert other != P and repr(other) not in keys, f.name
        keys.add(repr(other))
    assert eval(repr(P), {"CalibrationPolicy": C.CalibrationPolicy}) == P


def test_zoedepth_reexports_the_default_policy():
    import bodyslam_amd.zoedepth as ZD
    assert (ZD.AUTO_TOL_CLASS_M, ZD.AUTO_TOL_TOTAL_M, ZD.AUTO_TOL_ABS_M, ZD.TOLERANCE_M) == (4.0e-5, 6.0e-5, 8.0e-5, 1.0e-4)
    assert (ZD.AUTO_CAL_FRAMES, ZD.AUTO_HOLDOUT_FRAMES, ZD.AUTO_TOL_HOLDOUT_M, ZD.AUTO_TOL_NECK_CAP_M, ZD.AUTO_TOL_NECK_ABS_M) == (4, 4, 7.0e-5, 6.5e-5, 5.0e-5)
    assert ZD.AUTO_NECK_CANDIDATES == (ZD.NECK_RELHEAD_WONLY, "full") and ZD.AUTO_CANDIDATES == ("wmean", "wcls", "full")
