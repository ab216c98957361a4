"""Map correction after a pose-graph update, the host side (bodyslam_amd/map_correction.py) and the numpy statement of TSDF
de-integration (tests/_tsdf_correct_ref.py) against itself.  No GPU.  The gaps this file prints for the six-round experiment are the
measurement the bars of tests/test_map_correction_gpu.py rest on (8 x)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tsdf_correct_ref as CR      # noqa: E402


def _rot_z(a):
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    return T


def _poses(n, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        T = _rot_z(0.1 * i + 0.01 * rng.normal())
        T[:3, 3] = rng.normal(size=3)
        out.append(T)
    return out


def test_pose_change():
    from bodyslam_amd.map_correction import pose_change
    E = _poses(3)[2]
    assert max(pose_change(E, E)) < 1e-15             # (E inv(E) is the identity up to rounding)
    D = _rot_z(0.03)
    D[:3, 3] = (0.003, -0.004, 0.0)
    t, r = pose_change(E, D @ E)                      # E_new E_old^-1 = D
    assert abs(t - 0.005) < 1e-12 and abs(r - 0.03) < 1e-12
    t, r = pose_change(E, _rot_z(1e-9) @ E)           # small angles keep their digits (the skew part, not the arc cosine of the trace)
    assert t < 1e-15 and abs(r - 1e-9) < 1e-15
    t, r = pose_change(E, _rot_z(np.pi - 1e-3) @ E)
    assert abs(r - (np.pi - 1e-3)) < 1e-9


def test_plan_nothing_to_do_and_last_bit():
    from bodyslam_amd.map_correction import plan_map_correction
    P = _poses(10)
    plan = plan_map_correction([p.copy() for p in P], P, 9)
    assert plan.decision == "correct" and plan.added == [] and plan.moved == [] and plan.records == [] and plan.groups == []
    decision, added, moved, records = plan[:4]        # the four the caller needs come first
    assert (decision, added, moved, records) == ("correct", [], [], [])
    Q = [p.copy() for p in P]
    Q[6][0, 3] = np.nextafter(Q[6][0, 3], np.inf)     # one pose changed in its last bit
    plan = plan_map_correction(P, Q, 9)
    assert plan.moved == [6] and plan.added == []
    assert [(j, rm) for j, _, rm in plan.records] == [(6, True), (6, False)]
    assert np.array_equal(plan.records[0][1], P[6]) and np.array_equal(plan.records[1][1], Q[6])      # out with the old pose, in with the new
    assert plan_map_correction(P, Q, 5).moved == []   # frames past `upto` are not looked at


def test_plan_tolerances_cut_separately():
    from bodyslam_amd.map_correction import plan_map_correction
    P = _poses(4)
    Q = [p.copy() for p in P]
    shift = np.eye(4)
    shift[:3, 3] = (0.002, 0.0, 0.0)
    Q[1] = shift @ P[1]                               # 2 mm, no rotation
    Q[2] = _rot_z(0.01) @ P[2]                        # 0.01 rad about the origin of the camera frame: no translation of E_new E_old^-1
    assert plan_map_correction(P, Q, 3).moved == [1, 2]
    assert plan_map_correction(P, Q, 3, tol=(0.001, 0.1)).moved == [1]          # translation over, rotation under
    assert plan_map_correction(P, Q, 3, tol=(0.01, 0.005)).moved == [2]         # rotation over, translation under
    assert plan_map_correction(P, Q, 3, tol=(0.01, 0.1)).moved == []
    assert plan_map_correction(P, Q, 3, tol=(0.002 + 1e-9, 0.01 + 1e-9)).moved == []
    assert plan_map_correction(P, Q, 3, tol=(0.002 - 1e-9, 0.1)).moved == [1]
    with pytest.raises(ValueError):
        plan_map_correction(P, Q, 3, mode="rebuild")


def test_plan_none_entries_are_added_and_kept_frames_keep_their_pose():
    from bodyslam_amd.map_correction import plan_map_correction
    P = _poses(9)
    ledger = [p.copy() for p in P]
    ledger[4] = None
    ledger[8] = None
    Q = [p.copy() for p in P]
    small = np.eye(4)
    small[:3, 3] = (1.5e-4, 0, 0)
    big = np.eye(4)
    big[:3, 3] = (5e-3, 0, 0)
    Q[2], Q[5] = small @ P[2], big @ P[5]
    plan = plan_map_correction(ledger, Q, 8, tol=(1e-3, 1e-3))
    assert plan.added == [4, 8] and plan.moved == [5]
    assert [(j, rm) for j, _, rm in plan.records] == [(5, True), (4, False), (5, False), (8, False)]
    # the caller updates the ledger for moved + added only: frame 2 keeps its ledger pose, so a second small step is measured against
    # what the map holds and crosses the tolerance instead of hiding behind the first
    for j in plan.moved + plan.added:
        ledger[j] = Q[j]
    assert np.array_equal(ledger[2], P[2])
    R = [q.copy() for q in Q]
    for _ in range(6):                                # 0.9 mm from Q[2], 1.05 mm from what the map holds
        R[2] = small @ R[2]
    assert plan_map_correction(ledger, R, 8, tol=(1e-3, 1e-3)).moved == [2]
    assert plan_map_correction([q.copy() for q in Q], R, 8, tol=(1e-3, 1e-3)).moved == []      # an overwritten ledger would not see it


def test_plan_record_order_and_auto():
    from bodyslam_amd.map_correction import plan_map_correction
    n = 100
    P = _poses(n)
    ledger = [p.copy() for p in P]
    pending = [20, 50, 99]
    for j in pending:
        ledger[j] = None
    Q = [p.copy() for p in P]
    moved = [j for j in range(n) if j not in pending][:70]
    for j in moved:
        Q[j][2, 3] += 0.01
    plan = plan_map_correction(ledger, Q, n - 1)
    assert plan.decision == "correct" and plan.moved == moved and plan.added == pending
    assert len(plan.records) == 2 * 70 + 3 and len(plan.groups) == 3
    concerned = sorted(moved + pending)
    at = 0
    for g, (r0, r1) in enumerate(plan.groups):
        assert r0 == at and r1 - r0 <= 64
        at = r1
        frames = concerned[32 * g:32 * g + 32]
        want = [(j, True) for j in frames if j in moved] + [(j, False) for j in frames]
        assert [(j, rm) for j, _, rm in plan.records[r0:r1]] == want              # removals ascending, then additions ascending
        for j, E, rm in plan.records[r0:r1]:
            assert np.array_equal(E, ledger[j] if rm else Q[j])
    assert at == len(plan.records)
    # "auto": a fresh volume costs upto + 1 integrations, the correction 2 * moved + added
    assert plan_map_correction(ledger, Q, n - 1, mode="auto").decision == "rebuild"           # 143 >= 100
    few = [p.copy() for p in P]
    for j in moved[:48]:
        few[j][2, 3] += 0.01
    assert plan_map_correction(ledger, few, n - 1, mode="auto").decision == "correct"         # 2 * 48 + 3 = 99 < 100
    few[moved[48]][2, 3] += 0.01
    full = [p.copy() for p in P]
    assert plan_map_correction(full, few, n - 1, mode="auto").decision == "correct"           # 2 * 49 = 98 < 100
    assert plan_map_correction(ledger, few, n - 1, mode="auto").decision == "rebuild"         # 2 * 49 + 3 = 101 >= 100
    few2 = [p.copy() for p in few]
    few2[moved[49]][2, 3] += 0.01
    assert plan_map_correction(full, few2, n - 1, mode="auto").decision == "rebuild"          # 2 * 50 = 100 >= 100: the equality rebuilds
    assert plan_map_correction(ledger, Q, n - 1, mode="incremental").decision == "correct"


def test_statement_correction_against_fresh_build():
    """Six scene frames, then six rounds that each move three of them: after every round the corrected statement map against a statement
    map built fresh with the current poses -- the exact properties hold, the gaps are printed and held to the recorded values -- and
    taking all six frames out leaves every block all zero."""
    res, stride = 8, 4
    frames = [CR.scene(s) for s in range(CR.N_FRAMES)]
    held = [f[2] for f in frames]
    cor = CR.TSDFCorrectRef(CR.VL, CR.TRUNC, res=res, stride=stride)
    for d, c, E in frames:
        cor.integrate(d, c, CR.K, E)
    for r, which, poses in CR.correction_rounds():
        for j in which:                                                  # removals ascending, then additions ascending: the plan's order
            cor.deintegrate(frames[j][0], frames[j][1], CR.K, held[j])
        for j in which:
            cor.integrate(frames[j][0], frames[j][1], CR.K, poses[j])
        held = poses
        fresh = CR.TSDFCorrectRef(CR.VL, CR.TRUNC, res=res, stride=stride)
        for (d, c, _), E in zip(frames, poses):
            fresh.integrate(d, c, CR.K, E)
        gap_t, gap_c = CR.compare_maps(cor.units, fresh.units)
        print(f"round {r}: moved {which}, worst |dtsdf| {gap_t:.2e}, worst |dcolour| {gap_c:.2e} "
              f"(recorded {CR.STATEMENT_GAP_TSDF[r - 1]:.1e}, {CR.STATEMENT_GAP_COLOR[r - 1]:.1e})")
        assert cor.misuse == 0
        # the recorded gaps are this measurement rounded up: the GPU bars are 8 x the record, so the record may not drift from it
        assert gap_t <= CR.STATEMENT_GAP_TSDF[r - 1] and gap_c <= CR.STATEMENT_GAP_COLOR[r - 1]
        assert gap_t > 0.5 * CR.STATEMENT_GAP_TSDF[r - 1] or r > 1       # (and is not a loose one where it matters most: round 1)
    for j in (3, 0, 5, 1, 4, 2):
        cor.deintegrate(frames[j][0], frames[j][1], CR.K, held[j])
    assert cor.misuse == 0
    for key, vox in cor.units.items():
        assert not vox.view(np.uint32).any(), key
    # misuse: a frame the map never held is skipped and counted, no weight goes below 0
    cor.integrate(*frames[0][:2], CR.K, frames[0][2])
    before = {k: v.copy() for k, v in cor.units.items()}
    cor.deintegrate(*frames[3][:2], CR.K, frames[3][2])
    assert cor.misuse > 0 and min(float(v[..., 1].min()) for v in cor.units.values()) >= 0.0
    for k, v in cor.units.items():
        zero = before[k][..., 1] == 0
        assert np.array_equal(v[zero], before[k][zero])
