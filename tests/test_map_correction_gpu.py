"""TSDF de-integration and map correction on the GPU (TSDF.apply_batch / deintegrate, csrc/tsdf.hip tsdf_apply_batch_kernel<true>;
map_correction.plan_map_correction; run_slam_loop's map_correction modes).

What is exact is compared exactly: weights (small integers), emptied blocks (bit-equal to zeros), one pass against one record at a
time (bit-equal), the default loop against itself.  What rounds -- a corrected map against one built fresh -- is held to the
"statement bars": 8 x the gap the numpy statement (tests/_tsdf_correct_ref.py) measured for the same number of rounds in
tests/test_map_correction_cpu.py, which covers emulated against real fmaf and the path dependence of the rounding walk.  Measured
there (round 1 .. 6): |dtsdf| 2.98e-7 4.17e-7 4.77e-7 6.26e-7 8.94e-7 9.54e-7, |dcolour| (0..255) 6.10e-5 9.16e-5 9.16e-5 1.37e-4 1.53e-4
1.83e-4; the bars are 8 x CR.STATEMENT_GAP_*: 2.4e-6 / 5.0e-4 after one round, 7.7e-6 / 1.5e-3 after six.  No bar comes from the device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tsdf_correct_ref as CR      # noqa: E402

pytestmark = pytest.mark.gpu

H, W, K = CR.H, CR.W, CR.K
scene = CR.scene                    # tests/test_tsdf_gpu.py's small scene (the copy lives with the statement, which needs it too)


def intr():
    from bodyslam_amd.tsdf import PinholeCameraIntrinsic
    return PinholeCameraIntrinsic(W, H, *K)


def new_map(res=8, stride=4, **kw):
    from bodyslam_amd.tsdf import TSDF
    return TSDF(CR.VL, CR.TRUNC, volume_unit_resolution=res, depth_sampling_stride=stride, slab_bytes=1 << 16, **kw)      # several slabs


def blocks(t):
    """every unit's voxels, {unit index: fp32 [res, res, res, 5]}, in one read-back"""
    idx = t.index
    if not idx:
        return {}
    parts, left = [], len(idx)
    for s in t.slabs:
        parts.append(s[:min(left, s.shape[0])])
        left -= parts[-1].shape[0]
    allv = torch.cat(parts).cpu().numpy().reshape(len(idx), t.res, t.res, t.res, 5)
    return dict(zip(idx, allv))


def rgbd(seed, with_color=True):
    from bodyslam_amd.tsdf import RGBDImage
    d, c, _ = scene(seed)
    return RGBDImage(c if with_color else None, d)


def all_zero(a):
    return not np.ascontiguousarray(a).view(np.uint32).any()


# ---- 1. empty again ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_color,res,stride,batched", [(True, 8, 4, False), (False, 8, 4, False), (True, 4, 8, False), (True, 8, 4, True)])
def test_deintegrating_every_frame_leaves_an_empty_map(with_color, res, stride, batched):
    """five frames in, the same five out in another order: every block is bit-equal to zeros, the units stay, nothing is extracted, and
    a frame integrated afterwards lands as in a fresh map.  (4, 8): a unit has 64 voxels, fewer than the 256-thread block)"""
    t = new_map(res, stride)
    frames = [(rgbd(s, with_color), scene(s)[2]) for s in range(5)]
    if batched:
        t.build_3D_map_batch([r for r, _ in frames], intr(), [E for _, E in frames])
        t.sync()
    else:
        for r, E in frames:
            t.build_3D_map(r, intr(), E)
    units_before = set(t.index)
    assert t.frames_integrated == 5 and len(units_before) > 50 and max(float(v[..., 1].max()) for v in blocks(t).values()) == 5.0
    for j in (3, 0, 4, 1, 2):
        t.deintegrate(frames[j][0], intr(), frames[j][1])
    assert set(t.index) == units_before and t.frames_integrated == 0
    assert all(all_zero(v) for v in blocks(t).values())
    assert t.extract_pcd().points.shape == (0, 3) and t.extract_mesh().triangles.shape == (0, 3)
    t.build_3D_map(frames[2][0], intr(), frames[2][1])
    fresh = new_map(res, stride)
    fresh.build_3D_map(frames[2][0], intr(), frames[2][1])
    got, want = blocks(t), blocks(fresh)
    assert set(want) <= set(got) and t.frames_integrated == 1
    for key, v in got.items():
        assert np.array_equal(v.view(np.uint32), want[key].view(np.uint32)) if key in want else all_zero(v), key


# ---- 2. one pass equals one record at a time --------------------------------------------------------------------------------------
def _jittered(n, seed):
    """n frames: the images of scene(i % 6), its pose moved by a seeded jitter (distinct poses for frames that share an image)"""
    rng = np.random.default_rng(seed)
    return [CR.jitter(rng) @ scene(i % 6)[2] for i in range(n)]


def _one_pass_against_singly(base, records, with_color, cull=True):
    """base: [(seed, E)] integrated into both maps first; records: [(seed, E, remove)].  Map a takes them through apply_batch, map b
    one at a time through deintegrate / build_3D_map, in order"""
    if not cull:
        os.environ["BS_TSDF_NO_CULL"] = "1"
    try:
        a, b = new_map(), new_map()
        for t in (a, b):
            t.build_3D_map_batch([rgbd(s, with_color) for s, _ in base], intr(), [E for _, E in base])
            t.sync()
        a.apply_batch([rgbd(s, with_color) for s, _, _ in records], intr(), [E for _, E, _ in records], [rm for _, _, rm in records])
        na, _ = a.sync()
        for s, E, rm in records:
            if rm:
                b.deintegrate(rgbd(s, with_color), intr(), E)
            else:
                b.build_3D_map(rgbd(s, with_color), intr(), E)
        want_frames = len(base) + sum(-1 if rm else 1 for _, _, rm in records)
        assert na == b.n_units > 0 and a.frames_integrated == b.frames_integrated == want_frames
        ga, gb = blocks(a), blocks(b)
        assert set(ga) == set(gb)
        for key in ga:
            assert np.array_equal(ga[key].view(np.uint32), gb[key].view(np.uint32)), key
        assert int(a.table_fmask.abs().sum()) == 0 and int(b.table_fmask.abs().sum()) == 0        # clean for the next batch
        return a
    finally:
        os.environ.pop("BS_TSDF_NO_CULL", None)


@pytest.mark.parametrize("with_color,cull", [(True, True), (False, True), (True, False)])
def test_apply_batch_equals_one_record_at_a_time(with_color, cull):
    """a mixed record list -- two frames out with the pose they went in with, back in with another, a new frame in between -- into a
    map that holds other frames too; without colours; with the frustum test off"""
    old, new = _jittered(6, 3), _jittered(6, 4)
    base = [(s, old[s]) for s in range(5)]
    records = [(1, old[1], True), (3, old[3], True), (1, new[1], False), (5, new[5], False), (3, new[3], False), (0, old[0], True)]
    _one_pass_against_singly(base, records, with_color, cull)


def test_apply_batch_across_the_64_record_border():
    """33 moved frames = 66 records: two passes (64 + 2), the same blocks as 66 single calls"""
    old, new = _jittered(33, 5), _jittered(33, 6)
    base = [(i % 6, old[i]) for i in range(33)]
    records = [(i % 6, old[i], True) for i in range(33)] + [(i % 6, new[i], False) for i in range(33)]
    _one_pass_against_singly(base, records, True)


# ---- 3. against the statement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,stride", [(8, 4), (4, 8)])
def test_deintegrate_matches_the_statement(res, stride):
    """three frames in, the middle one out: the units and weights of the numpy statement, values within the project's
    device-against-oracle bar (test_tsdf_gpu.py: 2e-4, colours are 0..255 running means)"""
    t = new_map(res, stride)
    ref = CR.TSDFCorrectRef(CR.VL, CR.TRUNC, res=res, stride=stride)
    for s in range(3):
        d, c, E = scene(s)
        t.build_3D_map(rgbd(s), intr(), E)
        ref.integrate(d, c, K, E)
    d, c, E = scene(1)
    t.deintegrate(rgbd(1), intr(), E)
    ref.deintegrate(d, c, K, E)
    assert ref.misuse == 0 and t.frames_integrated == 2
    got = blocks(t)
    assert set(got) == set(ref.units)
    worst = 0.0
    for key, want in ref.units.items():
        assert np.array_equal(got[key][..., 1], want[..., 1]), f"weights of unit {key}"
        worst = max(worst, float(np.abs(got[key] - want).max()))
    print(f"deintegrate against the statement ({res}, {stride}): worst |delta| {worst:.2e}")
    assert worst < 2e-4
    assert max(float(v[..., 1].max()) for v in got.values()) == 2.0


# ---- 4. correction against rebuild ------------------------------------------------------------------------------------------------
def test_correction_rounds_against_a_fresh_build():
    """the six-round experiment of the CPU test on the device: plan_map_correction + apply_batch against build_3D_map_batch of a fresh map"""
    from bodyslam_amd.map_correction import plan_map_correction
    images = [rgbd(s) for s in range(CR.N_FRAMES)]
    ledger = [scene(s)[2] for s in range(CR.N_FRAMES)]
    cor = new_map()
    cor.build_3D_map_batch(images, intr(), ledger)
    cor.sync()
    for r, which, poses in CR.correction_rounds():
        plan = plan_map_correction(ledger, poses, CR.N_FRAMES - 1, mode="incremental")
        assert plan.decision == "correct" and plan.moved == which and plan.added == []
        cor.apply_batch([images[j] for j, _, _ in plan.records], intr(), [E for _, E, _ in plan.records], [rm for _, _, rm in plan.records])
        cor.sync()                                                       # (would raise had a removal met a voxel without the frame)
        for j in plan.moved:
            ledger[j] = poses[j]
        fresh = new_map()
        fresh.build_3D_map_batch(images, intr(), poses)
        fresh.sync()
        gap_t, gap_c = CR.compare_maps(blocks(cor), blocks(fresh))       # asserts: subset, extras zero, weights equal, weight 0 = all zero
        bar_t, bar_c = CR.BAR_FACTOR * CR.STATEMENT_GAP_TSDF[r - 1], CR.BAR_FACTOR * CR.STATEMENT_GAP_COLOR[r - 1]
        print(f"round {r}: worst |dtsdf| {gap_t:.2e} (bar {bar_t:.1e}), worst |dcolour| {gap_c:.2e} (bar {bar_c:.1e})")
        assert gap_t <= bar_t and gap_c <= bar_c
        assert cor.frames_integrated == CR.N_FRAMES


# ---- 5. misuse is reported, not absorbed ------------------------------------------------------------------------------------------
def test_removing_a_frame_that_was_never_integrated():
    t = new_map()
    for s in range(3):
        t.build_3D_map(rgbd(s), intr(), scene(s)[2])
    before = blocks(t)
    t.deintegrate(rgbd(4), intr(), scene(4)[2], sync=False)
    after = blocks(t)
    skipped = 0
    for key, v in after.items():
        assert float(v[..., 1].min()) >= 0.0, key
        if key in before:
            zero = before[key][..., 1] == 0
            assert np.array_equal(v[zero].view(np.uint32), before[key][zero].view(np.uint32)), key
            skipped += int(zero.sum())
        else:
            assert all_zero(v), key                                      # a unit the removal opened: nothing was written to it
    assert skipped > 0
    with pytest.raises(Exception, match="removed that the voxel never held"):
        t.sync()
    assert int(t.counters[2]) == 0
    t.sync()                                                             # the flag is clear: the map goes on
    # a full map is refused by the call itself, before anything of the chunk is applied (test_tsdf_frame_batch_equals_frame_by_frame's case)
    full = new_map(max_units=64)
    with pytest.raises(Exception, match="max_units|unit table full"):
        full.apply_batch([rgbd(0), rgbd(1)], intr(), [scene(0)[2], scene(1)[2]], [False, False])
    assert full.frames_integrated == 0 and int(full.table_fmask.abs().sum()) == 0 and int(full.counters[2]) == 0


# ---- 6. the loop ------------------------------------------------------------------------------------------------------------------
class _Loop:
    """test_slam_loop_with_the_device_solver's configuration: 9 frames of 160 x 192, target_hw (64, 96), posegraph_every 4, one closure
    (8, 0) 2 mm off the chain, TSDF 0.02 / 0.06 / res 8 / stride 8"""

    def __init__(self):
        import dataclasses
        from bodyslam_amd.pipeline import BodySlamPipeline
        from bodyslam_amd.synthetic import make_sequence
        from bodyslam_amd.zoedepth import ZoeConfig
        from oracle import cyclepose_ref as CP
        from oracle import zoedepth_ref as Z
        cfg_o = Z.ZoeConfig(hidden=128, layers=4, heads=2, intermediate=256, taps=(1, 2, 3, 4), image_size=64)
        names = {f.name for f in dataclasses.fields(ZoeConfig)}
        cfg_p = ZoeConfig(**{k: v for k, v in dataclasses.asdict(cfg_o).items() if k in names})
        self.pipe = BodySlamPipeline(Z.synth_weights(cfg_o, seed=2), CP.synth_weights(seed=2), cfg_p, batch=4, target_hw=(64, 96))
        self.frames = make_sequence(9, 160, 192, seed=5)
        self.chain = self.pipe.run_slam_loop(self.frames, posegraph_every=4).g_abs.cpu().numpy()      # no closure: the poses never move
        info = np.eye(6)
        info[5, 5] = 5000.0
        T80 = np.linalg.inv(self.chain[0]) @ self.chain[8]
        T80[:3, 3] += 2e-3
        self.pipe.loop_closures = [(8, 0, T80, info)]
        self.rebuild = self.run("rebuild")

    @staticmethod
    def volume():
        from bodyslam_amd.tsdf import TSDF
        return TSDF(voxel_length=0.02, sdf_trunc=0.06, volume_unit_resolution=8, depth_sampling_stride=8)

    def run(self, mode, tol=(0.0, 0.0)):
        pipe = self.pipe
        pipe.map_correction, pipe.map_correction_tol = mode, tol
        made = []

        def factory():
            made.append(1)
            return self.volume()
        try:
            first = self.volume()
            res = pipe.run_slam_loop(self.frames, tsdf=first, posegraph_every=4, tsdf_factory=factory)
        finally:
            pipe.map_correction, pipe.map_correction_tol = "rebuild", (0.0, 0.0)
        return {"g": res.g_abs.cpu().numpy(), "res": res, "first": first, "made": len(made), "blocks": blocks(res.tsdf),
                "log": list(pipe.last_map_corrections)}


@pytest.fixture(scope="module")
def loop():
    return _Loop()


def _bit_equal_maps(a, b):
    assert set(a) == set(b)
    for key in a:
        assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key


def test_loop_default_is_unchanged(loop):
    """map_correction = "rebuild" is the default and today's path: two runs give bit-equal poses and bit-equal map blocks"""
    assert loop.pipe.map_correction == "rebuild" and loop.pipe.map_correction_tol == (0.0, 0.0)
    again = loop.run("rebuild")
    assert np.array_equal(again["g"], loop.rebuild["g"])
    _bit_equal_maps(again["blocks"], loop.rebuild["blocks"])
    assert loop.rebuild["made"] == 1 and loop.rebuild["res"].tsdf is not loop.rebuild["first"] and loop.rebuild["log"] == []
    assert np.abs(loop.rebuild["g"] - loop.chain).max(axis=(1, 2))[8] > 2e-4          # the closure moved the chain


def test_loop_incremental_correction(loop):
    inc, reb = loop.run("incremental"), loop.rebuild
    assert np.array_equal(inc["g"], reb["g"])
    assert inc["made"] == 0 and inc["res"].tsdf is inc["first"] and inc["res"].tsdf.frames_integrated == 9
    moved = [j for j in range(9) if j not in (4, 8) and not np.array_equal(loop.chain[j], reb["g"][j])]
    assert len(moved) >= 6                                               # (frame 0 is the graph's fixed node)
    # one step, at frame 8: frames 4 (skipped by the optimise branch at i = 4) and 8 are added, the moved frames re-integrated
    assert inc["log"] == [(8, moved, [4, 8], "correct")]
    # (measured on the MI355X: 108 units, largest weight 1 -- in this configuration no voxel is seen by two frames, so the values agree
    # exactly here; voxels that several frames share are what test_correction_rounds_against_a_fresh_build covers)
    wmax = max(float(v[..., 1].max()) for v in reb["blocks"].values())
    print(f"loop map: {len(reb['blocks'])} units, largest weight {wmax:.0f}")
    assert len(reb["blocks"]) > 0 and wmax >= 1
    gap_t, gap_c = CR.compare_maps(inc["blocks"], reb["blocks"])
    bar_t, bar_c = CR.BAR_FACTOR * CR.STATEMENT_GAP_TSDF[0], CR.BAR_FACTOR * CR.STATEMENT_GAP_COLOR[0]
    print(f"loop, incremental against rebuild: worst |dtsdf| {gap_t:.2e} (bar {bar_t:.1e}), worst |dcolour| {gap_c:.2e} (bar {bar_c:.1e})")
    assert gap_t <= bar_t and gap_c <= bar_c


def test_loop_tolerance_leaves_frames_alone(loop):
    """tol = (1 m, 1 rad): nothing is moved, frames 4 and 8 are added with their new poses, and the seven others are what a map that
    never saw the optimisation holds -- bit for bit a map given the same frames with the chain's poses, in the loop's order"""
    from bodyslam_amd import _lib as L
    from bodyslam_amd.tsdf import PinholeCameraIntrinsic, RGBDImage
    tol = loop.run("incremental", tol=(1.0, 1.0))
    assert tol["log"] == [(8, [], [4, 8], "correct")] and tol["made"] == 0 and tol["res"].tsdf.frames_integrated == 9
    assert np.array_equal(tol["g"], loop.rebuild["g"])
    pipe, res = loop.pipe, tol["res"]
    dm = L.depth_u16_to_m(res.depth_u16.contiguous(), pipe.depth_scale, pipe.depth_trunc)
    fr = torch.as_tensor(loop.frames).to(dm.device)
    k = PinholeCameraIntrinsic(fr.shape[2], fr.shape[1], *[float(v) for v in pipe.K])
    hand = loop.volume()
    for js, poses in (((0, 1, 2, 3), loop.chain), ((5, 6, 7), loop.chain), ((4, 8), tol["g"])):
        hand.build_3D_map_batch([RGBDImage(fr[j], dm[j]) for j in js], k, [poses[j] for j in js])
    hand.sync()
    _bit_equal_maps(tol["blocks"], blocks(hand))


def test_loop_auto_decides_rebuild(loop):
    """2 * moved + added >= 9 on this input: "auto" rebuilds and equals the rebuild run bit for bit"""
    auto = loop.run("auto")
    assert len(auto["log"]) == 1 and auto["log"][0][0] == 8 and auto["log"][0][3] == "rebuild" and auto["made"] == 1
    assert np.array_equal(auto["g"], loop.rebuild["g"])
    _bit_equal_maps(auto["blocks"], loop.rebuild["blocks"])
