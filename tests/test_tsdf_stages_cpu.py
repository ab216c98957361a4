"""The cases of tests/_tsdf_cases.py are fair and reach what they are built for -- checked on the numpy restatement (oracle/tsdf_ref.py),
without a GPU.  tests/test_tsdf_stages_gpu.py runs the same cases through csrc/tsdf.hip."""
import numpy as np
import pytest

import _tsdf_cases as C
from oracle.tsdf_ref import TSDFRef


@pytest.mark.parametrize("variant", sorted(C.BOX_VARIANTS))
def test_open_box_is_what_the_oracle_opens(variant):
    """open_box returns exactly TSDFRef.touched: 2x2x2, 3x3x3, over index 0 on every axis (z included), exact ties on the upper face"""
    box = C.open_box(variant)
    # the camera -> world matrix the product derives from the extrinsic (numpy's inverse) is exact, so the point is exactly where it was put
    pose = np.linalg.inv(box["extrinsic"])
    p_cam = np.array([0.5 * 0.5 / 64.0, 0.5 * 0.5 / 64.0, 0.5, 1.0])
    assert np.array_equal((pose @ p_cam)[:3], box["point"])
    ref = TSDFRef(box["vl"], box["trunc"], res=box["res"], stride=box["stride"])
    assert ref.touched(box["depth"], box["K"], box["extrinsic"]) == box["keys"]
    n = {"2x2x2": 8, "3x3x3": 27, "straddle0": 8, "straddle0_3x3x3": 27, "tie": 8, "tie_negative": 8}[variant]
    assert len(box["keys"]) == n
    if "straddle0" in variant or variant == "tie_negative":
        zs = {k[2] for k in box["keys"]}
        assert min(zs) < 0 <= max(zs) and min(k[0] for k in box["keys"]) < 0
    if variant == "tie":            # (p + trunc) / L is a whole number on every axis, and that unit is in
        L = box["vl"] * box["res"]
        hi = (box["point"] + box["trunc"]) / L
        assert np.array_equal(hi, np.round(hi)) and tuple(int(h) for h in hi) in box["keys"]


@pytest.mark.parametrize("variant", sorted(C.TIE_VARIANTS))
def test_oracle_agrees_with_exact_arithmetic_on_the_projection_ties(variant):
    """fp64 with IEEE division decides every voxel of every tie case as exact rational arithmetic does -- which voxels are updated and from
    which pixel (read off the colour: no two pixels share one) -- so the cases are fair to the kernel's fma chain and reciprocal"""
    case, keys, model, notes = C.tie_case(variant)
    ref = TSDFRef(case["vl"], case["trunc"], res=case["res"], stride=case["stride"])
    ref.integrate(case["depth"], case["color"], case["K"], case["extrinsic"])
    assert set(ref.units) == set(model) == keys
    for key, (upd, pix, val) in model.items():
        vox = ref.units[key]
        assert np.array_equal(vox[..., 1], upd.astype(np.float32)), key
        want = case["color"][pix[..., 1], pix[..., 0]].astype(np.float32) * upd[..., None]
        assert np.array_equal(vox[..., 2:], want), key
        assert np.abs(vox[..., 0] - val * upd).max() < 1e-6, key
    # what the case is for is reached
    print(variant, notes)
    assert notes["updated"] > 500 and notes["cz_zero"] >= 16 and notes["cz_negative"] >= 64
    turns, shift, nudge = C.TIE_VARIANTS[variant]
    if shift == 0.0:
        assert notes["u_integer"] >= 20 and notes["v_integer"] >= 20
        assert notes["u_zero"] >= 1 and notes["u_W"] >= 1
    elif variant == "outside_0":
        assert notes["just_inside"] == 0 and notes["just_outside"] >= 2
    else:
        assert notes["just_inside"] >= 1 and notes["just_outside"] >= 1
    if nudge == 0:
        assert notes["sdf_minus_trunc"] >= 1 and notes["sdf_plus_trunc"] >= 1
    else:
        assert notes["sdf_near_minus"] >= 1 and notes["sdf_near_plus"] >= 1


def test_random_field_reaches_every_marching_cubes_case():
    """the random field over a 2x2x2 box holds every one of the 254 cases that cut a cube, counted in bodyslam_amd.marching_cubes' corner
    order; the mesh the oracle draws from it is not empty"""
    box = C.open_box("2x2x2", res=C.MC_RES)
    ref = TSDFRef(box["vl"], box["trunc"], res=C.MC_RES, stride=box["stride"])
    assert ref.touched(box["depth"], box["K"], box["extrinsic"]) == box["keys"]
    units = C.random_field(box["keys"], C.MC_RES, seed=C.MC_SEED)
    cases = C.cube_cases(units, C.MC_RES)
    assert cases.size == (2 * C.MC_RES - 1) ** 3
    assert set(range(1, 255)) <= set(cases.tolist())
    # the other fields: what they are for
    ref.units = units
    assert ref.extract_triangle_mesh()[2].shape[0] > 1000
    units = C.holes_field(box["keys"], 5, seed=0)
    assert 0 < C.cube_cases(units, 5).size < 9 ** 3                       # cubes with a corner of weight 0 are skipped
    plane = C.plane_field(box["keys"], 5, seed=0)
    f = np.concatenate([v[..., 0].ravel() for v in plane.values()])
    for want in (np.float32(0.98), np.float32(-0.98)):
        assert (f == want).sum() > 10
    assert ((f == 0) & ~np.signbit(f)).sum() > 10 and ((f == 0) & np.signbit(f)).sum() > 10


def test_plane_field_gives_the_oracle_zero_area_triangles():
    """f1 == 0 exactly puts the vertex on the voxel centre (w = 1): two edges that end in that voxel give the same position and the oracle
    (as Open3D) emits the triangle all the same"""
    box = C.open_box("2x2x2")
    ref = TSDFRef(box["vl"], box["trunc"], res=4, stride=4)
    ref.units = C.plane_field(box["keys"], 4, seed=0)
    v, _, t = ref.extract_triangle_mesh()
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    area = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    assert t.shape[0] > 20 and (area == 0).sum() > 0 and (area > 0).sum() > 0


def test_checkerboard_reaches_the_cap_of_three_points_per_voxel():
    box = C.open_box("2x2x2")
    ref = TSDFRef(box["vl"], box["trunc"], res=4, stride=4)
    ref.units = C.checkerboard_field(box["keys"], 4, seed=0)
    p, _ = ref.extract_point_cloud()
    assert p.shape[0] == 3 * 8 * 8 * 7                                     # every voxel pair of the 8^3 block along the three axes
    # the unit with all three +neighbours emits 3 res^3 rows
    lo = min(box["keys"])
    q = p - 0.5 * C.VL                              # (a crossing sits half a voxel past its voxel's centre: on the voxel's upper face)
    inside = np.all((q >= np.array(lo) * 4 * C.VL) & (q < (np.array(lo) + 1) * 4 * C.VL), axis=1)
    assert inside.sum() == 3 * 4 ** 3


def test_rim_case_has_zero_normals_in_the_oracle():
    """GetTSDFAt returns 0 when the unit under its first corner is missing; where all six samples of GetNormalAt do, the normal is the zero
    vector.  The oracle reaches that branch on the rim case (and the case builder has checked that the kernel's order of operations rounds
    the same way)."""
    case, fields = C.rim_case()
    ref = TSDFRef(case["vl"], case["trunc"], res=case["res"], stride=case["stride"])
    assert ref.touched(case["depth"], case["K"], case["extrinsic"]) == case["keys"]
    ref.units = {k: v.copy() for k, v in fields.items()}
    p, _, n = ref.extract_point_cloud(normals=True)
    ln = np.linalg.norm(n, axis=1)
    assert p.shape[0] == 5 and (ln == 0).sum() >= 1 and (np.abs(ln - 1) < 1e-6).sum() >= 1


def test_cull_poses_cull_a_unit_and_keep_one_at_the_image_edge():
    """per pose the bound of tsdf_assign_batch_kernel (restated in numpy) drops at least one opened unit and keeps at least one whose
    bounding interval reaches past a side of the image; the poses `face` and `inside` have units whose sphere reaches the camera plane
    (never culled) and units wholly behind the camera"""
    L = C.CULL_VL * C.CULL_RES
    for name, depth, color, E in C.cull_poses():
        ref = TSDFRef(C.CULL_VL, C.CULL_TRUNC, res=C.CULL_RES, stride=C.CULL_STRIDE)
        keys = ref.touched(depth, C.CULL_K, E)
        got = [C.cull_bound(k, L, E, C.CULL_K, C.SW, C.SH) for k in keys]
        assert sum(c for c, _ in got) >= 1, name
        assert sum(e for _, e in got) >= 1, name
        if name in ("face", "inside"):
            r = 0.8660254037844387 * L
            qz = np.array([E[2, :3] @ ((np.array(k) + 0.5) * L) + E[2, 3] for k in keys])
            assert ((qz <= r) & (qz + r > 0)).sum() >= 1 and (qz + r <= 0).sum() >= 1, name


def test_smooth_cases_stand_off_the_pixel_ties():
    """the smooth scenes, the cull poses and the drift input compare the kernel's fma chain and reciprocal with the oracle's separate
    multiplies and IEEE division where neither is exact (voxels of 0.01): no voxel centre projects within 1e-9 pixel of a pixel border,
    ten thousand times the rounding of either (the ties themselves are projection_ties' business, in dyadic numbers)"""
    for seed in range(3):
        depth, color = C.smooth_scene(seed)
        E = C.smooth_pose(seed)
        for res, trunc in ((4, 0.04), (5, 0.04), (6, 0.04), (7, 0.04), (16, 0.04)):
            keys = TSDFRef(0.01, trunc, res=res, stride=8).touched(depth, C.SMOOTH_K, E)
            assert C.pixel_tie_distance(keys, res, 0.01, E, C.SMOOTH_K, C.SW, C.SH) > 1e-9, (seed, res)
    for name, depth, color, E in C.cull_poses():
        keys = TSDFRef(C.CULL_VL, C.CULL_TRUNC, res=C.CULL_RES, stride=C.CULL_STRIDE).touched(depth, C.CULL_K, E)
        assert C.pixel_tie_distance(keys, C.CULL_RES, C.CULL_VL, E, C.CULL_K, C.SW, C.SH) > 1e-9, name
    keys, _, _ = C.drift_reference()
    assert C.pixel_tie_distance(keys, C.DRIFT_RES, C.DRIFT_VL, C.drift_frames()[2], C.DRIFT_K, C.DRIFT_W, C.DRIFT_H) > 1e-9


def test_drift_of_the_oracle_recurrence_is_recorded():
    """200 frames from one pose: weights reach 200 on surface voxels; the deviation of the fp32 recurrence (tsdf w + t) / (w + 1) from the
    fp64 mean of the same observations is what _tsdf_cases.DRIFT_ORACLE records"""
    depths, colors, E = C.drift_frames()
    keys, count, mean = C.drift_reference()
    ref = TSDFRef(C.DRIFT_VL, C.DRIFT_TRUNC, res=C.DRIFT_RES, stride=C.DRIFT_STRIDE)
    for n in range(C.DRIFT_N):
        ref.integrate(depths[n], colors[n], C.DRIFT_K, E)
    assert set(ref.units) == keys
    worst = np.zeros(4)
    full = 0
    for key in keys:
        vox = ref.units[key]
        assert np.array_equal(vox[..., 1].astype(np.float64), count[key])
        full += int((count[key] == C.DRIFT_N).sum())
        worst = np.maximum(worst, np.abs(vox[..., [0, 2, 3, 4]].astype(np.float64) - mean[key]).max(axis=(0, 1, 2)))
    print("drift of the oracle's recurrence (tsdf, r, g, b):", worst, "voxels at weight 200:", full)
    assert full > 100
    assert np.all(worst <= 2.0 * np.array(C.DRIFT_ORACLE)) and np.all(worst >= 0.5 * np.array(C.DRIFT_ORACLE))
