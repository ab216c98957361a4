"""The five kernels of csrc/tsdf.hip one by one -- unit discovery, block assignment with the frustum cull, the batched update, point
extraction, marching cubes -- against the numpy restatement (oracle/tsdf_ref.py) and, on the projection ties, against exact rational
arithmetic, on the inputs of tests/_tsdf_cases.py: unit borders, frame edges, ties and caps.  tests/test_tsdf_stages_cpu.py shows on the
CPU that every case is fair and reaches what it is built for.  Tolerances are those of tests/test_tsdf_gpu.py::test_tsdf_matches_oracle."""
import os
from collections import Counter

import numpy as np
import pytest
import torch

import _tsdf_cases as C

pytestmark = pytest.mark.gpu

_OFF = 1 << 20


# ---- helpers -------------------------------------------------------------------------------------------------------------------------------
def new_map(vl, trunc, res, stride, **kw):
    from bodyslam_amd.tsdf import TSDF
    kw.setdefault("max_units", 4096)
    return TSDF(vl, trunc, volume_unit_resolution=res, depth_sampling_stride=stride, slab_bytes=1 << 16, **kw)      # several slabs


def new_ref(vl, trunc, res, stride):
    from oracle.tsdf_ref import TSDFRef
    return TSDFRef(vl, trunc, res=res, stride=stride)


def intrinsic(W, H, K):
    from bodyslam_amd.tsdf import PinholeCameraIntrinsic
    return PinholeCameraIntrinsic(W, H, *K)


def frame(color, depth):
    from bodyslam_amd.tsdf import RGBDImage
    return RGBDImage(color, depth)


def block(t, s):
    """the device view of block s as [res, res, res, 5]"""
    return t.slabs[s // t.slab_units][s % t.slab_units].view(t.res, t.res, t.res, 5)


def units_of(t):
    """{key: float32 [res, res, res, 5]} of the whole map, one read-back"""
    idx = t.index
    if not idx:
        return {}
    flat = torch.cat(list(t.slabs))[:len(idx)].cpu().numpy().reshape(len(idx), t.res, t.res, t.res, 5)
    return {key: flat[s] for s, key in enumerate(idx)}


def assert_map_matches(t, ref, exact_weights=True):
    """test_tsdf_matches_oracle's comparison: the same units, weights equal, values within 2e-4"""
    got = units_of(t)
    assert set(got) == set(ref.units)
    worst = 0.0
    for key, vox in ref.units.items():
        assert np.array_equal(got[key][..., 1], vox[..., 1]), f"weights of unit {key}"
        worst = max(worst, float(np.abs(got[key] - vox).max()))
    assert worst < 2e-4, worst
    return got


def open_and_fill(box, fields, absent=()):
    """the box is opened through the public path (build_3D_map on the one-pixel frame), then the case's arrays are written into the map
    through the device views and into the oracle's dict.  absent: units left in the table WITHOUT a block (slot -1, the state discover()
    leaves) and taken out of the oracle: the kernels must treat them as missing."""
    t = new_map(box["vl"], box["trunc"], box["res"], box["stride"])
    ref = new_ref(box["vl"], box["trunc"], box["res"], box["stride"])
    t.build_3D_map(frame(None, box["depth"]), intrinsic(box["W"], box["H"], box["K"]), box["extrinsic"])
    assert set(t.index) == box["keys"] == set(fields)
    for s in t.slabs:
        s.zero_()
    for s, key in enumerate(t.index):
        if key in absent:
            packed = ((key[0] + _OFF) << 42) | ((key[1] + _OFF) << 21) | (key[2] + _OFF)
            h = torch.nonzero(t.table_keys == packed).view(-1)
            assert h.numel() == 1
            t.table_slots[h] = -1
        else:
            block(t, s).copy_(torch.from_numpy(fields[key]))
            ref.units[key] = fields[key].copy()
    return t, ref


def sorted_cloud(p, c, n):
    o = np.lexsort((p[:, 2], p[:, 1], p[:, 0]))
    return p[o], c[o], n[o]


def assert_cloud_matches(t, ref, min_rows=1):
    """extract_pcd() against extract_point_cloud(normals=True): equal row counts; after a lexsort points within 1e-6, colours 1e-5, normals
    2e-4 (the oracle evaluates them at the float32 point); every row finite; normals of length 1 or 0, zero where the oracle's are"""
    pcd = t.extract_pcd()
    rp, rc, rn = ref.extract_point_cloud(normals=True)
    assert pcd.points.shape == rp.shape and rp.shape[0] >= min_rows, (pcd.points.shape, rp.shape)
    if rp.shape[0] == 0:
        return pcd, rn
    gp, gc, gn = sorted_cloud(pcd.points, pcd.colors, pcd.normals)
    rp, rc, rn = sorted_cloud(rp, rc, rn)
    assert np.isfinite(gp).all() and np.isfinite(gc).all() and np.isfinite(gn).all()
    assert np.abs(gp - rp).max() < 1e-6 and np.abs(gc - rc).max() < 1e-5
    assert np.abs(gn - rn).max() < 2e-4
    ln = np.linalg.norm(gn, axis=1)
    assert np.all((np.abs(ln - 1.0) < 1e-5) | (ln == 0.0))
    assert np.array_equal(ln == 0.0, np.linalg.norm(rn, axis=1) == 0.0)
    return pcd, rn


def triangle_multiset(vertices, triangles):
    """every triangle as its three float32 vertex positions, rotated to the smallest of its three rotations: same triangles, same winding"""
    v = np.asarray(vertices, dtype=np.float32)
    out = Counter()
    for a, b, c in np.asarray(triangles):
        p = (tuple(v[a].tolist()), tuple(v[b].tolist()), tuple(v[c].tolist()))
        out[min(p, (p[1], p[2], p[0]), (p[2], p[0], p[1]))] += 1
    return out


def sorted_vertices(v, c):
    o = np.lexsort((c[:, 2], c[:, 1], c[:, 0], v[:, 2], v[:, 1], v[:, 0]))
    return v[o], c[o]


def assert_mesh_matches(t, ref, min_triangles=1):
    """extract_mesh() against extract_triangle_mesh(): equal vertex and triangle counts, sorted vertices within 1e-6 and colours 1e-5, and
    the same multiset of triangles"""
    mesh = t.extract_mesh()
    rv, rc, rt = ref.extract_triangle_mesh()
    assert mesh.triangles.shape[0] == rt.shape[0] >= min_triangles and mesh.vertices.shape == rv.shape, (mesh.triangles.shape, rt.shape,
                                                                                                            mesh.vertices.shape, rv.shape)
    if rt.shape[0] == 0:
        return mesh, (rv, rc, rt)
    gv, gc = sorted_vertices(mesh.vertices, mesh.vertex_colors)
    wv, wc = sorted_vertices(rv, rc)
    assert np.abs(gv - wv).max() < 1e-6 and np.abs(gc - wc).max() < 1e-5
    assert triangle_multiset(mesh.vertices, mesh.triangles) == triangle_multiset(rv, rt)
    return mesh, (rv, rc, rt)


# ---- discovery: tsdf_touch_batch_kernel, tsdf_assign_batch_kernel ------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(C.BOX_VARIANTS))
def test_discovery_opens_exactly_the_box(variant):
    """negative unit indices along x, y and z (floor, not truncation); a +-sdf_trunc box that ends exactly on a unit border (hi = floor((p +
    trunc) / L): the border unit is opened); boxes of 2 and 3 units per axis"""
    box = C.open_box(variant)
    t = new_map(box["vl"], box["trunc"], box["res"], box["stride"])
    t.build_3D_map(frame(None, box["depth"]), intrinsic(box["W"], box["H"], box["K"]), box["extrinsic"])
    assert len(t.index) == len(box["keys"]) and set(t.index) == box["keys"]


@pytest.mark.parametrize("trunc", [0.04, 0.1])
def test_discovery_stride_that_divides_neither_side_and_wide_truncation(trunc):
    """a stride of 8 on 50 x 37 (ws = ceil(W / stride) = 7, hs = 5: the last column and row of the sample are partial steps); sdf_trunc =
    2.5 unit lengths (span 7) on a whole image: the opened units are the oracle's"""
    depth, color = C.smooth_scene(0)
    E = C.smooth_pose(1)
    t = new_map(0.01, trunc, 4, 8)
    t.build_3D_map(frame(color, depth), intrinsic(C.SW, C.SH, C.SMOOTH_K), E)
    want = new_ref(0.01, trunc, 4, 8).touched(depth, C.SMOOTH_K, E)
    assert len(want) > 100 and len(t.index) == len(want) and set(t.index) == want


def test_discovery_batch_of_three_overlapping_frames():
    """three records in one pass whose boxes overlap: the units are the oracle's, and the per-unit record masks are right because every
    unit's weights are the oracle's"""
    t = new_map(0.01, 0.04, 4, 8)
    ref = new_ref(0.01, 0.04, 4, 8)
    rgbds, Es = [], []
    for seed in range(3):
        depth, color = C.smooth_scene(seed)
        rgbds.append(frame(color, depth))
        Es.append(C.smooth_pose(seed))
        ref.integrate(depth, color, C.SMOOTH_K, Es[-1])
    t.build_3D_map_batch(rgbds, intrinsic(C.SW, C.SH, C.SMOOTH_K), Es)
    got = assert_map_matches(t, ref)
    assert max(float(v[..., 1].max()) for v in got.values()) == 3.0


# ---- the frustum cull of tsdf_assign_batch_kernel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose", range(5), ids=["yaw40", "pitch-35", "roll90", "face", "inside"])
def test_cull_changes_nothing(pose):
    """focal length 20 on 50 x 37 (|qx| / qz is large, units sit at the image corners), a strongly rotated camera, a unit whose bounding
    sphere reaches the camera plane (the early-out qz > r), the camera inside an opened unit (voxels with cz <= 0): the map with culling is
    bit-equal to the map with BS_TSDF_NO_CULL=1 and both hold the oracle's weights.  (The CPU file shows that the bound does drop units at
    every one of these poses and keeps units that reach past the image's sides.)  The shipped library reads no environment variable
    (the switch acts in the diagnostic build only), so what binds here is the oracle, which has no cull at all: a unit dropped wrongly
    shows as missing weights.  Units are 8^3 voxels of 5 mm, so that voxel centres sit close to the units' corners."""
    name, depth, color, E = C.cull_poses()[pose]
    intr = intrinsic(C.SW, C.SH, C.CULL_K)

    def run(cull):
        if not cull:
            os.environ["BS_TSDF_NO_CULL"] = "1"
        try:
            t = new_map(C.CULL_VL, C.CULL_TRUNC, C.CULL_RES, C.CULL_STRIDE)
            t.build_3D_map(frame(color, depth), intr, E)
            return t
        finally:
            os.environ.pop("BS_TSDF_NO_CULL", None)

    a, b = run(True), run(False)
    ref = new_ref(C.CULL_VL, C.CULL_TRUNC, C.CULL_RES, C.CULL_STRIDE)
    ref.integrate(depth, color, C.CULL_K, E)
    ua = assert_map_matches(a, ref)
    ub = assert_map_matches(b, ref)
    for key in ua:
        assert np.array_equal(ua[key], ub[key]), key
    assert sum(float(v[..., 1].sum()) for v in ua.values()) > 100


# ---- integration: tsdf_observe, tsdf_apply_batch_kernel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [5, 6, 7, 16])
def test_integration_at_partial_waves_and_blocks(res):
    """res 5, 6, 7 = 125, 216, 343 voxels: a partial wave, a partial block, a partial second block under the readfirstlane broadcast of the
    record mask; res 16 = 16 blocks per unit.  Three frames in one pass against the oracle."""
    t = new_map(0.01, 0.04, res, 8)
    ref = new_ref(0.01, 0.04, res, 8)
    rgbds, Es = [], []
    for seed in range(3):
        depth, color = C.smooth_scene(seed)
        rgbds.append(frame(color, depth))
        Es.append(C.smooth_pose(seed))
        ref.integrate(depth, color, C.SMOOTH_K, Es[-1])
    t.build_3D_map_batch(rgbds, intrinsic(C.SW, C.SH, C.SMOOTH_K), Es)
    assert_map_matches(t, ref)


@pytest.mark.parametrize("variant", sorted(C.TIE_VARIANTS))
def test_integration_on_the_projection_ties(variant):
    """voxel centres whose u_f / v_f are exact integers (the fma chain and the v_rcp_f64 + Newton reciprocal against exact arithmetic, where
    one ulp picks the neighbouring pixel), exactly 0 and W and just inside / outside the 0.0001 margins, cz exactly 0 and negative with the
    camera inside the opened units, sdf exactly -sdf_trunc (not updated), exactly +sdf_trunc (tsdf 1) and one float either side: the
    weights are those of the exact model, the colour is that of the exact model's pixel, the map is the oracle's"""
    case, keys, model, notes = C.tie_case(variant)
    t = new_map(case["vl"], case["trunc"], case["res"], case["stride"])
    t.build_3D_map(frame(case["color"], case["depth"]), intrinsic(case["W"], case["H"], case["K"]), case["extrinsic"])
    ref = new_ref(case["vl"], case["trunc"], case["res"], case["stride"])
    ref.integrate(case["depth"], case["color"], case["K"], case["extrinsic"])
    got = assert_map_matches(t, ref)
    wrong = []
    for key, (upd, pix, val) in model.items():
        if not np.array_equal(got[key][..., 1], upd.astype(np.float32)):
            wrong.append((key, "weight"))
        want = case["color"][pix[..., 1], pix[..., 0]].astype(np.float32) * upd[..., None]
        if not np.array_equal(got[key][..., 2:], want):
            wrong.append((key, "pixel"))
        assert np.abs(got[key][..., 0] - val * upd).max() < 1e-6, key
    assert not wrong, wrong


def test_integration_colour_into_colourless_and_back():
    """a colourless pass into a map that holds colours raises the weight and leaves r, g, b alone (the stores are gated on frames[0].color);
    a coloured pass into a colourless map blends into the zeros (s[2..4] are loaded only if (F.color)); as separate passes, both orders"""
    intr = intrinsic(C.SW, C.SH, C.SMOOTH_K)
    for order in ((True, False, True), (False, True, False)):
        t = new_map(0.01, 0.04, 4, 8)
        ref = new_ref(0.01, 0.04, 4, 8)
        for seed, with_color in enumerate(order):
            depth, color = C.smooth_scene(seed)
            E = C.smooth_pose(seed)
            t.build_3D_map(frame(color if with_color else None, depth), intr, E)
            ref.integrate(depth, color if with_color else None, C.SMOOTH_K, E)
        got = assert_map_matches(t, ref)
        assert max(float(v[..., 2:].max()) for v in got.values()) > 50.0


def test_running_mean_after_200_frames():
    """200 frames from one pose (four passes), depth noise of +-2 voxels, random colours: weights are exact and reach 200; the values stay
    within 4 x the deviation of the oracle's own fp32 recurrence from the fp64 mean of the same observations.  Measured on the CPU
    (_tsdf_cases.DRIFT_ORACLE): 5.6e-7 (tsdf), 9.6e-5, 1.10e-4, 1.24e-4 (r, g, b); the bounds are 2.24e-6, 3.84e-4, 4.40e-4,
    4.96e-4.  The product's fmaf(v, w0, t) * (1 / w1) rounds about twice more per step than the oracle's (v w0 + t) / w1.
    Measured on the MI355X: 7.8e-7, 1.41e-4, 1.76e-4, 1.27e-4 -- about 1.4 times the oracle's own deviation."""
    depths, colors, E = C.drift_frames()
    keys, count, mean = C.drift_reference()
    t = new_map(C.DRIFT_VL, C.DRIFT_TRUNC, C.DRIFT_RES, C.DRIFT_STRIDE)
    t.build_3D_map_batch([frame(colors[n], depths[n]) for n in range(C.DRIFT_N)], intrinsic(C.DRIFT_W, C.DRIFT_H, C.DRIFT_K), [E] * C.DRIFT_N)
    got = units_of(t)
    assert set(got) == keys
    worst = np.zeros(4)
    for key in keys:
        assert np.array_equal(got[key][..., 1].astype(np.float64), count[key]), key
        worst = np.maximum(worst, np.abs(got[key][..., [0, 2, 3, 4]].astype(np.float64) - mean[key]).max(axis=(0, 1, 2)))
    print("drift of the product's running mean (tsdf, r, g, b):", worst, "bound:", 4.0 * np.array(C.DRIFT_ORACLE))
    assert max(float(c.max()) for c in count.values()) == C.DRIFT_N
    assert np.all(worst <= 4.0 * np.array(C.DRIFT_ORACLE)), worst


# ---- point extraction: tsdf_extract_kernel, ts_tsdf_at -----------------------------------------------------------------------------------
FIELD_CASES = [(b, f) for b in ("2x2x2", "straddle0_3x3x3") for f in sorted(C.FIELDS)]


@pytest.mark.parametrize("box_name,field", FIELD_CASES)
def test_extraction_of_written_fields(box_name, field):
    """random signs: most crossings have their neighbour in another unit or in none (the box's rim: missing units, normals whose GetTSDFAt
    loses corners); limits: f = -0.98f is in and 0.98f is out, f0 = +0.0f or -0.0f gives no point; holes: neighbours of weight 0;
    checkerboard: every voxel emits 3 points, the cap of 3 res^3 rows per unit, and the count pass agrees with the write pass; plane: no
    point where the field is exactly zero.  Over a box at positive indices and one that straddles index 0 on every axis."""
    box = C.open_box(box_name)
    t, ref = open_and_fill(box, C.FIELDS[field](box["keys"], box["res"], seed=1))
    pcd, _ = assert_cloud_matches(t, ref, min_rows=0 if field == "plane" else 200)       # (every voxel pair of the plane has a zero between its signs)
    if field == "checkerboard":
        n = box["res"] * round(len(box["keys"]) ** (1 / 3))
        assert pcd.points.shape[0] == 3 * n * n * (n - 1)


def test_extraction_next_to_a_unit_without_a_block():
    """a neighbouring unit that discover() entered into the table (a key, slot -1, no block): the point cloud and the mesh are what they
    were before it was entered, and the oracle's, which never heard of it"""
    box = C.open_box("2x2x2")
    t, ref = open_and_fill(box, C.random_field(box["keys"], box["res"], seed=2))
    before = t.extract_pcd()
    mesh_before = t.extract_mesh()
    for offset in ((2, 0, 0), (0, 0, -2)):
        more = C.open_box("2x2x2", offset=offset)
        t.discover(frame(None, more["depth"]), intrinsic(more["W"], more["H"], more["K"]), more["extrinsic"])
    assert int((t.table_keys != -1).sum()) == 24 and int(((t.table_keys != -1) & (t.table_slots < 0)).sum()) == 16 and t.n_units == 8
    after, _ = assert_cloud_matches(t, ref, min_rows=100)
    for a, b in zip(sorted_cloud(before.points, before.colors, before.normals), sorted_cloud(after.points, after.colors, after.normals)):
        assert np.array_equal(a, b)
    mesh_after, _ = assert_mesh_matches(t, ref, min_triangles=100)
    assert triangle_multiset(mesh_before.vertices, mesh_before.triangles) == triangle_multiset(mesh_after.vertices, mesh_after.triangles)


def test_extraction_zero_normals_at_the_rim():
    """normals at the rim of the map: ts_tsdf_at returns 0 when the first corner's unit is missing; where all six samples do, the normal
    is the zero vector and stays one (no division by its length) -- the same rows as in the oracle"""
    case, fields = C.rim_case()
    t, ref = open_and_fill(case, fields)
    pcd, rn = assert_cloud_matches(t, ref, min_rows=5)
    ln = np.linalg.norm(pcd.normals, axis=1)
    assert (ln == 0).sum() == (np.linalg.norm(rn, axis=1) == 0).sum() >= 1 and (ln > 0).sum() >= 1


# ---- marching cubes: tsdf_mesh_kernel, the key merge of TSDF.extract_mesh ----------------------------------------------------------------
@pytest.mark.parametrize("box_name,field", FIELD_CASES)
def test_mesh_of_written_fields(box_name, field):
    """cubes that take corners from all 7 neighbouring units; vertices merged across unit borders and across negative global voxel
    coordinates (the straddling box); holes: a corner of weight 0 skips the cube; plane: a corner with f1 == 0 exactly gives w = 1, a
    vertex on the voxel centre and zero-area triangles, emitted as the oracle (and Open3D) emits them; checkerboard: every cube is case
    0x69 or 0x96, four triangles each; host=False returns the same rows as host=True"""
    box = C.open_box(box_name)
    t, ref = open_and_fill(box, C.FIELDS[field](box["keys"], box["res"], seed=1))
    mesh, (rv, rc, rt) = assert_mesh_matches(t, ref, min_triangles=20)
    if field == "plane":
        def zero_area(v, tr):
            return int((np.linalg.norm(np.cross(v[tr[:, 1]] - v[tr[:, 0]], v[tr[:, 2]] - v[tr[:, 0]]), axis=1) == 0).sum())
        assert zero_area(mesh.vertices, mesh.triangles) == zero_area(rv, rt) > 0
    dev = t.extract_mesh(host=False)
    assert dev.vertices.is_cuda and np.array_equal(dev.vertices.cpu().numpy(), mesh.vertices)
    assert np.array_equal(dev.vertex_colors.cpu().numpy(), mesh.vertex_colors)
    assert triangle_multiset(mesh.vertices, dev.triangles.cpu().numpy()) == triangle_multiset(mesh.vertices, mesh.triangles)
    dp = t.extract_pcd(host=False)
    hp = t.extract_pcd()
    for a, b in zip(sorted_cloud(dp.points.cpu().numpy(), dp.colors.cpu().numpy(), dp.normals.cpu().numpy()), sorted_cloud(hp.points, hp.colors, hp.normals)):
        assert np.array_equal(a, b)


def test_mesh_reaches_all_254_cases_and_the_five_triangle_cap():
    """a smooth surface reaches a handful of the 256 cases on the device; the random field at res 6 holds all 254 that cut a cube (shown on
    the CPU), among them the cases of 5 triangles, the cap of the per-unit count; 216 voxels are a partial block"""
    from bodyslam_amd import marching_cubes as MC
    box = C.open_box("2x2x2", res=C.MC_RES)
    fields = C.random_field(box["keys"], C.MC_RES, seed=C.MC_SEED)
    t, ref = open_and_fill(box, fields)
    mesh, _ = assert_mesh_matches(t, ref, min_triangles=1000)
    cases = C.cube_cases(fields, C.MC_RES)
    assert mesh.triangles.shape[0] == int(MC.N_TRI[cases].sum()) and int(MC.N_TRI[cases].max()) == int(MC.N_TRI.max())
    assert_cloud_matches(t, ref, min_rows=1000)


@pytest.mark.parametrize("gone", [(1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1)])
def test_mesh_and_points_with_one_neighbour_missing(gone):
    """the 2x2x2 box with each of its 7 non-origin units missing in turn -- once present with every weight 0, once in the table without a
    block (as good as absent: the oracle has no such unit): cubes that would take a corner from it are skipped, crossings towards it are
    dropped, GetTSDFAt counts its corners as 0"""
    box = C.open_box("2x2x2")
    lo = min(box["keys"])
    key = tuple(a + b for a, b in zip(lo, gone))
    fields = C.random_field(box["keys"], box["res"], seed=3)
    # weight 0 in place
    zeroed = {k: v.copy() for k, v in fields.items()}
    zeroed[key][..., 1] = 0.0
    t, ref = open_and_fill(box, zeroed)
    assert_mesh_matches(t, ref, min_triangles=100)
    assert_cloud_matches(t, ref, min_rows=100)
    # no block
    t, ref = open_and_fill(box, fields, absent={key})
    assert key not in ref.units and len(ref.units) == 7
    assert_mesh_matches(t, ref, min_triangles=100)
    assert_cloud_matches(t, ref, min_rows=100)


def test_mesh_refuses_a_map_past_2_to_the_19_voxels_and_points_still_come():
    """the err path: a one-pixel frame at x = +530 m with the default 1 mm voxels lies past 2^19 voxels from the origin, where the 20-bit
    vertex identities would wrap: extract_mesh raises; extract_pcd needs no identities and works"""
    from bodyslam_amd.tsdf import TSDF
    depth = np.zeros((16, 16), np.float32)
    depth[8, 8] = 0.3
    pose = np.eye(4)
    pose[0, 3] = 530.0
    t = TSDF()
    t.build_3D_map(frame(None, depth), intrinsic(16, 16, (20.0, 20.0, 8.0, 8.0)), np.linalg.inv(pose))
    with pytest.raises(Exception, match="2\\^20 voxels"):
        t.extract_mesh()
    pcd = t.extract_pcd()
    assert pcd.points.shape[0] > 0 and np.abs(pcd.points[:, 0] - 530.0).max() < 0.05 and np.abs(pcd.points[:, 2] - 0.3).max() < 2e-3


def test_mesh_at_minus_524_metres():
    """global voxel coordinates down to -524 020 >= -2^19: the identities still hold, vertices merge across unit borders at negative
    coordinates, the mesh is the oracle's"""
    vl, trunc, res, stride = 0.001, 0.004, 8, 4
    v, u = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    depth = np.zeros((16, 16), np.float32)
    depth[6:11, 6:11] = (0.1 + 0.0007 * (u - 8) + 0.0004 * (v - 8)).astype(np.float32)[6:11, 6:11]
    pose = np.eye(4)
    pose[:3, 3] = (-524.0, 0.0, 0.0)
    E = np.linalg.inv(pose)
    K = (20.0, 20.0, 8.0, 8.0)
    t = new_map(vl, trunc, res, stride)
    ref = new_ref(vl, trunc, res, stride)
    t.build_3D_map(frame(None, depth), intrinsic(16, 16, K), E)
    ref.integrate(depth, None, K, E)
    assert_map_matches(t, ref)
    assert min(k[0] for k in ref.units) * res >= -(1 << 19) and max(k[0] for k in ref.units) < -65000
    assert_mesh_matches(t, ref, min_triangles=50)
