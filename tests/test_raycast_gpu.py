"""TSDF ray cast on the GPU (TSDF.raycast, MAP; csrc/tsdf.hip tsdf_raycast_kernel) against its numpy restatement
(tests/_raycast_ref.py, itself pinned to analytic truth by tests/test_raycast_cpu.py) cast through the DEVICE's own voxels, and
against the analytic renderer tests/_render.py.  Reference call sites: BodySLAM_not_refactored/3DM/tsdf.py:56-107 (MAP,
synthesize_model_frame after every integrate), 3DM/synthetic_depth_generator.py:74-97, 3DM/mapping_module.py:204-228.

The conditions of the comparison with the restatement (``compare``): hit masks differ on at most 0.5 % of the pixels; among pixels
hit by both at most 0.5 % differ by more than 1e-6 m in depth, and those by no more than half a voxel; on the agreeing pixels
vertices within 1e-6 m, normals within 2e-4 (what test_tsdf_matches_oracle allows the same central difference), colours within 1
of 255.  An fp64 kernel in the restatement's operation order is expected to flip nothing: the caps leave room for a different
rounding inside the eight-corner sum and none for a different algorithm."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _raycast_ref as RC      # noqa: E402
import _render as R            # noqa: E402

pytestmark = pytest.mark.gpu

H, W = RC.TOY_HW
K = RC.TOY_K


def intr(h=H, w=W, k=K):
    from bodyslam_amd.tsdf import PinholeCameraIntrinsic
    return PinholeCameraIntrinsic(w, h, *k)


def toy_frames():
    return [(P,) + R.render(P, K, H, W) for P in RC.toy_poses()]


def build_toy(vl, trunc, sync=True, **kw):
    from bodyslam_amd.tsdf import TSDF, RGBDImage
    prod = TSDF(vl, trunc, volume_unit_resolution=8, depth_sampling_stride=4, max_units=8192, **kw)
    if not sync:
        prod.reserve_ahead(4)
    for P, col, d in toy_frames():
        prod.build_3D_map(RGBDImage(col, d), intr(), np.linalg.inv(P), sync=sync)
    return prod


class DeviceUnits:
    """the ``units`` mapping of a TSDFRef-shaped object, fetched from the device through prod.unit(key) on first use"""

    def __init__(self, prod):
        self.prod, self.keys, self.cache = prod, set(prod.index), {}

    def get(self, key, default=None):
        key = tuple(int(v) for v in key)
        if key not in self.keys:
            return default
        if key not in self.cache:
            self.cache[key] = self.prod.unit(key)
        return self.cache[key]

    def __contains__(self, key):
        return tuple(int(v) for v in key) in self.keys


def device_ref(prod):
    from oracle.tsdf_ref import TSDFRef
    ref = TSDFRef(prod.voxel_length, prod.sdf_trunc, res=prod.res, stride=prod.stride)
    ref.units = DeviceUnits(prod)
    return ref


def compare(name, got, want, vl, pix=None):
    """got: RaycastFrame of ONE view (device tensors [H, W, ...]); want: the restatement's dict; pix: the (v, u) pairs it cast, or None"""
    def g(t):
        a = t.cpu().numpy()
        return a.reshape((-1,) + a.shape[2:]) if pix is None else a[pix[:, 0], pix[:, 1]]
    gd = g(got.depth).astype(np.float64)
    wd = want["depth"].reshape(-1)
    n = gd.shape[0]
    gh, wh = gd > 0, wd > 0
    flips = int(np.count_nonzero(gh != wh))
    both = gh & wh
    dd = np.abs(gd - wd)[both]
    off = dd > 1e-6
    print(f"{name}: {n} rays, hits {int(wh.sum())} (restatement) / {int(gh.sum())} (kernel), mask flips {flips}, depth off by > 1e-6 m on "
          f"{int(off.sum())}, max |d depth| {dd.max() if dd.size else 0.0:.3e} m")
    assert both.sum() > 0.5 * n, f"{name}: only {int(both.sum())} of {n} rays hit"
    assert flips <= 0.005 * n, f"{name}: hit masks differ on {flips} of {n} pixels"
    assert off.sum() <= 0.005 * both.sum(), f"{name}: depth differs by more than 1e-6 m on {int(off.sum())} of {int(both.sum())} hits"
    assert not off.any() or dd[off].max() <= 0.5 * vl, f"{name}: a depth differs by {dd[off].max()} m, more than half a voxel"
    agree = both.copy()
    agree[both] = ~off
    if got.vertex is not None:
        dv = np.abs(g(got.vertex).astype(np.float64) - want["vertex"].reshape(-1, 3))[agree]
        print(f"{name}: max |d vertex| {dv.max():.3e} m")
        assert dv.max() <= 1e-6
        assert not g(got.vertex)[~gh].any()
    if got.normal is not None and "normal" in want:
        dn = np.abs(g(got.normal).astype(np.float64) - want["normal"].reshape(-1, 3))[agree]
        print(f"{name}: max |d normal| {dn.max():.3e}")
        assert dn.max() <= 2e-4
        assert not g(got.normal)[~gh].any()
    if got.color is not None and "color" in want:
        dc = np.abs(g(got.color).astype(np.int64) - want["color"].reshape(-1, 3).astype(np.int64))[agree]
        print(f"{name}: max |d colour| {dc.max()} of 255")
        assert dc.max() <= 1
        assert not g(got.color)[~gh].any()
    return gd, wd


# ---- 1. against the restatement on the device's own voxels -----------------------------------------------------------------------
@pytest.mark.parametrize("vl,trunc", RC.TOY_MAPS)
def test_raycast_matches_restatement_on_device_voxels(vl, trunc):
    prod = build_toy(vl, trunc)
    ref = device_ref(prod)
    views = RC.toy_views()
    E = np.stack([np.linalg.inv(P) for P in views])
    frame = prod.raycast(intr(), E, depth_min=RC.DEPTH_MIN, depth_max=RC.DEPTH_MAX, vertex=True, normal=True, color=True)
    assert frame.depth.shape == (3, H, W) and frame.color.shape == (3, H, W, 3) and frame.color.dtype == torch.uint8
    inner = np.zeros((H, W), bool)
    inner[4:-4, 4:-4] = True
    from bodyslam_amd.tsdf import RaycastFrame
    for i, (name, P) in enumerate(zip(("seen0", "seen3", "unseen"), views)):
        want = RC.raycast(ref, K, E[i], H, W, RC.DEPTH_MIN, RC.DEPTH_MAX, normal=True, color=True)
        one = RaycastFrame(frame.depth[i], frame.color[i], frame.vertex[i], frame.normal[i])
        gd, _ = compare(f"vl {vl} {name}", one, want, vl)
        # and the kernel against analytic truth, as the CPU test holds the restatement: every interior pixel hit, half a voxel
        gd = gd.reshape(H, W)
        _, truth = R.render(P, K, H, W)
        assert (gd > 0)[inner].all()
        err = np.abs(gd - truth)[gd > 0] / vl
        print(f"vl {vl} {name}: kernel vs analytic depth, voxels: median {np.median(err):.3f} max {err.max():.3f}")
        assert err.max() <= 0.5


# ---- 2. full size at the reference's parameters ------------------------------------------------------------------------------------
def test_raycast_full_size_reference_parameters():
    """1 mm voxels, 0.1 m truncation, 32^3 units, stride 8, 640x480.  Interior = 40 px from the border: the toy tests' 4 px at ten
    times the resolution, the same margin in the scene.  Measured on MI355X (sampled interior hits, |depth - truth| in voxels,
    restatement and kernel alike): median 0.006-0.007, max 0.53 / 0.45 / 0.49 for the three views; no hit-mask flip, depth within
    1.5e-8 m of the restatement."""
    from bodyslam_amd.tsdf import TSDF, RGBDImage
    Hf, Wf = 480, 640
    Kf = tuple(10.0 * k for k in K)
    vl = 0.001
    prod = TSDF()                                                       # the reference's parameters (tsdf.py:6)
    try:
        prod.reserve(2048)                                              # 1.3 GB of blocks, before any frame
        frames = [(P,) + R.render(P, Kf, Hf, Wf) for P in RC.toy_poses()]
        prod.build_3D_map_batch([RGBDImage(col, d) for _, col, d in frames], intr(Hf, Wf, Kf), [np.linalg.inv(P) for P, _, _ in frames])
        prod.sync()
        views = RC.toy_views()
        E = np.stack([np.linalg.inv(P) for P in views])
        frame = prod.raycast(intr(Hf, Wf, Kf), E, depth_min=RC.DEPTH_MIN, depth_max=RC.DEPTH_MAX, vertex=True, normal=True, color=True)
        ref = device_ref(prod)
        from bodyslam_amd.tsdf import RaycastFrame
        worst_ref, worst_got = 0.0, 0.0
        for i, (name, P) in enumerate(zip(("seen0", "seen3", "unseen"), views)):
            rng = np.random.default_rng(100 + i)
            pix = np.stack([rng.integers(0, Hf, 2000), rng.integers(0, Wf, 2000)], 1)
            want = RC.raycast(ref, Kf, E[i], Hf, Wf, RC.DEPTH_MIN, RC.DEPTH_MAX, pixels=pix, normal=True, color=True)
            one = RaycastFrame(frame.depth[i], frame.color[i], frame.vertex[i], frame.normal[i])
            gd, wd = compare(f"full size {name}", one, want, vl, pix)
            _, truth = R.render(P, Kf, Hf, Wf)
            tr = truth[pix[:, 0], pix[:, 1]].astype(np.float64)
            inner = (pix[:, 0] >= 40) & (pix[:, 0] < Hf - 40) & (pix[:, 1] >= 40) & (pix[:, 1] < Wf - 40)
            er = np.abs(wd - tr)[inner & (wd > 0)] / vl
            eg = np.abs(gd - tr)[inner & (gd > 0)] / vl
            print(f"full size {name}: interior hits {er.size} / {eg.size} of {int(inner.sum())}; |depth - truth| in voxels: restatement median "
                  f"{np.median(er):.3f} max {er.max():.3f}, kernel median {np.median(eg):.3f} max {eg.max():.3f}")
            worst_ref, worst_got = max(worst_ref, er.max()), max(worst_got, eg.max())
        assert worst_ref <= 1.0, f"the RESTATEMENT is {worst_ref:.3f} voxels off analytic truth: the algorithm, not the kernel, misses one voxel"
        assert worst_got <= 1.0, f"the kernel is {worst_got:.3f} voxels off analytic truth"
    finally:
        del prod
        torch.cuda.empty_cache()


# ---- 3. batch and rerun invariance -------------------------------------------------------------------------------------------------
def frames_equal(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in ((a.depth, b.depth), (a.color, b.color), (a.vertex, b.vertex), (a.normal, b.normal)))


def test_raycast_batch_and_rerun_invariance():
    prod = build_toy(0.01, 0.04)
    views = RC.toy_views() + [R.small_pose(-0.02, 0.03, 0.02, 0.02, 0.015, -0.01), R.small_pose(0.05, -0.05, 0.0, -0.02, -0.01, 0.02)]
    E = [np.linalg.inv(P) for P in views]
    kw = dict(depth_min=RC.DEPTH_MIN, depth_max=RC.DEPTH_MAX, vertex=True, normal=True, color=True)
    batch = prod.raycast(intr(), E, **kw)
    again = prod.raycast(intr(), torch.from_numpy(np.stack(E)), **kw)
    assert batch.depth.shape == (5, H, W) and (batch.depth > 0).float().mean() > 0.8
    assert frames_equal(batch, again)
    from bodyslam_amd.tsdf import RaycastFrame
    for i in range(5):
        one = prod.raycast(intr(), E[i], **kw)
        assert one.depth.shape == (H, W)
        assert frames_equal(one, RaycastFrame(batch.depth[i], batch.color[i], batch.vertex[i], batch.normal[i])), f"view {i}"


def test_raycast_more_views_than_one_launch_carries():
    """the entry hands the kernel a fixed number of views per launch; a longer list is the same views"""
    prod = build_toy(0.01, 0.04)
    views = RC.toy_views()
    E = np.stack([np.linalg.inv(views[i % 3]) for i in range(70)])
    out = prod.raycast(intr(), E, depth_min=RC.DEPTH_MIN, depth_max=RC.DEPTH_MAX)
    assert out.depth.shape == (70, H, W) and (out.depth[0] > 0).any()
    for i in range(3, 70):
        assert torch.equal(out.depth[i], out.depth[i % 3]) and torch.equal(out.color[i], out.color[i % 3])


# ---- 4. streamed use ---------------------------------------------------------------------------------------------------------------
def test_raycast_behind_unsynchronised_integration():
    kw = dict(depth_min=RC.DEPTH_MIN, depth_max=RC.DEPTH_MAX, vertex=True, normal=True, color=True)
    E = np.stack([np.linalg.inv(P) for P in RC.toy_views()])
    streamed = build_toy(0.01, 0.04, sync=False)
    got = streamed.raycast(intr(), E, **kw)                               # no sync() in between
    want = build_toy(0.01, 0.04, sync=True).raycast(intr(), E, **kw)
    assert (want.depth > 0).float().mean() > 0.8
    assert frames_equal(got, want)
    streamed.sync()


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------------
def test_raycast_empty_map_and_no_views():
    from bodyslam_amd.tsdf import TSDF
    prod = TSDF(0.01, 0.04, volume_unit_resolution=8, depth_sampling_stride=4, max_units=1024)
    out = prod.raycast(intr(), np.eye(4), depth_min=RC.DEPTH_MIN, depth_max=RC.DEPTH_MAX, vertex=True, normal=True, color=True)
    assert out.depth.shape == (H, W)
    assert not out.depth.any() and not out.vertex.any() and not out.normal.any() and not out.color.any()
    none = prod.raycast(intr(), [], vertex=True)
    assert none.depth.shape == (0, H, W) and none.vertex.shape == (0, H, W, 3) and none.normal is None
    none = prod.raycast(intr(), np.zeros((0, 4, 4)))
    assert none.depth.shape == (0, H, W)


def test_raycast_odd_image_size_and_optional_outputs():
    prod = build_toy(0.01, 0.04)
    E = np.linalg.inv(RC.toy_views()[2])
    kw = dict(depth_min=RC.DEPTH_MIN, depth_max=RC.DEPTH_MAX)
    full = prod.raycast(intr(), E, vertex=True, normal=True, color=True, **kw)
    # a pixel's ray depends on K and the pose alone: a 37 x 53 image with the same K is the corner of the 48 x 64 one
    odd = prod.raycast(intr(37, 53), E, vertex=True, normal=True, color=True, **kw)
    assert odd.depth.shape == (37, 53) and (odd.depth > 0).any()
    for a, b in ((odd.depth, full.depth), (odd.vertex, full.vertex), (odd.normal, full.normal), (odd.color, full.color)):
        assert torch.equal(a, b[:37, :53])
    for v, n, c in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        part = prod.raycast(intr(), E, vertex=v, normal=n, color=c, **kw)
        assert torch.equal(part.depth, full.depth)
        assert (part.vertex is None) == (not v) and (part.normal is None) == (not n) and (part.color is None) == (not c)
        assert part.vertex is None or torch.equal(part.vertex, full.vertex)
        assert part.normal is None or torch.equal(part.normal, full.normal)
        assert part.color is None or torch.equal(part.color, full.color)
    # the surface lies at ~0.3 m: nothing is found short of it, or looking away from it
    assert not prod.raycast(intr(), E, depth_min=0.05, depth_max=0.2).depth.any()
    back = RC.toy_views()[0].copy()
    back[:3, :3] = back[:3, :3] @ np.diag([-1.0, 1.0, -1.0])
    assert not prod.raycast(intr(), np.linalg.inv(back), **kw).depth.any()


def test_raycast_table_entry_without_block_is_empty_space():
    """discover() without reserve_discovered(): most units of the frame sit in the table with no block (slot -1)"""
    from bodyslam_amd.tsdf import TSDF, RGBDImage
    vl, trunc = 0.01, 0.04
    prod = TSDF(vl, trunc, volume_unit_resolution=8, depth_sampling_stride=4, max_units=8192, slab_bytes=4 * 8 ** 3 * 20)      # 4 blocks exist
    P, col, d = toy_frames()[0]
    prod.discover(RGBDImage(col, d), intr(), np.linalg.inv(P))
    assert int(((prod.table_keys != -1) & (prod.table_slots < 0)).sum()) >= 10 and prod.alloc_units == 4
    out = prod.raycast(intr(), np.linalg.inv(P), depth_min=RC.DEPTH_MIN, depth_max=RC.DEPTH_MAX, vertex=True, normal=True, color=True)
    assert not out.depth.any() and not out.vertex.any() and not out.normal.any() and not out.color.any()
    prod.counters[2] = 0
    # the same table once the blocks exist and the frame is integrated: the surface is there
    prod.reserve_discovered()
    prod.build_3D_map(RGBDImage(col, d), intr(), np.linalg.inv(P))
    out = prod.raycast(intr(), np.linalg.inv(P), depth_min=RC.DEPTH_MIN, depth_max=RC.DEPTH_MAX)
    assert (out.depth > 0).float().mean() > 0.8


@pytest.mark.parametrize("seen,kept", [(0, 1), (1, 0)])
def test_discover_leaves_no_bits_for_the_next_pass(seen, kept):
    """discover(frame `seen`) marks units in table_fmask and no pass follows that clears it: a bit left behind would name record 0 of
    the next pass, and frame `kept` would be integrated into the units only frame `seen` opened.  (Toy frame 0 opens no unit that
    frame 1 does not; frame 1 opens two that frame 0 does not, oracle/tsdf_ref.py -- hence the second case.)"""
    from bodyslam_amd.tsdf import TSDF, RGBDImage

    def volume():
        return TSDF(0.01, 0.04, volume_unit_resolution=8, depth_sampling_stride=4, max_units=8192)

    fr = toy_frames()
    (Ps, cols, ds), (Pk, colk, dk) = fr[seen], fr[kept]
    prod = volume()
    prod.discover(RGBDImage(cols, ds), intr(), np.linalg.inv(Ps))
    opened = int((prod.table_keys != -1).sum())
    assert opened > 0 and not prod.table_fmask.any()
    prod.reserve_discovered()
    prod.build_3D_map(RGBDImage(colk, dk), intr(), np.linalg.inv(Pk))
    fresh = volume()
    fresh.build_3D_map(RGBDImage(colk, dk), intr(), np.linalg.inv(Pk))
    assert prod.sync()[0] == prod.n_units and set(fresh.index) <= set(prod.index)
    for key in fresh.index:
        assert np.array_equal(prod.unit(key), fresh.unit(key)), key
    # the units only the discovered frame opened: in the table, without a block or with one that holds zeros
    if (seen, kept) == (1, 0):
        assert int((prod.table_keys != -1).sum()) > len(fresh.index)
    for key in set(prod.index) - set(fresh.index):
        assert not prod.unit(key).any(), key
    assert sum(int(s.count_nonzero()) for s in prod.slabs) == sum(int(s.count_nonzero()) for s in fresh.slabs) > 0


def test_raycast_refuses_bad_arguments():
    from bodyslam_amd._lib import BodySlamHipError
    prod = build_toy(0.01, 0.04)
    sing = np.eye(4)
    sing[2, :3] = sing[1, :3]
    with pytest.raises(BodySlamHipError):
        prod.raycast(intr(), sing)
    with pytest.raises(BodySlamHipError):
        prod.raycast(intr(), [np.eye(4), sing])
    with pytest.raises(BodySlamHipError):
        prod.raycast(intr(), np.eye(4), depth_min=1.0, depth_max=1.0)
    with pytest.raises(BodySlamHipError):
        prod.raycast(intr(), np.eye(4), depth_min=-0.1, depth_max=1.0)
    assert (prod.raycast(intr(), np.eye(4), depth_min=RC.DEPTH_MIN, depth_max=RC.DEPTH_MAX).depth > 0).any()     # and still works


def test_raycast_writes_nothing_behind_its_outputs():
    from bodyslam_amd import _lib as L
    prod = build_toy(0.01, 0.04)
    n, h, w, guard = 2, 37, 53, 256
    E = np.ascontiguousarray(np.stack([np.linalg.inv(P) for P in RC.toy_views()[:n]]))
    Kd = np.array(K, dtype=np.float64)
    dev = prod.dev
    depth = torch.full((n * h * w + guard,), -7.0, device=dev)
    vertex = torch.full((n * h * w * 3 + guard,), -7.0, device=dev)
    normal = torch.full((n * h * w * 3 + guard,), -7.0, device=dev)
    color = torch.full((n * h * w * 3 + guard,), 0xAB, dtype=torch.uint8, device=dev)
    L.check(L.load_library().bs_tsdf_raycast(Kd.ctypes.data_as(C.c_void_p), E.ctypes.data_as(C.c_void_p), n, h, w, RC.DEPTH_MIN, RC.DEPTH_MAX,
                                             L.p(prod.table_keys), L.p(prod.table_slots), prod.table_cap, L.p(prod.slab_base), prod.slab_units,
                                             prod.res, prod.voxel_length, prod.sdf_trunc, L.p(depth), L.p(vertex), L.p(normal), L.p(color),
                                             L.stream_ptr()), "bs_tsdf_raycast")
    torch.cuda.synchronize()
    assert (depth[n * h * w:] == -7.0).all() and (vertex[n * h * w * 3:] == -7.0).all() and (normal[n * h * w * 3:] == -7.0).all()
    assert (color[n * h * w * 3:] == 0xAB).all()
    assert (depth[:n * h * w] >= 0).all() and (depth[:n * h * w] > 0).any() and (color[:n * h * w * 3] != 0xAB).any()
    want = prod.raycast(intr(h, w), E, depth_min=RC.DEPTH_MIN, depth_max=RC.DEPTH_MAX, vertex=True, normal=True)
    assert torch.equal(depth[:n * h * w].view(n, h, w), want.depth) and torch.equal(color[:n * h * w * 3].view(n, h, w, 3), want.color)
    assert torch.equal(vertex[:n * h * w * 3].view(n, h, w, 3), want.vertex) and torch.equal(normal[:n * h * w * 3].view(n, h, w, 3), want.normal)


# ---- 6. MAP ------------------------------------------------------------------------------------------------------------------------
def test_map_integrate_synthesises_the_model_frame():
    from bodyslam_amd.tsdf import MAP, RGBDImage
    vl = 0.004
    m = MAP(W, H, intr(), "cuda:0", 1000.0, voxel_size=vl, block_count=4096, trunc_voxel_multiplier=5.0)
    assert m.model.res == 16 and abs(m.model.sdf_trunc - 0.02) < 1e-12 and m.raycast_frame is None
    inner = np.zeros((H, W), bool)
    inner[4:-4, 4:-4] = True
    for i, (P, col, d) in enumerate(toy_frames()[:3]):
        rgbd = RGBDImage(col, d)
        rgbd.depth_min, rgbd.depth_max = RC.DEPTH_MIN, RC.DEPTH_MAX            # the reference's frames carry these
        m.integrate(rgbd, i, P)
        # (MAP widens the frame's range by the truncation distance on both sides)
        want = m.model.raycast(intr(), np.linalg.inv(P), depth_min=RC.DEPTH_MIN - m.model.sdf_trunc, depth_max=RC.DEPTH_MAX + m.model.sdf_trunc)
        assert m.raycast_frame.depth.shape == (H, W) and m.raycast_frame.color.shape == (H, W, 3)
        assert torch.equal(m.raycast_frame.depth, want.depth) and torch.equal(m.raycast_frame.color, want.color)
        got = m.raycast_frame.depth.cpu().numpy().astype(np.float64)
        assert (got > 0)[inner].all()
        err = np.abs(got - d)[got > 0] / vl
        print(f"MAP frame {i}: model depth vs analytic, voxels: median {np.median(err):.3f} max {err.max():.3f}")
        assert err.max() <= 0.5
    assert [i for i, _ in m.frame_poses] == [0, 1, 2]
    # a frame without depth_min / depth_max: the bounds come from its depth image
    P, col, d = toy_frames()[3]
    m.integrate(RGBDImage(col, np.rint(d * 1000.0).astype(np.uint16)), 3, torch.from_numpy(P))       # raw depth units / depth_scale
    got = m.raycast_frame.depth.cpu().numpy()
    assert (got > 0)[inner].all() and np.abs(got - d)[got > 0].max() <= 0.5 * vl + 0.0005      # (+ the u16 rounding of the input)
    pcd = m.extract_pcd()
    assert pcd.points.shape[0] > 500 and m.extract_mesh().triangles.shape[0] > 500


# ---- 7. round trip into the evaluation ---------------------------------------------------------------------------------------------
def test_raycast_depth_u16_feeds_the_depth_evaluation():
    from bodyslam_amd import evaluation
    vl, trunc = RC.TOY_MAPS[1]
    prod = build_toy(vl, trunc)
    P, col, d = toy_frames()[0]
    frame = prod.raycast(intr(), np.linalg.inv(P), depth_min=RC.DEPTH_MIN, depth_max=RC.DEPTH_MAX)
    pred = frame.depth_u16()
    assert pred.dtype == torch.int16 and pred.shape == (H, W) and pred.is_cuda
    hit = frame.depth.cpu().numpy() > 0
    assert np.array_equal(pred.cpu().numpy().view(np.uint16), np.rint(frame.depth.cpu().numpy().astype(np.float64) * 1000.0).astype(np.uint16))
    gt = np.rint(d.astype(np.float64) * 1000.0).astype(np.uint16)
    gt[~hit] = 0
    res = evaluation.evaluate_depth(pred, gt, gt_range=(0, 65535), scale=1.0).per_frame
    bound = (0.5 * vl * 1000.0 + 1.0) / gt[gt > 0].min()
    print(f"AbsRel {res['abs_rel_diff'][0]:.3e} (bound {bound:.3e}), delta<1.25 {res['accuracy_1.25'][0]}, pixels {res['n_mask'][0]}")
    assert res["n_mask"][0] == np.count_nonzero(gt) and hit.mean() > 0.9
    assert res["abs_rel_diff"][0] <= bound and res["accuracy_1.25"][0] == 1.0
    # to_rgbd: the model view goes back into a map as a frame
    rgbd = frame.to_rgbd()
    assert rgbd.depth is frame.depth and rgbd.color is frame.color
    from bodyslam_amd.tsdf import TSDF
    again = TSDF(vl, trunc, volume_unit_resolution=8, depth_sampling_stride=4, max_units=8192)
    again.build_3D_map(rgbd, intr(), np.linalg.inv(P))
    assert again.n_units > 100
