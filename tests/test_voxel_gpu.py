"""GPU checks of the voxel down-sampling (csrc/voxel.hip, bodyslam_amd/pointcloud.py): everything bit-equal to the statement
tests/_voxel_ref.py -- the bumpy target with colours and normals at four voxel sizes, the tie lattice, every table size, every order of the
points, non-finite rows, a translated cloud, the errors --, then PointCloud.voxel_down_sample and the thinned alignment of
evaluate_reconstruction_aligned.  The largest input is 2 806 points: ten blocks of 256 and a partial one."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _icp_ref as I  # noqa: E402
import _knn_ref as K  # noqa: E402
import _voxel_ref as V  # noqa: E402
from test_voxel_cpu import THIN, THINNED_RECOVERY_BOUND, rows_as_set, same_bits, thinned_pair  # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
T_TOL = 1e-9                     # tests/test_icp_gpu.py's tolerance between the device's transform and the statement's
FIELDS = ("points", "colors", "normals", "counts", "first_index", "row_of_point")
_REF = {}


@pytest.fixture(scope="module")
def PC():
    import bodyslam_amd.pointcloud as PC
    return PC


@pytest.fixture(scope="module")
def cloud():
    tgt, nrm = I.bumpy_target()
    return tgt, nrm, V.synthetic_colors(len(tgt))


def ref(name, *a, **k):
    """the statement's result, computed once per case"""
    if name not in _REF:
        _REF[name] = V.voxel_down_sample(*a, **k)
    return _REF[name]


def host(r):
    return {k: None if getattr(r, k) is None else getattr(r, k).cpu().numpy() for k in FIELDS}


def check(got, want, what):
    got = host(got) if not isinstance(got, dict) else got
    for k in FIELDS:
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert same_bits(got[k], want[k]), (what, k, got[k].shape, want[k].shape)
    return got


# ---- 1: the bumpy target with colours and normals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [0.001, 0.005, 0.02, 1.0])
def test_bumpy_target(PC, cloud, h):
    tgt, nrm, col = cloud
    for unit in (False, True):
        want = ref(("bumpy", h, unit), tgt, h, colors=col, normals=nrm, unit_normals=unit)
        r = PC.voxel_down_sample(tgt, h, colors=col, normals=nrm, unit_normals=unit)
        assert all(getattr(r, k).is_cuda for k in FIELDS) and r.counts.dtype == torch.int32 and r.points.dtype == torch.float32
        got = check(r, want, (h, unit))
    if h == 0.001:
        assert same_bits(got["points"], tgt) and same_bits(got["colors"], col)
        assert same_bits(host(PC.voxel_down_sample(tgt, h, normals=nrm))["normals"], nrm)
    if h == 1.0:
        assert got["counts"].tolist() == [2806]
    check(PC.voxel_down_sample(tgt.astype(f64), h, normals=nrm.astype(f64)), ref(("bumpy n", h), tgt, h, normals=nrm), (h, "fp64 in, normals only"))
    check(PC.voxel_down_sample(torch.from_numpy(tgt).cuda(), h), ref(("bumpy p", h), tgt, h), (h, "points only, device in"))


# ---- 2: the lattice ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [2.0 ** -7, 2.0 ** -8, 3 * 2.0 ** -8])
def test_tie_lattice(PC, h):
    lat = K.tie_lattice()
    got = check(PC.voxel_down_sample(lat, h), ref(("lattice", h), lat, h), h)
    if h != 3 * 2.0 ** -8:
        assert len(got["points"]) == {2.0 ** -7: 40, 2.0 ** -8: 189}[h]


# ---- 3: the table size, through the bindings -------------------------------------------------------------------------------------------
def test_table_size_and_two_runs(PC, cloud):
    tgt, nrm, col = cloud
    d = [torch.from_numpy(a).cuda() for a in (tgt, col, nrm)]
    for h in (0.005, 1.0):
        want = ref(("bumpy", h, False), tgt, h, colors=col, normals=nrm, unit_normals=False)
        lo, hi = V.P.bounds(tgt)
        origin, shift = PC.voxel_geometry(lo, hi, h)
        default = PC.voxel_table_slots(len(tgt))
        assert default == 8192
        for slots in (4096, default, default, 8 * default):                               # 4096: the tightest power of two above n = 2806
            check(PC._voxel_rows(d[0], d[1], d[2], origin, h, shift, False, slots), want, (h, slots))


def test_bindings_directly(PC, cloud):
    """the four launches as a caller of _lib sees them, on the tightest table"""
    from bodyslam_amd import _lib as L
    tgt, _, _ = cloud
    h, n, slots = 0.005, len(tgt), 4096
    want = ref(("bumpy p", h), tgt, h)
    pts = torch.from_numpy(tgt).cuda()
    L.init(0)
    origin, shift = PC.voxel_geometry(*V.P.bounds(tgt), h)
    i32 = dict(dtype=torch.int32, device="cuda")
    keys = torch.full((slots,), L.PC_VOXEL_EMPTY_KEY, dtype=torch.int64, device="cuda")
    first = torch.full((slots,), L.PC_VOXEL_NO_POINT, **i32)
    slot, leader, flag, row = (torch.empty(n, **i32) for _ in range(4))
    status = torch.zeros(1, **i32)
    L.pc_voxel_assign(pts, origin, h, keys, first, slot, status)
    L.pc_voxel_flags(slot, first, leader, flag)
    rank = torch.cumsum(flag, 0).to(torch.int32)
    m = int(rank[-1])
    assert m == len(want["points"]) and int((keys != L.PC_VOXEL_EMPTY_KEY).sum()) == m and int(status) == 0
    sums, counts, first_index = torch.zeros(m, 3, dtype=torch.int64, device="cuda"), torch.zeros(m, **i32), torch.empty(m, **i32)
    L.pc_voxel_accumulate(pts, None, None, origin, shift, leader, rank, sums, counts, first_index, row, status)
    out = torch.empty(m, 3, device="cuda")
    L.pc_voxel_finish(pts, None, None, sums, counts, first_index, origin, shift, False, out, None, None)
    assert int(status) == 0
    got = dict(points=out, colors=None, normals=None, counts=counts, first_index=first_index, row_of_point=row)
    check({k: None if v is None else v.cpu().numpy() for k, v in got.items()}, want, "bindings")


# ---- 4: the order of the points --------------------------------------------------------------------------------------------------------
def test_order(PC, cloud):
    tgt, nrm, col = cloud
    h = 0.005
    base = ref(("bumpy", h, False), tgt, h, colors=col, normals=nrm, unit_normals=False)
    perm = np.random.default_rng(31).permutation(len(tgt))
    by_voxel = np.argsort(base["row_of_point"], kind="stable")                            # runs of 1 .. 9 equal rows crossing wave and block borders
    for name, order in (("permuted", perm), ("sorted by voxel", by_voxel)):
        want = ref(("bumpy", name), tgt[order], h, colors=col[order], normals=nrm[order])
        got = check(PC.voxel_down_sample(tgt[order], h, colors=col[order], normals=nrm[order]), want, name)
        assert rows_as_set(got) == rows_as_set(base)
    coarse = ref(("bumpy", 0.02, False), tgt, 0.02, colors=col, normals=nrm, unit_normals=False)
    order = np.argsort(coarse["row_of_point"], kind="stable")                             # runs of up to 100: longer than a wave
    check(PC.voxel_down_sample(tgt[order], 0.02, colors=col[order]), ref(("bumpy", "long runs"), tgt[order], 0.02, colors=col[order]), "long runs")
    two = np.zeros((130, 3), f32)                                                         # two voxels alternating over two waves and two lanes
    two[:, 0] = np.where(np.arange(130) % 2 == 0, 0.001, 0.011) + np.arange(130) * 1e-6
    two[:, 1] = np.arange(130) * 2e-6
    got = check(PC.voxel_down_sample(two, 0.005, normals=np.tile(f32([0.6, 0.0, 0.8]), (130, 1))),
                ref("alternating", two, 0.005, normals=np.tile(f32([0.6, 0.0, 0.8]), (130, 1))), "alternating")
    assert got["counts"].tolist() == [65, 65]


# ---- 5: non-finite rows ------------------------------------------------------------------------------------------------------------------
def test_non_finite_rows(PC, cloud):
    tgt, nrm, col = cloud
    bad = tgt.copy()
    bad[[0, 1000, 2805]] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]]
    c = col.copy()
    c[0] = np.nan                                                                         # (the colour of a point in no voxel is not looked at)
    got = check(PC.voxel_down_sample(bad, 0.005, colors=c, normals=nrm), ref("non-finite", bad, 0.005, colors=c, normals=nrm), "non-finite")
    assert got["row_of_point"][[0, 1000, 2805]].tolist() == [-1, -1, -1] and (np.delete(got["row_of_point"], [0, 1000, 2805]) >= 0).all()
    ok = np.ones(len(tgt), bool)
    ok[[0, 1000, 2805]] = False
    rest = ref("non-finite rest", tgt[ok], 0.005, colors=col[ok], normals=nrm[ok])
    assert all(same_bits(got[k], rest[k]) for k in ("points", "colors", "normals", "counts"))
    r = PC.voxel_down_sample(np.full((5, 3), np.nan, f32), 0.01, normals=np.zeros((5, 3), f32))
    assert tuple(r.points.shape) == (0, 3) and tuple(r.normals.shape) == (0, 3) and r.colors is None and r.points.is_cuda
    assert r.counts.numel() == 0 and r.first_index.numel() == 0 and r.row_of_point.tolist() == [-1] * 5


# ---- 6: negative and large coordinates --------------------------------------------------------------------------------------------------
def test_translated(PC, cloud):
    tgt, nrm, col = cloud
    moved = (tgt.astype(f64) + np.array([-3.0, 100.0, 0.5])).astype(f32)
    for h in (0.005, 0.02):
        check(PC.voxel_down_sample(moved, h, colors=col), ref(("moved", h), moved, h, colors=col), ("moved", h))


# ---- 7: errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors(PC, cloud, monkeypatch):
    from bodyslam_amd import _lib as L
    tgt, nrm, col = cloud
    for v in (3.0, np.nan):
        c = col.copy()
        c[1234, 2] = v
        with pytest.raises(ValueError):
            PC.voxel_down_sample(tgt, 0.005, colors=c)
        with pytest.raises(ValueError):
            PC.voxel_down_sample(tgt, 0.005, colors=col, normals=c)

    def launched(*a, **k):
        raise AssertionError("a voxel kernel was launched")
    monkeypatch.setattr(L, "pc_voxel_assign", launched)
    with pytest.raises(ValueError, match="too small"):
        PC.voxel_down_sample(tgt, 1e-8)                                                   # 0.12 m / 1e-8 m = 1.2e7 voxels > 2^21 along x


# ---- 8: the PointCloud methods -------------------------------------------------------------------------------------------------------------
def test_point_cloud_methods(PC, cloud):
    import bodyslam_amd.tsdf as TS
    tgt, nrm, col = cloud
    h = 0.005
    want = ref(("bumpy", h, False), tgt, h, colors=col, normals=nrm, unit_normals=False)
    out = TS.PointCloud(tgt, col, nrm).voxel_down_sample(h)
    assert all(isinstance(a, np.ndarray) for a in (out.points, out.colors, out.normals))
    assert same_bits(out.points, want["points"]) and same_bits(out.colors, want["colors"]) and same_bits(out.normals, want["normals"])
    out, rows, counts = TS.PointCloud(tgt, col).voxel_down_sample_and_trace(h)
    assert out.normals is None and isinstance(rows, np.ndarray) and same_bits(rows, want["row_of_point"]) and same_bits(counts, want["counts"])
    dev = TS.PointCloud(torch.from_numpy(tgt).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(nrm).cuda())
    out, rows, counts = dev.voxel_down_sample_and_trace(h)
    assert all(a.is_cuda for a in (out.points, out.colors, out.normals, rows, counts))
    assert same_bits(out.points.cpu().numpy(), want["points"]) and same_bits(out.normals.cpu().numpy(), want["normals"])
    assert same_bits(rows.cpu().numpy(), want["row_of_point"]) and same_bits(dev.voxel_down_sample(h).colors.cpu().numpy(), want["colors"])


# ---- 9: the thinned alignment --------------------------------------------------------------------------------------------------------------
def test_evaluate_reconstruction_aligned_with_voxel_size(PC, cloud):
    import bodyslam_amd.evaluation as EV
    import bodyslam_amd.tsdf as TS
    tgt, nrm, _ = cloud
    src, thin_tgt, thin_nrm, medium, true = thinned_pair()
    want = I.icp(src, thin_tgt, I.RADIUS, estimation="point_to_plane", normals=thin_nrm)
    gt = TS.PointCloud(tgt, np.zeros_like(tgt), nrm)
    icp = dict(max_correspondence_distance=I.RADIUS)
    got = EV.evaluate_reconstruction_aligned(medium, gt, icp=dict(icp, voxel_size=THIN))
    T = got.alignment.transformation
    dT = np.abs(T - want["T"]).max()
    err = np.linalg.norm(I.moved(medium, T) - true, axis=1).max()
    print("thinned alignment:", got.alignment.status, got.alignment.iterations, "iterations (statement", want["iterations"], "), fitness",
          got.alignment.fitness, "(statement", want["fitness"], "), largest |T - T_statement|", dT, "largest distance to the true position", err)
    assert got.alignment.status == want["status"] == "converged" and dT <= T_TOL
    assert err <= THINNED_RECOVERY_BOUND
    under = EV.evaluate_reconstruction(medium, gt, transform=T)                            # the metrics are the full clouds' under that alignment
    assert got.as_dict() == under.as_dict() and got.n_pred == len(medium) and got.n_gt == len(tgt)
    plain, again = (EV.evaluate_reconstruction_aligned(medium, gt, icp=icp) for _ in range(2))
    direct = __import__("bodyslam_amd.registration", fromlist=["x"]).registration_icp(medium, gt, I.RADIUS)
    assert np.array_equal(plain.alignment.transformation.view(np.uint64), direct.transformation.view(np.uint64))        # without the key: today's
    assert plain.as_dict() == again.as_dict() and plain.alignment.log == direct.log
    # the swapped direction thins the map and its normals
    swapped = EV.evaluate_reconstruction_aligned(gt, medium, icp=dict(icp, voxel_size=THIN))
    err = np.linalg.norm(I.moved(medium, np.linalg.inv(swapped.alignment.transformation)) - true, axis=1).max()
    print("swapped direction, thinned: largest distance to the true position", err)
    assert swapped.alignment.status == "converged" and err <= THINNED_RECOVERY_BOUND
