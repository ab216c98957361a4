"""CPU checks of the voxel down-sampling: the statement (tests/_voxel_ref.py) on its own -- the derived error bound against the fp64 mean, the
tie lattice whose planes lie on voxel faces, permutation, the identity at a small voxel --, the public interface (signatures, argument
validation before any device call, no CPU fallback), and the usual recipe on the statement: ICP on thinned clouds recovers the pose."""
import dataclasses
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _icp_ref as I  # noqa: E402
import _knn_ref as K  # noqa: E402
import _voxel_ref as V  # noqa: E402

f32, f64 = np.float32, np.float64
SIZES = {0.001: (2806, 1), 0.005: (677, 9), 0.02: (71, 100), 1.0: (1, 2806)}            # h: (voxels, the largest count) on the bumpy target
THIN = 0.004
# The largest distance between a registered source point and its true position when the statement's point-to-plane ICP runs on the bumpy
# pair thinned by the statement at h = 0.004 (medium start; the target keeps 985 of 2806 points, the source 595 of 1937, the target's
# normals averaged and re-normalised; converged after 5 iterations; the error is measured on the full source).  Measured 5.05e-5 m (the
# full clouds: 1.37e-5 m); the bound is four times that, the margin tests/test_knn_gpu.py leaves.
THINNED_RECOVERY_MEASURED = 5.05e-5
THINNED_RECOVERY_BOUND = 4 * THINNED_RECOVERY_MEASURED


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope="module")
def cloud():
    tgt, nrm = I.bumpy_target()
    return tgt, nrm, V.synthetic_colors(len(tgt))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import bodyslam_amd.evaluation as EV
    import bodyslam_amd.pointcloud as PC
    import bodyslam_amd.tsdf as TS
    return PC, EV, TS


def thinned_pair():
    """(source thinned, target thinned, its unit normals, the full source, the true positions) at the medium start"""
    tgt, nrm = I.bumpy_target()
    true = I.bumpy_source_true()
    medium = I.displaced(true, I.MEDIUM)
    t = V.voxel_down_sample(tgt, THIN, normals=nrm, unit_normals=True)
    s = V.voxel_down_sample(medium, THIN)
    return s["points"], t["points"], t["normals"], medium, true


@pytest.mark.parametrize("h", list(SIZES))
def test_error_bound_against_the_fp64_mean(cloud, h):
    tgt, nrm, col = cloud
    r = V.voxel_down_sample(tgt, h, colors=col, normals=nrm)
    m = len(r["points"])
    assert (m, int(r["counts"].max())) == SIZES[h] and int(r["counts"].sum()) == len(tgt)
    mean = V.mean_f64(tgt, r["row_of_point"], m)
    err = np.abs(r["points"].astype(f64) - mean)
    s = r["shift"]
    lo, hi = V.P.bounds(tgt)
    ext = float((hi.astype(f64) - r["origin"]).max())
    ulp = np.spacing(np.abs(r["points"])).astype(f64)
    slack = 8 * np.spacing(np.abs(mean) + np.abs(r["origin"]))                          # the fp64 rounding of a division, a scaling and an addition
    bound = 2.0 ** -(s + 1) + 0.5 * ulp + slack
    print("h", h, "voxels", m, "shift", s, "largest |result - fp64 mean|", err.max(), "of the bound", (err / bound).max())
    assert 2.0 ** (31 - s) <= ext < 2.0 ** (32 - s) and 2.0 ** -(s + 1) < ext * 2.0 ** -32
    assert (err <= bound).all()
    # attributes: 30 fractional bits and half an fp32 ulp
    for name, a in (("colors", col), ("normals", nrm)):
        S = np.zeros((m, 3))
        np.add.at(S, r["row_of_point"], a.astype(f64))
        am = S / r["counts"][:, None]
        assert (np.abs(r[name].astype(f64) - am) <= 2.0 ** -31 + 0.5 * np.spacing(np.abs(r[name])).astype(f64) + 1e-15).all(), name
    # rows come in order of first appearance, and every point went to the voxel it lies in
    assert (np.diff(r["first_index"]) > 0).all() and r["first_index"][0] == 0
    assert np.array_equal(r["row_of_point"][r["first_index"]], np.arange(m))
    v = np.floor((tgt.astype(f64) - r["origin"]) / h)
    assert np.array_equal(v, v[r["first_index"]][r["row_of_point"]])


def test_small_voxel_returns_the_input(cloud):
    tgt, nrm, col = cloud
    r = V.voxel_down_sample(tgt, 0.001, colors=col, normals=nrm)
    assert same_bits(r["points"], tgt) and same_bits(r["colors"], col) and same_bits(r["normals"], nrm)
    assert np.array_equal(r["row_of_point"], np.arange(len(tgt))) and (r["counts"] == 1).all()
    # the rule is needed: the integer mean of a single point alone is not always that point
    s, o = r["shift"], r["origin"]
    plain = (o + np.ldexp(np.rint(np.ldexp(tgt.astype(f64) - o, s)), -s)).astype(f32)
    print("coordinates the integer mean of one point would change", int((plain != tgt).sum()), "of", tgt.size)
    assert 0 < (plain != tgt).sum() < 100
    u = V.voxel_down_sample(tgt, 0.001, normals=nrm, unit_normals=True)["normals"]
    assert np.abs(np.linalg.norm(u.astype(f64), axis=1) - 1.0).max() < 1e-7 and np.abs(u - nrm).max() < 2e-7


def test_tie_lattice():
    lat = K.tie_lattice()                                                             # 9 x 7 x 3 points at multiples of 2^-8 from the origin
    r = V.voxel_down_sample(lat, 2.0 ** -7)
    # o = -2^-8: a voxel of edge 2^-7 begins at every odd multiple of 2^-8, so every second plane lies exactly on a voxel face
    hist = dict(zip(*np.unique(r["counts"], return_counts=True)))
    print("lattice at 2^-7:", len(r["points"]), "voxels, counts", hist)
    assert len(r["points"]) == 40 and hist == {1: 1, 2: 8, 4: 19, 8: 12}
    mean = V.mean_f64(lat, r["row_of_point"], 40)
    assert np.array_equal(r["points"].astype(f64), mean)                              # every mean is exact here
    r = V.voxel_down_sample(lat, 2.0 ** -8)
    assert len(r["points"]) == 189 and (r["counts"] == 1).all() and same_bits(r["points"], lat)
    r = V.voxel_down_sample(lat, 3 * 2.0 ** -8)
    assert int(r["counts"].sum()) == 189 and np.array_equal(r["points"].astype(f64), V.mean_f64(lat, r["row_of_point"], len(r["points"])))


def rows_as_set(r):
    return sorted(zip(r["points"].view(np.uint32).reshape(-1, 3).tolist(), r["counts"].tolist()))


@pytest.mark.parametrize("h", [0.005, 0.02])
def test_permutation(cloud, h):
    tgt, nrm, col = cloud
    perm = np.random.default_rng(31).permutation(len(tgt))
    a = V.voxel_down_sample(tgt, h, colors=col, normals=nrm)
    b = V.voxel_down_sample(tgt[perm], h, colors=col[perm], normals=nrm[perm])
    assert rows_as_set(a) == rows_as_set(b)                                           # the same (point, count) rows, bit for bit
    assert (np.diff(b["first_index"]) > 0).all()
    # the permuted result is the unpermuted one with its rows in the new order of first appearance
    to_a = a["row_of_point"][perm[b["first_index"]]]
    for k in ("points", "colors", "normals", "counts"):
        assert same_bits(b[k], a[k][to_a]), k
    assert np.array_equal(b["row_of_point"], np.argsort(to_a)[a["row_of_point"][perm]])


def test_statement_edge_cases(cloud):
    tgt, nrm, col = cloud
    bad = tgt.copy()
    bad[[0, 1000, 2805]] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]]
    r = V.voxel_down_sample(bad, 0.005, colors=col)
    ok = np.ones(len(tgt), bool)
    ok[[0, 1000, 2805]] = False
    ref = V.voxel_down_sample(bad[ok], 0.005, colors=col[ok])
    assert (r["row_of_point"][~ok] == -1).all() and same_bits(r["row_of_point"][ok], ref["row_of_point"])
    assert same_bits(r["points"], ref["points"]) and same_bits(r["colors"], ref["colors"]) and same_bits(r["counts"], ref["counts"])
    assert np.array_equal(r["first_index"], np.nonzero(ok)[0][ref["first_index"]])
    e = V.voxel_down_sample(np.full((5, 3), np.nan, f32), 0.01, normals=np.zeros((5, 3), f32))
    assert e["points"].shape == (0, 3) and e["normals"].shape == (0, 3) and e["colors"] is None and (e["row_of_point"] == -1).all()
    with pytest.raises(ValueError, match="too small"):
        V.voxel_down_sample(tgt, 1e-8)
    for v in (3.0, np.nan, -2.5, np.inf):
        c = col.copy()
        c[17, 1] = v
        with pytest.raises(ValueError):
            V.voxel_down_sample(tgt, 0.005, colors=c)
    c = col.copy()
    c[0] = np.nan                                                                     # the attributes of a point in no voxel are not looked at
    assert same_bits(V.voxel_down_sample(bad, 0.005, colors=c)["colors"], r["colors"])
    flat = V.voxel_down_sample(np.array([[1, 0, 0], [1, 0, 0]], f32), 0.5, normals=np.array([[0, 0, 1], [0, 0, -1]], f32), unit_normals=True)
    assert flat["counts"].tolist() == [2] and flat["normals"].tolist() == [[0, 0, 0]]


def test_public_signatures(built):
    PC, EV, TS = built

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert params(PC.voxel_down_sample) == [("points", E), ("voxel_size", E), ("colors", None), ("normals", None), ("unit_normals", False), ("device", 0)]
    assert [f.name for f in dataclasses.fields(PC.VoxelDownSample)] == ["points", "colors", "normals", "counts", "first_index", "row_of_point"]
    assert params(TS.PointCloud.voxel_down_sample) == [("self", E), ("voxel_size", E)]
    assert params(TS.PointCloud.voxel_down_sample_and_trace) == [("self", E), ("voxel_size", E)]
    assert "voxel_size" in EV._ICP_KEYS
    import bodyslam_amd.registration as REG
    assert "voxel_size" not in inspect.signature(REG.registration_icp).parameters
    assert PC.voxel_table_slots(1) == 2 and PC.voxel_table_slots(2806) == 8192 and PC.voxel_table_slots(2048) == 4096
    assert "voxel down-sampling" not in PC.__doc__.split("Not built")[1]


def test_geometry_matches_the_statement(built, cloud):
    PC, EV, TS = built
    tgt = cloud[0]
    lo, hi = V.P.bounds(tgt)
    for h in (0.001, 0.005, 0.02, 1.0, 3 * 2.0 ** -8):
        _, o, s = V.geometry(tgt, h)
        go, gs = PC.voxel_geometry(lo, hi, h)
        assert same_bits(go, o) and gs == s
    with pytest.raises(ValueError, match="too small"):
        PC.voxel_geometry(lo, hi, 1e-8)


def test_argument_validation_before_any_device_call(built, cloud, monkeypatch):
    PC, EV, TS = built
    from bodyslam_amd import _lib
    tgt, nrm, col = cloud

    def touched(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "init", touched)
    for h in (0.0, -0.01, np.nan, np.inf, "0.01", True, None, [0.01]):
        with pytest.raises(ValueError):
            PC.voxel_down_sample(tgt, h)
        with pytest.raises(ValueError):
            TS.PointCloud(tgt, col, nrm).voxel_down_sample(h)
        if h is not None:                                                             # (None there: no thinning)
            with pytest.raises(ValueError):
                EV.evaluate_reconstruction_aligned(tgt, tgt, icp=dict(max_correspondence_distance=0.005, voxel_size=h))
    for bad in (np.zeros((4, 2), f32), np.zeros((0, 3), f32), None, tgt.astype(np.int32)):
        with pytest.raises(ValueError):
            PC.voxel_down_sample(bad, 0.01)
    for bad in (nrm[:-1], nrm[:, :2], nrm.astype(np.int32), nrm.astype(np.float16), "n", torch.zeros(len(tgt), 3, dtype=torch.int64)):
        with pytest.raises(ValueError):
            PC.voxel_down_sample(tgt, 0.01, colors=bad)
        with pytest.raises(ValueError):
            PC.voxel_down_sample(tgt, 0.01, normals=bad)


def test_no_cpu_fallback(built, cloud):
    PC, EV, TS = built
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from bodyslam_amd._lib import BodySlamHipError
    tgt, nrm, col = cloud
    with pytest.raises(BodySlamHipError):
        PC.voxel_down_sample(tgt, 0.005, colors=col, normals=nrm.astype(f64))
    with pytest.raises(BodySlamHipError):
        TS.PointCloud(tgt, col, nrm).voxel_down_sample(0.005)
    with pytest.raises(BodySlamHipError):
        TS.PointCloud(tgt, col).voxel_down_sample_and_trace(0.005)
    with pytest.raises(BodySlamHipError):
        EV.evaluate_reconstruction_aligned(tgt, tgt, icp=dict(max_correspondence_distance=0.005, voxel_size=0.004))


def test_thinned_alignment_recovers_the_pose():
    src, tgt, nrm, medium, true = thinned_pair()
    assert np.abs(np.linalg.norm(nrm.astype(f64), axis=1) - 1.0).max() < 1e-6
    r = I.icp(src, tgt, I.RADIUS, estimation="point_to_plane", normals=nrm)
    err = np.linalg.norm(I.moved(medium, r["T"]) - true, axis=1).max()
    print("thinned at", THIN, ":", len(src), "of", len(medium), "source and", len(tgt), "of", I.N_TARGET, "target points;", r["status"], r["iterations"],
          "iterations, fitness", r["fitness"], "largest distance of a full-cloud point to its true position", err)
    assert r["status"] == "converged"
    assert err <= THINNED_RECOVERY_BOUND
