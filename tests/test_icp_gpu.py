"""GPU tests of the rigid ICP registration (csrc/icp.hip, bodyslam_amd/registration.py) against the statement tests/_icp_ref.py on the bumpy pair:
2 806 target points, 1 937 source points = eight blocks, the last one partial."""
import csv
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _icp_ref as I  # noqa: E402
import _pointcloud_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
RECOVERY_BOUND = 5e-5            # tests/test_icp_cpu.py: the statement measures 1.37e-5 m
SUM_TOL = 1e-12                  # an fp64 sum of 2 000 terms in another order differs by at most n 2^-53 = 2e-13 of the sum of the absolute terms
T_TOL = 1e-9                     # step errors of 1e-13, the conditioning of the normal matrix and contraction give ~1e-11


@pytest.fixture(scope="module")
def REG():
    import bodyslam_amd.registration as REG
    return REG


@pytest.fixture(scope="module")
def pair():
    tgt, nrm = I.bumpy_target()
    true = I.bumpy_source_true()
    lo, hi = P.bounds(tgt)
    return dict(tgt=tgt, nrm=nrm, true=true, h0=P.default_cell_size(lo, hi, len(tgt)), small=I.displaced(true, I.SMALL),
                medium=I.displaced(true, I.MEDIUM), lattice=I.displaced(tgt[::3].astype(f64), I.LATTICE_MOTION))


RUNS = {"plane small": ("small", "point_to_plane"), "plane medium": ("medium", "point_to_plane"), "point lattice": ("lattice", "point_to_point")}


@pytest.fixture(scope="module")
def runs(pair):
    """the statement's whole runs, computed once"""
    return {k: I.icp(pair[s], pair["tgt"], I.RADIUS, estimation=e, normals=pair["nrm"]) for k, (s, e) in RUNS.items()}


def check_step(REG, src, tgt, nrm, init, est, h0, what):
    want = I.iteration(src, tgt, np.eye(4) if init is None else init, I.RADIUS, est, nrm)
    n = I.N_PLANE if est == "point_to_plane" else I.N_POINT
    first = None
    for factor in (1.0, 0.25, 4.0):                                            # a quarter of the default edge: multi-shell searches up to the radius
        partial, total = REG._step_sums(src, tgt, I.RADIUS, init=init, estimation=est, target_normals=nrm, cell_size=h0 * factor)
        assert partial.shape == (-(-len(src) // 256), 32)
        assert total[0] == want["count"] and total[1] == want["usable"], (what, factor, total[:2], want["count"], want["usable"])
        rel = np.abs(total[3:3 + n] - want["sums"]) / want["abs_sums"]
        rel_d2 = abs(total[2] - want["sum_d2"]) / want["sum_d2"]
        print(what, "cell factor", factor, "count", int(total[0]), "usable", int(total[1]), "largest relative difference of a sum", rel.max(), "of sum d2", rel_d2)
        assert rel.max() <= SUM_TOL and rel_d2 <= SUM_TOL
        assert np.all(total[3 + n:] == 0.0)
        if first is None:
            first = partial
        assert np.array_equal(first.view(np.uint64), partial.view(np.uint64)), f"{what}: the partials depend on the cell size ({factor})"
    return want


# ---- 1: one step against the statement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("est", ["point_to_plane", "point_to_point"])
@pytest.mark.parametrize("start", ["identity", "given"])
def test_one_step(REG, pair, est, start):
    init = None if start == "identity" else I.small_pose(*I.SMALL)              # the medium start as it is, and from a partial correction
    want = check_step(REG, pair["medium"], pair["tgt"], pair["nrm"], init, est, pair["h0"], f"{est} init {start}")
    assert 0.5 < want["fitness"] < 1.0                                          # some sources search up to the radius and find nothing


# ---- 2, 3: whole runs, and the recovery bound on the device result ------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(RUNS))
def test_whole_run(REG, pair, runs, case):
    s, est = RUNS[case]
    want = runs[case]
    got = REG.registration_icp(pair[s], pair["tgt"], I.RADIUS, estimation=est, target_normals=pair["nrm"])
    dT = np.abs(got.transformation - want["T"]).max()
    print(case, got.status, got.iterations, "fitness", got.fitness, "rmse", got.inlier_rmse, "largest |T - T_statement|", dT)
    assert got.status == want["status"] == "converged" and got.iterations == want["iterations"] == len(got.log)
    assert [r[2] for r in got.log] == [r[2] for r in want["log"]] and [r[0] for r in got.log] == [r[0] for r in want["log"]]
    # (one fp32 ulp at 0.3 m is 3e-8: a T within T_TOL of the statement's can round a coordinate of p the other way)
    assert np.abs(np.array([r[1] for r in got.log]) - np.array([r[1] for r in want["log"]])).max() <= 3e-8
    assert got.fitness == want["fitness"] and abs(got.inlier_rmse - want["rmse"]) <= 3e-8
    assert got.transformation.shape == (4, 4) and got.transformation.dtype == f64 and np.array_equal(got.transformation[3], [0, 0, 0, 1])
    assert dT <= T_TOL
    again = REG.registration_icp(pair[s], pair["tgt"], I.RADIUS, estimation=est, target_normals=pair["nrm"])
    assert np.array_equal(got.transformation.view(np.uint64), again.transformation.view(np.uint64)) and got.log == again.log
    assert (got.fitness, got.inlier_rmse, got.status) == (again.fitness, again.inlier_rmse, again.status)
    true = pair["true"] if s != "lattice" else pair["tgt"][::3].astype(f64)
    err = np.linalg.norm(I.moved(pair[s], got.transformation) - true, axis=1).max()
    print(case, "largest distance between a registered source point and its true position", err)
    assert err <= (RECOVERY_BOUND if s != "lattice" else 1e-6)


# ---- 4: other paths ------------------------------------------------------------------------------------------------------------------------
def test_nan_rows_and_bad_normals(REG, pair):
    src = pair["small"].copy()
    src[5] = np.nan
    src[300, 1] = np.inf
    src[1936, 2] = np.nan
    nrm = pair["nrm"].copy()
    nrm[::7] = 0.0
    nrm[3::11, 0] = np.nan
    want = check_step(REG, src, pair["tgt"], nrm, None, "point_to_plane", pair["h0"], "NaN rows, zero and NaN normals")
    assert want["count"] == len(src) - 3 and 6 <= want["usable"] < want["count"]
    check_step(REG, src, pair["tgt"], None, None, "point_to_point", pair["h0"], "NaN rows")
    ref = I.icp(src, pair["tgt"], I.RADIUS, estimation="point_to_plane", normals=nrm)
    got = REG.registration_icp(src, pair["tgt"], I.RADIUS, target_normals=nrm)                  # "auto": point-to-plane
    assert (got.status, got.iterations, [r[2] for r in got.log]) == (ref["status"], ref["iterations"], [r[2] for r in ref["log"]])
    assert got.fitness == ref["fitness"] < 1.0 and np.abs(got.transformation - ref["T"]).max() <= T_TOL


def test_fp64_device_tensor_and_prebuilt_index(REG, pair):
    import bodyslam_amd.pointcloud as PC
    import bodyslam_amd.tsdf as TS
    tgt, nrm = pair["tgt"], pair["nrm"]
    src64 = (pair["true"] @ np.linalg.inv(I.small_pose(*I.SMALL))[:3, :3].T + np.linalg.inv(I.small_pose(*I.SMALL))[:3, 3])     # not rounded to fp32
    ref = I.icp(src64, tgt, I.RADIUS, estimation="point_to_plane", normals=nrm)
    got = REG.registration_icp(src64, tgt.astype(f64), I.RADIUS, target_normals=nrm.astype(f64))
    assert (got.status, got.iterations, [r[2] for r in got.log]) == (ref["status"], ref["iterations"], [r[2] for r in ref["log"]])
    assert np.abs(got.transformation - ref["T"]).max() <= T_TOL
    check_step(REG, src64, tgt, nrm, I.small_pose(*I.SMALL), "point_to_plane", pair["h0"], "fp64 source")
    host = REG.registration_icp(pair["small"], tgt, I.RADIUS, target_normals=nrm)
    dev = torch.device("cuda", 0)
    on_device = REG.registration_icp(torch.from_numpy(pair["small"]).to(dev), torch.from_numpy(tgt).to(dev), I.RADIUS,
                                     target_normals=torch.from_numpy(nrm).to(dev))
    cloud = REG.registration_icp(pair["small"], TS.PointCloud(tgt, np.zeros_like(tgt), nrm), I.RADIUS)
    index = REG.registration_icp(pair["small"], PC.NearestNeighbours(tgt, cell_size=0.003), I.RADIUS, target_normals=nrm)
    for other in (on_device, cloud, index):
        assert np.array_equal(host.transformation.view(np.uint64), other.transformation.view(np.uint64)) and host.log == other.log
    p2p = REG.registration_icp(pair["lattice"], PC.NearestNeighbours(tgt), I.RADIUS)            # "auto" without normals: point-to-point
    assert p2p.status == "converged" and p2p.iterations == 3


def test_evaluate_registration(REG, pair):
    for src, T in ((pair["medium"], None), (pair["medium"], I.small_pose(*I.MEDIUM)), (pair["small"], I.small_pose(*I.SMALL))):
        fit, rmse, _ = I.evaluate(src, pair["tgt"], I.RADIUS, T)
        got = REG.evaluate_registration(src, pair["tgt"], I.RADIUS, T)
        print("evaluate_registration", got.fitness, got.inlier_rmse, "statement", fit, rmse)
        assert got.status == "evaluated" and got.fitness == fit and abs(got.inlier_rmse - rmse) <= 1e-12 * rmse
        assert np.array_equal(got.transformation, np.eye(4) if T is None else T)


def test_max_iteration_and_no_match(REG, pair):
    got = REG.registration_icp(pair["medium"], pair["tgt"], I.RADIUS, target_normals=pair["nrm"], max_iteration=1)
    assert got.status == "max_iteration" and got.iterations == 1 and not np.array_equal(got.transformation, np.eye(4))
    ref = I.icp(pair["medium"], pair["tgt"], I.RADIUS, normals=pair["nrm"], max_iteration=1)
    assert got.fitness == ref["fitness"] and np.abs(got.transformation - ref["T"]).max() <= T_TOL
    nine = REG.registration_icp(pair["lattice"], pair["tgt"], I.RADIUS, estimation="point_to_point", max_iteration=9, relative_rmse=0.0)
    assert nine.status == "max_iteration" and nine.iterations == 9                             # more than one chunk of launches
    init = I.small_pose(0.001, 0.002, -0.001, 1e-4, 0.0, -1e-4)
    for est in ("point_to_plane", "point_to_point"):
        far = REG.registration_icp(pair["small"] + f32(1.0), pair["tgt"], I.RADIUS, init=init, estimation=est, target_normals=pair["nrm"])
        assert far.status == "degenerate"
        two = REG.registration_icp(pair["small"][:2], pair["tgt"], I.RADIUS, init=init, estimation=est, target_normals=pair["nrm"])
        assert two.status == "degenerate" and np.array_equal(two.transformation, init)


# ---- 5: the reconstruction evaluation with an alignment ---------------------------------------------------------------------------------
KEYS = [f"{s}_{k}" for s in ("accuracy", "completeness") for k in ("mean", "median", "rmse", "max")] + ["chamfer"] + \
       [f"{k}@{float(f32(t))!r}" for t in (0.001, 0.002, 0.005) for k in ("precision", "recall", "fscore")] + \
       ["n_pred", "n_gt", "n_unmatched_pred", "n_unmatched_gt"]


def test_evaluate_reconstruction_aligned(REG, pair, tmp_path):
    import bodyslam_amd.evaluation as EV
    import bodyslam_amd.tsdf as TS
    tgt, nrm, true = pair["tgt"], pair["nrm"], pair["true"]
    gt = TS.PointCloud(tgt, np.zeros_like(tgt), nrm)
    icp = dict(max_correspondence_distance=I.RADIUS)
    best = EV.evaluate_reconstruction(true.astype(f32), gt)                                   # the undisplaced source
    plain = EV.evaluate_reconstruction(pair["medium"], gt)
    got = EV.evaluate_reconstruction_aligned(pair["medium"], gt, align="icp", icp=icp)
    print("accuracy mean: undisplaced", best.accuracy.mean, "displaced", plain.accuracy.mean, "aligned", got.accuracy.mean, "fscore at 1 mm",
          plain.fscore[0], "->", got.fscore[0])
    assert got.alignment.status == "converged" and plain.alignment is None
    assert abs(got.accuracy.mean - best.accuracy.mean) <= RECOVERY_BOUND                      # the nearest-neighbour distance is 1-Lipschitz in the point
    assert got.fscore[0] > plain.fscore[0]
    err = np.linalg.norm(I.moved(pair["medium"], got.alignment.transformation) - true, axis=1).max()
    assert err <= RECOVERY_BOUND
    # the swapped direction: the scan has no normals, the map has them
    pred = TS.PointCloud(tgt, np.zeros_like(tgt), nrm)
    swapped = EV.evaluate_reconstruction_aligned(pred, pair["medium"], align="icp", icp=icp)
    back = np.linalg.inv(swapped.alignment.transformation)
    err = np.linalg.norm(I.moved(pair["medium"], back) - true, axis=1).max()
    print("swapped direction: largest distance to the true position", err, swapped.alignment.status)
    assert swapped.alignment.status == "converged" and err <= RECOVERY_BOUND
    # with a similarity in front: the map's normals follow it
    sim = (I.small_pose(0.2, -0.1, 0.3, 0, 0, 0)[:3, :3], 0.5, np.array([0.01, 0.02, -0.03]))
    A = np.eye(4)
    A[:3, :3], A[:3, 3] = sim[1] * sim[0], sim[2]
    raw = TS.PointCloud(I.moved(tgt, np.linalg.inv(A)).astype(f32), np.zeros_like(tgt), (nrm.astype(f64) @ sim[0]).astype(f32))
    scaled = EV.evaluate_reconstruction_aligned(raw, pair["medium"], transform=sim, align="icp", icp=icp)
    err = np.linalg.norm(I.moved(pair["medium"], np.linalg.inv(scaled.alignment.transformation)) - true, axis=1).max()
    print("swapped direction behind a similarity", err)
    assert scaled.alignment.status == "converged" and err <= RECOVERY_BOUND
    # unchanged outputs
    assert list(plain.as_dict()) == KEYS == list(got.as_dict())
    with open(got.write_csv(str(tmp_path / "m.csv")), newline="") as f:
        rows = list(csv.DictReader(f))
    assert [r["Metric"] for r in rows] == KEYS
