"""CPU checks of the rigid ICP registration: the statement (tests/_icp_ref.py) on the bumpy pair -- well-posedness, point-to-plane recovery at
two starts, point-to-point on the lattice against itself, degenerate input --, argument validation before any device call, the public
signatures, and no CPU fallback."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _icp_ref as I  # noqa: E402

f32 = np.float32
# The largest distance between a registered source point and its true position, point-to-plane on the bumpy pair.  The statement measures
# 1.37e-5 m at both starts (the 2 mm sampling of the target: 3.4e-6 m on a 1 mm lattice); the bound leaves a factor 3.5.
RECOVERY_BOUND = 5e-5


@pytest.fixture(scope="module")
def pair():
    tgt, nrm = I.bumpy_target()
    return tgt, nrm, I.bumpy_source_true()


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import bodyslam_amd.evaluation as EV
    import bodyslam_amd.registration as REG
    import bodyslam_amd.tsdf as TS
    return REG, EV, TS


def test_bumpy_pair(pair):
    tgt, nrm, true = pair
    assert tgt.shape == (I.N_TARGET, 3) and nrm.shape == tgt.shape and true.shape == (I.N_SOURCE, 3) and tgt.dtype == f32 and nrm.dtype == f32
    assert len(true) % 256 and len(true) // 256 + 1 == 8                       # eight blocks, the last one partial
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    fit = {k: I.evaluate(I.displaced(true, m), tgt, I.RADIUS)[0] for k, m in (("small", I.SMALL), ("medium", I.MEDIUM))}
    print("fitness at the start", fit)
    assert fit["small"] == 1.0 and 0.5 < fit["medium"] < 0.8


def test_well_posed(pair):
    """The point-to-plane normal matrix at the truth, with lengths in units of the source's rms distance from c so that its rotation and
    translation blocks are commensurable (in metres the ratio is that length scale's, 1.4e4): eigenvalue ratio below 100 (measured 25;
    _render.g's height field: its in-plane directions slide)."""
    tgt, nrm, true = pair
    it = I.iteration(true.astype(f32), tgt, np.eye(4), I.RADIUS, "point_to_plane", nrm)
    A, _ = I.normal_matrix(it["sums"])
    scale = np.sqrt(((true - it["c"]) ** 2).sum(1).mean())
    S = np.diag([1 / scale] * 3 + [1.0] * 3)
    ev = np.linalg.eigvalsh(S @ A @ S)
    print("rms radius", scale, "eigenvalues", ev, "ratio", ev[-1] / ev[0], "unscaled ratio", np.linalg.cond(A))
    assert ev[0] > 0 and ev[-1] / ev[0] < 100.0


@pytest.mark.parametrize("start", ["small", "medium"])
def test_point_to_plane_recovers_the_pose(pair, start):
    tgt, nrm, true = pair
    src = I.displaced(true, getattr(I, start.upper()))
    r = I.icp(src, tgt, I.RADIUS, estimation="point_to_plane", normals=nrm)
    err = np.linalg.norm(I.moved(src, r["T"]) - true, axis=1).max()
    print(start, r["status"], r["iterations"], "fitness", r["fitness"], "rmse", r["rmse"], "largest distance to the true position", err)
    assert r["status"] == "converged" and r["iterations"] <= 12 and r["fitness"] == 1.0
    assert err <= RECOVERY_BOUND


def test_point_to_point_lattice_to_itself(pair):
    tgt, _, _ = pair
    X = tgt.astype(np.float64)
    sq = (X * X).sum(1)
    D2 = sq[:, None] + sq[None, :] - 2.0 * (X @ X.T)
    np.fill_diagonal(D2, np.inf)
    spacing = float(np.sqrt(D2.min()))                                         # the lattice's smallest point spacing
    true = tgt[::3].astype(np.float64)
    src = I.displaced(true, I.LATTICE_MOTION)
    moved_by = np.linalg.norm(src - true, axis=1).max()
    print("smallest spacing", spacing, "largest displacement", moved_by)
    assert moved_by < 0.3 * spacing
    it = I.iteration(src, tgt, np.eye(4), I.RADIUS, "point_to_point")
    assert it["count"] == len(src)
    assert np.array_equal(I.correspondences(src, tgt, np.eye(4), I.RADIUS)[1], np.arange(0, len(tgt), 3))     # the true pairs at iteration 0
    M = I.update(it, "point_to_point")
    err = np.linalg.norm(I.moved(src, M) - true, axis=1).max()
    print("after one update", err)
    assert err <= 1e-6
    r = I.icp(src, tgt, I.RADIUS, estimation="point_to_point")
    print(r["status"], r["iterations"], r["log"])
    assert r["status"] == "converged" and r["fitness"] == 1.0 and np.linalg.norm(I.moved(src, r["T"]) - true, axis=1).max() <= 1e-6


def test_degenerate_input(pair):
    tgt, nrm, true = pair
    init = I.small_pose(0.001, 0.002, -0.001, 1e-4, 0.0, -1e-4)
    for est in ("point_to_plane", "point_to_point"):
        r = I.icp(true[:2].astype(f32), tgt, I.RADIUS, init=init, estimation=est, normals=nrm)
        assert r["status"] == "degenerate" and np.array_equal(r["T"], init) and r["iterations"] == 1 and r["log"][0][2] == 2
        r = I.icp(true.astype(f32) + f32(1.0), tgt, I.RADIUS, init=init, estimation=est, normals=nrm)
        assert r["status"] == "degenerate" and np.array_equal(r["T"], init) and r["fitness"] == 0.0 and r["rmse"] == 0.0 and r["log"] == [(0.0, 0.0, 0)]


def test_public_signatures(built):
    REG, EV, TS = built

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert params(REG.registration_icp) == [("source", E), ("target", E), ("max_correspondence_distance", E), ("init", None), ("estimation", "auto"),
                                            ("target_normals", None), ("max_iteration", 30), ("relative_fitness", 1e-6), ("relative_rmse", 1e-6),
                                            ("cell_size", None), ("device", 0)]
    assert params(REG.evaluate_registration) == [("source", E), ("target", E), ("max_correspondence_distance", E), ("transformation", None)]
    assert [f.name for f in __import__("dataclasses").fields(REG.RegistrationResult)] == ["transformation", "fitness", "inlier_rmse", "iterations",
                                                                                         "status", "log"]
    # the default path of the reconstruction evaluation is unchanged; the alignment is a function of its own with the same leading arguments
    assert params(EV.evaluate_reconstruction) == [("pred", E), ("gt", E), ("thresholds", (0.001, 0.002, 0.005)), ("transform", None),
                                                  ("max_distance", None)]
    assert params(EV.evaluate_reconstruction_aligned) == params(EV.evaluate_reconstruction) + [("align", "icp"), ("icp", None)]
    f = {f.name: f for f in __import__("dataclasses").fields(EV.ReconstructionMetrics)}
    assert f["alignment"].default is None and list(f)[-1] == "alignment"


def test_argument_validation_before_any_device_call(built, pair, monkeypatch):
    REG, EV, TS = built
    from bodyslam_amd import _lib
    tgt, nrm, true = pair
    src = true.astype(f32)

    def touched(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "init", touched)
    for radius in (0.0, -1.0, np.nan, np.inf, 1e-60, 1e60, "1", True, None):
        with pytest.raises(ValueError):
            REG.registration_icp(src, tgt, radius)
        with pytest.raises(ValueError):
            REG.evaluate_registration(src, tgt, radius)
        with pytest.raises(ValueError):
            EV.evaluate_reconstruction_aligned(src, tgt, icp=dict(max_correspondence_distance=radius))
    for init in (np.eye(3), np.zeros((3, 4)), np.full((4, 4), np.nan), "x", [1.0, 2.0]):
        with pytest.raises(ValueError):
            REG.registration_icp(src, tgt, 0.005, init=init)
        with pytest.raises(ValueError):
            REG.evaluate_registration(src, tgt, 0.005, transformation=init)
    with pytest.raises(ValueError):
        REG.registration_icp(src, tgt, 0.005, estimation="generalized")
    with pytest.raises(ValueError):
        REG.registration_icp(src, tgt, 0.005, estimation="point_to_plane")                    # no normals
    with pytest.raises(ValueError):
        REG.registration_icp(src, TS.PointCloud(tgt, np.zeros_like(tgt)), 0.005, estimation="point_to_plane")
    for bad in (nrm[:-1], nrm[:, :2], nrm.astype(np.int32), "n"):
        with pytest.raises(ValueError):
            REG.registration_icp(src, tgt, 0.005, target_normals=bad)
    for bad in (np.zeros((4, 2), f32), np.zeros((0, 3), f32), None):
        with pytest.raises(ValueError):
            REG.registration_icp(bad, tgt, 0.005)
        with pytest.raises(ValueError):
            REG.registration_icp(src, bad, 0.005)
    for kw in (dict(max_iteration=0), dict(max_iteration=2.5), dict(max_iteration=True), dict(relative_fitness=np.nan), dict(relative_rmse="a"),
               dict(cell_size=0.0)):
        with pytest.raises(ValueError):
            REG.registration_icp(src, tgt, 0.005, **kw)
    for align, icp in (("icp", None), ("icp", {}), ("icp", dict(radius=0.005)), ("icp", dict(max_correspondence_distance=0.005, scale=True)),
                       ("icp", dict(max_correspondence_distance=0.005, estimation="point_to_plane")), ("umeyama", dict(max_correspondence_distance=0.005)),
                       (None, dict(max_correspondence_distance=0.005)), ("icp", dict(max_correspondence_distance=0.005, init=np.eye(3)))):
        with pytest.raises(ValueError):
            EV.evaluate_reconstruction_aligned(src, tgt, align=align, icp=icp)


def test_no_cpu_fallback(built, pair):
    REG, EV, TS = built
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from bodyslam_amd._lib import BodySlamHipError
    tgt, nrm, true = pair
    src = true.astype(f32)
    with pytest.raises(BodySlamHipError):
        REG.registration_icp(src, tgt, 0.005, target_normals=nrm)
    with pytest.raises(BodySlamHipError):
        REG.registration_icp(src, TS.PointCloud(tgt, np.zeros_like(tgt), nrm), 0.005)
    with pytest.raises(BodySlamHipError):
        REG.evaluate_registration(src, tgt, 0.005)
    with pytest.raises(BodySlamHipError):
        EV.evaluate_reconstruction_aligned(src, tgt, icp=dict(max_correspondence_distance=0.005))
