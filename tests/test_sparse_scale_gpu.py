"""The sparse-feature scale path on the device (bs_orb_* through bodyslam_amd.scaling_system): every stage against the numpy statement
tests/_orb_ref.py BIT FOR BIT, the block form against the pair form, rendered ground truth, a textureless frame, and the VO step.

The scene is tests/_corner_scene.py at 200 x 152: no multiple of any tile, more candidates at level 0 than the cut takes, levels 5-7
without an interior (tests/test_sparse_scale_cpu.py asserts these).  The statement of every frame is computed once per module."""
import types

import numpy as np
import pytest

import _corner_scene as S
import _orb_ref as R
from _orb_cases import level_view
from oracle.ukf_ref import LinearKF

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from bodyslam_amd import orb_tables as T  # noqa: E402
from bodyslam_amd import scaling_system as SS  # noqa: E402
from bodyslam_amd.visual_odometry import VO  # noqa: E402


def rgbd(frame):
    return types.SimpleNamespace(color=frame[0], depth=frame[1])


@pytest.fixture(scope="module")
def plane():
    """the plane pair: frames, the statement of both frames and of the pair, the device's stages of the pair call"""
    prev, curr, motion = S.pair("plane")
    f = [R.extract(prev[0]), R.extract(curr[0])]
    m = R.match(f[0]["desc"], f[1]["desc"])
    ref = {a: R.displacement(f[0]["pt"], f[1]["pt"], m, prev[1], curr[1], S.K, a) for a in ("reference", "matched")}
    eng = SS.SparseScale(S.K)
    out = eng(rgbd(curr), rgbd(prev))
    st = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in eng.last_stages.items()}
    return dict(prev=prev, curr=curr, motion=motion, f=f, m=m, ref=ref, out=out, counts=eng.last_counts.copy(), st=st)


# ---- stage outputs, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", ["grey", "smooth", "score"])
def test_image_stages_bit_equal(plane, stage):
    for frame in (0, 1):
        for l in range(T.N_LEVELS):
            got, want = level_view(plane["st"], stage, frame, l), plane["f"][frame][stage][l]
            assert got.shape == want.shape and np.array_equal(got, want), (stage, frame, l, int((got != want).sum()))


def test_selected_keypoints_position_and_order(plane):
    for frame in (0, 1):
        want, st = plane["f"][frame], plane["st"]
        n = int(want["counts"].sum())
        assert list(st["counts"][frame]) == list(want["counts"]) + [n]
        assert want["counts"][0] == T.features_per_level()[0] and want["counts"][7] == 0
        assert np.array_equal(st["kp"][frame, :n, :4], want["kp"][:, :4])                  # level, x, y, FAST score -- in order


def test_harris_response_bit_patterns(plane):
    for frame in (0, 1):
        want = plane["f"][frame]["resp"]
        assert np.array_equal(plane["st"]["resp"][frame, :len(want)].view(np.uint64), want.view(np.uint64))


def test_moments_and_bins(plane):
    for frame in (0, 1):
        want = plane["f"][frame]["kp"]
        assert np.array_equal(plane["st"]["kp"][frame, :len(want), 4:7], want[:, 4:7])
        assert len(np.unique(want[:, 6])) > 8                                              # the bins are exercised
        got_pt = plane["st"]["pt"][frame, :len(want)]
        assert np.array_equal(got_pt.view(np.uint32), plane["f"][frame]["pt"].view(np.uint32))


def test_descriptors_bit_equal(plane):
    for frame in (0, 1):
        want = plane["f"][frame]["desc"]
        assert np.array_equal(plane["st"]["desc"][frame, :len(want)].view(np.uint32), want)


def test_match_list_with_distances(plane):
    m, st = plane["m"], plane["st"]
    assert len(m) > 100 and int(st["match_counts"][0]) == len(m)
    assert np.array_equal(st["matches"][0, :len(m), :3], m)
    assert np.any(np.diff(m[:, 2]) == 0)                                                  # equal distances: the stable order is exercised


@pytest.mark.parametrize("association", ["reference", "matched"])
def test_displacement_and_counters(plane, association):
    eng = SS.SparseScale(S.K, association=association)
    got = eng(rgbd(plane["curr"]), rgbd(plane["prev"]))
    want, counts = plane["ref"][association]
    print(association, "device", got, "statement", want, "counts", eng.last_counts[0], counts)
    assert list(eng.last_counts[0]) == list(counts)
    assert got.dtype == np.float64 and np.max(np.abs(got - want)) <= 1e-12
    if association == "reference":
        assert counts[4] < counts[3]                                                      # the swapped index ran past a list: the zip misaligns


# ---- block form -------------------------------------------------------------------------------------------------------------------------
def test_block_of_three_frames_is_bit_equal_to_the_pair_calls(plane):
    third = S.render(S.translation_pose(2.0 * S.PLANE_T), "plane")
    frames = [plane["prev"], plane["curr"], third]
    for association in ("reference", "matched"):
        eng = SS.SparseScale(S.K, association=association)
        block = eng.displacements_block(np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]))
        block_counts = eng.last_counts.copy()
        assert block.shape == (2, 3)
        for p in range(2):
            one = eng(rgbd(frames[p + 1]), rgbd(frames[p]))
            assert np.array_equal(block[p].view(np.uint64), one.view(np.uint64)), (association, p, block[p], one)
            assert np.array_equal(block_counts[p], eng.last_counts[0])
    assert np.max(np.abs(block[0] - plane["ref"]["matched"][0])) <= 1e-12


# ---- rendered ground truth ----------------------------------------------------------------------------------------------------------------
# The numpy statement's error against the rendered motion, measured on the CPU (|mean displacement - motion|, metres):
#   plane, translation (12.5, -6.7, 0) mm, |motion| = 14.18 mm:       reference 7.985915e-04    matched 7.631555e-04
#   height field, translation (18.5, -9.7, 4) mm, |motion| = 21.27 mm:                          matched 1.400528e-03
# (the error is that of the mean over ~225 matches of which a handful are wrong; a wrong match is off by centimetres.)  The device
# differs from the statement in nothing, so twice the measured value only covers the statement's own scatter between the scenes.  The
# motions are 17.8, 18.6 and 15.2 times the measured errors: a result of "no motion" misses the bound by far.
MEASURED = {("plane", "reference"): 7.985915e-04, ("plane", "matched"): 7.631555e-04, ("field", "matched"): 1.400528e-03}


@pytest.mark.parametrize("surface,association", sorted(MEASURED))
def test_rendered_translation_is_recovered(surface, association):
    """plane: both association modes (depth is constant, so the reference's swapped index reads the same depth); height field: the
    matched mode.  The numpy statement's error against the rendered motion, measured on the CPU, in metres: plane reference 7.985915e-04,
    plane matched 7.631555e-04 (motion 1.418e-02), height field matched 1.400528e-03 (motion 2.127e-02).  Bound: twice that value."""
    prev, curr, motion = S.pair(surface)
    eng = SS.SparseScale(S.K, association=association)
    got = eng(rgbd(curr), rgbd(prev))
    err, bound = float(np.linalg.norm(got - motion)), 2.0 * MEASURED[(surface, association)]
    print(surface, association, "device", got, "motion", motion, "error", err, "bound", bound, "counts", eng.last_counts[0])
    assert np.linalg.norm(motion) >= 10.0 * MEASURED[(surface, association)]
    assert err <= bound


# ---- a textureless frame ------------------------------------------------------------------------------------------------------------------
class FakeMPEM:
    def infer_relative_pose_between(self, a, b):
        M = np.eye(4, dtype=np.float32)
        M[:3, :3] = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dtype=np.float32)
        M[:3, 3] = (9.0, 9.0, 9.0)                  # a translation the fusion must NOT use
        return M


def test_textureless_frame(plane):
    blank = S.blank()
    eng = SS.SparseScale(S.K)
    out = eng(rgbd(blank), rgbd(plane["prev"]))
    assert np.all(np.isnan(out)) and list(eng.last_counts[0]) == [int(plane["f"][0]["counts"].sum()), 0, 0, 0, 0, 0]
    kps, desc = SS.extract_features_orb(blank[0][..., ::-1])
    assert kps == [] and desc is None and SS.match_features_orb(desc, desc) == []
    sf = SS.compute_scaling_factor(blank[0], plane["prev"][0][..., ::-1], blank[1], plane["prev"][1], S.K)
    assert sf.shape == (3,) and np.all(np.isnan(sf))
    vo = VO(FakeMPEM(), intrinsic=S.K)
    vo.estimate_relative_pose_between("f0", "f1", rgbd(plane["prev"]), rgbd(plane["curr"]), 1, rgbd_odo=False)
    x, P = vo.ukf.x.copy(), vo.ukf.P.copy()
    with pytest.raises(RuntimeError, match="frame 2"):
        vo.estimate_relative_pose_between("f1", "f2", rgbd(plane["curr"]), rgbd(blank), 2, rgbd_odo=False)
    assert np.array_equal(vo.ukf.x, x) and np.array_equal(vo.ukf.P, P)


# ---- VO -----------------------------------------------------------------------------------------------------------------------------------
def test_vo_sparse_step_uses_mpem_rotation_and_filtered_displacement(plane):
    want = plane["ref"]["reference"][0]
    vo = VO(FakeMPEM(), intrinsic=S.K)
    kf = LinearKF()
    for i in range(1, 6):
        M = vo.estimate_relative_pose_between(f"f{i - 1}", f"f{i}", rgbd(plane["prev"]), rgbd(plane["curr"]), i, rgbd_odo=False)
        kf.predict()
        kf.update(want)
        assert np.allclose(M[:3, :3], [[0, -1, 0], [1, 0, 0], [0, 0, 1]])
        assert np.allclose(M[:3, 3], kf.x, atol=1e-6) and not np.allclose(M[:3, 3], 9.0)
    assert isinstance(vo.sparse_scale, SS.SparseScale)
    # an object with cv2_color / cv2_depth is read through those (BGR, as the reference's frames carry it)
    cv = types.SimpleNamespace(cv2_color=plane["curr"][0][..., ::-1], cv2_depth=plane["curr"][1], color=None, depth=None)
    assert np.array_equal(vo.sparse_scale(cv, rgbd(plane["prev"])), plane["out"])


# ---- the reference module's functions --------------------------------------------------------------------------------------------------------
def test_drop_in_functions_compose_to_compute_scaling_factor(plane):
    prev, curr = plane["prev"], plane["curr"]
    bgr = lambda c: np.ascontiguousarray(c[..., ::-1])
    k1, d1 = SS.extract_features_orb(bgr(prev[0]))
    k2, d2 = SS.extract_features_orb(bgr(curr[0]))
    assert d1.dtype == np.uint8 and d1.shape == (len(k1), 32) and np.array_equal(d1.view(np.uint32), plane["f"][0]["desc"])
    assert np.array_equal(np.array([k.pt for k in k2], dtype=np.float32), plane["f"][1]["pt"])
    ms = SS.match_features_orb(d1, d2)
    assert [(m.queryIdx, m.trainIdx, int(m.distance)) for m in ms] == [tuple(r) for r in plane["m"]]
    a = SS.associate_depth(k1, k2, ms, prev[1])
    b = SS.associate_depth(k2, k1, ms, curr[1])
    disp = SS.calculate_displacements(k1, k2, a, b, *S.K)
    want, counts = plane["ref"]["reference"]
    assert (len(a), len(b), len(disp)) == tuple(counts[3:])
    assert np.max(np.abs(np.mean(disp, axis=0) - want)) <= 1e-9          # (depth fp32 promoted on the host here; one call per pair list)
    sf = SS.compute_scaling_factor(bgr(curr[0]), bgr(prev[0]), curr[1], prev[1], S.K)
    assert np.array_equal(sf.view(np.uint64), plane["out"].view(np.uint64))
