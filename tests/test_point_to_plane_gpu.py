"""Frame-to-model tracking on the GPU (bodyslam_amd.rgbd_odometry.PointToPlaneOdometry, MAP.track_frame_to_model /
track_and_integrate; csrc/odometry.hip odo_p2p_*) against its numpy restatement tests/_point_to_plane_ref.py (itself held to analytic
truth by tests/test_point_to_plane_cpu.py), step by step and end to end, and through a MAP built on the analytic scene.

Bounds: one step's sums within 2e-5 relative (fp32 images summed in fp64, the hybrid odometry's bound); a full run within 5e-5 of
the restatement with inlier counts within max(2, 0.002 H W) (the caps tests/test_rgbd_odometry_gpu.py uses for nearest-pixel
association: a point within 1e-7 of a half-pixel boundary may round either way)."""
import os
import time

import numpy as np
import pytest

import _point_to_plane_ref as P2P
from conftest import TWO_PROC
from _render import render, small_pose
from _point_to_plane_ref import FULL, K_FULL, K_SMALL, MEDIUM, SMALL, pair

pytestmark = pytest.mark.gpu

H, W = 120, 160
K = K_SMALL
OUT = os.path.dirname(TWO_PROC["dir"])       # the suite's report directory (tests/conftest.py keeps the two-process run's files under it)


def record(name, line):
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, name), "a") as f:
        f.write(line + "\n")
    print(line)


def errors(T, truth):
    return np.abs(T[:3, 3] - truth[:3, 3]).max(), np.abs(T[:3, :3] - truth[:3, :3]).max()


def test_one_step_matches_the_restatement():
    """the sums of the first step at a start a hair off the identity (no projections exactly on the image border: the hybrid
    test's start), level and inlier count equal, A, b and cost within 2e-5 relative"""
    from bodyslam_amd.rgbd_odometry import PointToPlaneOdometry
    from oracle import rgbd_odometry_ref as R
    _, ds, dt = pair(MEDIUM, K, H, W, holes=True)
    init = R.se3_exp(np.array([3e-4, -2e-4, 1e-4, 2e-4, 1e-4, -1e-4]))
    odo = PointToPlaneOdometry(K)
    odo.estimate(ds, dt, 3.0, init=init, trace=True)
    ref = []
    P2P.point_to_plane(ds, dt, K, 3.0, init=init, trace=ref)
    g, r = odo.last_trace[0], ref[0]
    print(f"first step: level {g[0]} / {r[0]}, inliers {g[4]} / {r[4]}, |dA| / |A| = {np.abs(g[1] - r[1]).max() / np.abs(r[1]).max():.2e}, "
          f"|db| / |b| = {np.abs(g[2] - r[2]).max() / np.abs(r[2]).max():.2e}, |dcost| / cost = {abs(g[3] - r[3]) / r[3]:.2e}")
    assert g[0] == r[0] == 2 and g[4] == r[4]
    assert np.abs(g[1] - r[1]).max() <= 2e-5 * np.abs(r[1]).max() and np.abs(g[2] - r[2]).max() <= 2e-5 * np.abs(r[2]).max() + 1e-9
    assert abs(g[3] - r[3]) <= 2e-5 * r[3]


@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("motion", [SMALL, MEDIUM], ids=["small", "medium"])
def test_full_run_matches_restatement_and_truth(motion, holes):
    from bodyslam_amd.rgbd_odometry import PointToPlaneOdometry
    pose_s, ds, dt = pair(motion, K, H, W, holes=holes)
    odo = PointToPlaneOdometry(K)
    T = odo.estimate(ds, dt, 3.0, trace=True)
    ref = []
    T_ref = P2P.point_to_plane(ds, dt, K, 3.0, trace=ref)
    assert len(odo.last_trace) == len(ref) == 10
    worst = max(abs(a[4] - b[4]) for a, b in zip(odo.last_trace, ref))
    et, er = errors(T, pose_s)
    print(f"holes={holes}: largest inlier-count difference over the 10 steps {worst}; |T - T_restatement| = {np.abs(T - T_ref).max():.2e}; "
          f"against truth: translation {et:.2e} m, rotation {er:.2e}")
    assert worst <= max(2, int(0.002 * H * W))
    assert np.abs(T - T_ref).max() < 5e-5
    dev1 = odo.estimate(ds, dt, 3.0)                      # the device loop: solve and pose update in a kernel, one read-back
    assert np.abs(dev1 - T).max() < 1e-9 and odo.last_trace is None
    assert np.array_equal(odo.estimate(ds, dt, 3.0), dev1)             # fixed-order reduction: run-to-run identical


def test_batch_is_bit_equal_to_single_pairs():
    import torch
    from bodyslam_amd.rgbd_odometry import PointToPlaneOdometry
    cases = [pair(SMALL, K, H, W), pair(MEDIUM, K, H, W), pair(MEDIUM, K, H, W, holes=True), pair(FULL, K, H, W)]
    dev = torch.device("cuda:0")
    src = torch.stack([torch.from_numpy(c[1]) for c in cases]).to(dev)
    tgt = torch.stack([torch.from_numpy(c[2]) for c in cases]).to(dev)
    odo = PointToPlaneOdometry(K)
    single = [PointToPlaneOdometry(K).estimate(c[1], c[2], 3.0) for c in cases]        # (a tracker that never saw a batch)
    got = odo.estimate_batch(src, tgt)
    assert got.is_cuda and got.shape == (4, 12) and got.dtype == torch.float64
    for i, T in enumerate(single):
        assert np.array_equal(got[i].cpu().numpy().reshape(3, 4), T[:3]), i
        assert np.array_equal(odo.estimate(cases[i][1], cases[i][2], 3.0), T), i      # one pair in buffers sized for four
    part = odo.estimate_batch(src[1:], tgt[1:])           # a smaller batch in the same buffers
    assert torch.equal(part, got[1:])
    init = np.stack([small_pose(1e-3, 0, 0, 0, 1e-3, 0)] * 4)
    a, b = odo.estimate_batch(src, tgt, init=init), odo.estimate(cases[2][1], cases[2][2], 3.0, init=init[2])
    assert np.array_equal(a[2].cpu().numpy().reshape(3, 4), b[:3])
    assert odo.estimate_batch(src[:0], tgt[:0]).shape == (0, 12)


# ---- through the map -----------------------------------------------------------------------------------------------------------------
VOXEL = 0.001            # the scene sits at 0.3 m with +-5 cm relief: 1 mm voxels (the 5.8 mm default is too coarse for it)


def new_map():
    from bodyslam_amd.tsdf import MAP, PinholeCameraIntrinsic
    return MAP(W, H, PinholeCameraIntrinsic(W, H, *K), "cuda:0", 1000.0, voxel_size=VOXEL, block_count=16384)


def rgbd(P):
    from bodyslam_amd.tsdf import RGBDImage
    col, d = render(P, K, H, W)
    return RGBDImage(col, d)


def orbit(n=12, radius=0.012):
    """camera -> world poses on a circle in front of the scene, each turned a little towards its centre"""
    a = 2.0 * np.pi * np.arange(n) / n
    x, y = radius * (np.cos(a) - 1.0), radius * np.sin(a)
    return [small_pose(yi / 0.3 * 0.5, -xi / 0.3 * 0.5, 0.002 * i, xi, yi, 0.0) for i, (xi, yi) in enumerate(zip(x, y))]


def test_track_frame_to_model():
    m = new_map()
    poses = [small_pose(0.004 * i, -0.006 * i, 0.003 * i, 0.003 * i, -0.002 * i, 0.001 * i) for i in range(4)]
    with pytest.raises(RuntimeError, match="integrate"):
        m.track_frame_to_model(rgbd(poses[0]))
    for i in range(3):
        m.integrate(rgbd(poses[i]), i, poses[i])                       # at their TRUE poses
    frame = rgbd(poses[3])
    model_depth = m.raycast_frame.depth.cpu().numpy()
    res = m.track_frame_to_model(frame)
    ref = []
    T_ref = P2P.point_to_plane(frame.depth, model_depth, K, 3.0, trace=ref)
    truth = np.linalg.inv(poses[2]) @ poses[3]
    et, er = errors(res.transformation, truth)
    record("model_tracking.txt", f"one frame against a 3-frame map ({VOXEL * 1e3:.1f} mm voxels): translation error {et:.2e} m (untracked "
           f"{np.abs(truth[:3, 3]).max():.2e}), rotation error {er:.2e}; fitness {res.fitness:.3f} (restatement {ref[-1][4] / (H * W):.3f}), "
           f"model depth hit {np.mean(model_depth > 0):.3f}; |T - T_restatement| = {np.abs(res.transformation - T_ref).max():.2e}")
    assert np.abs(res.transformation - T_ref).max() < 5e-5
    assert ref[-1][4] / (H * W) >= 0.5 and res.fitness >= 0.5
    assert res.inliers == round(res.fitness * H * W) and res.cost >= 0.0
    assert et < np.abs(truth[:3, 3]).max()
    assert np.allclose(res.pose, poses[2] @ res.transformation, atol=1e-15) and m.last_tracking is res
    # integer depth follows integrate's convention: raw units / depth_scale.  (The frame rounded to millimetres: a per-pixel error of
    # at most 0.5 mm on the source points alone, averaged over ~19 000 of them -- far inside 1 mm; a frame read as raw units, a
    # thousand times too far, would find no inliers and return the identity, 3 mm away)
    from bodyslam_amd.tsdf import RGBDImage
    res_u16 = m.track_frame_to_model(RGBDImage(None, np.rint(frame.depth * 1000.0).astype(np.uint16)))
    assert np.abs(res_u16.transformation - res.transformation).max() < 1e-3


def test_track_and_integrate_sequence():
    """a 12-frame orbit with only frame 0's pose given: every frame is tracked against the map built so far and integrated at the
    tracked pose.  Recorded beside it: PointToPlaneOdometry chained frame to frame over the same frames."""
    import torch
    from bodyslam_amd.rgbd_odometry import PointToPlaneOdometry
    poses = orbit()
    frames = [rgbd(P) for P in poses]
    m = new_map()
    got = [m.track_and_integrate(frames[0], 0, init=poses[0])]
    assert np.array_equal(got[0], poses[0]) and m.last_tracking is None
    for i in range(1, len(poses)):
        model_depth = m.raycast_frame.depth.cpu().numpy()
        before = m.frame_poses[-1][1]
        got.append(m.track_and_integrate(frames[i], i))
        res = m.last_tracking
        assert np.array_equal(got[i], res.pose) and np.array_equal(m.frame_poses[-1][1], res.pose) and m.frame_poses[-1][0] == i
        assert np.allclose(res.pose, before @ res.transformation, atol=1e-15)
        T_ref = P2P.point_to_plane(frames[i].depth, model_depth, K, 3.0)
        d = np.abs(res.transformation - T_ref).max()
        et, er = errors(got[i], poses[i])
        record("model_tracking.txt", f"frame-to-model, frame {i:2d}: translation error {et:.2e} m, rotation error {er:.2e}, fitness {res.fitness:.3f}, "
               f"|T - T_restatement| = {d:.2e}")
        assert d < 5e-5 and res.fitness >= 0.5, i
    # the same frames chained frame to frame (no map): recorded, not asserted
    odo = PointToPlaneOdometry(K)
    dev = torch.device("cuda:0")
    deps = torch.stack([torch.from_numpy(f.depth) for f in frames]).to(dev)
    rel = odo.estimate_batch(deps[1:], deps[:-1]).cpu().numpy().reshape(-1, 3, 4)
    P = poses[0].copy()
    for i, r in enumerate(rel, 1):
        T = np.eye(4)
        T[:3] = r
        P = P @ T
        et, er = errors(P, poses[i])
        record("model_tracking.txt", f"frame-to-frame chain, frame {i:2d}: translation error {et:.2e} m, rotation error {er:.2e}")
    et, er = errors(got[-1], poses[-1])
    record("model_tracking.txt", f"final: frame-to-model {et:.2e} m / {er:.2e}; frame-to-frame chain {errors(P, poses[-1])[0]:.2e} m / {errors(P, poses[-1])[1]:.2e}")


def test_no_slower_than_the_hybrid_device_loop():
    """640x480, the reference's intrinsics: pyramids, target maps and the 10 steps of one pair (no ray cast) against the hybrid
    odometry's device loop (pyramids, gradients, 35 steps) on the same pair; both warmed, repeats alternating, medians of 25,
    every timing ends in a synchronise"""
    import torch
    from bodyslam_amd.rgbd_odometry import PointToPlaneOdometry, RGBDOdometry
    dev = torch.device("cuda:0")
    pose_s = small_pose(*FULL)
    ct, dt = render(np.eye(4), K_FULL, 480, 640)
    cs, ds = render(pose_s, K_FULL, 480, 640)
    cs_d, ds_d, ct_d, dt_d = (torch.from_numpy(a).to(dev) for a in (cs, ds, ct, dt))
    hyb, p2p = RGBDOdometry(K_FULL), PointToPlaneOdometry(K_FULL)

    def run_hybrid():
        T = hyb.estimate(cs_d, ds_d, ct_d, dt_d, 3.0)
        torch.cuda.synchronize()
        return T

    def run_p2p():
        T = p2p.estimate_batch(ds_d[None], dt_d[None])
        torch.cuda.synchronize()
        return T

    for _ in range(3):
        run_hybrid()
        run_p2p()
    t_h, t_p = [], []
    for _ in range(25):
        t0 = time.perf_counter()
        run_hybrid()
        t1 = time.perf_counter()
        T = run_p2p()
        t2 = time.perf_counter()
        t_h.append(t1 - t0)
        t_p.append(t2 - t1)
    ms_h, ms_p = np.median(t_h) * 1e3, np.median(t_p) * 1e3
    Tm = np.eye(4)
    Tm[:3] = T.cpu().numpy().reshape(3, 4)
    et, er = errors(Tm, pose_s)
    record("point_to_plane_timing.txt", f"640x480 pair: point-to-plane estimate_batch {ms_p:.3f} ms (10 steps), hybrid estimate device loop {ms_h:.3f} ms "
           f"(35 steps); point-to-plane against truth: {et:.2e} m / {er:.2e}")
    assert ms_p <= ms_h
