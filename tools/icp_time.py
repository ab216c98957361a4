"""Times the rigid ICP registration on the extract_pcd cloud of the 256-frame 640x480 map that tools/map_correction_time.py builds (the
reference's TSDF parameters; its normals are the map's) against a copy displaced by a small rigid motion: one iteration of the fused
step (bs_icp_step + bs_icp_finish, point-to-plane and point-to-point), next to it bs_pc_transform + bs_pc_query_grid alone on the same
inputs -- the kernels that were there before doing the correspondence part only, a floor for any composition of existing calls, which
would add the sums, a host round trip and the solve --, and a whole registration_icp call with its index build and read-backs.  HIP
events, one warm-up run, then the median of five.  Reported, not asserted: there is no earlier implementation and no target.

    python tools/icp_time.py [--out profiles/icp_time.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_correction_time as M  # noqa: E402
from bodyslam_amd import _lib as L  # noqa: E402
from bodyslam_amd import pointcloud as PC  # noqa: E402
from bodyslam_amd import registration as REG  # noqa: E402
from bodyslam_amd.tsdf import BATCH_MAX, TSDF, PinholeCameraIntrinsic  # noqa: E402
from reconstruction_eval_time import timed  # noqa: E402

RADIUS = 0.005
MOTION = (0.004, -0.003, 0.005, 0.0008, -0.0006, 0.0004)            # rotations (rad) about x, y, z and a translation (m)
ITERATIONS = 16                                                    # per timed run of the fused step


def small_pose(rx, ry, rz, tx, ty, tz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rz @ Ry @ Rx, (tx, ty, tz)
    return T


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_time.txt"))
    a = ap.parse_args()
    L.init(0)
    dev = torch.device("cuda", 0)
    intr = PinholeCameraIntrinsic(M.W, M.H, *M.K)
    rgbds, poses = M.sequence(dev)
    tsdf = TSDF()
    for j0 in range(0, M.N, BATCH_MAX):
        tsdf.build_3D_map_batch(rgbds[j0:j0 + BATCH_MAX], intr, poses[j0:j0 + BATCH_MAX])
    tsdf.sync()
    pcd = tsdf.extract_pcd(host=False)
    target, normals = pcd.points.contiguous(), pcd.normals.contiguous()
    n = int(target.shape[0])
    del rgbds
    # the source: the cloud moved about its centroid by the inverse of MOTION, so that the registration finds MOTION about that point
    centre = target.mean(0).cpu().numpy().astype(np.float64)
    C, Ci = np.eye(4), np.eye(4)
    C[:3, 3], Ci[:3, 3] = centre, -centre
    truth = C @ small_pose(*MOTION) @ Ci
    source = PC.transform_points(target, np.linalg.inv(truth))
    nn = PC.NearestNeighbours(target)
    lines = [f"Rigid ICP on {torch.cuda.get_device_name(0)}: the extract_pcd cloud of {M.N} frames of {M.W}x{M.H} (TSDF 1 mm / 0.1 m / 32^3 / stride 8), "
             f"{n} points with the map's normals, against a copy displaced by {MOTION}; radius {RADIUS} m; grid {nn.dims[0]} x {nn.dims[1]} x "
             f"{nn.dims[2]} cells of {nn.cell_size:.6g} m; HIP events, median of 5 after a warm-up"]
    for name, est, nrm in (("point-to-plane", L.ICP_POINT_TO_PLANE, normals), ("point-to-point", L.ICP_POINT_TO_POINT, None)):
        crit = (ITERATIONS, 0.0, 0.0)                              # never "converged": every launch of a run does its work
        run = REG._Run(source, None, nn, nrm, float(np.float32(RADIUS)), est, None, 0, np.eye(4), *crit)
        fresh = run.state.clone()

        def iterate():
            run.state.copy_(fresh)
            for _ in range(ITERATIONS):
                run.launch(L.ICP_ITERATE)

        ms = timed(iterate)
        host = run.read()
        its = int(host[1])
        log = host[L.ICP_STATE_FIELDS:L.ICP_STATE_FIELDS + L.ICP_LOG_FIELDS * its].reshape(its, -1)
        err = np.abs(REG._Run.transformation(host) - truth).max()
        lines.append(f"fused step, {name:15s} {ms / ITERATIONS * 1e3:9.1f} us per iteration ({ITERATIONS} iterations enqueued back to back, {ms:.3f} ms; "
                     f"{n / (ms / ITERATIONS) / 1e3:8.1f} M source points/s; status {REG.STATUS[int(host[0])]}, fitness {log[0, 0]:.4f} -> {log[-1, 0]:.4f}, "
                     f"rmse {log[0, 1]:.3e} -> {log[-1, 1]:.3e} m, largest |T - truth| {err:.2e})")
    moved = torch.empty(n, 3, dtype=torch.float32, device=dev)
    state = {}

    def floor():
        L.pc_transform(source, np.eye(4)[:3], moved)
        state["d"], state["i"] = nn.query(moved, max_distance=RADIUS)

    ms = timed(floor)
    lines.append(f"bs_pc_transform + bs_pc_query_grid   {ms * 1e3:9.1f} us (the correspondence part only, with the query's 4-byte read-back; "
                 f"{nn.last_fallback} sources in the fallback)")
    for name, kw in (("point-to-plane", dict(target_normals=normals)), ("point-to-point", dict(estimation="point_to_point"))):
        def whole():
            state["r"] = REG.registration_icp(source, target, RADIUS, **kw)

        ms = timed(whole)
        r = state["r"]
        lines.append(f"registration_icp, {name:15s} {ms:9.2f} ms with the index build and the read-backs ({r.status} after {r.iterations} iterations, chunks of "
                     f"{REG.CHUNK}; fitness {r.fitness:.4f}, rmse {r.inlier_rmse:.3e} m, largest |T - truth| {np.abs(r.transformation - truth).max():.2e})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
