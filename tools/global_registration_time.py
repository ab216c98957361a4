"""Times the global registration on the extract_pcd cloud of the 256-frame 640x480 map that tools/map_correction_time.py builds (the
reference's TSDF parameters) against a displaced copy of itself (50 degrees about (0.3, -0.5, 0.8), shifted by (0.11, -0.07, 0.2) m), with the
map's own normals: per stage on the clouds thinned at `voxel_size` -- the radius lists (query_radius at the feature radius, max_nn = 100),
the SPFH launch, the FPFH launch, the match launch (beside it, from the same run, torch.cdist + argmin on the same features), one RANSAC
chunk (hypotheses, compaction, score, winner, read-back) -- and the whole of registration_global with normal_sign "given" and "either".
HIP events, one warm-up run, then the median of five.  Reported, not asserted: there is no earlier implementation and no target.

    python tools/global_registration_time.py [--out profiles/global_registration_time.txt] [--voxels 4]
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


def pose():
    a = np.array([0.3, -0.5, 0.8])
    a /= np.linalg.norm(a)
    th = np.deg2rad(50.0)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)
    T[:3, 3] = (0.11, -0.07, 0.2)
    return T


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_registration_time.txt"))
    ap.add_argument("--voxels", type=float, default=4.0, help="voxel_size of the recipe in voxel lengths of the map")
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
    order = torch.argsort(pcd.points[:, 0] * 1e6 + pcd.points[:, 1] * 1e3 + pcd.points[:, 2])      # (the extraction's order differs from call to call)
    cloud, normals = pcd.points[order].contiguous(), pcd.normals[order].contiguous()
    n = int(cloud.shape[0])
    vl = float(tsdf.voxel_length)
    del rgbds
    T = pose()
    Ti = np.linalg.inv(T)
    Rm, t = torch.from_numpy(Ti[:3, :3]).to(dev), torch.from_numpy(Ti[:3, 3]).to(dev)
    moved = (cloud.double() @ Rm.T + t).float().contiguous()                   # registering `moved` onto `cloud` finds T
    moved_n = (normals.double() @ Rm.T).float().contiguous()
    h = a.voxels * vl
    fr, tau = 5.0 * h, 1.5 * h
    lines = [f"global registration on {torch.cuda.get_device_name(0)}: the extract_pcd cloud of {M.N} frames of {M.W}x{M.H} (TSDF 1 mm / 0.1 m / 32^3 / "
             f"stride 8), {n} points with the map's normals, against a copy moved by 50 degrees and 0.24 m; voxel_size {h:.6g} m, feature radius "
             f"{fr:.6g} m, max_correspondence_distance {tau:.6g} m; HIP events, median of 5 after a warm-up"]
    state = {}
    thin = {}
    for name, c, nr in (("source", moved, moved_n), ("target", cloud, normals)):
        def down():
            state["v"] = PC.voxel_down_sample(c, h, normals=nr, unit_normals=True)

        ms = timed(down)
        thin[name] = (state["v"].points, state["v"].normals)
        lines.append(f"{name}: voxel_down_sample {n} -> {int(state['v'].points.shape[0])} points {ms:9.2f} ms")
    feats = {}
    for name, (p, nr) in thin.items():
        m = int(p.shape[0])
        nn = PC.NearestNeighbours.for_radius(p, fr)

        def lists():
            state["l"] = nn.query_radius(p, fr, max_nn=100)

        ms_lists = timed(lists)
        rs, idx, d2 = state["l"]
        total = int(idx.numel())
        table = torch.zeros(m, 8, dtype=torch.float32, device=dev)
        table[:, 0:3], table[:, 4:7] = p, nr
        spfh = torch.zeros(m, L.FPFH_ROW, dtype=torch.int32, device=dev)
        f = torch.zeros(m, L.FPFH_DIM, dtype=torch.float32, device=dev)

        def do_spfh():
            L.fpfh_spfh(table, rs, idx, d2, 0, spfh)

        def do_fpfh():
            L.fpfh_features(spfh, rs, idx, d2, 0, f)

        def whole():
            state["f"] = REG.compute_fpfh_feature(p, nr, fr)

        ms_spfh, ms_fpfh, ms_whole = timed(do_spfh), timed(do_fpfh), timed(whole)
        same = bool(torch.equal(state["f"], f))
        feats[name] = state["f"]
        lines.append(f"{name}: {m} points, {total} list entries ({total / m:.1f} per point, max_nn = 100)")
        lines.append(f"  lists: query_radius(max_nn = 100)        {ms_lists:9.2f} ms")
        lines.append(f"  bs_fpfh_spfh                             {ms_spfh * 1e3:9.1f} us ({total / ms_spfh / 1e3:8.1f} M pairs/s)")
        lines.append(f"  bs_fpfh_features                         {ms_fpfh * 1e3:9.1f} us ({total / ms_fpfh / 1e3:8.1f} M entries/s)")
        lines.append(f"  compute_fpfh_feature (index, count, lists, both launches) {ms_whole:9.2f} ms (the same bits as the launches alone: {same})")
    fs, ft = feats["source"], feats["target"]
    m, k = int(fs.shape[0]), int(ft.shape[0])

    def match():
        state["m"] = REG._nearest_feature(fs, ft)

    def cdist():
        state["c"] = torch.cdist(fs, ft).argmin(1)

    def mutual():
        state["mm"] = REG.match_features(fs, ft, True)

    ms_match, ms_cdist, ms_mutual = timed(match), timed(cdist), timed(mutual)
    agree = float((state["m"] == state["c"]).float().mean())
    lines.append(f"match {m} x {k} rows of 33: bs_feature_match {ms_match * 1e3:9.1f} us ({m * k / ms_match / 1e6:8.2f} G row pairs/s); torch.cdist + argmin "
                 f"{ms_cdist * 1e3:9.1f} us on the same features ({100.0 * agree:.2f} % the same index: cdist's arithmetic is another one); match_features "
                 f"with the mutual filter {ms_mutual:9.2f} ms, {int(state['mm'].shape[0])} correspondences")
    corres = state["mm"]
    ps, pt = thin["source"][0], thin["target"][0]
    c = int(corres.shape[0])
    cr = corres.long()
    corr = torch.cat([ps.double()[cr[:, 0]], pt.double()[cr[:, 1]]], 1).contiguous()
    fits = torch.empty(REG.RANSAC_CHUNK * 12, dtype=torch.float64, device=dev)
    valid = torch.empty(REG.RANSAC_CHUNK, dtype=torch.int32, device=dev)
    score = torch.empty(REG.RANSAC_CHUNK, dtype=torch.int32, device=dev)
    best = torch.zeros(1, dtype=torch.int64, device=dev)

    def hyp():
        L.gr_hypotheses(corr, 0, 0, REG.RANSAC_CHUNK, 0.9, tau, fits, valid)

    ms_hyp = timed(hyp)
    lst = torch.nonzero(valid).reshape(-1).to(torch.int32)
    splits = max(1, min(-(-c // L.GR_BLOCK), -(-512 // -(-int(lst.numel()) // L.GR_BLOCK)), 65535))

    def do_score():
        score.zero_()
        L.gr_score(corr, fits, lst, REG.RANSAC_CHUNK, splits, tau, score)

    def chunk():
        hyp()
        score.zero_()
        ls = torch.nonzero(valid).reshape(-1).to(torch.int32)
        if ls.numel():
            L.gr_score(corr, fits, ls, REG.RANSAC_CHUNK, splits, tau, score)
            L.gr_winner(score, REG.RANSAC_CHUNK, 0, best)
        state["k"] = int(best.cpu())

    ms_score = timed(do_score) if lst.numel() else float("nan")
    ms_chunk = timed(chunk)
    lines.append(f"RANSAC over {c} correspondences, a chunk of {REG.RANSAC_CHUNK} hypotheses: bs_gr_hypotheses {ms_hyp * 1e3:9.1f} us, {int(lst.numel())} "
                 f"valid after the checkers; bs_gr_score {ms_score * 1e3:9.1f} us ({splits} splits); the whole chunk with compaction, winner and "
                 f"read-back {ms_chunk:9.2f} ms")
    for sign in ("given", "either"):
        def whole():
            state["r"] = REG.registration_global(moved, cloud, h, source_normals=moved_n, target_normals=normals, normal_sign=sign)

        ms = timed(whole)
        r = state["r"]
        err = float(np.linalg.norm((moved.double().cpu().numpy() @ r.transformation[:3, :3].T + r.transformation[:3, 3]) - cloud.double().cpu().numpy(),
                                   axis=1).max())
        lines.append(f"registration_global(normal_sign = {sign!r}): {ms:9.2f} ms; {r.status}, {r.hypotheses} hypotheses, h = {r.h}, {r.inliers} inliers of "
                     f"{int(r.correspondences.shape[0])}, rmse {r.inlier_rmse:.3e} m; the farthest point lands {err:.3e} m from its true place")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
