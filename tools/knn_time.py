"""Times the k nearest neighbours, the normal estimation and the statistical outlier removal on the extract_pcd cloud of the 256-frame
640x480 map that tools/map_correction_time.py builds (the reference's TSDF parameters): the k = 30 query of the cloud on itself
(bs_pc_query_knn), the normals kernel on its lists (bs_pc_normals), a whole estimate_normals call with its index build, a whole
remove_statistical_outlier call with nb_neighbors = 20, and beside them the k = 1 query (bs_pc_query_grid) of the cloud on itself as the
yardstick.  HIP events, one warm-up run, then the median of five.  Reported, not asserted: there is no earlier implementation and no target.

    python tools/knn_time.py [--out profiles/knn_time.txt]
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
from bodyslam_amd.tsdf import BATCH_MAX, TSDF, PinholeCameraIntrinsic  # noqa: E402
from reconstruction_eval_time import timed  # noqa: E402

K_NORMALS, NB_OUTLIER = 30, 20


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_time.txt"))
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
    cloud, map_normals = pcd.points.contiguous(), pcd.normals.contiguous()
    n = int(cloud.shape[0])
    del rgbds
    nn = PC.NearestNeighbours(cloud)
    lines = [f"k nearest neighbours on {torch.cuda.get_device_name(0)}: the extract_pcd cloud of {M.N} frames of {M.W}x{M.H} (TSDF 1 mm / 0.1 m / 32^3 / "
             f"stride 8), {n} points, queried on itself; grid {nn.dims[0]} x {nn.dims[1]} x {nn.dims[2]} cells of {nn.cell_size:.6g} m; HIP events, "
             f"median of 5 after a warm-up"]
    state = {}

    def yardstick():
        state["q"] = nn.query(cloud)

    ms = timed(yardstick)
    lines.append(f"bs_pc_query_grid, k = 1 (the yardstick) {ms * 1e3:9.1f} us with its 4-byte read-back ({nn.last_fallback} sources in the fallback; "
                 f"{n / ms / 1e3:8.1f} M points/s)")
    for k in (8, 16, K_NORMALS):
        def knn():
            state["knn"] = nn.query_knn(cloud, k)

        ms = timed(knn)
        cnt = state["knn"][2]
        lines.append(f"bs_pc_query_knn, k = {k:2d}                 {ms * 1e3:9.1f} us ({n / ms / 1e3:8.1f} M points/s; shortest list {int(cnt.min())})")
    index, d2, count = state["knn"]
    normals = torch.empty(n, 3, dtype=torch.float32, device=dev)

    def nrm():
        L.pc_normals(cloud, index, count, K_NORMALS, L.PC_ORIENT_AXIS, None, normals)

    ms = timed(nrm)
    cosang = (normals * map_normals).sum(1).abs()
    ok = (map_normals.abs().sum(1) > 0) & (normals.abs().sum(1) > 0)
    ang = torch.rad2deg(torch.acos(cosang[ok].clamp(max=1.0)))
    lines.append(f"bs_pc_normals on the k = {K_NORMALS} lists        {ms * 1e3:9.1f} us ({n / ms / 1e3:8.1f} M points/s; angle to the map's own normals: median "
                 f"{float(ang.median()):.2f} deg, 95th percentile {float(ang.kthvalue(int(0.95 * ang.numel()))[0]):.2f} deg over {int(ok.sum())} points)")

    def whole_normals():
        state["n"] = PC.estimate_normals(cloud, k=K_NORMALS)

    ms = timed(whole_normals)
    lines.append(f"estimate_normals(k = {K_NORMALS})               {ms:9.2f} ms with the index build (bounds read-back, count, scan, scatter), the query and the normals")

    def outliers():
        state["o"] = PC.remove_statistical_outlier(cloud, nb_neighbors=NB_OUTLIER, std_ratio=2.0)

    ms = timed(outliers)
    kept = int(state["o"][0].numel())
    lines.append(f"remove_statistical_outlier({NB_OUTLIER}, 2.0)      {ms:9.2f} ms with the index build, the k = {NB_OUTLIER} query, the mean distances, bs_pc_stats and "
                 f"its read-back, the mask and the compaction ({n - kept} of {n} points removed)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
