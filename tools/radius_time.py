"""Times the radius search, the radius outlier removal and DBSCAN on the extract_pcd cloud of the 256-frame 640x480 map that
tools/map_correction_time.py builds (the reference's TSDF parameters), queried on itself: the count, fill, sort and unpack launches
(bs_pc_radius_*) at radii of 1, 2, 4 and 8 voxel lengths on an index whose cell is the radius, a whole query_radius call, a whole
remove_radius_outlier call, and cluster_dbscan with its rounds (one hook launch and one compress launch timed alone as well).  Beside every
count launch: the hybrid query query_knn(k, radius) on the same index at k = 5, 17 and 32 -- for nb_points <= 31,
query_knn(nb_points + 1, radius).count > nb_points is remove_radius_outlier's mask, and that path existed before this one.  HIP events, one
warm-up run, then the median of five.  Reported, not asserted: there is no earlier implementation and no target.

    python tools/radius_time.py [--out profiles/radius_time.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_correction_time as M  # noqa: E402
from bodyslam_amd import _lib as L  # noqa: E402
from bodyslam_amd import pointcloud as PC  # noqa: E402
from bodyslam_amd.tsdf import BATCH_MAX, TSDF, PinholeCameraIntrinsic  # noqa: E402
from reconstruction_eval_time import timed  # noqa: E402

RADII = (1, 2, 4, 8)                    # in voxel lengths
KNN_K = (5, 17, 32)                     # nb_points + 1 for nb_points = 4, 16, 31
NB_POINTS = 16
DBSCAN = ((2, 4), (4, 10), (8, 10))     # (eps in voxel lengths, min_points)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radius_time.txt"))
    a = ap.parse_args()
    L.init(0)
    dev = torch.device("cuda", 0)
    intr = PinholeCameraIntrinsic(M.W, M.H, *M.K)
    rgbds, poses = M.sequence(dev)
    tsdf = TSDF()
    for j0 in range(0, M.N, BATCH_MAX):
        tsdf.build_3D_map_batch(rgbds[j0:j0 + BATCH_MAX], intr, poses[j0:j0 + BATCH_MAX])
    tsdf.sync()
    cloud = tsdf.extract_pcd(host=False).points.contiguous()
    n = int(cloud.shape[0])
    vl = float(tsdf.voxel_length)
    del rgbds
    lines = [f"radius search on {torch.cuda.get_device_name(0)}: the extract_pcd cloud of {M.N} frames of {M.W}x{M.H} (TSDF 1 mm / 0.1 m / 32^3 / "
             f"stride 8), {n} points, queried on itself; voxel length {vl:.6g} m; the index of a radius has cells of that radius; HIP events, "
             f"median of 5 after a warm-up"]
    state = {}
    for mult in RADII:
        r = mult * vl
        nn = PC.NearestNeighbours.for_radius(cloud, r)
        idx = nn._index()
        count = torch.empty(n, dtype=torch.int32, device=dev)

        def do_count():
            L.pc_radius_count(idx, cloud, r, count)

        ms_count = timed(do_count)
        row_start = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        row_start[1:] = torch.cumsum(count, 0, dtype=torch.int64)
        total = int(row_start[-1].cpu())
        lines.append(f"radius {mult:2d} voxel lengths = {r:.6g} m: grid {nn.dims[0]} x {nn.dims[1]} x {nn.dims[2]} cells of {nn.cell_size:.6g} m; "
                     f"{total} neighbours in all, {total / n:.1f} per point, at most {int(count.max())}")
        lines.append(f"  bs_pc_radius_count                    {ms_count * 1e3:9.1f} us ({n / ms_count / 1e3:8.1f} M points/s)")
        for k in KNN_K:
            def hybrid():
                state["knn"] = nn.query_knn(cloud, k, r)

            ms = timed(hybrid)
            same = bool(torch.equal(state["knn"][2] > k - 1, count > k - 1))
            lines.append(f"  bs_pc_query_knn(k = {k:2d}, radius)        {ms * 1e3:9.1f} us (count launch / hybrid = {ms_count / ms:.2f}; the mask for "
                         f"nb_points = {k - 1} is {'the same' if same else 'DIFFERENT'})")
        if total >= 2 ** 31:
            lines.append("  lists: not built, 2^31 neighbours or more")
            continue
        keys, ordered = torch.empty(total, dtype=torch.int64, device=dev), torch.empty(total, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        index, d2 = torch.empty(total, dtype=torch.int32, device=dev), torch.empty(total, dtype=torch.float32, device=dev)

        def do_fill():
            L.pc_radius_fill(idx, cloud, r, row_start, total, keys, status)

        def do_sort():
            L.pc_radius_sort(keys, row_start, ordered)

        def do_unpack():
            L.pc_radius_unpack(ordered, index, d2)

        def whole():
            state["q"] = nn.query_radius(cloud, r)

        ms_fill, ms_sort, ms_unpack, ms_whole = timed(do_fill), timed(do_sort), timed(do_unpack), timed(whole)
        assert int(status.cpu()) == 0
        long_rows = int((count > 64).sum())
        lines.append(f"  bs_pc_radius_fill                     {ms_fill * 1e3:9.1f} us ({total / ms_fill / 1e3:8.1f} M keys/s)")
        lines.append(f"  bs_pc_radius_sort                     {ms_sort * 1e3:9.1f} us ({total / ms_sort / 1e3:8.1f} M keys/s; {long_rows} rows of more than 64 keys "
                     f"go by rank counting)")
        lines.append(f"  bs_pc_radius_unpack                   {ms_unpack * 1e3:9.1f} us")
        lines.append(f"  query_radius (count, scan, read-back, fill, sort, unpack) {ms_whole:9.2f} ms")
        del keys, ordered, index, d2, state["q"]

    r = 4 * vl

    def outliers():
        state["o"] = PC.remove_radius_outlier(cloud, NB_POINTS, r)

    ms = timed(outliers)
    kept = int(state["o"][0].numel())
    lines.append(f"remove_radius_outlier({NB_POINTS}, {r:.6g})       {ms:9.2f} ms with the index build, the count launch, the mask and the compaction "
                 f"({n - kept} of {n} points removed)")
    for mult, mp in DBSCAN:
        eps = mult * vl

        def dbscan():
            state["l"] = PC.cluster_dbscan(cloud, eps, mp)

        ms = timed(dbscan)
        labels = state["l"]
        rounds, clusters = PC.last_rounds, PC.last_clusters
        nn = PC.NearestNeighbours.for_radius(cloud, eps)
        idx = nn._index()
        count = nn.count_radius(cloud, eps)
        parent = torch.arange(n, dtype=torch.int32, device=dev)
        changed = torch.zeros(1, dtype=torch.int32, device=dev)

        def hook():                                     # (after the first run the parents are final: the cost of a round that finds nothing to do)
            L.pc_dbscan_hook(idx, cloud, eps, count, mp, parent, changed)

        def compress():
            L.pc_dbscan_compress(parent)

        ms_hook, ms_compress = timed(hook), timed(compress)
        lines.append(f"cluster_dbscan(eps = {mult} voxel lengths = {eps:.6g} m, min_points = {mp}): {ms:9.2f} ms with the index build, the count launch, "
                     f"{rounds} rounds and their read-backs, the roots, the scan and the labels; {clusters} clusters, {int((labels < 0).sum())} noise "
                     f"points; a settled round alone: hook {ms_hook * 1e3:.1f} us + compress {ms_compress * 1e3:.1f} us")
    lines.append("where count launch / hybrid is above 1: the hybrid search ends its walk as soon as its k slots are full and the worst of them is below "
                 "the bound on everything unvisited; a count has to see every record of the cells that cover the radius")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
