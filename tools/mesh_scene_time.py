"""Times the triangle-mesh scene on the extract_mesh() mesh of the 256-frame 640x480 map that tools/map_correction_time.py builds (the
reference's TSDF parameters): the scene build with its index (bs_mesh_records, bs_mesh_grid_count, the scan, bs_mesh_grid_scatter), a
640x480 cast_rays through the grid beside brute force on every 64th ray, compute_distance of the map's own cloud beside the k = 1 point
query of the same points on the mesh's vertices (bs_pc_query_grid, the yardstick), and sample_points_uniformly of 2^18 points.  HIP
events, one warm-up run, then the median of five.  Reported, not asserted: there is no earlier implementation and no target.

    python tools/mesh_scene_time.py [--out profiles/mesh_scene_time.txt]
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
from bodyslam_amd.raycasting import RaycastingScene  # noqa: E402
from bodyslam_amd.tsdf import BATCH_MAX, TSDF, PinholeCameraIntrinsic  # noqa: E402
from reconstruction_eval_time import timed  # noqa: E402

EVERY, N_SAMPLES = 64, 1 << 18


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_scene_time.txt"))
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
    mesh = tsdf.extract_mesh()
    del rgbds
    vertices, triangles = torch.as_tensor(mesh.vertices).to(dev), torch.as_tensor(mesh.triangles).to(dev)
    T = int(triangles.shape[0])
    lines = [f"triangle-mesh scene on {torch.cuda.get_device_name(0)}: the extract_mesh() mesh of {M.N} frames of {M.W}x{M.H} (TSDF 1 mm / 0.1 m / 32^3 / "
             f"stride 8), {int(vertices.shape[0])} vertices, {T} triangles; HIP events, median of 5 after a warm-up"]
    state = {}

    def build():
        s = RaycastingScene()
        s.add_triangles(vertices, triangles)
        s._build()
        state["scene"] = s

    ms = timed(build)
    scene = state["scene"]
    lines.append(f"scene build (index check, records, bounds, count, scan, scatter, read-backs)   {ms:9.3f} ms ({scene.n_kept} of {T} triangles kept; grid "
                 f"{scene.dims[0]} x {scene.dims[1]} x {scene.dims[2]} cells of {scene.cell_size:.6g} m, {scene.n_references} references)")
    K = np.array([[M.K[0], 0, M.K[2]], [0, M.K[1], M.K[3]], [0, 0, 1.0]])
    rays = RaycastingScene.create_rays_pinhole(K, poses[M.N // 2], M.W, M.H).reshape(-1, 6).contiguous().to(dev)      # (world -> camera)
    part = rays[::EVERY].contiguous()

    def cast():
        state["cast"] = scene.cast_rays(rays)

    ms = timed(cast)
    hits = int(torch.isfinite(state["cast"]["t_hit"]).sum())
    lines.append(f"cast_rays, grid, a {M.W}x{M.H} view ({rays.shape[0]} rays)  {ms:9.3f} ms ({hits} hits, {scene.last_fallback} rays in the fallback)")

    def cast_brute():
        state["brute"] = scene.cast_rays(part, method="brute")

    ms = timed(cast_brute)
    same = all(torch.equal(state["brute"][k], state["cast"][k][::EVERY]) for k in state["brute"])
    lines.append(f"cast_rays, brute force, every {EVERY}th of those rays ({part.shape[0]} rays)  {ms:9.3f} ms ({part.shape[0] * T / ms / 1e6:8.1f} G ray-triangle "
                 f"tests/s; the same bits as the grid: {same})")
    q = cloud

    def dist():
        state["d"] = scene.compute_distance(q)

    ms = timed(dist)
    d = state["d"]
    lines.append(f"compute_distance, grid, the map's cloud ({q.shape[0]} points)  {ms:9.3f} ms (median distance {float(d.median()):.3g} m, "
                 f"{scene.last_fallback} points in the fallback)")
    nn = PC.NearestNeighbours(vertices)

    def yardstick():
        state["q"] = nn.query(q)

    ms = timed(yardstick)
    lines.append(f"bs_pc_query_grid, k = 1, the same points on the mesh's vertices (the yardstick)  {ms * 1e3:9.1f} us (median distance "
                 f"{float(state['q'][0].median()):.3g} m)")

    def sample():
        state["s"] = PC.sample_mesh(vertices, triangles, N_SAMPLES, vertex_colors=torch.as_tensor(mesh.vertex_colors).to(dev), seed=0)

    ms = timed(sample)
    lines.append(f"sample_mesh, 2^18 points with colours            {ms:9.3f} ms with the index check, bs_mesh_records, the weights, the scan and its read-back "
                 f"({N_SAMPLES / ms / 1e3:8.1f} M samples/s)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
