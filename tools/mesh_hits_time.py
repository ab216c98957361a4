"""Times the counting queries of the triangle-mesh scene on the extract_mesh() mesh of the 256-frame 640x480 map that
tools/map_correction_time.py builds (the scene of tools/mesh_scene_time.py): a 640x480 view's count_intersections, test_occlusions and
list_intersections beside cast_rays of the same rays, and compute_occupancy and compute_signed_distance of the map's own cloud beside
compute_distance of the same points.  HIP events, one warm-up run, then the median of five.  Reported, not asserted: there is no earlier
implementation and no target.  (The mesh of a TSDF map is open: the side it reports says nothing; the time does.)

    python tools/mesh_hits_time.py [--out profiles/mesh_hits_time.txt]
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
from bodyslam_amd.raycasting import RaycastingScene  # noqa: E402
from bodyslam_amd.tsdf import BATCH_MAX, TSDF, PinholeCameraIntrinsic  # noqa: E402
from reconstruction_eval_time import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_hits_time.txt"))
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
    scene = RaycastingScene()
    scene.add_triangles(vertices, triangles)
    scene._build()
    lines = [f"counting queries of the triangle-mesh scene on {torch.cuda.get_device_name(0)}: the extract_mesh() mesh of {M.N} frames of {M.W}x{M.H}, "
             f"{int(vertices.shape[0])} vertices, {T} triangles; grid {scene.dims[0]} x {scene.dims[1]} x {scene.dims[2]} cells of {scene.cell_size:.6g} m, "
             f"{scene.n_references} references; HIP events, median of 5 after a warm-up"]
    K = np.array([[M.K[0], 0, M.K[2]], [0, M.K[1], M.K[3]], [0, 0, 1.0]])
    rays = RaycastingScene.create_rays_pinhole(K, poses[M.N // 2], M.W, M.H).reshape(-1, 6).contiguous().to(dev)      # (world -> camera)
    state = {}

    def run(name, fn):
        def once():
            state[name] = fn()
        return timed(once)

    n = int(rays.shape[0])
    ms = run("cast", lambda: scene.cast_rays(rays))
    hits = torch.isfinite(state["cast"]["t_hit"])
    lines.append(f"cast_rays, grid, a {M.W}x{M.H} view ({n} rays)            {ms:9.3f} ms ({int(hits.sum())} hits; the yardstick of the three below)")
    ms = run("occ", lambda: scene.test_occlusions(rays))
    lines.append(f"test_occlusions, grid, the same rays                      {ms:9.3f} ms (equal to isfinite(t_hit): {torch.equal(state['occ'], hits)})")
    ms = run("count", lambda: scene.count_intersections(rays))
    c = state["count"]
    lines.append(f"count_intersections, grid, the same rays                  {ms:9.3f} ms ({int(c.sum())} hits, at most {int(c.max())} on a ray, "
                 f"{scene.last_fallback} rays in the fallback)")
    ms = run("list", lambda: scene.list_intersections(rays))
    ls = state["list"]
    lines.append(f"list_intersections, grid, the same rays                   {ms:9.3f} ms (count, scan, fill, sort, unpack; {int(ls['t_hit'].numel())} rows; "
                 f"diff(ray_splits) == count: {torch.equal(torch.diff(ls['ray_splits']), c.long())})")
    q = cloud
    ms = run("d", lambda: scene.compute_distance(q))
    lines.append(f"compute_distance, grid, the map's cloud ({q.shape[0]} points)  {ms:9.3f} ms (the yardstick of the two below)")
    for k in (1, 3):
        ms = run("o", lambda: scene.compute_occupancy(q, nsamples=k))
        lines.append(f"compute_occupancy, nsamples {k}, the same points             {ms:9.3f} ms ({float(state['o'].mean()):.3f} of them inside: the map's mesh is open)")
    ms = run("sd", lambda: scene.compute_signed_distance(q))
    lines.append(f"compute_signed_distance, nsamples 1, the same points       {ms:9.3f} ms (|.| has compute_distance's bits: "
                 f"{torch.equal(state['sd'].abs().view(torch.int32), state['d'].abs().view(torch.int32))})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
