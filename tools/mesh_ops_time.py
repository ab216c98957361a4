"""Times the mesh clean-up on the extract_mesh(host=False) mesh of the 256-frame 640x480 map that tools/map_correction_time.py builds (the
reference's TSDF parameters): the edge table, the connected components with their rounds, a whole remove_small_components, the vertex
normals and ten Taubin iterations; then the components again with the triangle rows randomly permuted, the hard case for the hooking
rounds.  Beside the components, what a user composes from torch today in the same run: torch.unique of the edge keys, the first triangle of
every edge by scatter_reduce, and minimum-label propagation with pointer jumping until nothing changes -- the same labels.  HIP events, one
warm-up run, then the median of five.  Reported, not asserted: there is no earlier implementation and no target.

    python tools/mesh_ops_time.py [--out profiles/mesh_ops_time.txt]
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
from bodyslam_amd import mesh as MO  # noqa: E402
from bodyslam_amd.tsdf import BATCH_MAX, TSDF, PinholeCameraIntrinsic, TriangleMesh  # noqa: E402
from reconstruction_eval_time import timed  # noqa: E402

TAUBIN = 10


def torch_labels(triangles):
    """the smallest triangle index of every triangle's edge-connected component, from torch alone -> (labels int64 [T], rounds)"""
    t = triangles.to(torch.int64)
    T = t.shape[0]
    a, b = t.reshape(-1), t[:, [1, 2, 0]].reshape(-1)
    key = (torch.minimum(a, b) << 32) | torch.maximum(a, b)
    uniq, inverse = torch.unique(key, return_inverse=True)
    tri = torch.arange(3 * T, device=t.device) // 3
    first = torch.full((uniq.numel(),), T, dtype=torch.int64, device=t.device).scatter_reduce_(0, inverse, tri, reduce="amin")
    other = first[inverse]
    label = torch.arange(T, device=t.device)
    rounds = 0
    while True:
        rounds += 1
        m = torch.minimum(label[tri], label[other])
        new = label.clone().scatter_reduce_(0, tri, m, reduce="amin").scatter_reduce_(0, other, m, reduce="amin")
        new = new[new]                                             # pointer jumping
        if torch.equal(new, label):
            return label, rounds
        label = new


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_ops_time.txt"))
    a = ap.parse_args()
    L.init(0)
    dev = torch.device("cuda", 0)
    intr = PinholeCameraIntrinsic(M.W, M.H, *M.K)
    rgbds, poses = M.sequence(dev)
    tsdf = TSDF()
    for j0 in range(0, M.N, BATCH_MAX):
        tsdf.build_3D_map_batch(rgbds[j0:j0 + BATCH_MAX], intr, poses[j0:j0 + BATCH_MAX])
    tsdf.sync()
    mesh = tsdf.extract_mesh(host=False)
    del rgbds, tsdf
    v, t = mesh.vertices.contiguous(), mesh.triangles.contiguous()
    V, T = int(v.shape[0]), int(t.shape[0])
    lines = [f"mesh clean-up on {torch.cuda.get_device_name(0)}: the extract_mesh(host=False) mesh of {M.N} frames of {M.W}x{M.H} (TSDF 1 mm / 0.1 m / 32^3 / "
             f"stride 8), {V} vertices, {T} triangles; HIP events, median of 5 after a warm-up"]
    state = {}

    def edges():
        state["e"] = MO.edge_topology(v, t)

    ms = timed(edges)
    e = state["e"]
    lines.append(f"edge_topology (fills, insert, flags, scan, rows, one read-back)      {ms:9.3f} ms ({int(e.edges.shape[0])} edges in {MO.edge_table_slots(T)} slots, "
                 f"{int(e.get_boundary_edges().shape[0])} boundary, {int(e.get_non_manifold_edges().shape[0])} non-manifold, consistently oriented: "
                 f"{e.is_consistently_oriented()}, {e.n_invalid_triangles} invalid triangles)")

    def labels():
        state["p"] = MO._labels(e, T)

    ms = timed(labels)
    lines.append(f"component labels alone (hook, compress and a read-back per round)    {ms:9.3f} ms ({MO.last_rounds} rounds)")

    def clusters():
        state["c"] = MO.cluster_connected_triangles(v, t)

    ms = timed(clusters)
    cl, n_tri, area = state["c"]
    lines.append(f"cluster_connected_triangles (edges, labels, ids, sizes, areas)       {ms:9.3f} ms ({MO.last_rounds} rounds; {n_tri.numel()} clusters, the largest "
                 f"{int(n_tri.max())} triangles, {int((n_tri < 100).sum())} below 100 triangles; area {float(area.sum()):.6f} m^2)")

    def composed():
        state["t"] = torch_labels(t)

    ms = timed(composed)
    same = torch.equal(state["t"][0].to(torch.int32), state["p"])
    lines.append(f"torch.unique + scatter_reduce label propagation (today)              {ms:9.3f} ms ({state['t'][1]} rounds; the same labels: {same})")

    def remove():
        state["r"] = mesh.remove_small_components(min_triangles=100)

    ms = timed(remove)
    clean = state["r"][0]
    lines.append(f"remove_small_components(min_triangles=100), the whole call           {ms:9.3f} ms ({int(clean.triangles.shape[0])} triangles and "
                 f"{int(clean.vertices.shape[0])} vertices stay)")
    ms = timed(lambda: MO.compute_vertex_normals(v, t))
    lines.append(f"compute_vertex_normals (geometry, corner sort, per-vertex sums)      {ms:9.3f} ms")
    ms = timed(lambda: MO.compute_triangle_normals(v, t))
    lines.append(f"compute_triangle_normals                                             {ms:9.3f} ms")
    ms = timed(lambda: MO.get_surface_area(v, t))
    lines.append(f"get_surface_area (areas, one wave's sum, a read-back)                {ms:9.3f} ms")
    ms = timed(lambda: MO.filter_smooth_taubin(v, t, TAUBIN))
    lines.append(f"filter_smooth_taubin, {TAUBIN} iterations (edges, adjacency, {2 * TAUBIN} steps)        {ms:9.3f} ms")
    ms = timed(lambda: MO.filter_smooth_taubin(v, t, TAUBIN, vertex_colors=mesh.vertex_colors))
    lines.append(f"filter_smooth_taubin, {TAUBIN} iterations, with the colours                   {ms:9.3f} ms")
    perm = torch.randperm(T, generator=torch.Generator().manual_seed(0)).to(dev)
    tp = t[perm].contiguous()

    def permuted():
        state["cp"] = MO.cluster_connected_triangles(v, tp)

    ms = timed(permuted)
    lines.append(f"cluster_connected_triangles, triangle rows randomly permuted         {ms:9.3f} ms ({MO.last_rounds} rounds; {state['cp'][1].numel()} clusters)")

    def composed_permuted():
        state["tp"] = torch_labels(tp)

    ms = timed(composed_permuted)
    lines.append(f"torch label propagation, the permuted rows                           {ms:9.3f} ms ({state['tp'][1]} rounds)")
    assert isinstance(clean, TriangleMesh)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
