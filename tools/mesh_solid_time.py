"""Times "is this mesh a solid" on the extract_mesh(host=False) mesh of the 256-frame 640x480 map that tools/map_correction_time.py builds
(the reference's TSDF parameters): the vertex-fan rounds, the COUNT launch of the pair search, a whole get_self_intersecting_triangles and
is_self_intersecting, component_volumes, a whole check_solid; then the brute-force COUNT launch on the first SUBSET query triangles against
the whole mesh, scaled per pair, to show what the grid saves.  HIP events, one warm-up run, then the median of five.  Reported, not
asserted: nothing here has an earlier implementation or a target.

    python tools/mesh_solid_time.py [--out profiles/mesh_solid_time.txt]
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
from bodyslam_amd.tsdf import BATCH_MAX, TSDF, PinholeCameraIntrinsic  # noqa: E402
from reconstruction_eval_time import timed  # noqa: E402

SUBSET = 16384              # query triangles of the brute-force launch: 16 384 x T pairs, seconds at most


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_solid_time.txt"))
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
    lines = [f"is this mesh a solid on {torch.cuda.get_device_name(0)}: the extract_mesh(host=False) mesh of {M.N} frames of {M.W}x{M.H} (TSDF 1 mm / 0.1 m / "
             f"32^3 / stride 8), {V} vertices, {T} triangles; HIP events, median of 5 after a warm-up"]
    state = {}
    e = MO.edge_topology(v, t)

    def fans():
        state["f"] = MO._fan_counts(t, V, e)

    ms = timed(fans)
    lines.append(f"vertex fans alone (hook, compress and a read-back per round, count)  {ms:9.3f} ms ({MO.last_fan_rounds} rounds; "
                 f"{int((state['f'] > 1).sum())} non-manifold vertices)")
    ms = timed(lambda: MO.get_non_manifold_vertices(v, t))
    lines.append(f"get_non_manifold_vertices, the whole call (edges included)           {ms:9.3f} ms")
    rec, kept = MO._solid_records(v, t)
    grid, cell_start, refs = MO._pair_grid(rec, kept, None)
    i32 = dict(dtype=torch.int32, device=dev)
    counts, fb_list, fb_count = torch.zeros(T, **i32), torch.empty(T, **i32), torch.empty(1, **i32)
    ms = timed(lambda: L.mesh_pairs_grid(rec, rec, refs, cell_start, grid, True, MO.PAIR_CELL_CAP, L.MESH_PAIRS_COUNT, counts, None, None, None, fb_list,
                                         fb_count))
    dims = grid[3]
    lines.append(f"pair search, the COUNT launch on the grid                            {ms:9.3f} ms ({kept} kept triangles, {dims[0]} x {dims[1]} x {dims[2]} cells of "
                 f"{grid[2]:.6f} m, {int(refs.numel())} references, {int(fb_count.cpu())} triangles left to brute force, {int(counts.sum())} pairs)")

    def pairs():
        state["p"] = MO.get_self_intersecting_triangles(v, t, method="grid")

    ms = timed(pairs)
    lines.append(f"get_self_intersecting_triangles (records, grid, count, fill, sort)   {ms:9.3f} ms ({int(state['p'].shape[0])} pairs, "
                 f"{MO.last_fallback} triangles by brute force)")

    def flag():
        state["a"] = MO.is_self_intersecting(v, t, method="grid")

    ms = timed(flag)
    lines.append(f"is_self_intersecting (records, grid, the ANY launch)                 {ms:9.3f} ms ({state['a']})")

    def volumes():
        state["v"] = MO.component_volumes(v, t)

    ms = timed(volumes)
    vol = state["v"][1]
    lines.append(f"component_volumes (edges, labels, per-triangle volumes, sums)        {ms:9.3f} ms ({vol.numel()} clusters, {int((~torch.isnan(vol)).sum())} with a "
                 f"volume)")

    def solid():
        state["s"] = MO.check_solid(v, t, method="grid")

    ms = timed(solid)
    lines.append(f"check_solid, the whole call                                          {ms:9.3f} ms ({state['s']})")
    m = min(SUBSET, T)
    sub = torch.arange(m, **i32)
    out = torch.zeros(T, **i32)
    ms = timed(lambda: L.mesh_pairs_brute(rec, sub, m, rec, True, L.MESH_PAIRS_COUNT, out, None, None, None, None))
    tested = m * T - m * (m + 1) // 2
    lines.append(f"brute force, the COUNT launch for the first {m} query triangles     {ms:9.3f} ms ({tested} pairs i < j: {ms * 1e6 / tested:.4f} ns per pair; all "
                 f"{T * (T - 1) // 2} pairs at that rate: {ms * (T * (T - 1) // 2) / tested / 1e3:.1f} s)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
