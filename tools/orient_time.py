"""Times the consistent orientation of normals and of the winding on the 256-frame 640x480 map that tools/map_correction_time.py builds (the
reference's TSDF parameters): orient_normals_consistent_tangent_plane on the extract_pcd cloud with normals estimated at the same k under
the largest-component rule, at k = 10 and k = 30 -- the rounds, the time per launch kind summed over the rounds, and the whole call --, and
orient_triangles on the extract_mesh mesh with a random half of its triangles flipped.  Beside the cloud,
scipy.sparse.csgraph.minimum_spanning_tree on the same graph on the CPU (the tree alone: no orientation, the graph already built).  HIP events
around every launch of one run (after a warm-up run) for the launch kinds, a read-back per round as in the call; the whole calls: one
warm-up run, then the median of five.  Reported, not asserted: there is no earlier implementation and no target.

    python tools/orient_time.py [--out profiles/orient_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_correction_time as M  # noqa: E402
from bodyslam_amd import _lib as L  # noqa: E402
from bodyslam_amd import mesh as MO  # noqa: E402
from bodyslam_amd import pointcloud as PC  # noqa: E402
from bodyslam_amd.tsdf import BATCH_MAX, TSDF, PinholeCameraIntrinsic  # noqa: E402
from reconstruction_eval_time import timed  # noqa: E402

KS = (10, 30)


class Kinds:
    """the time of every launch kind, summed: HIP events around each launch"""

    def __init__(self):
        self.ms, self.n = {}, {}

    def run(self, kind, fn, *args):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(*args)
        e1.record()
        e1.synchronize()
        self.ms[kind] = self.ms.get(kind, 0.0) + e0.elapsed_time(e1)
        self.n[kind] = self.n.get(kind, 0) + 1

    def lines(self):
        return [f"  {kind:28s} {self.n[kind]:3d} launches {self.ms[kind] * 1e3:10.1f} us in all" for kind in self.ms]


def cloud_launches(nn, cloud, normals, k):
    """pointcloud.orient_normals_consistent_tangent_plane's launches, each timed -> (Kinds, rounds, index, keys)"""
    dev, n = cloud.device, int(cloud.shape[0])
    kinds = Kinds()
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
    state = {}
    kinds.run("bs_pc_query_knn", lambda: state.update(q=nn.query_knn(cloud, k)))
    index, _, count = state["q"]
    keys, valid = torch.empty(n * k, **i64), torch.empty(n, **i32)
    kinds.run("bs_pc_orient_edges", L.pc_orient_edges, cloud, normals, index, count, keys, valid)
    word = torch.arange(n, **i32) * 2
    best, best_hi, crossing = torch.empty(n, **i64), torch.empty(n, **i32), torch.zeros(1, **i32)
    rounds = 0
    while True:
        crossing.zero_()
        kinds.run("bs_pc_orient_clear", L.pc_orient_clear, best, best_hi)
        kinds.run("bs_pc_orient_select", L.pc_orient_select, keys, index, word, best, crossing)
        rounds += 1
        if int(crossing.cpu()) == 0:
            break
        kinds.run("bs_pc_orient_select_hi", L.pc_orient_select_hi, keys, index, word, best, best_hi)
        kinds.run("bs_pc_orient_hook", L.pc_orient_hook, normals, word, best, best_hi)
        kinds.run("bs_pc_orient_compress", L.pc_orient_compress, word)
    kinds.run("bs_pc_orient_clear", L.pc_orient_clear, best)
    kinds.run("bs_pc_orient_seed", L.pc_orient_seed, cloud, valid, word, best)
    out, flipped = torch.empty(n, 3, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    kinds.run("bs_pc_orient_flip", L.pc_orient_flip, normals, valid, word, best, (0.0, 0.0, 1.0), out, flipped)
    return kinds, rounds, index, keys


def scipy_tree(index, keys, n):
    """scipy's minimum spanning tree of the same graph on the CPU -> (seconds for the tree alone, its edges), or None without scipy"""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import minimum_spanning_tree
    except ImportError:
        return None
    k = index.shape[1]
    key = keys.cpu().numpy().view(np.uint64)
    use = key != np.uint64(0xffffffffffffffff)
    i = np.repeat(np.arange(n), k)[use]
    j = index.cpu().numpy().reshape(-1)[use].astype(np.int64)
    w = (key[use] >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(np.float64) + 1e-12      # (scipy reads a stored 0 as no edge)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    _, first = np.unique(lo * n + hi, return_index=True)                                                # (an edge may lie in both rows)
    g = coo_matrix((w[first], (lo[first], hi[first])), shape=(n, n)).tocsr()
    t0 = time.perf_counter()
    tree = minimum_spanning_tree(g)
    return time.perf_counter() - t0, int(tree.nnz)


def mesh_launches(v, t):
    """mesh.orient_triangles' launches, each timed -> (Kinds, rounds)"""
    dev, T = t.device, int(t.shape[0])
    kinds = Kinds()
    i32 = dict(dtype=torch.int32, device=dev)
    state = {}
    kinds.run("the edge table (_edge_rows)", lambda: state.update(me=MO._edge_rows(t, int(v.shape[0]), MO.edge_table_slots(T))))
    me = state["me"]
    word, changed = torch.arange(T, **i32) * 2, torch.zeros(1, **i32)
    rounds = 0
    while True:
        changed.zero_()
        kinds.run("bs_mesh_orient_hook", L.mesh_orient_hook, me, word, changed)
        kinds.run("bs_mesh_orient_compress", L.mesh_orient_compress, word)
        rounds += 1
        if int(changed.cpu()) == 0:
            break
    bad = torch.zeros(T, **i32)
    kinds.run("bs_mesh_orient_check", L.mesh_orient_check, me, word, bad)
    out, flipped = torch.empty_like(t), torch.empty(T, dtype=torch.uint8, device=dev)
    kinds.run("bs_mesh_orient_flip", L.mesh_orient_flip, t, me.edge_of_half, word, bad, out, flipped)
    return kinds, rounds


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orient_time.txt"))
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
    mesh = tsdf.extract_mesh(host=False)
    n = int(cloud.shape[0])
    del rgbds
    lines = [f"consistent orientation on {torch.cuda.get_device_name(0)}: the extract_pcd cloud ({n} points) and the extract_mesh mesh of {M.N} frames "
             f"of {M.W}x{M.H} (TSDF 1 mm / 0.1 m / 32^3 / stride 8); HIP events; launch kinds: one run after a warm-up run, every launch timed and summed "
             f"over the rounds; whole calls: median of 5 after a warm-up"]
    state = {}
    for k in KS:
        normals = PC.estimate_normals(cloud, k=k)
        nn = PC.NearestNeighbours(cloud)
        cloud_launches(nn, cloud, normals, k)                                 # (a warm-up run: the first launch of a kernel loads its code)
        kinds, rounds, index, keys = cloud_launches(nn, cloud, normals, k)

        def whole():
            state["o"] = PC.orient_normals_consistent_tangent_plane(cloud, normals, k)

        ms = timed(whole)
        first = state["o"]
        whole()
        same = bool(torch.equal(first[0].view(torch.int32), state["o"][0].view(torch.int32)) and torch.equal(first[1], state["o"][1]))
        flipped = int(state["o"][1].sum())
        edges = int((keys != L.ORIENT_NO_KEY).sum())
        lines.append(f"orient_normals_consistent_tangent_plane(k = {k}) from estimate_normals(k = {k}): {ms:9.2f} ms with the index build, the k-NN "
                     f"query, {PC.last_rounds} rounds and their read-backs, the seeds and the flips; {edges} slots of {n * k} are edges; "
                     f"{PC.last_components} trees, {flipped} of {n} normals flipped; a further run gives {'the same bits' if same else 'OTHER BITS'}")
        lines += kinds.lines()
        ref = scipy_tree(index, keys, n)
        if ref is None:
            lines.append("  scipy is not installed: no CPU minimum spanning tree beside it")
        else:
            lines.append(f"  scipy.sparse.csgraph.minimum_spanning_tree of the same graph on the CPU, the tree alone (graph built, no orientation): "
                         f"{ref[0] * 1e3:9.2f} ms, {ref[1]} tree edges")
        del normals, index, keys, first, state["o"]

    v, t = MO._on_device(mesh.vertices, mesh.triangles, dev)
    T = int(t.shape[0])
    g = torch.Generator(device="cpu").manual_seed(7)
    pick = (torch.rand(T, generator=g) < 0.5).to(dev)
    t = torch.where(pick[:, None], t[:, [0, 2, 1]], t).contiguous()
    mesh_launches(v, t)                                                       # (a warm-up run)
    kinds, rounds = mesh_launches(v, t)

    def whole_mesh():
        state["m"] = MO.orient_triangles(v, t)

    ms = timed(whole_mesh)
    out, flipped, ok = state["m"]
    whole_mesh()
    same = bool(torch.equal(out, state["m"][0]) and torch.equal(flipped, state["m"][1]))
    comp, verdict = MO.orientable_components(v, t)
    lines.append(f"orient_triangles on the mesh of {T} triangles with a random half flipped ({int(pick.sum())}): {ms:9.2f} ms with the edge table, "
                 f"{MO.last_orient_rounds} rounds and their read-backs, the check and the flips; {int(flipped.sum())} triangles flipped, "
                 f"{int(verdict.numel())} components of which {int((~verdict).sum())} are not orientable; consistently oriented afterwards: "
                 f"{MO.edge_topology(v, out).is_consistently_oriented()}; a further run gives {'the same bits' if same else 'OTHER BITS'}")
    lines += kinds.lines()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
