"""Times PoseGraph.optimize() with the host solver and with the device solver on drifted rings: 500 / 2 000 / 4 000 nodes with 4 / 16 loop
closures (noisy odometry, true closures: several LM iterations).  Every run optimises a fresh copy of the graph; wall-clock time around the
call (it ends with the poses on the host for both solvers, the device solver's readback synchronises), two warm-up runs, then the median of
seven.  Reported, not asserted: the comparison is with the host path of the same commit on the same machine; there is no target.

    python tools/posegraph_time.py [--out profiles/posegraph_time.txt]
"""
import argparse
import copy
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bodyslam_amd import _lib  # noqa: E402
from bodyslam_amd.posegraph import PoseGraph, solve_plan  # noqa: E402

SIZES = ((500, 4), (2000, 4), (2000, 16), (4000, 4), (4000, 16))


def _rot(axis, a):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def _se3(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def ring(n, closures, noise=2e-4, seed=0):
    """a camera on a circle looking inwards: noisy odometry edges, `closures` true closures between nodes far apart"""
    rng = np.random.default_rng(seed)
    true = [_se3(_rot([0, 1, 0], 2 * np.pi * i / n), [np.sin(2 * np.pi * i / n), 0.02 * i / n, 1 - np.cos(2 * np.pi * i / n)]) for i in range(n)]
    pg = PoseGraph()
    pose = true[0].copy()
    pg.add_node(pose)
    for i in range(1, n):
        T = np.linalg.inv(true[i - 1]) @ true[i] @ _se3(_rot(rng.normal(size=3), noise * rng.normal()), noise * rng.normal(size=3))
        pose = pose @ T
        pg.add_node(pose)
        pg.add_edge(T, i, i - 1, False)
    info = np.eye(6) * 50.0
    info[5, 5] = 200000.0
    for k in range(closures):
        s, t = n - 1 - k * (n // (2 * closures)), k * (n // (2 * closures)) + (2 if k else 0)
        pg.add_edge(np.linalg.inv(true[t]) @ true[s], s, t, True, info)
    return pg


def median_ms(graph, solver, reps=7, warm=2):
    ts, log = [], None
    for r in range(warm + reps):
        pg = PoseGraph(solver=solver)
        pg.pose_graph = copy.deepcopy(graph.pose_graph)
        if solver == "device":
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        pg.optimize()
        t1 = time.perf_counter()
        if r >= warm:
            ts.append(1e3 * (t1 - t0))
        log = pg.last_log
    return float(np.median(ts)), log


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posegraph_time.txt"))
    a = ap.parse_args()
    _lib.init(0)
    lines = [f"PoseGraph.optimize(): host solver (numpy + sparse LU on {os.cpu_count()} CPUs) against the device solver on {torch.cuda.get_device_name(0)} "
             f"(wall clock, median of 7, warmed)"]
    for n, closures in SIZES:
        graph = ring(n, closures)
        g = graph.pose_graph
        plan = solve_plan(n, [e.source_node_id for e in g.edges], [e.target_node_id for e in g.edges])
        host_ms, host_log = median_ms(graph, "host")
        dev_ms, dev_log = median_ms(graph, "device")
        lines.append(f"N = {n:5d}, {closures:2d} closures ({plan['S']:3d} separators, segments of <= {plan['segment_length']}): host {host_ms:9.2f} ms "
                     f"({host_log['iterations']} iterations), device {dev_ms:9.2f} ms ({dev_log['iterations']} iterations"
                     f"{', FALLBACK ' + dev_log['fallback'] if 'fallback' in dev_log else ''}) = {host_ms / dev_ms:6.2f} x")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
