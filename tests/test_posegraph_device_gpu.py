"""PoseGraph(solver="device") on the GPU (csrc/posegraph.hip): every stage against the numpy statement
(tests/_posegraph_solve_ref.py), the optimiser end to end against the dense oracle and the host path, determinism, the capacity fallback, the
chain-only graph and the SLAM loop.  `pytest -m gpu`."""
import functools
import os

import numpy as np
import pytest
import torch

import _posegraph_graphs as G
import _posegraph_solve_ref as PS
import test_posegraph_cpu as TP
from bodyslam_amd import _lib as L
from bodyslam_amd.posegraph import update_global_extrinsic
from test_posegraph_device_cpu import _closure_cases

pytestmark = pytest.mark.gpu
BAR = dict(rtol=1e-9, atol=1e-9)            # the project's fp64 bar (test_trajectory_eval_gpu.py, test_loop_closure_gpu.py)


def _dev(a, dt=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()


def _f64(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def _plan_dev(plan):
    return {k: _dev(plan[k], np.int32) for k in ("segments", "sep_node", "node_slot", "adjacent", "long_edges", "row_ptr", "adj")}


@pytest.mark.parametrize("name", list(G.CASES))
def test_linearise_assemble_update_against_the_statement(name):
    L.init(0)
    pg = G.build(name)
    a, plan, mu = G.arrays(pg), G.plan_of(pg), G.mu_of(pg, G.arrays(pg))
    N, E = plan["N"], plan["E"]
    ref = PS.linearise(a["X"], a["T"], a["info"], a["src"], a["tgt"], a["unc"], mu)
    X, T, info = _dev(a["X"]), _dev(a["T"]), _dev(a["info"])
    src, tgt, unc = _dev(a["src"], np.int32), _dev(a["tgt"], np.int32), _dev(a["unc"], np.int32)
    lw, z, q, Hss, g, ct, cost = _f64(E), _f64(E, 6), _f64(E), _f64(E, 6, 6), _f64(E, 6), _f64(E), _f64(1)
    L.pg_linearise(X, T, info, src, tgt, unc, mu, L.PG_LINE_PROCESS | L.PG_SYSTEM, lw, z, q, Hss, g, ct, cost)
    for got, key in ((z, "z"), (q, "q"), (lw, "lw"), (Hss, "Hss"), (g, "g"), (ct, "cterm")):
        assert np.allclose(got.cpu().numpy(), ref[key], **BAR), key
    assert np.isclose(float(cost[0]), ref["cost"], **BAR) and float(cost[0]) == PS.wave_sum(ct.cpu().numpy())      # the fixed summation order
    assert ref["lw"][a["unc"]].max() < 1.0 and (ref["lw"][~a["unc"]] == 1.0).all()
    # the cost-only mode: given weights, Hss and g untouched
    lw2 = _dev(np.linspace(0.3, 0.9, E))
    Hss_before = Hss.clone()
    L.pg_linearise(X, T, info, src, tgt, unc, mu, 0, lw2, z, q, Hss, g, ct, cost)
    ref2 = PS.linearise(a["X"], a["T"], a["info"], a["src"], a["tgt"], a["unc"], mu, lw=lw2.cpu().numpy(), system=False)
    assert np.allclose(ct.cpu().numpy(), ref2["cterm"], **BAR) and np.isclose(float(cost[0]), ref2["cost"], **BAR) and torch.equal(Hss, Hss_before)
    # assembly, from the statement's edge blocks
    D0, b0, Cc0, bmax, dmax = PS.assemble(plan, ref["Hss"], ref["g"])
    pd = _plan_dev(plan)
    D, b, Cc, mx = _f64(N, 6, 6), _f64(N, 6), _f64(N, 6, 6), _f64(2)
    L.pg_assemble(_dev(ref["Hss"]), _dev(ref["g"]), pd["row_ptr"], pd["adj"], pg.reference_node, D, b, Cc, mx)
    assert np.allclose(D.cpu().numpy(), D0, **BAR) and np.allclose(b.cpu().numpy(), b0, **BAR) and np.allclose(Cc.cpu().numpy(), Cc0, **BAR)
    assert np.array_equal(D[pg.reference_node].cpu().numpy(), np.eye(6)) and not b[pg.reference_node].any()
    assert np.float32(float(mx[0])) == np.float32(bmax) and np.float32(float(mx[1])) == np.float32(dmax)
    # update
    rng = np.random.default_rng(5)
    delta = rng.normal(size=(N, 6)) * 1e-2
    Xn0, xn2 = PS.update(a["X"], delta)
    Xn, terms, out = _f64(N, 4, 4), _f64(N), _f64(1)
    L.pg_update(X, _dev(delta), Xn, terms, out)
    got = Xn.cpu().numpy()
    assert np.abs(got - Xn0).max() < 1e-12 and np.array_equal(got[:, 3], np.tile([0, 0, 0, 1.0], (N, 1)))
    assert abs(float(out[0]) - xn2) < 1e-12 * xn2


@pytest.mark.parametrize("k", range(len(G.LAMBDA_FACTORS)))
@pytest.mark.parametrize("name", list(G.CASES))
def test_solve_stages_against_the_statement(name, k):
    """bs_pg_solve on the systems of tests/test_posegraph_device_cpu.py::test_statement_against_dense_solve (PoseGraph's own system(), captured):
    the segment slots and the reduced matrix against the statement at the fp64 bar, delta against numpy's dense solve within the bar measured
    there (8 x the splu-against-numpy gap on these systems)."""
    L.init(0)
    row = G.solve_cases()[name][k]
    plan, lam = row["plan"], row["lam"]
    N, E, S, nseg = plan["N"], plan["E"], plan["S"], len(plan["segments"])
    st = PS.solve(plan, row["D"], row["b"], row["Cc"], row["blocks"], lam)
    Hss = np.zeros((E, 6, 6))
    for (e, _, _), blk in zip(plan["long_edges"], row["blocks"]):
        Hss[e] = -blk
    pd = _plan_dev(plan)
    D, b, Cc, Hd = _dev(row["D"]), _dev(row["b"]), _dev(row["Cc"]), _dev(Hss)
    ws, slots, M, vec, delta, sums = _f64(N, L.PG_NODE_WORKSPACE), _f64(max(nseg, 1), L.PG_SLOT_FIELDS), _f64(6 * S, 6 * S), _f64(24 * S), _f64(N, 6), _f64(2)
    args = (D, b, Cc, Hd, lam, pd["segments"], pd["sep_node"], pd["node_slot"], pd["adjacent"], pd["long_edges"])
    L.pg_solve(*args, L.PG_STAGE_SWEEP | L.PG_STAGE_REDUCED, ws, slots, M, vec, delta)
    scale = np.abs(st["M"]).max()
    assert np.abs(slots.cpu().numpy()[:nseg] - st["slots"]).max() <= 1e-9 * scale
    assert np.abs(M.cpu().numpy() - st["M"]).max() <= 1e-9 * scale
    assert np.allclose(vec.cpu().numpy()[:6 * S], st["r"], **BAR)
    L.pg_solve(*args, L.PG_STAGE_ALL, ws, slots, M, vec, delta, sums)
    got = delta.cpu().numpy()
    ref = row["numpy"]
    err = float(np.abs(got.ravel() - ref).max() / np.abs(ref).max())
    print(f"{name} lambda x{G.LAMBDA_FACTORS[k]:g}: device-numpy {err:.3e}, bar {G.solve_bar(k):.3e}")
    assert np.isfinite(got).all() and err <= G.solve_bar(k)
    d = got.ravel()
    assert np.allclose(sums.cpu().numpy(), [PS.wave_sum(d * d), PS.wave_sum(d * (lam * d + row["b"].ravel()))], rtol=1e-12, atol=0)


def _oracle_run(pg):
    return TP._oracle(pg)


@pytest.mark.parametrize("case", [0, 1])
def test_device_optimiser_matches_the_dense_oracle(case):
    """the two closure cases of tests/test_posegraph_cpu.py at that file's own bars for the sparse host path: 1e-9 (true closures), 1e-8 (one
    false closure, pruned).  The iteration count is the oracle's where nothing is pruned; with the pruned edge last_log is the second run's, which the
    oracle does not make, so it is compared with the host path's."""
    chain, rel, lc = list(_closure_cases())[case]
    pg = TP._build(chain, rel, lc)
    pg.solver = "device"
    host = TP._build(chain, rel, lc)
    Xo, lo, keep_o, log_o = _oracle_run(pg)
    assert (np.abs(lo - pg.edge_prune_threshold) > 1e-6).all()          # no decision of the pruning sits on its threshold
    pg.optimize()
    host.optimize()
    X = np.stack(update_global_extrinsic(pg.pose_graph))
    err = np.abs(X - Xo).max()
    print(f"case {case}: device-oracle {err:.3e}, iterations {pg.last_log['iterations']} (host {host.last_log['iterations']}, oracle {log_o['iterations']})")
    assert err < (1e-9, 1e-8)[case]
    assert pg.last_log["solver"] == "device" and "fallback" not in pg.last_log
    assert pg.last_log["iterations"] == host.last_log["iterations"]
    if case == 0:
        assert pg.last_log["iterations"] == log_o["iterations"]
    kept = [(e.source_node_id, e.target_node_id) for e in pg.pose_graph.edges]
    assert kept == [(e.source_node_id, e.target_node_id) for e in host.pose_graph.edges]
    edges0 = [(i, i - 1) for i in range(1, len(chain))] + [(s, t) for s, t, _, _ in lc]
    assert kept == [e for e, k in zip(edges0, keep_o) if k]
    assert np.array_equal(X[0], chain[0])                               # the reference node does not move
    assert np.array_equal(X[:, 3], np.tile([0, 0, 0, 1.0], (len(chain), 1)))


N300_CLOSURES = [(299, 0), (150, 3), (220, 40)]


def _ring300(solver, segment_length=None):
    return G.build(None, n=300, noise=2e-3, solver=solver, closures=N300_CLOSURES, segment_length=segment_length)


@functools.lru_cache(maxsize=None)
def _ring300_reference():
    """the host path and the dense oracle on the N = 300 ring, once: (host poses, host weights, host log, host-against-oracle gap)"""
    host = _ring300("host")
    Xo, _, _, log_o = _oracle_run(host)
    host.optimize()
    Xh = np.stack(update_global_extrinsic(host.pose_graph))
    return Xh, [e.weight for e in host.pose_graph.edges], host.last_log, float(np.abs(Xh - Xo).max()), log_o


@pytest.mark.parametrize("segment_length", [None, 7])
def test_device_matches_the_host_where_segments_are_cut(segment_length):
    """A ring of 300 nodes (noise 2e-3, three closures): the chain is cut into segments (37 separators at the automatic length of 8, 40 at
    segment_length = 7).  The bar on the poses is 8 x the measured gap between the host path and the dense oracle on this same graph
    (measured on an x86-64 host: gap 4.3e-14, bar 3.4e-13; the statement run through the same LM on the CPU differed from the host by 1.4e-14), and the LM iteration count is the host's.  Run twice: the same bits."""
    Xh, wh, log_h, gap, log_o = _ring300_reference()
    bar = 8.0 * gap
    runs = []
    for _ in range(2):
        pg = _ring300("device", segment_length)
        pg.optimize()
        runs.append((np.stack(update_global_extrinsic(pg.pose_graph)), [e.weight for e in pg.pose_graph.edges], pg.last_log))
    X, w, log = runs[0]
    err = float(np.abs(X - Xh).max())
    print(f"N = 300, segment_length {segment_length}: device-host {err:.3e}, host-oracle gap {gap:.3e}, bar {bar:.3e}, iterations {log['iterations']} "
          f"(host {log_h['iterations']}, oracle {log_o['iterations']})")
    assert log["solver"] == "device" and "fallback" not in log
    assert bar > 0 and err <= bar
    assert log["iterations"] == log_h["iterations"] and len(w) == len(wh)
    assert np.array_equal(runs[1][0], X) and runs[1][1] == w and runs[1][2] == log          # determinism: bit-equal poses and weights


def test_over_capacity_graph_is_the_hosts():
    """130 long edges on distinct nodes, N = 400: more than 128 separators -- exactly the host result, and last_log says why"""
    true, rel, chain = TP._ring(400, 2e-3, 2)
    lc = [(202 + i, 2 + i, np.linalg.inv(true[2 + i]) @ true[202 + i], G.INFO) for i in range(130)]
    dev = TP._build(chain, rel, lc)
    dev.solver = "device"
    host = TP._build(chain, rel, lc)
    dev.optimize()
    host.optimize()
    assert dev.last_log["solver"] == "host" and "capacity" in dev.last_log["fallback"]
    assert all(np.array_equal(a, b) for a, b in zip(update_global_extrinsic(dev.pose_graph), update_global_extrinsic(host.pose_graph)))
    assert [e.weight for e in dev.pose_graph.edges] == [e.weight for e in host.pose_graph.edges]
    assert all(dev.last_log[k] == host.last_log[k] for k in ("iterations", "residual0", "residual"))


def test_chain_only_graph_is_left_untouched(golden_dir):
    g = np.load(os.path.join(golden_dir, "geom3d_chain.npz"))
    t_rel, g_abs = g["t_rel"][:600].astype(np.float64), g["g_abs"][:601]
    pg = TP._build(list(g_abs), list(t_rel), [])
    pg.solver = "device"
    pg.optimize()
    assert pg.last_log["solver"] == "device" and pg.last_log["iterations"] == 0 and pg.last_log["residual0"] < 1e-6
    out = update_global_extrinsic(pg.pose_graph)
    assert len(out) == 601 and all(np.array_equal(a, b) for a, b in zip(out, g_abs)) and len(pg.pose_graph.edges) == 600


def test_slam_loop_with_the_device_solver():
    """run_slam_loop over the frames of test_sequence_with_posegraph_relinearisation with one closure and posegraph_every = 4: the device solver's
    final extrinsics within 1e-8 of the host solver's, the map rebuilt at the same frames; two host runs bit-equal (off means unchanged)."""
    import dataclasses
    from bodyslam_amd.pipeline import BodySlamPipeline
    from bodyslam_amd.synthetic import make_sequence
    from bodyslam_amd.tsdf import TSDF
    from bodyslam_amd.zoedepth import ZoeConfig
    from oracle import cyclepose_ref as CP
    from oracle import zoedepth_ref as Z
    cfg_o = Z.ZoeConfig(hidden=128, layers=4, heads=2, intermediate=256, taps=(1, 2, 3, 4), image_size=64)
    names = {f.name for f in dataclasses.fields(ZoeConfig)}
    cfg_p = ZoeConfig(**{k: v for k, v in dataclasses.asdict(cfg_o).items() if k in names})
    pipe = BodySlamPipeline(Z.synth_weights(cfg_o, seed=2), CP.synth_weights(seed=2), cfg_p, batch=4, target_hw=(64, 96))
    assert pipe.posegraph_solver == "host"
    frames = make_sequence(9, 160, 192, seed=5)
    ga = pipe.run_slam_loop(frames, posegraph_every=4).g_abs.cpu().numpy()
    info = np.eye(6)
    info[5, 5] = 5000.0
    T80 = np.linalg.inv(ga[0]) @ ga[8]
    T80[:3, 3] += 2e-3                                   # disagrees with the chain by 2 mm: kept, and spread over the chain
    pipe.loop_closures = [(8, 0, T80, info)]

    def run(solver):
        pipe.posegraph_solver = solver
        rebuilt = []

        def factory():
            rebuilt.append(len(seen))
            return TSDF(voxel_length=0.02, sdf_trunc=0.06, volume_unit_resolution=8, depth_sampling_stride=8)
        seen = []
        res = pipe.run_slam_loop(frames, tsdf=factory(), posegraph_every=4, tsdf_factory=factory, on_frame=lambda i, pose, pcd: seen.append(i))
        return res.g_abs.cpu().numpy(), rebuilt[1:], res.tsdf.frames_integrated

    h1, h2, d = run("host"), run("host"), run("device")
    assert np.array_equal(h1[0], h2[0]) and h1[1:] == h2[1:]
    assert np.abs(h1[0] - ga).max(axis=(1, 2))[8] > 2e-4 and len(h1[1]) == 1        # the closure moved the chain: one rebuild
    err = np.abs(d[0] - h1[0]).max()
    print(f"slam loop: device-host {err:.3e}")
    assert err < 1e-8 and d[1:] == h1[1:] and np.array_equal(d[0][0], h1[0][0])
