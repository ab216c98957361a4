"""The device pose-graph solver's host side (no GPU): ``posegraph.solve_plan``, the numpy statement of the kernels
(tests/_posegraph_solve_ref.py) against numpy's dense solve, and the ``solver=`` keyword's default path."""
import copy

import numpy as np
import pytest

import _posegraph_graphs as G
import _posegraph_solve_ref as PS
import test_posegraph_cpu as TP
from bodyslam_amd.posegraph import PG_MAX_SEPARATORS, PoseGraph, solve_plan, update_global_extrinsic


@pytest.mark.parametrize("name", list(G.CASES))
def test_solve_plan_properties(name):
    pg = G.build(name)
    a = G.arrays(pg)
    plan = G.plan_of(pg)
    N, ref = len(pg.pose_graph.nodes), pg.reference_node
    owner = np.full(N, -1)
    for si, (p, m) in enumerate(plan["segments"]):
        assert m >= 1 and 0 <= p and p + m <= N
        assert (owner[p:p + m] == -1).all()
        owner[p:p + m] = si
        assert (p == 0 or plan["node_slot"][p - 1] >= 0) and (p + m == N or plan["node_slot"][p + m] >= 0)      # maximal runs
        if G.CASES[name][1] is not None:
            assert m <= G.CASES[name][1]
    sep = plan["node_slot"] >= 0
    assert sep[ref] and plan["S"] == sep.sum() <= PG_MAX_SEPARATORS and not plan["over_capacity"]
    assert np.array_equal(plan["sep_node"], np.flatnonzero(sep)) and np.array_equal(plan["node_slot"][sep], np.arange(plan["S"]))
    assert ((owner >= 0) ^ sep).all()                        # every node is in exactly one segment or is a separator
    for s, t in zip(a["src"], a["tgt"]):
        if owner[s] >= 0 and owner[t] >= 0:
            assert owner[s] == owner[t]                      # no edge joins two segments' interiors
        for x, y in ((s, t), (t, s)):
            if owner[x] >= 0:
                assert abs(x - y) == 1                       # an interior node's neighbours are its index neighbours
    # the gather lists: every edge once per endpoint, ascending edge index per node
    adj, rp = plan["adj"], plan["row_ptr"]
    assert rp[0] == 0 and rp[-1] == len(adj) == 2 * len(a["src"])
    for n in range(N):
        rows = adj[rp[n]:rp[n + 1]]
        assert (np.diff(rows[:, 0]) > 0).all()
        for e, o, sg in rows:
            assert (a["src"][e], a["tgt"][e]) == ((n, o) if sg < 0 else (o, n))
    longs = {int(e) for e, _, _ in plan["long_edges"]}
    assert longs == {e for e, (s, t) in enumerate(zip(a["src"], a["tgt"])) if abs(s - t) >= 2 and ref not in (s, t)}
    assert set(plan["adjacent"]) == {i for i in range(N - 1) if sep[i] and sep[i + 1]}


def test_solve_plan_capacity():
    """4 000 nodes with 16 closures fit at the automatic segment length; a graph beyond 128 separators reports itself"""
    N = 4000
    rng = np.random.default_rng(3)
    ends = rng.choice(np.arange(1, N), size=32, replace=False)
    src = np.concatenate([np.arange(1, N), ends[:16]])
    tgt = np.concatenate([np.arange(0, N - 1), ends[16:]])
    plan = solve_plan(N, src, tgt)
    assert not plan["over_capacity"] and plan["S"] <= PG_MAX_SEPARATORS and plan["reason"] is None
    assert max(m for _, m in plan["segments"]) <= plan["segment_length"]
    N = 400
    far_s, far_t = np.arange(2, 132), np.arange(202, 332)            # 130 long edges on distinct nodes
    plan = solve_plan(N, np.concatenate([np.arange(1, N), far_s]), np.concatenate([np.arange(0, N - 1), far_t]))
    assert plan["over_capacity"] and plan["S"] > PG_MAX_SEPARATORS and "capacity" in plan["reason"]
    with pytest.raises(ValueError):
        solve_plan(4, [1, 5], [0, 1])
    with pytest.raises(ValueError):
        solve_plan(4, [1], [0], reference_node=4)


@pytest.mark.parametrize("k", range(len(G.LAMBDA_FACTORS)))
@pytest.mark.parametrize("name", list(G.CASES))
def test_statement_against_dense_solve(name, k):
    """The statement's substructured solve against numpy.linalg.solve of the dense H + lambda I, the system taken from PoseGraph's own
    system() (captured where it reaches the sparse LU) at lambda = 1e-5 max diag H and 1e4 times that.  The bar is measured, not chosen: the
    relative gap max |splu - numpy| / max |numpy| between scipy's sparse LU (the host path's solver) and numpy on these same systems, the
    largest over the graphs, times 8 -- the statement is a third fp64 elimination order of the same matrix.  Measured (numpy /
    scipy on x86-64): gap 1.9e-13 at lambda0 and 1.7e-15 at 1e4 lambda0 (bars 1.5e-12 and 1.4e-14); the statement's own distance from numpy was at
    most 2.0e-13 and 1.3e-15."""
    row = G.solve_cases()[name][k]
    bar = G.solve_bar(k)
    got = PS.solve(row["plan"], row["D"], row["b"], row["Cc"], row["blocks"], row["lam"])
    err = float(np.abs(got["delta"].ravel() - row["numpy"]).max() / np.abs(row["numpy"]).max())
    print(f"{name} lambda x{G.LAMBDA_FACTORS[k]:g}: splu-numpy gap {row['gap']:.3e}, bar {bar:.3e}, statement-numpy {err:.3e}")
    assert bar > 0 and err <= bar
    d = got["delta"].ravel()
    assert abs(got["sums"][0] - d @ d) <= 1e-12 * (d @ d)


def test_statement_system_is_the_hosts():
    """the statement's linearisation and gather assembly give the blocks of PoseGraph's own system (closed-form inverse against np.linalg.inv)"""
    for name in G.CASES:
        pg = G.build(name)
        a, plan = G.arrays(pg), G.plan_of(pg)
        lin = PS.linearise(a["X"], a["T"], a["info"], a["src"], a["tgt"], a["unc"], G.mu_of(pg, a))
        D, b, Cc, bmax, dmax = PS.assemble(plan, lin["Hss"], lin["g"])
        row = G.solve_cases()[name][0]
        scale = np.abs(row["D"]).max()
        assert np.abs(D - row["D"]).max() < 1e-9 * scale and np.abs(Cc - row["Cc"]).max() < 1e-9 * scale
        assert np.abs(b - row["b"]).max() < 1e-9 * max(1.0, np.abs(row["b"]).max())
        assert abs(dmax * 1e-5 - row["lam"]) < 1e-9 * row["lam"]


def _closure_cases():
    true, rel, chain = TP._ring()
    n = len(chain)
    info = np.eye(6)
    info[5, 5] = 4000.0
    yield chain, rel, [(n - 1, 0, np.linalg.inv(true[0]) @ true[n - 1], info * 50.0), (n // 2, 1, np.linalg.inv(true[1]) @ true[n // 2], info * 50.0)]
    true, rel, chain = TP._ring(seed=1)
    info = np.eye(6) * 30.0
    info[5, 5] = 3000.0
    wrong = TP._se3(TP._rot([1, 0, 0], 0.9), [0.4, -0.3, 0.2])
    yield chain, rel, [(n - 1, 0, np.linalg.inv(true[0]) @ true[n - 1], info), (n // 3, 2, wrong, info)]


def test_default_solver_is_the_host_path():
    for chain, rel, lc in _closure_cases():
        a = TP._build(chain, rel, lc)
        b = PoseGraph(solver="host")
        b.pose_graph = copy.deepcopy(a.pose_graph)
        a.optimize()
        b.optimize()
        assert a.solver == "host" and a.last_log["solver"] == b.last_log["solver"] == "host" and "fallback" not in a.last_log
        assert all(np.array_equal(x, y) for x, y in zip(update_global_extrinsic(a.pose_graph), update_global_extrinsic(b.pose_graph)))
        assert [(e.source_node_id, e.target_node_id, e.weight) for e in a.pose_graph.edges] == \
               [(e.source_node_id, e.target_node_id, e.weight) for e in b.pose_graph.edges]
        assert all(a.last_log[k] == b.last_log[k] for k in ("iterations", "residual0", "residual"))


def test_solver_keyword():
    import torch
    from bodyslam_amd._lib import BodySlamHipError
    with pytest.raises(ValueError):
        PoseGraph(solver="nonsense")
    if torch.cuda.is_available():
        return                                                # (with a GPU the device path runs: tests/test_posegraph_device_gpu.py)
    chain, rel, lc = next(_closure_cases())
    pg = TP._build(chain, rel, lc)
    pg.solver = "device"
    before = copy.deepcopy(pg.pose_graph)
    with pytest.raises(BodySlamHipError):
        pg.optimize()
    with pytest.raises(BodySlamHipError):
        G.build("ring", solver="device").optimize()
    assert all(np.array_equal(x.pose, y.pose) for x, y in zip(before.nodes, pg.pose_graph.nodes))
