"""The graphs of tests/test_posegraph_device_*.py, built with the helpers of tests/test_posegraph_cpu.py, and the measured fp64 bar of the
solve: the gap between scipy's sparse LU (what the host path uses) and numpy's dense solve on the very systems the tests solve."""
import copy
import functools

import numpy as np

import _posegraph_solve_ref as PS
from bodyslam_amd.posegraph import PoseGraph, solve_plan
from test_posegraph_cpu import _ring

INFO = np.eye(6)
INFO[5, 5] = 4000.0
INFO = INFO * 50.0

# name -> (closures (source, target), segment_length, reference node, variant)
CASES = {
    "ring": ([(23, 0), (12, 1)], None, 0, None),
    "ring_cut4": ([(23, 0), (12, 1)], 4, 0, None),
    "adjacent_closures": ([(12, 1), (13, 3)], 4, 0, None),        # separators 0 1 3 12 13: segments of length 0 and 1
    "reference5": ([(23, 0), (12, 1)], 4, 5, None),
    "reversed_edge": ([(23, 0), (12, 1)], 4, 0, "reversed"),      # the chain edge 6 -> 7 (source below target)
    "double_edge": ([(23, 0), (23, 0), (12, 1)], 4, 0, None),     # two edges on the same pair
    "isolated_node": ([(23, 0), (12, 1)], 4, 0, "isolated"),      # node 24 has no edge at all
    "missing_chain_edge": ([(23, 0), (12, 1)], 4, 0, "missing"),  # no edge between 7 and 8
}


def build(name, n=24, noise=2e-3, seed=0, solver="host", closures=None, segment_length=None, reference_node=0, variant=None):
    if name is not None:
        closures, segment_length, reference_node, variant = CASES[name]
    true, rel, chain = _ring(n, noise, seed)
    pg = PoseGraph(reference_node=reference_node, solver=solver)
    pg.segment_length = segment_length
    pg.add_node(chain[0])
    for i in range(1, n):
        pg.add_node(chain[i])
        if variant == "missing" and i == 8:
            continue
        if variant == "reversed" and i == 7:
            pg.add_edge(np.linalg.inv(rel[i - 1]), i - 1, i, False)
        else:
            pg.add_edge(rel[i - 1], i, i - 1, False)
    if variant == "isolated":
        pg.add_node(chain[-1] @ rel[0])
    for k, (s, t) in enumerate(closures):
        T = np.linalg.inv(true[t]) @ true[s]
        T[:3, 3] += 1e-4 * k                                        # (a second edge on a pair is not a copy of the first)
        pg.add_edge(T, s, t, True, INFO)
    return pg


def arrays(pg):
    g = pg.pose_graph
    return dict(X=np.stack([n.pose for n in g.nodes]), T=np.stack([e.transformation for e in g.edges]), info=np.stack([e.information for e in g.edges]),
                src=np.array([e.source_node_id for e in g.edges]), tgt=np.array([e.target_node_id for e in g.edges]),
                unc=np.array([e.uncertain for e in g.edges]))


def mu_of(pg, a):
    return pg.preference_loop_closure * pg.max_correspondence_distance ** 2 * float(a["info"][a["unc"], 5, 5].mean()) if a["unc"].any() else 0.0


def plan_of(pg):
    a = arrays(pg)
    return solve_plan(len(pg.pose_graph.nodes), a["src"], a["tgt"], pg.reference_node, pg.segment_length)


class _Captured(Exception):
    pass


def captured_system(pg):
    """(H dense, b, lambda0): the first system PoseGraph's own system() hands to its sparse LU (H without lambda, lambda0 = 1e-5 max diag H)"""
    import scipy.sparse.linalg as spla
    got = {}
    real = spla.splu

    class _Spy:
        def __init__(self, A):
            got["A"] = A.toarray()

        def solve(self, b):
            got["b"] = np.array(b)
            raise _Captured()

    spla.splu = _Spy
    try:
        copy.deepcopy(pg).optimize()
    except _Captured:
        pass
    finally:
        spla.splu = real
    A = got["A"]
    lam0 = 1e-5 * float(A.diagonal().max()) / (1.0 + 1e-5)
    return A - lam0 * np.eye(A.shape[0]), got["b"], lam0


LAMBDA_FACTORS = (1.0, 1.0e4)


@functools.lru_cache(maxsize=None)
def solve_cases():
    """name -> [per lambda factor: dict(plan, D, b, Cc, blocks, lam, numpy, splu, gap)], gap = max |splu - numpy| / max |numpy|"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    out = {}
    for name in CASES:
        pg = build(name)
        H, b, lam0 = captured_system(pg)
        plan = plan_of(pg)
        D, bb, Cc, blocks = PS.blocks_from_dense(plan, H, b)
        rows = []
        for f in LAMBDA_FACTORS:
            lam = lam0 * f
            Hl = H + lam * np.eye(H.shape[0])
            x_np = np.linalg.solve(Hl, b)
            x_lu = spla.splu(sp.csc_matrix(Hl)).solve(b)
            rows.append(dict(plan=plan, D=D, b=bb, Cc=Cc, blocks=blocks, lam=lam, numpy=x_np, splu=x_lu,
                             gap=float(np.abs(x_lu - x_np).max() / np.abs(x_np).max())))
        out[name] = rows
    return out


def solve_bar(k):
    """the relative bar on delta at LAMBDA_FACTORS[k]: 8 x the largest splu-against-numpy gap over the cases"""
    return 8.0 * max(rows[k]["gap"] for rows in solve_cases().values())
