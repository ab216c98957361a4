"""Pose graph of the SLAM loop: drop-in for BodySLAM_not_refactored/3DM/posegraph.py:5-43.

The reference keeps an Open3D ``PoseGraph`` of the chain's absolute poses with one odometry edge per frame
(3DM/slam.py:156-157: ``add_node(curr_absolute_pose)``, ``add_edge(transformation, i, i - 1, False)``), runs Open3D's
Levenberg-Marquardt global optimisation every 500 frames (:159-165) and reads the node poses back
(``update_global_extrinsic``, 3DM/slam_utils.py:88-90).  Same class, method names, argument meaning and defaults here; the
optimiser is a restatement of Open3D's GlobalOptimization (Choi, Zhou, Koltun, CVPR 2015: pose graph with line processes,
see oracle/posegraph_ref.py for the formulas) on the host, as in the reference: edges are linearised in one vectorised pass
(fp64), the 6N x 6N normal equations are assembled block-sparse (block tridiagonal for a chain, plus one off-diagonal block
pair per loop closure) and solved by a sparse LU per LM step -- 4 000 nodes (BASELINE config 5) take milliseconds per step
where a dense solve would need 4.6 GB.  With odometry edges only, the chain itself is the optimum: the residual is below
``min_residual`` at entry and the poses are returned untouched (what the reference's log line "posegraph non fa nulla" reports).
Open3D is not vendored with the reference and not installable offline: parity against it is unpinned; tests/ check this
module against the independent dense oracle and against the chain's golden vectors.

``PoseGraph(solver="device")`` (off by default) evaluates the same algorithm's four numerical pieces on the GPU (csrc/posegraph.hip, DESIGN.md
section 3.14): the LM control flow below stays on the host line by line and reads back a handful of doubles per inner step; poses, edge data and
all intermediates stay in device memory for the whole ``optimize()``.  ``solve_plan`` is the host-side plan of its linear solve.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List

import numpy as np


@dataclass
class PoseGraphNode:
    pose: np.ndarray


@dataclass
class PoseGraphEdge:
    source_node_id: int
    target_node_id: int
    transformation: np.ndarray
    information: np.ndarray
    uncertain: bool
    weight: float = 1.0          # line process value after optimize() (Open3D keeps it in confidence_)


@dataclass
class _Graph:
    nodes: List[PoseGraphNode] = field(default_factory=list)
    edges: List[PoseGraphEdge] = field(default_factory=list)


@dataclass
class ConvergenceCriteria:       # o3d GlobalOptimizationConvergenceCriteria() defaults
    max_iteration: int = 100
    min_relative_increment: float = 1e-6
    min_relative_residual_increment: float = 1e-6
    min_right_term: float = 1e-6
    min_residual: float = 1e-6
    max_iteration_lm: int = 20
    upper_scale_factor: float = 2.0 / 3.0
    lower_scale_factor: float = 1.0 / 3.0


_GEN = np.zeros((6, 4, 4))
_GEN[0, 1, 2], _GEN[0, 2, 1] = -1, 1
_GEN[1, 2, 0], _GEN[1, 0, 2] = -1, 1
_GEN[2, 0, 1], _GEN[2, 1, 0] = -1, 1
_GEN[3, 0, 3] = _GEN[4, 1, 3] = _GEN[5, 2, 3] = 1


def _lin6(M: np.ndarray) -> np.ndarray:
    """[..., 4, 4] -> [..., 6]: the linearised 6-vector of a near-identity transform"""
    return np.stack([(M[..., 2, 1] - M[..., 1, 2]) / 2, (M[..., 0, 2] - M[..., 2, 0]) / 2, (M[..., 1, 0] - M[..., 0, 1]) / 2,
                     M[..., 0, 3], M[..., 1, 3], M[..., 2, 3]], axis=-1)


def _exp6(d: np.ndarray) -> np.ndarray:
    """[N, 6] -> [N, 4, 4]: Rz(d2) Ry(d1) Rx(d0) and the translation d3:6"""
    cx, sx, cy, sy, cz, sz = np.cos(d[:, 0]), np.sin(d[:, 0]), np.cos(d[:, 1]), np.sin(d[:, 1]), np.cos(d[:, 2]), np.sin(d[:, 2])
    T = np.zeros((d.shape[0], 4, 4))
    T[:, 0, 0], T[:, 0, 1], T[:, 0, 2] = cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx
    T[:, 1, 0], T[:, 1, 1], T[:, 1, 2] = sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx
    T[:, 2, 0], T[:, 2, 1], T[:, 2, 2] = -sy, cy * sx, cy * cx
    T[:, :3, 3] = d[:, 3:6]
    T[:, 3, 3] = 1.0
    return T


def _inv_rigid(T: np.ndarray) -> np.ndarray:
    return np.linalg.inv(T)


class PoseGraph:
    def __init__(self, max_correspondence_distance=0.005, edge_prune_threshold=0.05, preference_loop_closure=0.01,
                 reference_node=0, solver="host"):
        if solver not in ("host", "device"):
            raise ValueError(f"solver {solver!r}: 'host' (the default) or 'device'")
        self.solver = solver
        self.device = 0                  # the GPU the device solver runs on
        self.segment_length = None       # the device solver's cut length (None: solve_plan picks it from N)
        self.pose_graph = _Graph()
        self.max_correspondence_distance = max_correspondence_distance
        self.edge_prune_threshold = edge_prune_threshold
        self.preference_loop_closure = preference_loop_closure
        self.reference_node = reference_node
        self.convergence_criteria = ConvergenceCriteria()
        self.last_log = None

    # ---- the reference's surface -----------------------------------------------------------------
    def add_node(self, extrinsic_matrix):
        self.pose_graph.nodes.append(PoseGraphNode(np.array(self._check_type(extrinsic_matrix), dtype=np.float64)))

    def add_edge(self, motion_matrix, source_id, target_id, uncertain, info=np.eye(6)):
        self.pose_graph.edges.append(PoseGraphEdge(int(source_id), int(target_id), np.array(self._check_type(motion_matrix), dtype=np.float64),
                                                   np.array(self._check_type(info), dtype=np.float64), bool(uncertain)))

    def _check_type(self, matrix):
        if not isinstance(matrix, np.ndarray):
            return matrix.cpu().numpy()
        return matrix

    def optimize(self):
        g = self.pose_graph
        N, E = len(g.nodes), len(g.edges)
        if N == 0 or E == 0:
            return
        for e in g.edges:
            if not (0 <= e.source_node_id < N and 0 <= e.target_node_id < N):
                raise ValueError(f"edge ({e.source_node_id}, {e.target_node_id}) refers to a node outside 0..{N - 1}")
        X = np.stack([n.pose for n in g.nodes])
        src = np.array([e.source_node_id for e in g.edges])
        tgt = np.array([e.target_node_id for e in g.edges])
        L = np.stack([e.information for e in g.edges])
        unc = np.array([e.uncertain for e in g.edges])
        if self.solver == "device":
            fallback = self._optimize_device(X, src, tgt, L, unc)
            if fallback is None:
                return
        Tinv = _inv_rigid(np.stack([e.transformation for e in g.edges]))
        X, lw, log = self._levenberg_marquardt(X, src, tgt, Tinv, L, unc)
        # edges the line process switched off are dropped (uncertain ones only) and the pruned graph is optimised again: Open3D's
        # global_optimization runs optimise -> prune -> optimise
        keep = (~unc) | (lw >= self.edge_prune_threshold)
        if not keep.all():
            for e, w_ in zip(g.edges, lw):
                e.weight = float(w_)
            g.edges = [e for e, k in zip(g.edges, keep) if k]
            X, lw2, log2 = self._levenberg_marquardt(X, src[keep], tgt[keep], Tinv[keep], L[keep], unc[keep])
            log = log + log2 if isinstance(log, list) and isinstance(log2, list) else log2
            lw = lw2
        self.last_log = log
        log["solver"] = "host"
        if self.solver == "device":
            log["fallback"] = fallback
        for n, P in zip(g.nodes, X):
            n.pose = P
        for e, w_ in zip(g.edges, lw):
            e.weight = float(w_)

    # ---- Levenberg-Marquardt with line processes ------------------------------------------------
    def _levenberg_marquardt(self, X, src, tgt, Tinv, L, unc):
        import scipy.sparse as sp
        import scipy.sparse.linalg as spla
        c = self.convergence_criteria
        N, E = X.shape[0], src.shape[0]
        ref = self.reference_node
        mu = 0.0
        if unc.any():
            mu = self.preference_loop_closure * self.max_correspondence_distance ** 2 * float(L[unc, 5, 5].mean())

        def zeta(P):
            return _lin6(Tinv @ _inv_rigid(P[tgt]) @ P[src])                        # [E, 6]

        def quad(z):
            return np.einsum("ei,eij,ej->e", z, L, z)

        def line_process(z):
            lw = np.ones(E)
            if unc.any():
                q = quad(z)
                lw[unc] = (mu / (mu + q[unc])) ** 2
            return lw

        def total(z, lw):
            return float((lw * quad(z)).sum() + (mu * (np.sqrt(lw[unc]) - 1.0) ** 2).sum())

        rows_s, rows_t = 6 * src[:, None] + np.arange(6), 6 * tgt[:, None] + np.arange(6)           # [E, 6] unknown indices
        keep = np.ones(6 * N)
        keep[6 * ref:6 * ref + 6] = 0.0

        def system(P, z, lw):
            A = Tinv @ _inv_rigid(P[tgt])                                           # [E, 4, 4]
            Js = np.stack([_lin6(A @ _GEN[i] @ P[src]) for i in range(6)], axis=2)  # [E, 6, 6], column i = generator i
            W = lw[:, None, None] * L
            JtW = np.swapaxes(Js, 1, 2) @ W                                         # Js^T (l L)
            Hss = JtW @ Js                                                          # = Htt; Hst = Hts = -Hss  (Jt = -Js)
            g_ = np.einsum("eij,ej->ei", JtW, z)                                    # Js^T (l L) r
            b = np.zeros(6 * N)
            np.add.at(b, rows_s, -g_)
            np.add.at(b, rows_t, g_)
            ri = np.concatenate([np.repeat(rows_s, 6, 1), np.repeat(rows_s, 6, 1), np.repeat(rows_t, 6, 1), np.repeat(rows_t, 6, 1)]).ravel()
            ci = np.concatenate([np.tile(rows_s, (1, 6)), np.tile(rows_t, (1, 6)), np.tile(rows_s, (1, 6)), np.tile(rows_t, (1, 6))]).ravel()
            vals = np.concatenate([Hss.reshape(E, 36), -Hss.reshape(E, 36), -Hss.reshape(E, 36), Hss.reshape(E, 36)]).ravel()
            vals = vals * keep[ri] * keep[ci]                                       # the reference node stays where it is
            H = sp.coo_matrix((vals, (ri, ci)), shape=(6 * N, 6 * N)).tocsc()
            H = H + sp.diags(1.0 - keep)
            return H, b * keep

        z = zeta(X)
        lw = line_process(z)
        cur = total(z, lw)
        H, b = system(X, z, lw)
        lam = 1e-5 * float(H.diagonal().max())
        ni, rho = 2.0, 0.0
        stop = float(b.max()) <= c.min_right_term or cur < c.min_residual
        log = dict(iterations=0, residual0=cur)
        it = 0
        eye = sp.identity(6 * N, format="csc")
        while it < c.max_iteration and not stop:
            it += 1
            lm = 0
            while True:
                delta = spla.splu((H + lam * eye).tocsc()).solve(b)
                xnorm = float(np.sqrt((_lin6(X) ** 2).sum()))
                if np.linalg.norm(delta) <= c.min_relative_increment * (xnorm + c.min_relative_increment):
                    stop = True
                if not stop:
                    Xn = _exp6(delta.reshape(N, 6)) @ X
                    zn = zeta(Xn)
                    new = total(zn, lw)
                    rho = (cur - new) / (float(delta @ (lam * delta + b)) + 1e-3)
                    if rho > 0:
                        if cur - new < c.min_relative_residual_increment * cur:
                            stop = True
                        alpha = min(1.0 - (2.0 * rho - 1.0) ** 3, c.upper_scale_factor)
                        lam *= max(c.lower_scale_factor, alpha)
                        ni = 2.0
                        X, z = Xn, zn
                        lw = line_process(z)
                        cur = total(z, lw)
                        H, b = system(X, z, lw)
                        if float(b.max()) <= c.min_right_term:
                            stop = True
                    else:
                        lam *= ni
                        ni *= 2.0
                lm += 1
                if lm > c.max_iteration_lm:
                    stop = True
                if rho > 0 or stop:
                    break
            if cur < c.min_residual:
                stop = True
        log.update(iterations=it, residual=cur)
        return X, lw, log

    # ---- the same on the device ------------------------------------------------------------------
    def _optimize_device(self, X, src, tgt, L, unc):
        """optimize() with the numerical pieces on the GPU.  Returns None when done, or the reason why this graph is the host path's
        (nothing has been changed then)."""
        import torch
        from . import _lib as Lb
        Lb.init(self.device)                                                        # no GPU: BodySlamHipError, there is no CPU fallback
        g = self.pose_graph
        N = X.shape[0]
        plan = solve_plan(N, src, tgt, self.reference_node, self.segment_length)
        if plan["over_capacity"]:
            return plan["reason"]
        if not np.array_equal(L, np.swapaxes(L, 1, 2)):
            return "an information matrix is not symmetric"
        dev = torch.device("cuda", self.device)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(dev)
        Xd = up(X, np.float64)
        Td = up(np.stack([e.transformation for e in g.edges]), np.float64)
        Ld = up(L, np.float64)
        sd, td, ud = up(src, np.int32), up(tgt, np.int32), up(unc, np.int32)
        Xd, lw, log = self._levenberg_marquardt_device(Xd, sd, td, Td, Ld, ud, L, unc, plan)
        keep = (~unc) | (lw >= self.edge_prune_threshold)
        if not keep.all():
            for e, w_ in zip(g.edges, lw):
                e.weight = float(w_)
            g.edges = [e for e, k in zip(g.edges, keep) if k]
            kd = torch.from_numpy(np.flatnonzero(keep)).to(dev)
            plan2 = solve_plan(N, src[keep], tgt[keep], self.reference_node, self.segment_length)      # (fewer edges: never more separators)
            Xd, lw, log = self._levenberg_marquardt_device(Xd, sd[kd].contiguous(), td[kd].contiguous(), Td[kd].contiguous(), Ld[kd].contiguous(),
                                                           ud[kd].contiguous(), L[keep], unc[keep], plan2)
        log["solver"] = "device"
        self.last_log = log
        Xh = Xd.cpu().numpy()                                                       # the poses come back once
        for n, P in zip(g.nodes, Xh):
            n.pose = P
        for e, w_ in zip(g.edges, lw):
            e.weight = float(w_)
        return None

    def _levenberg_marquardt_device(self, X, src, tgt, T, Ld, unc_d, L, unc, plan):
        """_levenberg_marquardt with zeta / line_process / total, system, the solve and the update as device calls: the lambda schedule, rho, ni
        and the stop flags are the lines below, in the same order.  X ... unc_d are device tensors; L, unc the host copies (for mu)."""
        import torch
        from . import _lib as Lb
        c = self.convergence_criteria
        N, E = X.shape[0], src.numel()
        dev = X.device
        mu = 0.0
        if unc.any():
            mu = self.preference_loop_closure * self.max_correspondence_distance ** 2 * float(L[unc, 5, 5].mean())
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)
        segments, sep_node, node_slot = i32(plan["segments"]), i32(plan["sep_node"]), i32(plan["node_slot"])
        adjacent, long_edges, row_ptr, adj = i32(plan["adjacent"]), i32(plan["long_edges"]), i32(plan["row_ptr"]), i32(plan["adj"])
        S, nseg = plan["S"], plan["segments"].shape[0]
        lw, z, q, Hss, g_, cterm = f64(E), f64(E, 6), f64(E), f64(E, 6, 6), f64(E, 6), f64(E)
        zn, qn, ctn = f64(E, 6), f64(E), f64(E)
        D, b, Cc, delta, Xn, terms = f64(N, 6, 6), f64(N, 6), f64(N, 6, 6), f64(N, 6), f64(N, 4, 4), f64(N)
        node_ws, slots = f64(N, Lb.PG_NODE_WORKSPACE), f64(max(nseg, 1), Lb.PG_SLOT_FIELDS)
        M, vec = f64(6 * S, 6 * S), f64(24 * S)
        sc = torch.zeros(8, dtype=torch.float64, device=dev)       # 0 cost, 1 |delta|^2, 2 delta.(lam delta + b), 3 |lin6(X)|^2, 4 max b, 5 max diag H

        def linearise_and_system():
            Lb.pg_linearise(X, T, Ld, src, tgt, unc_d, mu, Lb.PG_LINE_PROCESS | Lb.PG_SYSTEM, lw, z, q, Hss, g_, cterm, sc[0:])
            Lb.pg_assemble(Hss, g_, row_ptr, adj, self.reference_node, D, b, Cc, sc[4:])
            h = sc.cpu().numpy()
            return float(h[0]), float(h[4]), float(h[5])

        cur, bmax, dmax = linearise_and_system()
        lam = 1e-5 * dmax
        ni, rho = 2.0, 0.0
        stop = bmax <= c.min_right_term or cur < c.min_residual
        log = dict(iterations=0, residual0=cur)
        it = 0
        while it < c.max_iteration and not stop:
            it += 1
            lm = 0
            while True:
                Lb.pg_solve(D, b, Cc, Hss, lam, segments, sep_node, node_slot, adjacent, long_edges, Lb.PG_STAGE_ALL, node_ws, slots, M, vec, delta, sc[1:])
                Lb.pg_update(X, delta, Xn, terms, sc[3:])
                Lb.pg_linearise(Xn, T, Ld, src, tgt, unc_d, mu, 0, lw, zn, qn, None, None, ctn, sc[0:])      # the trial step's total(zn, lw)
                h = sc.cpu().numpy()                                             # ONE readback per inner step
                new, dnorm, dot, xnorm = float(h[0]), float(np.sqrt(h[1])), float(h[2]), float(np.sqrt(h[3]))
                if dnorm <= c.min_relative_increment * (xnorm + c.min_relative_increment):
                    stop = True
                if not stop:
                    rho = (cur - new) / (dot + 1e-3)
                    if rho > 0:
                        if cur - new < c.min_relative_residual_increment * cur:
                            stop = True
                        alpha = min(1.0 - (2.0 * rho - 1.0) ** 3, c.upper_scale_factor)
                        lam *= max(c.lower_scale_factor, alpha)
                        ni = 2.0
                        X, Xn = Xn, X
                        cur, bmax, _ = linearise_and_system()                    # line_process, total, system of the accepted step
                        if bmax <= c.min_right_term:
                            stop = True
                    else:
                        lam *= ni
                        ni *= 2.0
                lm += 1
                if lm > c.max_iteration_lm:
                    stop = True
                if rho > 0 or stop:
                    break
            if cur < c.min_residual:
                stop = True
        log.update(iterations=it, residual=cur)
        return X, lw.cpu().numpy(), log                                          # the line-process weights come back once per LM run


PG_MAX_SEPARATORS = 128          # include/bodyslam_hip.h BS_PG_MAX_SEPARATORS


def solve_plan(N, src, tgt, reference_node=0, segment_length=None) -> dict:
    """The plan of the device solve of (H + lambda I) delta = b (one level of substructuring); pure Python, no GPU.

    Separators: the reference node, both endpoints of every edge with |s - t| != 1, then every (segment_length + 1)-th node of any longer run of
    consecutive non-separator indices.  Segments: the maximal runs of consecutive non-separator indices -- block-tridiagonal paths whose only
    outside couplings are to the separator (or the chain end) on their left and right.  ``segment_length=None`` picks max(8, ceil(N / 48)) and
    doubles it while more than PG_MAX_SEPARATORS separators result; a given value is taken as it is.  Returns S, segment_length, sep_node [S],
    node_slot [N] (-1: not a separator), segments [n, 2] = (first node, length), adjacent [k] = nodes i with i and i + 1 both separators,
    long_edges [m, 3] = (edge, source slot, target slot) of the edges with |s - t| >= 2 that do not touch the reference node, the gather CSR
    row_ptr [N + 1] / adj [nnz, 3] = (edge, other endpoint, -1 source / +1 target; ascending edge index, self-edges left out), and
    over_capacity / reason."""
    src, tgt = np.asarray(src, dtype=np.int64).reshape(-1), np.asarray(tgt, dtype=np.int64).reshape(-1)
    N, ref = int(N), int(reference_node)
    if not 0 <= ref < N:
        raise ValueError(f"reference node {ref} outside 0..{N - 1}")
    if src.size and not ((0 <= src).all() and (src < N).all() and (0 <= tgt).all() and (tgt < N).all()):
        raise ValueError(f"an edge refers to a node outside 0..{N - 1}")
    base = np.zeros(N, dtype=bool)
    base[ref] = True
    far = np.abs(src - tgt) != 1
    base[src[far]] = True
    base[tgt[far]] = True

    def cut(length):
        sep = base.copy()
        run = 0
        for i in range(N):
            if sep[i]:
                run = 0
            elif run == length:
                sep[i] = True
                run = 0
            else:
                run += 1
        return sep

    if segment_length is None:
        length = max(8, -(-N // 48))
        sep = cut(length)
        while sep.sum() > PG_MAX_SEPARATORS and length < N:
            length *= 2
            sep = cut(length)
    else:
        length = int(segment_length)
        if length < 1:
            raise ValueError(f"segment_length {length} (>= 1)")
        sep = cut(length)
    sep_node = np.flatnonzero(sep).astype(np.int32)
    S = int(sep_node.size)
    node_slot = np.full(N, -1, dtype=np.int32)
    node_slot[sep_node] = np.arange(S, dtype=np.int32)
    segments = []
    i = 0
    while i < N:
        if sep[i]:
            i += 1
            continue
        j = i
        while j < N and not sep[j]:
            j += 1
        segments.append((i, j - i))
        i = j
    adjacent = [i for i in range(N - 1) if sep[i] and sep[i + 1]]
    long_edges = [(e, node_slot[s], node_slot[t]) for e, (s, t) in enumerate(zip(src, tgt)) if abs(s - t) >= 2 and s != ref and t != ref]
    per_node = [[] for _ in range(N)]
    for e, (s, t) in enumerate(zip(src, tgt)):
        if s != t:
            per_node[s].append((e, t, -1))
            per_node[t].append((e, s, 1))
    row_ptr = np.zeros(N + 1, dtype=np.int32)
    row_ptr[1:] = np.cumsum([len(a) for a in per_node])
    adj = np.array([x for a in per_node for x in a], dtype=np.int32).reshape(-1, 3)
    over = S > PG_MAX_SEPARATORS
    return dict(N=N, E=int(src.size), S=S, segment_length=length, reference_node=ref, sep_node=sep_node, node_slot=node_slot,
                segments=np.array(segments, dtype=np.int32).reshape(-1, 2), adjacent=np.array(adjacent, dtype=np.int32),
                long_edges=np.array(long_edges, dtype=np.int32).reshape(-1, 3), row_ptr=row_ptr, adj=adj, over_capacity=over,
                reason=f"{S} separators exceed the device solver's capacity of {PG_MAX_SEPARATORS}" if over else None)


def update_global_extrinsic(global_pose_graph) -> list:
    """3DM/slam_utils.py:88-90"""
    return [node.pose for node in global_pose_graph.nodes]
