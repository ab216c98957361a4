"""The numpy statement of csrc/posegraph.hip -- TEST INFRASTRUCTURE ONLY.

What ``posegraph.solve_plan`` is consumed by: the same separators, the same block sweep and the same summation order as the kernels, structured
so that the device can be compared stage by stage (edge linearisation, gather assembly, segment slots, reduced matrix, delta, update).  It is
not a copy of oracle/posegraph_ref.py: the dense oracle and the host path of bodyslam_amd/posegraph.py remain the independent checks.
Loop-based on purpose; the graphs of the tests are small."""
import numpy as np

NODE_WS, SLOT = 114, 120


def wave_sum(v):
    """one wave: lane l adds its elements l, l + 64, ... in order, then the xor butterfly 32, 16, ..., 1"""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    p = np.zeros(64)
    for i in range(v.size):
        p[i % 64] += v[i]
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        p = p + p[lanes ^ off]
    return float(p[0])


def rigid_inv(T):
    O = np.zeros((4, 4))
    O[:3, :3] = T[:3, :3].T
    for r in range(3):
        O[r, 3] = -(T[0, r] * T[0, 3] + T[1, r] * T[1, 3] + T[2, r] * T[2, 3])
    O[3, 3] = 1.0
    return O


def lin6(M):
    return np.array([(M[2, 1] - M[1, 2]) / 2, (M[0, 2] - M[2, 0]) / 2, (M[1, 0] - M[0, 1]) / 2, M[0, 3], M[1, 3], M[2, 3]])


def gen_mul(i, X):
    O = np.zeros((4, 4))
    a, b = (1, 2, 0, 0, 1, 2)[i], (2, 0, 1, 3, 3, 3)[i]
    if i < 3:
        O[a], O[b] = -X[b], X[a]
    else:
        O[a] = X[3]
    return O


def linearise(X, T, info, src, tgt, unc, mu, lw=None, system=True):
    """-> dict(z [E, 6], q [E], lw [E], cterm [E], cost, Hss [E, 6, 6], g [E, 6]); lw given: the cost-only mode's weights"""
    E = len(src)
    z, q, l, ct = np.zeros((E, 6)), np.zeros(E), np.ones(E), np.zeros(E)
    Hss, g = np.zeros((E, 6, 6)), np.zeros((E, 6))
    for e in range(E):
        A = rigid_inv(T[e]) @ rigid_inv(X[tgt[e]])
        Xs = X[src[e]]
        z[e] = lin6(A @ Xs)
        q[e] = z[e] @ (info[e] @ z[e])
        if lw is None:
            l[e] = (mu / (mu + q[e])) ** 2 if unc[e] else 1.0
        else:
            l[e] = lw[e]
        ct[e] = l[e] * q[e] + (mu * (np.sqrt(l[e]) - 1.0) ** 2 if unc[e] else 0.0)
        if system:
            Js = np.stack([lin6(A @ gen_mul(i, Xs)) for i in range(6)], axis=1)
            JtW = Js.T @ (l[e] * info[e])
            Hss[e], g[e] = JtW @ Js, JtW @ z[e]
    return dict(z=z, q=q, lw=l, cterm=ct, cost=wave_sum(ct), Hss=Hss, g=g)


def assemble(plan, Hss, g):
    """-> D [N, 6, 6], b [N, 6], Cc [N, 6, 6] (Cc[i] = H[i][i + 1]), max b, max diag H"""
    N, ref = plan["N"], plan["reference_node"]
    D, b, Cc = np.zeros((N, 6, 6)), np.zeros((N, 6)), np.zeros((N, 6, 6))
    for n in range(N):
        for k in range(plan["row_ptr"][n], plan["row_ptr"][n + 1]):
            e, o, sg = plan["adj"][k]
            D[n] += Hss[e]
            b[n] += -g[e] if sg < 0 else g[e]
            if o == n + 1:
                Cc[n] += -Hss[e]
        if n == ref:
            D[n], b[n] = np.eye(6), 0.0
        if n == ref or n + 1 == ref:
            Cc[n] = 0.0
    return D, b, Cc, float(b.max()), float(np.max(np.diagonal(D, axis1=1, axis2=2)))


def chol6(A):
    L = np.zeros((6, 6))
    for j in range(6):
        s = A[j, j]
        for k in range(j):
            s -= L[j, k] * L[j, k]
        d = np.sqrt(s)
        L[j, j] = d
        for i in range(j + 1, 6):
            a = A[i, j]
            for k in range(j):
                a -= L[i, k] * L[j, k]
            L[i, j] = a / d
    return L


def lsolve6(L, B):
    B = np.asarray(B, dtype=np.float64)
    Y = np.zeros_like(B)
    for i in range(6):
        a = B[i].copy()
        for k in range(i):
            a = a - L[i, k] * Y[k]
        Y[i] = a / L[i, i]
    return Y


def sweep(plan, D, b, Cc, lam):
    """stage A -> node_ws [N, 114] (L | GU | GF | gb per interior node), slots [n_segments, 120] (Saa | Sca | Scc | ra | rc)"""
    N = plan["N"]
    ws, slots = np.zeros((N, NODE_WS)), np.zeros((len(plan["segments"]), SLOT))
    for si, (p, m) in enumerate(plan["segments"]):
        At, bt = D[p] + lam * np.eye(6), b[p].copy()
        F = Cc[p - 1].T.copy() if p > 0 else np.zeros((6, 6))
        Saa, ra = np.zeros((6, 6)), np.zeros(6)
        for k in range(p, p + m):
            L = chol6(At)
            U = Cc[k] if k < N - 1 else np.zeros((6, 6))
            GU, GF, gb = lsolve6(L, U), lsolve6(L, F), lsolve6(L, bt)
            ws[k] = np.concatenate([L.ravel(), GU.ravel(), GF.ravel(), gb])
            Saa -= GF.T @ GF
            ra -= GF.T @ gb
            if k < p + m - 1:
                At = D[k + 1] + lam * np.eye(6) - GU.T @ GU
                F = -(GU.T @ GF)
                bt = b[k + 1] - GU.T @ gb
            else:
                slots[si] = np.concatenate([Saa.ravel(), (-(GU.T @ GF)).ravel(), (-(GU.T @ GU)).ravel(), ra, -(GU.T @ gb)])
    return ws, slots


def reduced(plan, D, b, Cc, long_blocks, slots, lam):
    """stage B, first half -> M [6 S, 6 S], r [6 S]; long_blocks[k] = H[s][t] of plan["long_edges"][k] (the kernel's -Hss[edge])"""
    S, N = plan["S"], plan["N"]
    M, r = np.zeros((6 * S, 6 * S)), np.zeros(6 * S)
    blk = lambda i, j: (slice(6 * i, 6 * i + 6), slice(6 * j, 6 * j + 6))
    for s, node in enumerate(plan["sep_node"]):
        M[blk(s, s)] = D[node] + lam * np.eye(6)
        r[6 * s:6 * s + 6] = b[node]
    for node in plan["adjacent"]:
        sa, sb = plan["node_slot"][node], plan["node_slot"][node + 1]
        M[blk(sa, sb)], M[blk(sb, sa)] = Cc[node], Cc[node].T
    for k, (_, ss, st) in enumerate(plan["long_edges"]):
        M[blk(ss, st)] += long_blocks[k]
        M[blk(st, ss)] += long_blocks[k]
    for si, (p, m) in enumerate(plan["segments"]):
        sa = plan["node_slot"][p - 1] if p > 0 else -1
        sc = plan["node_slot"][p + m] if p + m < N else -1
        sl = slots[si]
        if sa >= 0:
            M[blk(sa, sa)] += sl[0:36].reshape(6, 6)
            r[6 * sa:6 * sa + 6] += sl[108:114]
        if sc >= 0:
            M[blk(sc, sc)] += sl[72:108].reshape(6, 6)
            r[6 * sc:6 * sc + 6] += sl[114:120]
        if sa >= 0 and sc >= 0:
            M[blk(sc, sa)] += sl[36:72].reshape(6, 6)
            M[blk(sa, sc)] += sl[36:72].reshape(6, 6).T
    return M, r


def dense_solve(M, r):
    """stage B, second half: left-looking Cholesky (the sum over k ascending), L y = r, L^T x = y"""
    n = M.shape[0]
    Lt = np.zeros((n, n))                       # Lt[k, i] = L(i, k), the kernel's in-place layout
    for j in range(n):
        col = M[j, j:].copy()
        for k in range(j):
            col -= Lt[k, j:] * Lt[k, j]
        d = np.sqrt(col[0])
        Lt[j, j], Lt[j, j + 1:] = d, col[1:] / d
    rv, y, x = r.copy(), np.zeros(n), np.zeros(n)
    for j in range(n):
        y[j] = rv[j] / Lt[j, j]
        rv[j + 1:] -= Lt[j, j + 1:] * y[j]
    for j in range(n - 1, -1, -1):
        x[j] = y[j] / Lt[j, j]
        y[:j] -= Lt[:j, j] * x[j]
    return x


def backsub(plan, ws, xsep):
    """stage C -> delta [N, 6]"""
    N = plan["N"]
    delta = np.zeros((N, 6))
    delta[plan["sep_node"]] = xsep.reshape(-1, 6)
    for (p, m) in plan["segments"]:
        xa = delta[p - 1] if p > 0 else np.zeros(6)
        xn = delta[p + m] if p + m < N else np.zeros(6)
        for k in range(p + m - 1, p - 1, -1):
            L, GU, GF, gb = ws[k, :36].reshape(6, 6), ws[k, 36:72].reshape(6, 6), ws[k, 72:108].reshape(6, 6), ws[k, 108:]
            x = gb - GU @ xn - GF @ xa
            for i in range(5, -1, -1):
                a = x[i]
                for j in range(i + 1, 6):
                    a -= L[j, i] * x[j]
                x[i] = a / L[i, i]
            delta[k] = x
            xn = x
    return delta


def solve(plan, D, b, Cc, long_blocks, lam):
    """-> dict(node_ws, slots, M, r, delta [N, 6], sums = (|delta|^2, delta . (lam delta + b)))"""
    ws, slots = sweep(plan, D, b, Cc, lam)
    M, r = reduced(plan, D, b, Cc, long_blocks, slots, lam)
    delta = backsub(plan, ws, dense_solve(M, r))
    d, bb = delta.ravel(), b.ravel()
    return dict(node_ws=ws, slots=slots, M=M, r=r, delta=delta, sums=(wave_sum(d * d), wave_sum(d * (lam * d + bb))))


def blocks_from_dense(plan, H, b):
    """D, b, Cc and the long-edge blocks of a dense 6N x 6N matrix (the reference node's rows already identity / zero, no lambda); with several
    long edges on one pair of nodes the first of them gets the pair's whole block"""
    N = plan["N"]
    B = lambda i, j: H[6 * i:6 * i + 6, 6 * j:6 * j + 6]
    D = np.stack([B(i, i) for i in range(N)])
    Cc = np.stack([B(i, i + 1) if i < N - 1 else np.zeros((6, 6)) for i in range(N)])
    seen, blocks = set(), []
    for (_, ss, st) in plan["long_edges"]:
        key = (min(ss, st), max(ss, st))
        s, t = plan["sep_node"][ss], plan["sep_node"][st]
        blocks.append(np.zeros((6, 6)) if key in seen else B(s, t).copy())
        seen.add(key)
    return D, np.asarray(b, dtype=np.float64).reshape(N, 6), Cc, blocks


def exp6(d):
    cx, sx, cy, sy, cz, sz = np.cos(d[0]), np.sin(d[0]), np.cos(d[1]), np.sin(d[1]), np.cos(d[2]), np.sin(d[2])
    T = np.zeros((4, 4))
    T[0, :3] = cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx
    T[1, :3] = sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx
    T[2, :3] = -sy, cy * sx, cy * cx
    T[:3, 3] = d[3:6]
    T[3, 3] = 1.0
    return T


def update(X, delta):
    """-> Xn [N, 4, 4], sum |lin6(X)|^2 of the input poses"""
    Xn = np.stack([exp6(delta[i]) @ X[i] for i in range(len(X))])
    return Xn, wave_sum([lin6(P) @ lin6(P) for P in X])
