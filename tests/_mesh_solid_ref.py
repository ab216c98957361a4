"""Numpy / Python statement of "is this mesh a solid" (csrc/mesh_solid.hip, bodyslam_amd/mesh.py) -- TEST
INFRASTRUCTURE ONLY.

Restated from the documented meaning of Open3D's TriangleMesh.get_non_manifold_vertices, is_vertex_manifold,
get_self_intersecting_triangles, is_self_intersecting, is_intersecting, is_watertight, get_volume; nothing here comes from Open3D's code.
Parity with Open3D is UNPINNED.  Python floats are IEEE doubles and do not contract; every operation and order is written out: the device
must return these results, equal, whatever grid it walks.

Vertex fans.  The elements are the corners 3 t + c of the VALID triangles.  Half-edge h = 3 t + c (a = tri[t][c] -> b = tri[t][(c + 1) % 3])
of edge e with first triangle u = edge_first_triangle[e] joins the corner of a in t with the corner of a in u, and likewise for b.  A
vertex is NON-MANIFOLD when its corners form more than one class.  An edge of three or more triangles joins all of them (they all meet the
edge's first triangle), so its end points are not reported for that reason alone; a vertex in no valid triangle has no class.

Intersecting pairs.  Only KEPT triangles (tests/_mesh_ops_ref.py triangle_geometry) take part.  Self mode: pairs i < j that share no vertex
INDEX; two meshes: every pair (i of A, j of B).  A vertex id is (mesh, row), A before B.  Candidates: the closed fp32 boxes overlap.
  orient3d(a, b, c, d): sort the four ids ascending (P0 .. P3), u = P1 - P0, v = P2 - P0, w = P3 - P0 in fp64 (the fp32 coordinates
  converted), det = (ux (vy wz - vz wy) + uy (vz wx - vx wz)) + uz (vx wy - vy wx); the sign is sign(det) times the parity of the sort.
  orient2d(a, b, c) on two coordinates (X, Y): sort the three ids, u = P1 - P0, v = P2 - P0, det = ux vy - uy vx, sign times parity.
  s1[k] = orient3d(T2[0], T2[1], T2[2], T1[k]) and s2[k] = orient3d(T1[0], T1[1], T1[2], T2[k]).  All of s1 (or of s2) strictly on one
  side: no.  All of s1 or all of s2 zero: the coplanar test.  Otherwise (Guigue & Devillers 2003, restated): T1 is rotated so that its
  first vertex is ALONE -- the first k (0, 1, 2) with s > 0 and both others <= 0, or s < 0 and both others >= 0, or s = 0 and the others
  strictly on one side --; when the alone vertex lies on the non-positive side the last two vertices of T2 are swapped.  The same for T2
  against s2, swapping the last two vertices of T1.  Then: yes iff orient3d(p1, q1, p2, q2) <= 0 and orient3d(p1, r1, r2, p2) <= 0.
  Coplanar: n = the fp64 cross product of the LOWER triangle (T1); drop the axis of the largest |n| (the first on ties), keep the other
  two in ascending order.  o = orient2d of a triangle; an edge (a, b) of it separates when orient2d(a, b, x) o < 0 for all three x of the
  other triangle.  yes iff none of the six edges separates (the closed triangles of a plane are disjoint iff an edge line of one has the
  other strictly beyond it).
Output: int32 [n, 2] rows (i, j) in ascending order of i << 32 | j.

Volume.  parent[t] = the smallest triangle of t's edge-connected component, ref = v[tri[parent[t]][0]]; a, b, c = the fp64 differences of
the triangle's vertices to ref; vol6[t] = (ax (by cz - bz cy) + ay (bz cx - bx cz)) + az (bx cy - by cx) for a kept triangle, 0 otherwise;
the volume of a cluster = wave_sum(vol6 of its triangles, ascending) * (1 / 6), NaN when an edge of the cluster does not have exactly two
triangles or is not run once in each direction.
"""
from fractions import Fraction

import numpy as np

import _mesh_ops_ref as R

f32, f64, i32, i64 = np.float32, np.float64, np.int32, np.int64


# ---- vertex fans ---------------------------------------------------------------------------------------------------------------------------
def non_manifold_vertices(vertices, triangles):
    """int32 [n]: the vertices whose corners form more than one class, ascending"""
    v, t = R._vt(vertices, triangles)
    table = R.edge_table(v, t)
    eoh, eft = table["edge_of_half"], table["edge_first_triangle"]
    parent = list(range(3 * len(t)))

    def root(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for h in np.nonzero(eoh >= 0)[0]:
        tt, c = int(h) // 3, int(h) % 3
        u = int(eft[eoh[h]])
        for vert in (int(t[tt, c]), int(t[tt, (c + 1) % 3])):
            x = 3 * tt + [int(k) for k in t[tt]].index(vert)
            y = 3 * u + [int(k) for k in t[u]].index(vert)
            r, s = root(x), root(y)
            if r != s:
                parent[max(r, s)] = min(r, s)
    count = np.zeros(len(v), i64)
    for x in range(3 * len(t)):
        if eoh[x] >= 0 and root(x) == x:
            count[t[x // 3, x % 3]] += 1
    return np.nonzero(count > 1)[0].astype(i32)


def non_manifold_vertices_bfs(vertices, triangles):
    """the same by a plain search per vertex: the valid triangles at a vertex, joined when they share an edge that contains it"""
    v, t = R._vt(vertices, triangles)
    valid = R.valid_triangles(len(v), t)
    at = {}
    for k in np.nonzero(valid)[0]:
        for a in t[k]:
            at.setdefault(int(a), []).append(int(k))
    out = []
    for a, tris in at.items():
        seen, todo = {tris[0]}, [tris[0]]
        while todo:
            x = todo.pop()
            for y in tris:
                if y not in seen and len((set(t[x].tolist()) & set(t[y].tolist())) - {a}) >= 1:
                    seen.add(y)
                    todo.append(y)
        if len(seen) < len(tris):
            out.append(a)
    return np.array(sorted(out), i32).reshape(-1)


# ---- the predicate -------------------------------------------------------------------------------------------------------------------------
def _sgn(x):
    return (x > 0.0) - (x < 0.0)


def orient3d(a, b, c, d):
    """a .. d: (id, x, y, z) with Python floats -> -1, 0, 1"""
    p = [a, b, c, d]
    par = 1
    for i, j in ((0, 1), (2, 3), (0, 2), (1, 3), (1, 2)):
        if p[j][0] < p[i][0]:
            p[i], p[j] = p[j], p[i]
            par = -par
    ux, uy, uz = p[1][1] - p[0][1], p[1][2] - p[0][2], p[1][3] - p[0][3]
    vx, vy, vz = p[2][1] - p[0][1], p[2][2] - p[0][2], p[2][3] - p[0][3]
    wx, wy, wz = p[3][1] - p[0][1], p[3][2] - p[0][2], p[3][3] - p[0][3]
    det = (ux * (vy * wz - vz * wy) + uy * (vz * wx - vx * wz)) + uz * (vx * wy - vy * wx)
    return _sgn(det) * par


def orient2d(a, b, c, X, Y):
    p = [a, b, c]
    par = 1
    for i, j in ((0, 1), (1, 2), (0, 1)):
        if p[j][0] < p[i][0]:
            p[i], p[j] = p[j], p[i]
            par = -par
    ux, uy = p[1][X] - p[0][X], p[1][Y] - p[0][Y]
    vx, vy = p[2][X] - p[0][X], p[2][Y] - p[0][Y]
    return _sgn(ux * vy - uy * vx) * par


def _alone(s):
    """-> (k, side): the first alone vertex of the signs s, and the side it lies on (+1 / -1)"""
    for k in range(3):
        a, b = s[(k + 1) % 3], s[(k + 2) % 3]
        if s[k] > 0 and a <= 0 and b <= 0:
            return k, 1
        if s[k] < 0 and a >= 0 and b >= 0:
            return k, -1
        if s[k] == 0 and a * b > 0:
            return k, -a
    raise AssertionError(s)


def _coplanar(T1, T2):
    (_, ax, ay, az), (_, bx, by, bz), (_, cx, cy, cz) = T1
    e1x, e1y, e1z, e2x, e2y, e2z = bx - ax, by - ay, bz - az, cx - ax, cy - ay, cz - az
    n = (abs(e1y * e2z - e1z * e2y), abs(e1z * e2x - e1x * e2z), abs(e1x * e2y - e1y * e2x))
    drop = 0
    if n[1] > n[drop]:
        drop = 1
    if n[2] > n[drop]:
        drop = 2
    X, Y = [k + 1 for k in range(3) if k != drop]
    for A, B in ((T1, T2), (T2, T1)):
        o = orient2d(A[0], A[1], A[2], X, Y)
        for k in range(3):
            a, b = A[k], A[(k + 1) % 3]
            if all(orient2d(a, b, x, X, Y) * o < 0 for x in B):
                return False
    return True


def tri_tri(T1, T2):
    """T1, T2: three (id, x, y, z) each, every id distinct; T1 the lower triangle -> bool: the closed triangles meet, as stated above"""
    s1 = [orient3d(T2[0], T2[1], T2[2], x) for x in T1]
    if min(s1) > 0 or max(s1) < 0:
        return False
    s2 = [orient3d(T1[0], T1[1], T1[2], x) for x in T2]
    if min(s2) > 0 or max(s2) < 0:
        return False
    if s1 == [0, 0, 0] or s2 == [0, 0, 0]:
        return _coplanar(T1, T2)
    k, side = _alone(s1)
    p1, q1, r1 = T1[k], T1[(k + 1) % 3], T1[(k + 2) % 3]
    p2, q2, r2 = T2
    if side < 0:
        q2, r2 = r2, q2
    s2 = [s2[0], s2[2], s2[1]] if side < 0 else s2
    T2 = (p2, q2, r2)
    k, side = _alone(s2)
    p2, q2, r2 = T2[k], T2[(k + 1) % 3], T2[(k + 2) % 3]
    if side < 0:
        q1, r1 = r1, q1
    return orient3d(p1, q1, p2, q2) <= 0 and orient3d(p1, r1, r2, p2) <= 0


def _tagged(v, t, mesh):
    """the triangles of a mesh as ((id, x, y, z) x 3) with Python floats; id = mesh << 32 | row"""
    vv = v.astype(f64).tolist()
    return [tuple(((mesh << 32) | int(a), *vv[int(a)]) for a in row) for row in np.clip(t, 0, max(len(v) - 1, 0))]


def intersecting_pairs(vertices, triangles, vertices_b=None, triangles_b=None, predicate=None):
    """-> int32 [n, 2]: the pairs in ascending (i, j); one mesh: i < j sharing no vertex index; two: every (i of A, j of B)"""
    predicate = tri_tri if predicate is None else predicate
    va, ta = R._vt(vertices, triangles)
    self_mode = vertices_b is None
    vb, tb = (va, ta) if self_mode else R._vt(vertices_b, triangles_b)
    out = []
    ka, kb = R.triangle_geometry(va, ta)[1], R.triangle_geometry(vb, tb)[1]
    if ka.any() and kb.any():
        def boxes(v, t, k):
            p = v[np.where(k[:, None], t, 0)]
            return p.min(1), p.max(1)
        lo_a, hi_a = boxes(va, ta, ka)
        lo_b, hi_b = boxes(vb, tb, kb)
        A, B = _tagged(va, ta, 0), _tagged(vb, tb, 0 if self_mode else 1)
        for i in np.nonzero(ka)[0]:
            cand = kb & (lo_b <= hi_a[i]).all(1) & (hi_b >= lo_a[i]).all(1)
            if self_mode:
                cand &= np.arange(len(tb)) > i
                cand &= ~(tb[:, :, None] == ta[i][None, None, :]).any((1, 2))
            for j in np.nonzero(cand)[0]:
                if predicate(A[i], B[j]):
                    out.append((int(i), int(j)))
    return np.array(out, i32).reshape(-1, 2)


# ---- the exact oracle: Python integers and fractions, for integer coordinates ---------------------------------------------------------------
def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _crs(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dt(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _o2(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def _seg_seg_2d(p, q, a, b):
    d1, d2, d3, d4 = _o2(a, b, p), _o2(a, b, q), _o2(p, q, a), _o2(p, q, b)
    if ((d1 > 0 and d2 < 0) or (d1 < 0 and d2 > 0)) and ((d3 > 0 and d4 < 0) or (d3 < 0 and d4 > 0)):
        return True

    def on(a, b, x):          # x collinear with a b: inside the closed segment
        return min(a[0], b[0]) <= x[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= x[1] <= max(a[1], b[1])
    return (d1 == 0 and on(a, b, p)) or (d2 == 0 and on(a, b, q)) or (d3 == 0 and on(p, q, a)) or (d4 == 0 and on(p, q, b))


def _in_tri_2d(x, a, b, c):
    d = (_o2(a, b, x), _o2(b, c, x), _o2(c, a, x))
    return min(d) >= 0 or max(d) <= 0


def exact_segment_triangle(p, q, a, b, c):
    """the closed segment p q meets the closed triangle a b c (integer or Fraction coordinates, a b c not collinear)"""
    n = _crs(_sub(b, a), _sub(c, a))
    dp, dq = _dt(n, _sub(p, a)), _dt(n, _sub(q, a))
    if (dp > 0 and dq > 0) or (dp < 0 and dq < 0):
        return False
    if dp == 0 and dq == 0:
        k = max(range(3), key=lambda i: abs(n[i]))
        P = [tuple(x[i] for i in range(3) if i != k) for x in (p, q, a, b, c)]
        return (_in_tri_2d(P[0], *P[2:]) or _in_tri_2d(P[1], *P[2:]) or _seg_seg_2d(P[0], P[1], P[2], P[3]) or
                _seg_seg_2d(P[0], P[1], P[3], P[4]) or _seg_seg_2d(P[0], P[1], P[4], P[2]))
    s = Fraction(dp, dp - dq)
    x = tuple(p[i] + s * (q[i] - p[i]) for i in range(3))
    d = [_dt(n, _crs(_sub(e1, e0), _sub(x, e0))) for e0, e1 in ((a, b), (b, c), (c, a))]
    return min(d) >= 0


def exact_tri_tri(A, B):
    """two closed triangles meet iff an edge of one meets the other triangle"""
    return any(exact_segment_triangle(A[k], A[(k + 1) % 3], *B) or exact_segment_triangle(B[k], B[(k + 1) % 3], *A) for k in range(3))


def exact_predicate(T1, T2):
    """exact_tri_tri as a predicate of intersecting_pairs: integer coordinates only"""
    A, B = ([tuple(int(c) for c in x[1:]) for x in T] for T in (T1, T2))
    assert all(float(c) == f for T, I in ((T1, A), (T2, B)) for x, y in zip(T, I) for c, f in zip(y, x[1:]))
    return exact_tri_tri(A, B)


# ---- volume --------------------------------------------------------------------------------------------------------------------------------
def component_volumes(vertices, triangles):
    """-> (triangle_clusters int32 [T], volume float64 [C])"""
    v, t = R._vt(vertices, triangles)
    T = len(t)
    table = R.edge_table(v, t)
    cluster = R.cluster_connected_triangles(v, t)[0]
    label = R.component_labels(table, T)
    kept = R.triangle_geometry(v, t)[1]
    C = int(cluster.max()) + 1 if T else 0
    vol6 = np.zeros(T, f64)
    d = v.astype(f64)
    for k in np.nonzero(kept)[0]:
        ref = d[t[label[k], 0]]
        (ax, ay, az), (bx, by, bz), (cx, cy, cz) = ((float(x) for x in (d[t[k, c]] - ref)) for c in range(3))
        vol6[k] = (ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz)) + az * (bx * cy - by * cx)
    eoh = table["edge_of_half"]
    bad_half = (eoh >= 0) & ((table["edge_count"][eoh] != 2) | (table["edge_forward"][eoh] != 1)) if T else np.zeros(0, bool)
    out = np.empty(C, f64)
    for c in range(C):
        rows = cluster == c
        out[c] = np.nan if bad_half.reshape(-1, 3)[rows].any() else R.wave_sum(vol6[rows]) * (1.0 / 6.0)
    return cluster, out


def orient_outward(vertices, triangles):
    """-> (triangles int32 [T, 3], flipped bool [T], solid bool [C]): tests/_orient_ref.py orient_triangles, then the last two corners of
    every triangle of a cluster with a negative volume swapped; solid: the cluster has a volume (closed and consistently wound)"""
    import _orient_ref as O
    v, t = R._vt(vertices, triangles)
    out, flipped = O.orient_triangles(v, t)[:2]
    out, flipped = np.asarray(out).astype(i32).copy(), np.asarray(flipped).astype(bool).copy()
    cluster, vol = component_volumes(v, out)
    turn = (cluster >= 0) & (vol[np.maximum(cluster, 0)] < 0.0) if len(vol) else np.zeros(len(t), bool)
    out[turn] = out[turn][:, [0, 2, 1]]
    return out, flipped ^ turn, ~np.isnan(vol)


def check_solid(vertices, triangles):
    v, t = R._vt(vertices, triangles)
    table = R.edge_table(v, t)
    nmv, pairs = non_manifold_vertices(v, t), intersecting_pairs(v, t)
    d = dict(edge_manifold=R.is_edge_manifold(table, False), vertex_manifold=len(nmv) == 0, self_intersecting=len(pairs) > 0,
             consistently_oriented=R.is_consistently_oriented(table), n_boundary_edges=len(R.boundary_edges(table)),
             n_non_manifold_edges=len(R.non_manifold_edges(table)), n_non_manifold_vertices=len(nmv), n_intersecting_pairs=len(pairs))
    d["watertight"] = d["edge_manifold"] and d["vertex_manifold"] and not d["self_intersecting"]
    d["volume"] = abs(float(R.wave_sum(component_volumes(v, t)[1]))) if d["watertight"] and d["consistently_oriented"] else None
    return d
