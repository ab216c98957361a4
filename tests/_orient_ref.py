"""Numpy statement of the consistent orientation of normals along a minimum spanning tree and of the winding of a mesh (csrc/orient.hip,
csrc/mesh_ops.hip bs_mesh_orient_*, csrc/union_parity.h, bodyslam_amd/pointcloud.py, bodyslam_amd/mesh.py) -- TEST
INFRASTRUCTURE ONLY, independent of the product code.

The roles are Open3D's ``PointCloud.orient_normals_consistent_tangent_plane`` (Hoppe et al. 1992), ``TriangleMesh.orient_triangles`` and
``TriangleMesh.is_orientable``.  Open3D is not available: **parity unpinned**; the text below restates the documented meaning and is the
contract.

normals   A point is VALID when its coordinates are finite and its normal is finite and not all zero.  The undirected edge {i, j}, i != j,
          exists when j is in row i of `_knn_ref.knn_brute(cloud, cloud, k)` or i in row j, and both ends are valid; k counts the point
          itself, 2 <= k <= 32.  In float64, one product and one add each, on the float32 normals: d = (ax bx + ay by) + az bz; the weight
          w = float32(max(1 - |d|, 0)); the sign link s = (d < 0).  Edges are ordered by (the bits of w as uint32, min(i, j), max(i, j)):
          a total order, so the minimum spanning forest is unique (Kruskal below).  No Delaunay edges are added (the departure from
          Open3D): a disconnected graph gives several trees.  Per tree the seed is the valid point of largest float32 z (-0 equals +0), ties
          to the lowest index; it is flipped when (nx dx + ny dy) + nz dz < 0 in float64; flip(x) = the seed's flip xor the parity of the s
          along the tree path from x to the seed.  A flipped normal has its three sign bits toggled; every other row comes back bit for bit.
winding   A triangle is VALID when its indices lie in [0, V) and are pairwise distinct.  Half-edge 3 t + c runs from tri[t][c] to
          tri[t][(c + 1) % 3]; an undirected edge with exactly two half-edges links their triangles t, u with s = (the number of the two
          that run from the lower to the higher vertex != 1): flip(t) xor flip(u) = s.  Edges with any other count link nothing and connect
          nothing.  Components are those of the links, numbered in the order of their first triangle (-1: invalid).  A component is
          ORIENTABLE when one flip assignment satisfies all its links; then its smallest triangle keeps its winding, flip = the parity of
          any path to it, and a flipped [a, b, c] becomes [a, c, b].  A component that is not is returned unchanged.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_ref as K  # noqa: E402

f32, f64 = np.float32, np.float64
K_MIN, K_MAX = 2, 32
SIGN = np.uint32(0x80000000)


# ---- normals -----------------------------------------------------------------------------------------------------------------------------
def valid_rows(points, normals):
    p, n = np.asarray(points).astype(f32), np.asarray(normals).astype(f32)
    return np.isfinite(p).all(1) & np.isfinite(n).all(1) & (n != 0).any(1)


def dot64(a, b):
    a, b = np.asarray(a).astype(f64), np.asarray(b).astype(f64)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def knn_edges(points, normals, k):
    """the unique edges -> (lo int64 [E], hi int64 [E], w float32 [E], s bool [E]), in no particular order"""
    if not K_MIN <= k <= K_MAX:
        raise ValueError(f"k = {k}")
    p, nr = np.asarray(points).astype(f32), np.asarray(normals).astype(f32)
    n = len(p)
    ok = valid_rows(p, nr)
    idx, _, cnt = K.knn_brute(p, p, k)
    i = np.repeat(np.arange(n), k)
    j = idx.reshape(-1).astype(np.int64)
    use = (np.tile(np.arange(k), n) < np.repeat(cnt, k)) & (j >= 0) & (j != i)
    i, j = i[use], j[use]
    use = ok[i] & ok[j]
    i, j = i[use], j[use]
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    _, first = np.unique(lo * n + hi, return_index=True)
    lo, hi = lo[first], hi[first]
    with np.errstate(invalid="ignore"):
        d = dot64(nr[lo], nr[hi])
        w = np.maximum(1.0 - np.abs(d), 0.0).astype(f32)
    return lo, hi, w, d < 0


def spanning_forest(n, lo, hi, w):
    """Kruskal under the total order (bits of w, lo, hi) -> the positions of the forest's edges, in that order"""
    order = np.lexsort((hi, lo, np.ascontiguousarray(w).view(np.uint32)))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    tree = []
    for e in order:
        a, b = find(int(lo[e])), find(int(hi[e]))
        if a != b:
            parent[max(a, b)] = min(a, b)
            tree.append(int(e))
    return np.array(tree, np.int64)


def orient_normals(points, normals, k, direction=(0.0, 0.0, 1.0), details=False):
    """-> (normals float32 [n, 3], flipped bool [n], components); details: also (lo, hi, w, s, the forest's edge positions, the seeds)"""
    p, nr = np.asarray(points).astype(f32), np.asarray(normals).astype(f32)
    n = len(p)
    ok = valid_rows(p, nr)
    lo, hi, w, s = knn_edges(p, nr, k)
    tree = spanning_forest(n, lo, hi, w)
    nbr = [[] for _ in range(n)]
    for e in tree:
        a, b, se = int(lo[e]), int(hi[e]), bool(s[e])
        nbr[a].append((b, se))
        nbr[b].append((a, se))
    label = np.full(n, -1, np.int64)
    members = []
    for x in range(n):                                                        # components in ascending order of their smallest index
        if not ok[x] or label[x] >= 0:
            continue
        c, stack = len(members), [x]
        label[x] = c
        got = [x]
        while stack:
            a = stack.pop()
            for b, _ in nbr[a]:
                if label[b] < 0:
                    label[b] = c
                    got.append(b)
                    stack.append(b)
        members.append(np.sort(np.array(got, np.int64)))
    d = np.asarray(direction, f64)
    flipped = np.zeros(n, bool)
    seeds = []
    for m in members:
        seed = int(m[np.argmax(p[m, 2])])                                      # the first maximum: ties to the lowest index; -0 == +0
        seeds.append(seed)
        seen = {seed}
        flipped[seed] = bool(dot64(nr[seed], d) < 0)
        stack = [seed]
        while stack:
            a = stack.pop()
            for b, se in nbr[a]:
                if b not in seen:
                    seen.add(b)
                    flipped[b] = flipped[a] ^ se
                    stack.append(b)
    out = nr.copy()
    bits = out.view(np.uint32)
    bits[flipped] ^= SIGN
    if details:
        return out, flipped, len(members), (lo, hi, w, s, tree, np.array(seeds, np.int64))
    return out, flipped, len(members)


def axis_rule(normals):
    """estimate_normals' rule without direction or camera: the component of largest magnitude (the first such) is made positive"""
    v = np.asarray(normals).astype(f32)
    dot = v[np.arange(len(v)), np.argmax(np.abs(v), 1)]
    return np.where((dot < 0)[:, None], -v, v)


# ---- winding -----------------------------------------------------------------------------------------------------------------------------
def triangle_links(n_vertices, triangles):
    """-> (valid bool [T], links [(t, u, s)] with t > u the second and first triangle of every two-triangle edge)"""
    tri = np.asarray(triangles).astype(np.int64).reshape(-1, 3)
    valid = ((tri >= 0) & (tri < n_vertices)).all(1) & (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    table = {}
    for t in np.nonzero(valid)[0]:
        for c in range(3):
            a, b = int(tri[t, c]), int(tri[t, (c + 1) % 3])
            table.setdefault((min(a, b), max(a, b)), []).append((int(t), a < b))
    links = []
    for halves in table.values():
        if len(halves) == 2:
            (u, fu), (t, ft) = halves
            links.append((t, u, (int(fu) + int(ft)) != 1))
    return valid, links


def orient_triangles(vertices, triangles):
    """-> (triangles int32 [T, 3], flipped bool [T], orientable bool, triangle_components int32 [T], component_orientable bool [C])"""
    tri = np.asarray(triangles).astype(np.int32).reshape(-1, 3)
    T = len(tri)
    valid, links = triangle_links(len(np.asarray(vertices).reshape(-1, 3)), tri)
    nbr = [[] for _ in range(T)]
    for t, u, s in links:
        nbr[t].append((u, s))
        nbr[u].append((t, s))
    comp = np.full(T, -1, np.int32)
    parity = np.zeros(T, bool)
    n_comp = 0
    for x in range(T):
        if not valid[x] or comp[x] >= 0:
            continue
        comp[x] = n_comp
        stack = [x]
        while stack:
            a = stack.pop()
            for b, s in nbr[a]:
                if comp[b] < 0:
                    comp[b] = n_comp
                    parity[b] = parity[a] ^ s
                    stack.append(b)
        n_comp += 1
    verdict = np.ones(n_comp, bool)
    for t, u, s in links:
        if (parity[t] ^ parity[u]) != s:
            verdict[comp[t]] = False
    flipped = valid & parity
    flipped[valid] &= verdict[comp[valid]]
    out = tri.copy()
    out[flipped] = tri[flipped][:, [0, 2, 1]]
    return out, flipped, bool(verdict.all()), comp, verdict


def consistently_oriented(n_vertices, triangles):
    """every two-triangle edge is run once in each direction"""
    return not any(s for _, _, s in triangle_links(n_vertices, triangles)[1])


# ---- the test clouds -------------------------------------------------------------------------------------------------------------------
TUBE_NX, TUBE_NT, TUBE_PITCH, TUBE_SEED = 61, 46, 0.002, 29


def tube(offset=(0.0, 0.0, 0.0)):
    """(points float32 [2806, 3], outward unit normals float32 [2806, 3]): a tube along x of radius 0.02 + 0.003 sin 40 x, a 61 x 46
    lattice of 2 mm pitch along the axis and 46 steps around it, jittered by +-0.2 of a step in both"""
    rng = np.random.default_rng(TUBE_SEED)
    i, j = np.meshgrid(np.arange(TUBE_NX) - 30, np.arange(TUBE_NT), indexing="ij")
    x = (i.ravel() + rng.uniform(-0.2, 0.2, i.size)) * TUBE_PITCH
    th = (j.ravel() + rng.uniform(-0.2, 0.2, j.size)) * (2.0 * np.pi / TUBE_NT)
    r = 0.02 + 0.003 * np.sin(40.0 * x)
    pts = np.stack([x, r * np.cos(th), r * np.sin(th)], 1) + np.asarray(offset, f64)
    nrm = np.stack([-0.12 * np.cos(40.0 * x), np.cos(th), np.sin(th)], 1)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    return pts.astype(f32), nrm.astype(f32)


def tube_outward(points, normals, offset=(0.0, 0.0, 0.0)):
    """n . (the radial direction at the point): positive for an outward normal"""
    q = np.asarray(points).astype(f64) - np.asarray(offset, f64)
    rad = q[:, 1:] / np.linalg.norm(q[:, 1:], axis=1)[:, None]
    nr = np.asarray(normals).astype(f64)
    return nr[:, 1] * rad[:, 0] + nr[:, 2] * rad[:, 1]


def random_signs(normals, seed):
    """the normals with the signs of a random half toggled (bitwise)"""
    out = np.asarray(normals).astype(f32).copy()
    pick = np.random.default_rng(seed).random(len(out)) < 0.5
    out.view(np.uint32)[pick] ^= SIGN
    return out


def plane_lattice():
    """(the 9 x 7 integer lattice scaled by 2^-8 at z = 0, x fastest: float32 [63, 3]; normals +-z at random): every weight is exactly 0"""
    y, x = np.meshgrid(np.arange(7), np.arange(9), indexing="ij")
    pts = (np.stack([x.ravel(), y.ravel(), np.zeros(63)], 1) * 2.0 ** -8).astype(f32)
    nrm = np.zeros((63, 3), f32)
    nrm[:, 2] = np.random.default_rng(31).choice([-1.0, 1.0], 63)
    return pts, nrm


def moebius_cloud():
    """(points float32 [1500, 3], the analytic unit normals of the parametrisation float32 [1500, 3]): 150 x 10 samples of a Moebius band of
    radius 0.05 and width 0.02, jittered; the field is continuous along u and comes back reversed after one turn"""
    rng = np.random.default_rng(37)
    i, j = np.meshgrid(np.arange(150), np.arange(10), indexing="ij")
    u = (i.ravel() + rng.uniform(-0.2, 0.2, i.size)) * (2.0 * np.pi / 150)
    v = ((j.ravel() + rng.uniform(-0.2, 0.2, j.size)) / 9.0 - 0.5) * 0.02
    R = 0.05
    c, s, ch, sh = np.cos(u), np.sin(u), np.cos(u / 2), np.sin(u / 2)
    pts = np.stack([(R + v * ch) * c, (R + v * ch) * s, v * sh], 1)
    du = np.stack([-0.5 * v * sh * c - (R + v * ch) * s, -0.5 * v * sh * s + (R + v * ch) * c, 0.5 * v * ch], 1)
    dv = np.stack([ch * c, ch * s, sh], 1)
    nrm = np.cross(du, dv)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    return pts.astype(f32), nrm.astype(f32)


def bad_rows_tube():
    """(the tube with five NaN points, five zero normals and one NaN normal, signs random; the rows that were made invalid, ascending)"""
    pts, nrm = tube()
    nrm = random_signs(nrm, 41)
    rows = np.sort(np.random.default_rng(43).choice(len(pts), 11, replace=False))
    pts, nrm = pts.copy(), nrm.copy()
    pts[rows[:5], 1] = np.nan
    nrm[rows[5:10]] = 0.0
    nrm[rows[5], 0] = -0.0
    nrm[rows[10], 2] = np.nan
    return pts, nrm, rows


# ---- the test meshes -------------------------------------------------------------------------------------------------------------------
def torus(nu=16, nv=12):
    """(vertices float32 [nu nv, 3], triangles int32 [2 nu nv, 3]) of a closed, consistently wound torus"""
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    u, v = i.ravel() * (2 * np.pi / nu), j.ravel() * (2 * np.pi / nv)
    vert = np.stack([(0.05 + 0.02 * np.cos(v)) * np.cos(u), (0.05 + 0.02 * np.cos(v)) * np.sin(u), 0.02 * np.sin(v)], 1)
    tri = []
    for a in range(nu):
        for b in range(nv):
            p00, p10 = a * nv + b, ((a + 1) % nu) * nv + b
            p01, p11 = a * nv + (b + 1) % nv, ((a + 1) % nu) * nv + (b + 1) % nv
            tri += [[p00, p10, p11], [p00, p11, p01]]
    return vert.astype(f32), np.array(tri, np.int32)


def flip_rows(triangles, rows):
    out = np.asarray(triangles).copy()
    out[rows] = out[rows][:, [0, 2, 1]]
    return out


def moebius_strip(n=16):
    """(vertices float32 [2 n, 3], triangles int32 [2 n, 3]): n quads around, the last joined to the first with the two rims swapped"""
    u = np.arange(n) * (2 * np.pi / n)
    vert = []
    for side in (-1.0, 1.0):
        v = side * 0.01
        vert.append(np.stack([(0.05 + v * np.cos(u / 2)) * np.cos(u), (0.05 + v * np.cos(u / 2)) * np.sin(u), v * np.sin(u / 2)], 1))
    vert = np.concatenate(vert)
    tri = []
    for a in range(n):
        lo0, hi0 = a, n + a
        lo1, hi1 = (a + 1, n + a + 1) if a + 1 < n else (n, 0)                # the twist
        tri += [[lo0, lo1, hi1], [lo0, hi1, hi0]]
    return vert.astype(f32), np.array(tri, np.int32)


def long_strip(n=1000, seed=47):
    """(vertices, triangles int32 [n, 3], the consistently wound strip in the same row order): a flat strip of n triangles, alternately
    flipped, the rows randomly permuted -- neighbours in the strip are far apart in memory, so root walks are deep"""
    m = n // 2
    vert = np.zeros((2 * (m + 1), 3))
    vert[:m + 1, 0] = vert[m + 1:, 0] = np.arange(m + 1) * 0.001
    vert[m + 1:, 1] = 0.001
    tri = []
    for a in range(m):
        tri += [[a, a + 1, m + 1 + a + 1], [a, m + 1 + a + 1, m + 1 + a]]
    tri = np.array(tri, np.int32)
    perm = np.random.default_rng(seed).permutation(n)
    good = tri[perm]
    return vert.astype(f32), flip_rows(good, np.nonzero(perm % 2 == 1)[0]), good


def book():
    """three pages of two triangles each on the spine (0, 1): the spine has three triangles and links nothing; in every page the second
    triangle is wound against the first"""
    vert = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0], [1, 0, 1], [0, 1, 0], [0, 1, 1], [-1, -1, 0], [-1, -1, 1]], f32)
    tri = np.array([[0, 1, 2], [1, 2, 3], [1, 0, 4], [1, 4, 5], [0, 1, 6], [1, 6, 7]], np.int32)
    return vert, tri


def merged(*meshes):
    """the meshes in one, vertices and triangles concatenated"""
    vs, ts, base = [], [], 0
    for v, t in meshes:
        vs.append(v)
        ts.append(t + base)
        base += len(v)
    return np.concatenate(vs).astype(f32), np.concatenate(ts).astype(np.int32)
