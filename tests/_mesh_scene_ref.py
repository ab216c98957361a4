"""Numpy statement of the triangle-mesh scene (csrc/mesh_scene.hip) -- TEST INFRASTRUCTURE ONLY.

Restated from the documented interface of Open3D's t.geometry.RaycastingScene (add_triangles, create_rays_pinhole, cast_rays,
compute_closest_points, compute_distance) and TriangleMesh.sample_points_uniformly; nothing here comes from Open3D's or Embree's code, or
from the reference, which only calls them (3DM/mapping_module.py:204-237,289, 3DM/synthetic_depth_generator.py:24-97).  Parity with
Open3D / Embree is UNPINNED.  Everything is float32 unless it says float64, numpy does not contract, and every operation is written out:
the device must return these bits.

Triangles.  The scene is the concatenation of its geometries; the global index of a triangle is its row in that concatenation.  With
e1 = v1 - v0, e2 = v2 - v0 and n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), a triangle is KEPT when its nine
coordinates and n are finite and n != 0; the others are in no result.  Unit normal: m = max |n_a|, s = n / m,
s / sqrt((sx sx + sy sy) + sz sz).

Ray / triangle (Woop, Benthin, Wald, "Watertight Ray/Triangle Intersection", JCGT 2013, restated).  kz = the first axis of largest
|d|, kx = kz + 1, ky = kx + 1 (mod 3), swapped when d[kz] < 0; Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].  For a vertex P:
A = P - o, Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz], Az = Sz A[kz].  Edge functions U = Cx By - Cy Bx, V = Ax Cy - Ay Cx,
W = Bx Ay - By Ax: the two triangles at a shared edge compute exactly negated values.  When one of them is exactly 0, all three are
recomputed in float64 (products exact, one rounding), the signs are taken there and the values rounded to float32.  Two-sided: a miss when
one is < 0 and another > 0.  det = (U + V) + W, a miss when det == 0; t = ((U Az + V Bz) + W Cz) / det, one division; a hit needs
0 <= t < inf, and -0 is returned as +0.  uv = (V / det, W / det): p = (1 - u - v) v0 + u v1 + v v2.  The answer of a ray is the minimum of
(t, global index); a ray with a non-finite component or a zero direction hits nothing.

Closest point (Ericson, "Real-Time Collision Detection", 5.1.5, restated): the region tests below in float32, dot(a, b) =
(ax bx + ay by) + az bz, the point clamped per coordinate into the triangle's box, d2 = (dx dx + dy dy) + dz dz with d = q - p; the answer
is the minimum of (d2, global index).

An edge-on triangle is no hit: |det| must be at least 2^-12 of the sum of the six |products| the edge functions are made of (float32).

The grid (class Grid, cast_rays_grid, closest_points_grid) is the device's index and its two walks, restated; they must equal the brute
force above bit for bit at every cell size (tests/test_mesh_scene_cpu.py).  The bound is derived at the top of csrc/mesh_scene.hip.

Sampling: see sample_mesh.
"""
import numpy as np

f32, f64, u64 = np.float32, np.float64, np.uint64
INVALID = 0xFFFFFFFF
CHUNK = 64


# ---- triangles -----------------------------------------------------------------------------------------------------------------------------
def _cross(e1, e2):
    return np.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1], e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                     e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], -1)


def corners(vertices, triangles):
    """-> (v0, v1, v2) float32 [T, 3] each"""
    v = np.asarray(vertices).astype(f32)
    t = np.asarray(triangles).astype(np.int64)
    return v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]


def kept_and_normals(v0, v1, v2):
    """-> (kept bool [T], unit normals float32 [T, 3], zero where not kept)"""
    with np.errstate(all="ignore"):
        n = _cross(v1 - v0, v2 - v0)
        kept = np.isfinite(v0).all(1) & np.isfinite(v1).all(1) & np.isfinite(v2).all(1) & np.isfinite(n).all(1) & (n != 0).any(1)
        m = np.maximum(np.maximum(np.abs(n[:, 0]), np.abs(n[:, 1])), np.abs(n[:, 2]))
        s = n / m[:, None]
        unit = s / np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])[:, None]
    return kept, np.where(kept[:, None], unit, f32(0)).astype(f32)


class Scene:
    """the concatenation of (vertices, triangles) pairs"""

    def __init__(self, *geometries):
        c = [corners(v, t) for v, t in geometries]
        self.n_geom = len(c)
        self.geom_start = np.concatenate([[0], np.cumsum([len(a[0]) for a in c])]).astype(np.int64)
        z = np.zeros((0, 3), f32)
        self.v0, self.v1, self.v2 = (np.concatenate([a[k] for a in c] + [z]).astype(f32) for k in range(3))
        self.kept, self.normals = kept_and_normals(self.v0, self.v1, self.v2)

    def ids(self, gi):
        """global index int64 [n] (-1: none) -> (geometry_ids, primitive_ids) uint32"""
        geom = np.searchsorted(self.geom_start, np.maximum(gi, 0), side="right") - 1
        none = gi < 0
        prim = gi - self.geom_start[np.minimum(geom, max(self.n_geom - 1, 0))]
        return (np.where(none, INVALID, geom).astype(np.uint32), np.where(none, INVALID, prim).astype(np.uint32))


# ---- rays ----------------------------------------------------------------------------------------------------------------------------------
def create_rays_pinhole(intrinsic_matrix, extrinsic_matrix, width_px, height_px, pixel_center=0.5):
    """[h, w, 6] float32: origin = the camera centre -R^T t of the world -> camera extrinsic [R | t]; direction = R^T ((u + pc - cx) / fx,
    (v + pc - cy) / fy, 1), float64 with the sums as written, rounded once"""
    K, E = np.asarray(intrinsic_matrix, f64), np.asarray(extrinsic_matrix, f64)
    R, t = E[:3, :3], E[:3, 3]
    v, u = np.meshgrid(np.arange(height_px, dtype=f64), np.arange(width_px, dtype=f64), indexing="ij")
    x = ((u + f64(pixel_center)) - K[0, 2]) / K[0, 0]
    y = ((v + f64(pixel_center)) - K[1, 2]) / K[1, 1]
    out = np.empty((height_px, width_px, 6), f64)
    for k in range(3):
        out[..., k] = -((R[0, k] * t[0] + R[1, k] * t[1]) + R[2, k] * t[2])
        out[..., 3 + k] = (R[0, k] * x + R[1, k] * y) + R[2, k]
    return out.astype(f32)


def _ray_frame(rays):
    o, d = rays[:, :3], rays[:, 3:]
    ok = np.isfinite(rays).all(1) & (d != 0).any(1)
    d = np.where(ok[:, None], d, f32(1))
    kz = np.argmax(np.abs(d), 1)                                   # the first maximum
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    r = np.arange(len(d))
    swap = d[r, kz] < 0
    kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
    dz = d[r, kz]
    return o, ok, kx, ky, kz, d[r, kx] / dz, d[r, ky] / dz, f32(1) / dz


def _edge(Px, Py, Qx, Qy):
    return Qx * Py - Qy * Px


def _intersect(scene, o, kx, ky, kz, Sx, Sy, Sz):
    """rays [n] against every triangle -> (hit bool, t, u, v) [n, T]"""
    def shear(P):
        A = P[None, :, :] - o[:, None, :]
        Akz = np.take_along_axis(A, kz[:, None, None], 2)[..., 0]
        return (np.take_along_axis(A, kx[:, None, None], 2)[..., 0] - Sx[:, None] * Akz,
                np.take_along_axis(A, ky[:, None, None], 2)[..., 0] - Sy[:, None] * Akz, Sz[:, None] * Akz)
    with np.errstate(all="ignore"):
        (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = shear(scene.v0), shear(scene.v1), shear(scene.v2)
        U, V, W = _edge(Bx, By, Cx, Cy), _edge(Cx, Cy, Ax, Ay), _edge(Ax, Ay, Bx, By)
        z = (U == 0) | (V == 0) | (W == 0)
        D = lambda a: a.astype(f64)
        Ud, Vd, Wd = _edge(D(Bx), D(By), D(Cx), D(Cy)), _edge(D(Cx), D(Cy), D(Ax), D(Ay)), _edge(D(Ax), D(Ay), D(Bx), D(By))
        neg = np.where(z, (Ud < 0) | (Vd < 0) | (Wd < 0), (U < 0) | (V < 0) | (W < 0))
        pos = np.where(z, (Ud > 0) | (Vd > 0) | (Wd > 0), (U > 0) | (V > 0) | (W > 0))
        U, V, W = np.where(z, Ud.astype(f32), U), np.where(z, Vd.astype(f32), V), np.where(z, Wd.astype(f32), W)
        det = (U + V) + W
        t = ((U * Az + V * Bz) + W * Cz) / det
        prod = ((np.abs(Cx * By) + np.abs(Cy * Bx)) + (np.abs(Ax * Cy) + np.abs(Ay * Cx))) + (np.abs(Bx * Ay) + np.abs(By * Ax))
        hit = ~(neg & pos) & (det != 0) & (np.abs(det) >= prod * f32(2.0 ** -12)) & (t >= 0) & (t < np.inf) & scene.kept[None, :]
        t = np.where(t == 0, f32(0), t)
        return hit, t, V / det, W / det


def cast_rays(scene, rays):
    """rays [..., 6] -> dict of t_hit float32, geometry_ids / primitive_ids uint32, primitive_uvs [..., 2], primitive_normals [..., 3]"""
    rays = np.asarray(rays).astype(f32)
    shape = rays.shape[:-1]
    rays = rays.reshape(-1, 6)
    n = len(rays)
    t_hit, gi = np.full(n, np.inf, f32), np.full(n, -1, np.int64)
    uv = np.zeros((n, 2), f32)
    o, ok, kx, ky, kz, Sx, Sy, Sz = _ray_frame(rays)
    if len(scene.v0):
        for a in range(0, n, CHUNK):
            s = slice(a, a + CHUNK)
            hit, t, u, v = _intersect(scene, o[s], kx[s], ky[s], kz[s], Sx[s], Sy[s], Sz[s])
            t = np.where(hit & ok[s, None], t, f32(np.inf))
            i = np.argmin(t, 1)                                    # the first minimum: the lowest global index
            r = np.arange(len(i))
            found = t[r, i] < np.inf
            t_hit[s] = t[r, i]
            gi[s] = np.where(found, i, -1)
            uv[s] = np.where(found[:, None], np.stack([u[r, i], v[r, i]], 1), f32(0))
    geom, prim = scene.ids(gi)
    normals = np.zeros((n, 3), f32)
    normals[gi >= 0] = scene.normals[gi[gi >= 0]]
    return dict(t_hit=t_hit.reshape(shape), geometry_ids=geom.reshape(shape), primitive_ids=prim.reshape(shape),
                primitive_uvs=uv.reshape(shape + (2,)), primitive_normals=normals.reshape(shape + (3,)))


# ---- closest point -------------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _closest(scene, q):
    """queries [n, 3] against every triangle -> (point [n, T, 3], u, v, d2 [n, T])"""
    a, b, c = scene.v0[None], scene.v1[None], scene.v2[None]
    p = q[:, None, :]
    with np.errstate(all="ignore"):
        ab, ac, bc = b - a, c - a, c - b
        ap, bp, cp = p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        one = f32(1)
        w_ab, w_ac, w_bc = d1 / (d1 - d3), d2 / (d2 - d6), e43 / (e43 + e56)
        den = one / ((va + vb) + vc)
        vi, wi = vb * den, vc * den
        A_, B_, C_ = (np.broadcast_to(x, ap.shape) for x in (a, b, c))
        z, o = np.zeros(d1.shape, f32), np.ones(d1.shape, f32)
        # the regions in the order they are tested, the first that holds wins; a vertex region returns the vertex itself
        regions = [
            ((d1 <= 0) & (d2 <= 0), A_, z, z),
            ((d3 >= 0) & (d4 <= d3), B_, o, z),
            ((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + w_ab[..., None] * ab, w_ab, z),
            ((d6 >= 0) & (d5 <= d6), C_, z, o),
            ((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + w_ac[..., None] * ac, z, w_ac),
            ((va <= 0) & (e43 >= 0) & (e56 >= 0), b + w_bc[..., None] * bc, one - w_bc, w_bc),
        ]
        pt, u, v = (a + vi[..., None] * ab) + wi[..., None] * ac, vi, wi
        for cond, rp, ru, rv in reversed(regions):
            pt, u, v = np.where(cond[..., None], rp, pt), np.where(cond, ru, u), np.where(cond, rv, v)
        lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)          # into the triangle's box; a NaN stays one
        pt = np.where(pt < lo, lo, np.where(pt > hi, hi, pt))
        d = p - pt
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return pt, u, v, dd


def closest_points(scene, query, max_distance=None):
    """query [..., 3] -> dict of points [..., 3], distance, d2 float32, geometry_ids / primitive_ids uint32, primitive_uvs [..., 2].  No
    triangle (or none within max_distance, compared with the float32 distance): points NaN, distance and d2 +inf, invalid ids, uv 0.  A
    query with a non-finite coordinate: points, distance and d2 NaN, invalid ids, uv 0."""
    q = np.asarray(query).astype(f32)
    shape = q.shape[:-1]
    q = q.reshape(-1, 3)
    n = len(q)
    ok = np.isfinite(q).all(1)
    pts, d2o, gi = np.full((n, 3), np.nan, f32), np.full(n, np.inf, f32), np.full(n, -1, np.int64)
    uv = np.zeros((n, 2), f32)
    if len(scene.v0):
        for a in range(0, n, CHUNK):
            s = slice(a, a + CHUNK)
            pt, u, v, dd = _closest(scene, np.where(ok[s, None], q[s], f32(0)))
            with np.errstate(invalid="ignore"):
                dd = np.where(scene.kept[None, :] & ok[s, None] & (dd == dd), dd, f32(np.inf))
            i = np.argmin(dd, 1)
            r = np.arange(len(i))
            found = dd[r, i] < np.inf
            d2o[s] = dd[r, i]
            gi[s] = np.where(found, i, -1)
            pts[s] = np.where(found[:, None], pt[r, i], f32(np.nan))
            uv[s] = np.where(found[:, None], np.stack([u[r, i], v[r, i]], 1), f32(0))
    dist = np.sqrt(d2o)
    if max_distance is not None:
        miss = dist > f32(max_distance)
        gi[miss], d2o[miss], dist[miss], pts[miss], uv[miss] = -1, np.inf, np.inf, np.nan, 0
    bad = ~ok
    gi[bad], d2o[bad], dist[bad], pts[bad], uv[bad] = -1, np.nan, np.nan, np.nan, 0
    geom, prim = scene.ids(gi)
    return dict(points=pts.reshape(shape + (3,)), distance=dist.reshape(shape), d2=d2o.reshape(shape), geometry_ids=geom.reshape(shape),
                primitive_ids=prim.reshape(shape), primitive_uvs=uv.reshape(shape + (2,)))


# ---- sampling ------------------------------------------------------------------------------------------------------------------------------
GOLDEN, M1, M2 = u64(0x9E3779B97F4A7C15), u64(0xBF58476D1CE4E5B9), u64(0x94D049BB133111EB)


def mix64(z):
    """the finaliser of splitmix64 on uint64 arrays (arithmetic modulo 2^64)"""
    z = np.asarray(z, u64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> u64(30))) * M1
        z = (z ^ (z >> u64(27))) * M2
    return z ^ (z >> u64(31))


def sample_hash(seed, i, j):
    """value j (0, 1, 2) of sample i: mix64(mix64(seed) + (3 i + j + 1) GOLDEN)"""
    with np.errstate(over="ignore"):
        return mix64(mix64(u64(seed)) + (u64(3) * np.asarray(i, u64) + u64(j + 1)) * GOLDEN)


def mulhi64(a, b):
    """floor(a b / 2^64) for uint64 arrays a and a uint64 b"""
    return np.array([(int(x) * int(b)) >> 64 for x in np.asarray(a).ravel()], u64).reshape(np.shape(a))


def cross_and_area(v0, v1, v2):
    """-> (n float64 [T, 3], area float64 [T]): the float64 cross product of the float64 differences of the float32 vertices, and
    area = 0.5 sqrt((nx nx + ny ny) + nz nz)"""
    a, b, c = v0.astype(f64), v1.astype(f64), v2.astype(f64)
    with np.errstate(all="ignore"):
        n = _cross(b - a, c - a)
        return n, 0.5 * np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])


def sample_weights(v0, v1, v2, kept):
    """uint64 [T]: floor(area / max area 2^40) with cross_and_area's area; 0 for a triangle that is not kept"""
    area = np.where(kept, cross_and_area(v0, v1, v2)[1], 0.0)
    top = area.max() if len(area) else 0.0
    if not (top > 0.0 and np.isfinite(top)):
        return np.zeros(len(area), u64)
    return np.floor(area / top * 2.0 ** 40).astype(u64)


def sample_mesh(vertices, triangles, n, seed=0, vertex_colors=None, first=0):
    """samples first .. first + n - 1 -> (points float32 [n, 3], colours float32 [n, 3] or None, normals float32 [n, 3], triangle int32 [n]).
    cum = the inclusive scan of sample_weights; triangle = the first row with cum > mulhi64(h0, cum[-1]); r1, r2 = float32(2 (h >> 40) + 1)
    2^-25 -- (k + 0.5) 2^-24 rounded once --, s = sqrt(r1), weights (1 - s, s (1 - r2), s r2), p = (wa A + wb B) + wc C; colours alike from
    the vertex colours; the normal is the triangle's unit normal.  No kept triangle: empty arrays."""
    v0, v1, v2 = corners(vertices, triangles)
    kept, normals = kept_and_normals(v0, v1, v2)
    cum = np.cumsum(sample_weights(v0, v1, v2, kept).astype(np.int64)).astype(u64)
    if not len(cum) or cum[-1] == 0:
        return np.zeros((0, 3), f32), None if vertex_colors is None else np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros(0, np.int32)
    i = np.arange(first, first + n, dtype=u64)
    tri = np.searchsorted(cum, mulhi64(sample_hash(seed, i, 0), cum[-1]), side="right")
    r1 = ((sample_hash(seed, i, 1) >> u64(40)) * u64(2) + u64(1)).astype(np.uint32).astype(f32) * f32(2.0 ** -25)
    r2 = ((sample_hash(seed, i, 2) >> u64(40)) * u64(2) + u64(1)).astype(np.uint32).astype(f32) * f32(2.0 ** -25)
    s = np.sqrt(r1)
    wa, wb, wc = (f32(1) - s)[:, None], (s * (f32(1) - r2))[:, None], (s * r2)[:, None]
    pts = (wa * v0[tri] + wb * v1[tri]) + wc * v2[tri]
    col = None
    if vertex_colors is not None:
        c = np.asarray(vertex_colors).astype(f32)
        t = np.asarray(triangles).astype(np.int64)[tri]
        col = (wa * c[t[:, 0]] + wb * c[t[:, 1]]) + wc * c[t[:, 2]]
    return pts.astype(f32), col, normals[tri], tri.astype(np.int32)


# ---- the scenes of the tests ---------------------------------------------------------------------------------------------------------------
def grid_patch(x, y, zfun):
    """the lattice x [nx] by y [ny] (vertex j * nx + i), two triangles per square -> (vertices float32, triangles int32)"""
    X, Y = np.meshgrid(np.asarray(x, f64), np.asarray(y, f64), indexing="xy")
    v = np.stack([X.ravel(), Y.ravel(), zfun(X.ravel(), Y.ravel())], 1).astype(f32)
    nx, ny = len(x), len(y)
    j, i = np.meshgrid(np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    p = (j * nx + i).ravel()
    t = np.concatenate([np.stack([p, p + 1, p + nx + 1], 1), np.stack([p, p + nx + 1, p + nx], 1)])
    return v, t.astype(np.int32)


def cube():
    """[-1, 1]^3, every face a 5 x 5 lattice of pitch 0.5 cut into 4 x 4 x 2 triangles: 192 triangles on 150 vertices (the faces do not
    share vertex rows; their edges and corners coincide)"""
    x = np.linspace(-1.0, 1.0, 5)
    vs, ts, base = [], [], 0
    for axis in range(3):
        for side in (-1.0, 1.0):
            v, t = grid_patch(x, x, lambda X, Y: np.full_like(X, side))
            v = np.roll(v, axis + 1, axis=1)                       # the constant coordinate goes to `axis`
            vs.append(v)
            ts.append(t + base)
            base += len(v)
    return np.concatenate(vs).astype(f32), np.concatenate(ts).astype(np.int32)


def icosphere(level=2):
    """the unit icosphere: 20 4^level triangles"""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1),
         (-g, 0, 1)]
    v = [np.array(p, f64) / np.linalg.norm(p) for p in v]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, out = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in t:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = out
    return np.array(v).astype(f32), np.array(t, np.int32)


def height_field(pitch=0.002):
    """tests/_render.py's surface g triangulated on a lattice of the given pitch.  0.002: the unjittered 61 x 46 lattice of
    tests/_pointcloud_ref.py's base target, 5 400 triangles; any other pitch: the lattice over the footprint of map_gt_samples
    (|x| <= 0.16, |y| <= 0.13 and one pitch more)"""
    import _render as R
    if pitch == 0.002:
        x, y = (np.arange(61) - 30) * pitch, (np.arange(46) - 22.5) * pitch
    else:
        nx, ny = int(np.ceil(0.16 / pitch)) + 1, int(np.ceil(0.13 / pitch)) + 1
        x, y = np.arange(-nx, nx + 1) * pitch, np.arange(-ny, ny + 1) * pitch
    return grid_patch(x, y, R.g)


def pinhole_matrix(K4):
    fx, fy, cx, cy = K4
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


# ---- the grid ------------------------------------------------------------------------------------------------------------------------------
import _pointcloud_ref as _P  # noqa: E402

MAX_CELLS, SHELL_CAP = 2 ** 24, 8


def max_refs(n_triangles):
    return min(max(8 * n_triangles, 2 ** 16), 2 ** 31 - 1)


class Sub:
    """the triangles `ids` of a scene, for _intersect and _closest"""

    def __init__(self, scene, ids):
        self.v0, self.v1, self.v2, self.kept = scene.v0[ids], scene.v1[ids], scene.v2[ids], scene.kept[ids]


class Grid:
    """lo, hi: the float32 bounds of the kept triangles' vertices; M = max |lo|, |hi| + the largest extent; pad = 2^-9 largest extent +
    2^-14 M (float32); a kept triangle is listed in every cell from cell(min - pad) to cell(max + pad) per axis, cell = the point grid's
    function (tests/_pointcloud_ref.py cells_of).  cell_size None: default_cell_size(lo, hi, kept), grown by 1.25 until the grid has at
    most 2^24 cells and the table at most max(8 T, 2^16) references; an explicit one that breaks a limit: ValueError."""

    def __init__(self, scene, cell_size=None):
        self.scene = scene
        k = scene.kept
        pts = np.concatenate([scene.v0[k], scene.v1[k], scene.v2[k]])
        self.lo, self.hi = (pts.min(0), pts.max(0)) if len(pts) else (np.zeros(3, f32), np.zeros(3, f32))
        ext = self.hi - self.lo
        self.M = f32(max(np.abs(self.lo).max(), np.abs(self.hi).max())) + ext.max()
        self.pad = ext.max() * f32(2.0 ** -9) + self.M * f32(2.0 ** -14)
        self.o_limit = f32(8) * self.M
        h = f32(_P.default_cell_size(self.lo, self.hi, int(k.sum())) if cell_size is None else cell_size)
        tmin = np.minimum(np.minimum(scene.v0, scene.v1), scene.v2) - self.pad
        tmax = np.maximum(np.maximum(scene.v0, scene.v1), scene.v2) + self.pad
        while True:
            dims = _P.dims_for(self.lo, self.hi, h)
            cells = int(dims[0]) * int(dims[1]) * int(dims[2])
            if cells <= MAX_CELLS:
                c0 = _P.cells_of(np.where(k[:, None], tmin, f32(0)), self.lo, h, dims)
                c1 = _P.cells_of(np.where(k[:, None], tmax, f32(0)), self.lo, h, dims)
                n_refs = int(((c1 - c0 + 1).prod(1) * k).sum())
                if n_refs <= max_refs(len(k)):
                    break
            if cell_size is not None:
                raise ValueError("cell_size breaks a limit of the grid")
            h = f32(h * f32(1.25))
        self.h, self.dims, self.n_refs = h, dims, n_refs
        nx, ny, nz = (int(v) for v in dims)
        lists = {}
        for i in np.nonzero(k)[0]:
            for z in range(c0[i, 2], c1[i, 2] + 1):
                for y in range(c0[i, 1], c1[i, 1] + 1):
                    for x in range(c0[i, 0], c1[i, 0] + 1):
                        lists.setdefault((z * ny + y) * nx + x, []).append(i)
        self.lists = {c: np.array(v, np.int64) for c, v in lists.items()}

    def cell(self, p):
        return [int(v) for v in _P.cells_of(np.asarray(p, f32)[None, :], self.lo, self.h, self.dims)[0]]


def cast_rays_grid(grid, rays, stats_out=None):
    """the walk of the device: a ray with an origin coordinate beyond 8 M in magnitude or a non-zero direction component outside
    2^-60 .. 2^60 goes to brute force; the others enter the box grown by pad (a miss when the line has no part of it in front of the
    origin), start in the cell of the entry point and step to the nearest of the three next cell boundaries, each computed from the cell
    index; the walk stops when the best t is strictly below the cell's exit parameter less (2^-10 largest extent + pad) |Sz| 1.01"""
    scene = grid.scene
    rays = np.asarray(rays).astype(f32)
    shape = rays.shape[:-1]
    rays = rays.reshape(-1, 6)
    out = cast_rays(Scene(), rays)                       # all misses, the right shapes
    gi = np.full(len(rays), -1, np.int64)
    o_all, ok, kx, ky, kz, Sx, Sy, Sz = _ray_frame(rays)
    nx, ny, nz = (int(v) for v in grid.dims)
    lo, hi, h, pad = grid.lo, grid.hi, grid.h, grid.pad
    slack_ext = (hi - lo).max() * f32(2.0 ** -10)
    fallback = []
    with np.errstate(all="ignore"):
        for i in range(len(rays)):
            if not ok[i]:
                continue
            o, d = rays[i, :3], rays[i, 3:]
            ad = np.abs(d)
            if ((d != 0) & ((ad < f32(2.0 ** -60)) | (ad > f32(2.0 ** 60)))).any() or (np.abs(o) > grid.o_limit).any():
                fallback.append(i)
                continue
            inv = np.where(d != 0, f32(1) / np.where(d != 0, d, f32(1)), f32(0))
            t_in, t_out, miss = f32(0), f32(np.inf), False
            for a in range(3):
                if d[a] == 0:
                    miss = miss or o[a] < lo[a] - pad or o[a] > hi[a] + pad
                else:
                    ta, tb = ((lo[a] - pad) - o[a]) * inv[a], ((hi[a] + pad) - o[a]) * inv[a]
                    t_in, t_out = max(t_in, min(ta, tb)), min(t_out, max(ta, tb))
            if miss or not t_in <= t_out:
                continue
            c = grid.cell(o + t_in * d)
            n = (nx, ny, nz)
            step = [1 if v > 0 else (-1 if v < 0 else 0) for v in d]
            slack = (slack_ext + pad) * abs(Sz[i]) * f32(1.01)
            best, bi = f32(np.inf), -1
            sl = slice(i, i + 1)
            for _ in range(nx + ny + nz + 3):
                ids = grid.lists.get((c[2] * ny + c[1]) * nx + c[0])
                if ids is not None:
                    hit, t, _, _ = _intersect(Sub(scene, ids), o_all[sl], kx[sl], ky[sl], kz[sl], Sx[sl], Sy[sl], Sz[sl])
                    t = np.where(hit[0], t[0], f32(np.inf))
                    m = t.min()
                    if m < np.inf:
                        j = int(ids[t == m].min())
                        if m < best or (m == best and j < bi):
                            best, bi = m, j
                tn = [((lo[a] + f32(c[a] + (step[a] > 0)) * h) - o[a]) * inv[a] if step[a] else f32(np.inf) for a in range(3)]
                if best < min(tn) - slack:
                    break
                a = 0 if (tn[0] <= tn[1] and tn[0] <= tn[2]) else (1 if tn[1] <= tn[2] else 2)
                c[a] += step[a]
                if c[a] < 0 or c[a] >= n[a]:
                    break
            gi[i] = bi
    if fallback:
        fb = cast_rays(scene, rays[fallback])
        for k in ("t_hit", "geometry_ids", "primitive_ids", "primitive_uvs", "primitive_normals"):
            out[k][fallback] = fb[k]
    done = np.nonzero(gi >= 0)[0]
    for i in done:                                       # the winner evaluated again: the brute force on that one triangle
        one = cast_rays(_One(scene, gi[i]), rays[i:i + 1])
        for k in ("t_hit", "primitive_uvs", "primitive_normals"):
            out[k][i] = one[k][0]
    g, p = scene.ids(gi)
    out["geometry_ids"][done], out["primitive_ids"][done] = g[done], p[done]
    if stats_out is not None:
        stats_out["fallback"] = len(fallback)
    return {k: v.reshape(shape + v.shape[1:]) for k, v in out.items()}


class _One:
    """a scene view of the single global triangle i (ids are taken from the full scene by the caller)"""

    def __init__(self, scene, i):
        s = slice(i, i + 1)
        self.v0, self.v1, self.v2, self.kept, self.normals = scene.v0[s], scene.v1[s], scene.v2[s], scene.kept[s], scene.normals[s]
        self.n_geom, self.geom_start = 1, np.array([0, 1], np.int64)

    ids = Scene.ids


def closest_points_grid(grid, query, max_distance=None, shell_cap=SHELL_CAP, stats_out=None):
    """the Chebyshev shells of tests/_pointcloud_ref.py nn_grid over triangle references, with its slack taken over hi + 2 pad; a query still
    searching after shell_cap is finished by brute force"""
    scene = grid.scene
    q = np.asarray(query).astype(f32)
    shape = q.shape[:-1]
    q = q.reshape(-1, 3)
    n = len(q)
    nx, ny, nz = (int(v) for v in grid.dims)
    lo, h = grid.lo, grid.h
    ext = (grid.hi + f32(2) * grid.pad) - lo
    md = f32(np.inf) if max_distance is None else f32(max_distance)
    ok = np.isfinite(q).all(1)
    gi = np.full(n, -1, np.int64)
    fallback = []
    with np.errstate(all="ignore"):
        for i in range(n):
            if not ok[i]:
                continue
            s = q[i]
            cx, cy, cz = grid.cell(s)
            slack = f32(np.max(ext + np.abs(s - lo))) * f32(2.0 ** -21)
            r_all = max(cx, nx - 1 - cx, cy, ny - 1 - cy, cz, nz - 1 - cz)
            best, bi, r = f32(np.inf), 2 ** 31 - 1, 0
            while True:
                ids = []
                for z in range(max(cz - r, 0), min(cz + r, nz - 1) + 1):
                    for y in range(max(cy - r, 0), min(cy + r, ny - 1) + 1):
                        face = abs(z - cz) == r or abs(y - cy) == r
                        xs = range(max(cx - r, 0), min(cx + r, nx - 1) + 1) if face else [x for x in (cx - r, cx + r) if 0 <= x < nx]
                        for x in xs:
                            v = grid.lists.get((z * ny + y) * nx + x)
                            if v is not None:
                                ids.append(v)
                if ids:
                    ids = np.unique(np.concatenate(ids))
                    dd = _closest(Sub(scene, ids), s[None, :])[3][0]
                    dd = np.where(dd == dd, dd, f32(np.inf))
                    m = dd.min()
                    if m < np.inf:
                        j = int(ids[dd == m].min())
                        if m < best or (m == best and j < bi):
                            best, bi = m, j
                if r >= r_all:
                    break
                lb = (f32(r) * h - slack) * f32(0.99999)
                if lb > 0 and best < lb * lb:
                    break
                if lb * f32(0.9999) > md:
                    break
                if r >= shell_cap:
                    fallback.append(i)
                    bi = -2
                    break
                r += 1
            if bi >= 0 and bi != 2 ** 31 - 1:
                gi[i] = bi
    out = closest_points(Scene(), q, max_distance)
    rest = np.nonzero(gi >= 0)[0]
    for i in list(rest):
        one = closest_points(_One(scene, gi[i]), q[i:i + 1], max_distance)
        for k in ("points", "distance", "d2", "primitive_uvs"):
            out[k][i] = one[k][0]
        if np.isfinite(one["distance"][0]):
            g, p = scene.ids(gi[i:i + 1])
            out["geometry_ids"][i], out["primitive_ids"][i] = g[0], p[0]
    if fallback:
        fb = closest_points(scene, q[fallback], max_distance)
        for k in out:
            out[k][fallback] = fb[k]
    if stats_out is not None:
        stats_out["fallback"] = len(fallback)
    return {k: v.reshape(shape + v.shape[1:]) for k, v in out.items()}
