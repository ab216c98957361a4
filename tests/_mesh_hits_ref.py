"""Numpy statement of the scene's counting queries (csrc/mesh_scene.hip) -- TEST INFRASTRUCTURE ONLY.

Restated from the documented interface of Open3D's t.geometry.RaycastingScene (test_occlusions, count_intersections, list_intersections,
compute_signed_distance, compute_occupancy); nothing here comes from Open3D's or Embree's code.  Parity with Open3D / Embree is UNPINNED.
Everything is float32 unless it says float64, numpy does not contract, and every operation is written out: the device must return these
bits.  The arithmetic is tests/_mesh_scene_ref.py's (sheared vertices, float32 edge values, the float64 recomputation when one of them
is 0, |det| >= 2^-12 P, 0 <= t < inf) with ONE difference, the tie rule.

The tie rule.  The closed predicate of cast_rays lets an edge value of exactly 0 count as inside for both triangles at a shared edge:
right for a minimum, wrong for a parity.  Here an edge value E = Qx Py - Qy Px of the edge P -> Q that is exactly 0 in float64 takes its
sign from the first non-zero of (Qy - Py) and -(Qx - Px), compared exactly: the sign E would have with the ray moved by (eps, eps^2) in
the sheared plane, E + eps (Qy - Py) + eps^2 (Px - Qx).  Both 0: the value stays 0 (an edge-on triangle, which det rejects).  The two
triangles at a shared edge see the same P and Q reversed and decide opposite signs; around a shared vertex exactly one triangle of a fan
claims the ray.  det, t, u and v are computed from the unperturbed values.

count_intersections: the hits of the tie predicate with tnear <= t <= tfar.  list_intersections: those hits in ray order and, within a
ray, ascending in (t, global index).  test_occlusions: any hit of the CLOSED predicate with tnear <= t <= tfar, so that with the defaults
it is isfinite(cast_rays t_hit).  occupancy: sample j casts from the query along DIRECTIONS[j]; inside when the majority of the counts is
odd.  signed distance: closest_points' distance, negated where occupied.

hits_grid is the device's walk restated: cast_rays_grid's start, no early stop, and a triangle is tested only in the first visited cell
of its padded cell box -- the start cell, or a cell whose predecessor was outside the box along the axis just stepped.
"""
import numpy as np

import _mesh_scene_ref as M
import _pointcloud_ref as _P

f32, f64 = np.float32, np.float64
CHUNK = 64
COUNT, ANY, FILL = 0, 1, 2

# sample j of an occupancy query casts along row j: exactly representable, so the rays are the same bits wherever they are composed
DIRECTIONS = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, 0, 0), (0, -1, 0), (0, 0, -1),
                       (-1, -1, -1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1), (1, 2, 3)], f32)


# ---- the predicate -------------------------------------------------------------------------------------------------------------------------
def _tie_sign(E, Px, Py, Qx, Qy):
    """the sign (-1, 0, 1) of the float64 edge value E of P -> Q; an exact 0 decided by (Qy - Py), then -(Qx - Px), compared exactly"""
    s = (E > 0).astype(np.int8) - (E < 0).astype(np.int8)
    t1 = (Qy > Py).astype(np.int8) - (Qy < Py).astype(np.int8)
    t2 = (Qx < Px).astype(np.int8) - (Qx > Px).astype(np.int8)
    return np.where(s != 0, s, np.where(t1 != 0, t1, t2))


def intersect(scene, o, kx, ky, kz, Sx, Sy, Sz, tie=True):
    """rays [n] (their _ray_frame) against every triangle -> (hit bool, t, u, v) [n, T].  tie False: _mesh_scene_ref._intersect, the
    closed predicate, the same bits"""
    def shear(P):
        A = P[None, :, :] - o[:, None, :]
        Akz = np.take_along_axis(A, kz[:, None, None], 2)[..., 0]
        return (np.take_along_axis(A, kx[:, None, None], 2)[..., 0] - Sx[:, None] * Akz,
                np.take_along_axis(A, ky[:, None, None], 2)[..., 0] - Sy[:, None] * Akz, Sz[:, None] * Akz)
    E = M._edge
    with np.errstate(all="ignore"):
        (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = shear(scene.v0), shear(scene.v1), shear(scene.v2)
        U, V, W = E(Bx, By, Cx, Cy), E(Cx, Cy, Ax, Ay), E(Ax, Ay, Bx, By)
        z = (U == 0) | (V == 0) | (W == 0)
        D = lambda a: a.astype(f64)
        Ud, Vd, Wd = E(D(Bx), D(By), D(Cx), D(Cy)), E(D(Cx), D(Cy), D(Ax), D(Ay)), E(D(Ax), D(Ay), D(Bx), D(By))
        if tie:
            su, sv, sw = _tie_sign(Ud, Bx, By, Cx, Cy), _tie_sign(Vd, Cx, Cy, Ax, Ay), _tie_sign(Wd, Ax, Ay, Bx, By)
            negd, posd = (su < 0) | (sv < 0) | (sw < 0), (su > 0) | (sv > 0) | (sw > 0)
        else:
            negd, posd = (Ud < 0) | (Vd < 0) | (Wd < 0), (Ud > 0) | (Vd > 0) | (Wd > 0)
        neg = np.where(z, negd, (U < 0) | (V < 0) | (W < 0))
        pos = np.where(z, posd, (U > 0) | (V > 0) | (W > 0))
        U, V, W = np.where(z, Ud.astype(f32), U), np.where(z, Vd.astype(f32), V), np.where(z, Wd.astype(f32), W)
        det = (U + V) + W
        t = ((U * Az + V * Bz) + W * Cz) / det
        prod = ((np.abs(Cx * By) + np.abs(Cy * Bx)) + (np.abs(Ax * Cy) + np.abs(Ay * Cx))) + (np.abs(Bx * Ay) + np.abs(By * Ax))
        hit = ~(neg & pos) & (det != 0) & (np.abs(det) >= prod * f32(2.0 ** -12)) & (t >= 0) & (t < np.inf) & scene.kept[None, :]
        t = np.where(t == 0, f32(0), t)
        return hit, t, V / det, W / det


def _flat(rays):
    rays = np.asarray(rays).astype(f32)
    return rays.shape[:-1], rays.reshape(-1, 6)


def hit_matrix(scene, rays, tie=True, tnear=0.0, tfar=np.inf):
    """rays [n, 6] -> (hit bool, t, u, v) [n, T] of the predicate with tnear <= t <= tfar (compared in float32); a ray with a non-finite
    component or a zero direction hits nothing"""
    n, T = len(rays), len(scene.v0)
    hit, t, u, v = np.zeros((n, T), bool), np.zeros((n, T), f32), np.zeros((n, T), f32), np.zeros((n, T), f32)
    o, ok, kx, ky, kz, Sx, Sy, Sz = M._ray_frame(rays)
    if T:
        for a in range(0, n, CHUNK):
            s = slice(a, a + CHUNK)
            h, t[s], u[s], v[s] = intersect(scene, o[s], kx[s], ky[s], kz[s], Sx[s], Sy[s], Sz[s], tie)
            hit[s] = h & ok[s, None] & (t[s] >= f32(tnear)) & (t[s] <= f32(tfar))
    return hit, t, u, v


# ---- brute force ---------------------------------------------------------------------------------------------------------------------------
def count_intersections(scene, rays, tnear=0.0, tfar=np.inf, tie=True):
    """rays [..., 6] -> int32 [...]"""
    shape, rays = _flat(rays)
    return hit_matrix(scene, rays, tie, tnear, tfar)[0].sum(1).astype(np.int32).reshape(shape)


def test_occlusions(scene, rays, tnear=0.0, tfar=np.inf):
    """rays [..., 6] -> bool [...]: the CLOSED predicate"""
    shape, rays = _flat(rays)
    return hit_matrix(scene, rays, False, tnear, tfar)[0].any(1).reshape(shape)


def _rows(scene, rays, hit, t, u, v):
    """the hit matrix -> the dict of list_intersections"""
    n = len(rays)
    ray_ids, gi = np.nonzero(hit)
    order = np.lexsort((gi, t[ray_ids, gi], ray_ids))              # ray, then t, then global index
    ray_ids, gi = ray_ids[order], gi[order]
    geom, prim = scene.ids(gi.astype(np.int64))
    splits = np.concatenate([[0], np.cumsum(hit.sum(1))]).astype(np.int64)
    return dict(ray_splits=splits, ray_ids=ray_ids.astype(np.int64), t_hit=t[ray_ids, gi].astype(f32), geometry_ids=geom, primitive_ids=prim,
                primitive_uvs=np.stack([u[ray_ids, gi], v[ray_ids, gi]], 1).astype(f32).reshape(-1, 2), global_ids=gi.astype(np.int64))


def list_intersections(scene, rays):
    """rays [..., 6] -> dict of ray_splits int64 [m + 1], ray_ids int64, t_hit float32, geometry_ids / primitive_ids uint32 [total],
    primitive_uvs [total, 2] (and global_ids int64 [total], the statement's own); m = the number of rays, flattened"""
    _, rays = _flat(rays)
    return _rows(scene, rays, *hit_matrix(scene, rays, True))


# ---- the grid walk -------------------------------------------------------------------------------------------------------------------------
def cell_boxes(grid):
    """(c0, c1) int [T, 3]: the cells a kept triangle is referenced from, cell(min - pad) .. cell(max + pad) per axis -- Grid's expression"""
    s = grid.scene
    tmin = np.minimum(np.minimum(s.v0, s.v1), s.v2) - grid.pad
    tmax = np.maximum(np.maximum(s.v0, s.v1), s.v2) + grid.pad
    k = s.kept[:, None]
    return (_P.cells_of(np.where(k, tmin, f32(0)), grid.lo, grid.h, grid.dims), _P.cells_of(np.where(k, tmax, f32(0)), grid.lo, grid.h, grid.dims))


def hits_grid(grid, rays, mode=COUNT, tnear=0.0, tfar=np.inf, stats_out=None):
    """the walk of the device -> the hit matrix (hit, t, u, v) [n, T] it finds: COUNT / FILL the tie predicate and every cell until the ray
    leaves the grid, ANY the closed predicate and a stop at the first hit (only the row's any() is meaningful then).  A triangle is tested
    only in the first visited cell of its cell box.  stats_out: "fallback" rays finished by brute force, "tests" ray / triangle tests"""
    scene = grid.scene
    _, rays = _flat(rays)
    n, T = len(rays), len(scene.v0)
    tie = mode != ANY
    hit, t, u, v = np.zeros((n, T), bool), np.zeros((n, T), f32), np.zeros((n, T), f32), np.zeros((n, T), f32)
    o_all, ok, kx, ky, kz, Sx, Sy, Sz = M._ray_frame(rays)
    nx, ny, nz = (int(x) for x in grid.dims)
    lo, hi, h, pad = grid.lo, grid.hi, grid.h, grid.pad
    c0, c1 = cell_boxes(grid)
    fallback, tests = [], 0
    with np.errstate(all="ignore"):
        for i in range(n):
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
            dims = (nx, ny, nz)
            step = [1 if x > 0 else (-1 if x < 0 else 0) for x in d]
            sl = slice(i, i + 1)
            last = -1                                              # the axis just stepped; -1: the start cell
            for _ in range(nx + ny + nz + 3):
                ids = grid.lists.get((c[2] * ny + c[1]) * nx + c[0])
                if ids is not None:
                    if last >= 0:                                  # first cell of the run: the predecessor was outside the box
                        prev = c[last] - step[last]
                        ids = ids[(prev < c0[ids, last]) | (prev > c1[ids, last])]
                    if len(ids):
                        tests += len(ids)
                        hh, tt, uu, vv = intersect(M.Sub(scene, ids), o_all[sl], kx[sl], ky[sl], kz[sl], Sx[sl], Sy[sl], Sz[sl], tie)
                        hh = hh[0] & (tt[0] >= f32(tnear)) & (tt[0] <= f32(tfar))
                        assert not hit[i, ids[hh]].any()           # each hit exactly once
                        hit[i, ids], t[i, ids], u[i, ids], v[i, ids] = hh, tt[0], uu[0], vv[0]
                        if mode == ANY and hh.any():
                            break
                tn = [((lo[a] + f32(c[a] + (step[a] > 0)) * h) - o[a]) * inv[a] if step[a] else f32(np.inf) for a in range(3)]
                last = 0 if (tn[0] <= tn[1] and tn[0] <= tn[2]) else (1 if tn[1] <= tn[2] else 2)
                if not step[last]:
                    break
                c[last] += step[last]
                if c[last] < 0 or c[last] >= dims[last]:
                    break
    if fallback:
        hit[fallback], t[fallback], u[fallback], v[fallback] = hit_matrix(scene, rays[fallback], tie, tnear, tfar)
    if stats_out is not None:
        stats_out["fallback"], stats_out["tests"] = len(fallback), tests
    return hit, t, u, v


def count_intersections_grid(grid, rays, tnear=0.0, tfar=np.inf, stats_out=None):
    shape, flat = _flat(rays)
    return hits_grid(grid, flat, COUNT, tnear, tfar, stats_out)[0].sum(1).astype(np.int32).reshape(shape)


def test_occlusions_grid(grid, rays, tnear=0.0, tfar=np.inf, stats_out=None):
    shape, flat = _flat(rays)
    return hits_grid(grid, flat, ANY, tnear, tfar, stats_out)[0].any(1).reshape(shape)



def list_intersections_grid(grid, rays, stats_out=None):
    _, flat = _flat(rays)
    return _rows(grid.scene, flat, *hits_grid(grid, flat, FILL, stats_out=stats_out))


# ---- occupancy and signed distance ---------------------------------------------------------------------------------------------------------
def occupancy_rays(query, nsamples=1):
    """query [n, 3] float32 -> rays [nsamples, n, 6]: sample j from the query along DIRECTIONS[j]"""
    q = np.asarray(query).astype(f32).reshape(-1, 3)
    r = np.empty((nsamples, len(q), 6), f32)
    r[:, :, :3] = q[None]
    r[:, :, 3:] = DIRECTIONS[:nsamples, None, :]
    return r


def compute_occupancy(scene, query, nsamples=1):
    """query [..., 3] -> float32 [...]: 1 inside, 0 outside, NaN for a query with a non-finite coordinate.  Inside: the majority of the
    nsamples (odd, 1 .. 15) counts is odd"""
    assert nsamples % 2 == 1 and 1 <= nsamples <= len(DIRECTIONS)
    q = np.asarray(query).astype(f32)
    shape = q.shape[:-1]
    q = q.reshape(-1, 3)
    odd = (count_intersections(scene, occupancy_rays(q, nsamples)) & 1).sum(0)
    occ = (2 * odd > nsamples).astype(f32)
    occ[~np.isfinite(q).all(1)] = np.nan
    return occ.reshape(shape)


def compute_signed_distance(scene, query, nsamples=1):
    """closest_points' distance with its sign bit set where occupied (NaN stays NaN, no kept triangle: +inf)"""
    d = M.closest_points(scene, query)["distance"]
    return np.where(compute_occupancy(scene, query, nsamples) == 1, -d, d).astype(f32)


# ---- the experiment of the tests -------------------------------------------------------------------------------------------------------------
PARITY_DIRECTIONS = np.array([(1, 0, 0), (0, 0, -1), (1, 1, 0), (1, 1, 1), (-1, 2, 0), (1, -1, 0.5), (0.3, 0.7, -0.2)], f32)


def cube_lattice():
    """the 1 811 points of the 0.25 lattice in [-1.5, 1.5]^3 that are not on the surface of cube() -> (points float32, inside bool)"""
    a = np.arange(-6, 7) * 0.25
    p = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    m = np.abs(p).max(1)
    keep = m != 1.0
    return p[keep].astype(f32), (m < 1.0)[keep]


def rays_from(points, direction):
    return np.concatenate([points, np.broadcast_to(np.asarray(direction, f32), points.shape)], 1).astype(f32)


def edge_rays():
    """rays at the cube that run through shared edges, shared vertices, a cube edge and corner, lie in a face plane, start on the surface,
    miss, and are no rays at all"""
    r = [[0.25, 0.25, -3, 0, 0, 1],           # a diagonal of a lattice square: the edge shared by its two triangles
         [0.5, 0.25, -3, 0, 0, 1],            # a lattice edge
         [0.5, 0.5, -3, 0, 0, 1],             # a lattice vertex: a fan of six triangles
         [0.0, 0.0, -3, 0, 0, 1],             # the centre vertex
         [1.0, 0.25, -3, 0, 0, 1],            # in the plane of the face x = 1: edge-on triangles, and the rim of the faces z = +-1
         [1.0, 1.0, -3, 0, 0, 1],             # along a cube edge
         [-3, -3, -3, 1, 1, 1],               # through two cube corners
         [-3, 0.5, 0.5, 2, 0, 0],             # a vertex, direction not normalised
         [0.5, 0.5, -1, 0, 0, 1],             # starts on the surface, at a vertex: t = 0 counts
         [0.3, 0.2, 1, 0, 0, 1],              # starts on the surface and leaves
         [0.3, 0.2, 1, 0, 0, -1],             # starts on the surface and crosses
         [0.1, 0.2, 0.3, 0.3, 0.7, -0.2],     # from inside
         [3, 3, 3, 1, 0, 0],                  # a miss
         [0, 0, 0, 0, 0, 0], [np.nan, 0, 0, 1, 0, 0], [0, 0, 0, np.inf, 0, 0],
         [0.5, 0.5, -300, 0, 0, 1],           # origin beyond 8 M: the fallback list
         [0.25, 0.25, -3, 0, 2.0 ** -70, 1]]  # a direction component below 2^-60: the fallback list
    return np.array(r, f32)
