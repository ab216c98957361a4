// A scene of triangle meshes on the device (bs_mesh_*; include/bodyslam_hip.h): the nearest hit of a ray, the closest point of the surface
// to a query point, and uniform samples of the surface -- Open3D's t.geometry.RaycastingScene (add_triangles, cast_rays,
// compute_closest_points, compute_distance) and TriangleMesh.sample_points_uniformly, which the reference calls at
// BodySLAM_not_refactored/3DM/mapping_module.py:204-237,289 and 3DM/synthetic_depth_generator.py:24-97.  Restated from Open3D's documented
// interface; parity with Open3D / Embree is UNPINNED.  The statement is tests/_mesh_scene_ref.py, and every result here is bit-equal to it.
//
// Arithmetic (fp32, no contraction, every division and square root correctly rounded -- sqrtf, not __fsqrt_rn, which is the native
// approximation in this toolchain; the whole feature follows from it).
//   triangle    (triangle.h: tri_cross, tri_unit_normal, tri_cross64, tri_area64 -- the functions mesh_ops.hip's triangle geometry calls too)
//               global index = its row in the concatenation of the scene's geometries.  e1 = v1 - v0, e2 = v2 - v0,
//               n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x); KEPT when the nine coordinates and n are finite and n != 0,
//               the others are in no result.  Unit normal: m = max |n_a|, s = n / m, s / sqrt((sx sx + sy sy) + sz sz)
//   ray         (Woop, Benthin, Wald, "Watertight Ray/Triangle Intersection", JCGT 2013, restated)  kz = the first axis of largest |d|,
//               kx = kz + 1, ky = kx + 1 (mod 3), swapped when d[kz] < 0; Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].  For a
//               vertex P: A = P - o, Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz], Az = Sz A[kz].  U = Cx By - Cy Bx, V = Ax Cy - Ay Cx,
//               W = Bx Ay - By Ax.  The sheared coordinates of a vertex depend on the vertex and the ray alone, a product commutes and
//               x - y = -(y - x) exactly, so the two triangles at a shared edge compute exactly negated edge values: no ray slips between
//               them.  When one of the three is exactly 0 all three are recomputed in fp64 (the products are exact there, one rounding),
//               the signs are taken there and the values rounded to fp32; a non-zero fp32 value already has the exact sign, because
//               rounding is monotone.  Two-sided: a miss when one value is < 0 and another > 0.  det = (U + V) + W, a miss when det == 0;
//               t = ((U Az + V Bz) + W Cz) / det, one division, a hit needs 0 <= t < inf, and -0 is returned as +0;
//               uv = (V / det, W / det): p = (1 - u - v) v0 + u v1 + v v2.  The answer is the minimum of (t, global index).  A ray with a
//               non-finite component or a zero direction hits nothing
//   closest     (Ericson, "Real-Time Collision Detection", 5.1.5, restated)  the region tests of ms_closest below, dot(a, b) =
//               (ax bx + ay by) + az bz, a vertex region returns the vertex itself; d2 = (dx dx + dy dy) + dz dz with d = q - p, as
//               pc_candidate; the answer is the minimum of (d2, global index), a NaN d2 never compares
//   sampling    weight w = floor(area / max area 2^40) as a 64-bit integer, area = 0.5 sqrt((cx cx + cy cy) + cz cz) of the fp64 cross
//               product of the fp64 differences of the fp32 vertices, 0 when not kept; cum = the caller's inclusive integer scan.  Sample i
//               draws h_j = mix(mix(seed) + (3 i + j + 1) 0x9E3779B97F4A7C15), mix = the finaliser of splitmix64; its triangle is the
//               first row with cum > mulhi64(h_0, cum[T - 1]); r1, r2 = fl32(2 (h >> 40) + 1) 2^-25 -- (k + 0.5) 2^-24 rounded once --,
//               s = sqrt(r1), weights (1 - s, s (1 - r2), s r2), p = (wa A + wb B) + wc C, colours alike.  Integer weights and a counter-based
//               hash: a sample depends on (seed, i) alone, not on the launch, the batch or any order of execution
// A minimum under a total order does not depend on the order of the candidates: nothing below cares how blocks and waves share the work.
//
// Launches.
//   bs_mesh_records        one: triangle i -> three 16-byte records (v0, bit-cast global index or -1 when not kept), (v1, 0), (v2, 0); an
//                          index outside [0, V) drops the triangle before any vertex is read; counts the kept ones (integer atomic)
//   bs_mesh_cast_brute     two: a block per 64 rays (lane = ray, in each of its four waves) and per chunk of triangles, the chunk streamed
//   bs_mesh_closest_brute  through LDS tiles of 256 triangles; wave w takes triangles w, w + 4, ... of a tile, every LDS read is one 16-byte
//                          record per lane at a wave-uniform address (DESIGN section 7's rule for kernels that may run beside a second
//                          stream); the block's result goes into a 64-bit key (t or d2 bits << 32 | global index) by an integer atomicMin
//                          -- t, d2 >= +0, so the key order IS the total order.  The second launch evaluates the winning triangle again (the
//                          same function, the same bits) and writes the outputs.  Loops: tiles of a chunk, triangles of a tile -- bounded
//                          by n_triangles; the geometry of a global index by a bisection of at most 32 steps
//   bs_mesh_sample_weights two: areas and the maximum's bits (integer atomicMax: a non-negative double orders like its bits), then weights
//   bs_mesh_sample         one: a thread per sample; the bisection of cum takes at most 32 steps
//   bs_mesh_grid_count / _scatter   a thread per triangle over the cells of its padded box (its own cell range, inside the grid); integer atomics
//   bs_mesh_cast_grid      one: a thread per ray, the walk below; at most nx + ny + nz + 3 steps
//   bs_mesh_closest_grid   one: a thread per point, pc_walk (pc_grid.h) over triangle references
//   bs_mesh_hits_grid / _brute / _unpack   one each: the walk or the brute-force block with a COUNT, ANY or FILL sink; see Counting below
// No floating-point atomics anywhere: the same bits in every run.
//
// The grid and its bound.  lo, hi: the fp32 bounds of the kept triangles' vertices; cells by pc_cell; ext = the largest extent,
// M = max |lo|, |hi| + ext, pad = 2^-9 ext + 2^-14 M; a kept triangle is referenced from cell(min - pad) .. cell(max + pad) per axis.
//   Two rules of the arithmetic exist for this bound.  (1) A hit needs |det| >= 2^-12 P, P the sum of the six |products| of the edge
//   functions: an edge-on triangle, whose t would be rounding noise, is no hit.  (2) The closest point is clamped into its triangle's box.
//   Rays.  U, V, W have the exact sign for the ROUNDED sheared vertices (fp32 non-zero: monotone rounding; else fp64, exact), so for a hit the
//   origin of the sheared plane lies in the triangle of the rounded vertices: with its exact barycentrics l there, Q = sum l_i P_i is a
//   point of the true triangle within eps_s of the ray's line (the rounding of the sheared coordinates, <= 2^-21 (|o| + |P|) per axis), at
//   parameter t_Q.  The computed weights U_i / det differ from l by at most 2^-23 P / |det| <= 2^-11 (rule 1), they sum to 1 up to
//   rounding, and all have one sign, so t = sum (U_i / det) Az_i is off t_Q by at most 2^-11 of the triangle's extent in t -- at most
//   2^-11 ext |Sz| -- plus the roundings of Az and of the sum, <= 2^-20 (|o| + M) |Sz|.  slack = (2^-10 ext + pad) |Sz| 1.01 covers both
//   twice for every ray the walk takes: |o_a| <= 8 M, non-zero direction components in 2^-60 .. 2^60; the others go onto the list.
//   (b) The path.  The next boundary of axis a is ((lo_a + fl(i h)) - o_a) / d_a from the cell index i, so a boundary has ONE computed
//   parameter whatever path led to it, and the walk visits the cells in the order of these computed parameters: its states are the
//   prefixes of that order.  A computed parameter differs from the exact one by dt_a with |d_a| dt_a = delta_a <= 2^-20 (|o_a| + M): for
//   any exact t, the state "all boundaries with computed parameter <= t" differs from the ray's true cell only by boundaries the exact
//   point x(t) is within delta_a of, per axis.  So x(t) is within delta (<= 2^-17 M < pad / 4) of a visited cell -- a corner the exact ray
//   only clips is stepped around, and its triangles are listed in the cells beside it.  Clamping the start cell into the grid moves it
//   towards every Q (Q is inside the box).  With x(t_Q) within eps_s of Q and within delta of the cell of the state at t_Q, the box of
//   the triangle grown by pad > eps_s + delta + the cell function's own 2^-23 |x - lo| meets that cell: the triangle is tested there.
//   (a) Termination.  The state at t_Q has been visited once t_Q is below the current cell's computed exit t_exit.  An untested triangle
//   therefore has t_Q >= t_exit and t >= t_exit - slack / 2; the walk stops only when best < t_exit - slack, strictly, so neither a nearer
//   hit nor an equal t with a lower index is left behind.  A triangle met early whose hit lies in a later cell is just a candidate.  Start:
//   the line is cut with the box grown by pad; fp32 decides that exactly for faces moved by <= delta, so a line it rejects stays further
//   than pad - delta > eps_s from the box and hits nothing; t_Q >= -slack / 2 for a hit with t >= 0, and pad >= |d_a| slack / |d_kz| puts
//   such a Q in the start cell's lists.  A direction component of +-0: that axis has no boundary (parameter +inf, never 0 inf) and only
//   the slab test o_a in [lo_a - pad, hi_a + pad].  A late stop costs time; an early one would be a wrong answer.
//   Closest points.  After shell r the padded box of an unseen triangle is disjoint from the visited block, so pointcloud.hip's bound
//   holds for every point of the box, and rule 2 puts the computed closest point in it; its slack is taken over hi + 2 pad.
// Counting (bs_mesh_hits_*: count_intersections, list_intersections, test_occlusions; occupancy and the sign of a distance are composed
//   from the counts; the statement is tests/_mesh_hits_ref.py, parity UNPINNED).  The closed predicate above lets an edge value of exactly
//   0 be inside for both triangles at a shared edge: right for a minimum, wrong for a parity.  The COUNTING predicate (ms_ray_tri<true>)
//   is the same arithmetic with one difference: an edge value E = Qx Py - Qy Px of the edge P -> Q that is exactly 0 in fp64 takes the
//   sign of the first non-zero of (Qy - Py), -(Qx - Px), compared exactly -- the sign of E + eps (Qy - Py) + eps^2 (Px - Qx), E with the
//   ray moved by (eps, eps^2) in the sheared plane.  Both zero: E stays 0, the triangle is edge-on and det rejects it.  The two triangles
//   at an edge see P and Q reversed and decide opposite signs; around a vertex exactly one triangle of a fan claims the moved ray.  det, t,
//   u, v come from the unperturbed values.
//   Each hit exactly once.  A triangle is referenced from every cell of its box (ms_cell_range, the one expression of build and walk).
//   Along a walk every cell index is monotone per axis, so the visited cells inside a box -- a product of three intervals -- are ONE
//   contiguous run of the walk.  A triangle is tested only in the first cell of that run: the start cell, or a cell whose predecessor was
//   outside the box; the predecessor differs in the one axis just stepped, so only that axis' range is computed.
//   The bound still holds: (b) above shows that a triangle the closed predicate accepts is referenced in the VISITED cell of the state at
//   t_Q, and the counting predicate accepts a subset of those (a tie only turns a zero into a sign).  The counting walk has no early stop
//   -- (a) is not needed --, so it visits every cell the nearest-hit walk visits and more: the run of such a triangle is not empty, and
//   its first cell tests it.  ANY stops at its first hit, which is a hit whatever lies beyond.  The fallback tests are those of
//   ms_cast_grid_kernel; ms_hits_brute_kernel meets every (ray, triangle) pair in exactly one wave of one block.
//   Loops: nx + ny + nz + 3 steps, the references of a cell, n_triangles.  Integer atomics only (counts, flags, a cursor per ray for
//   keys); the rows are sorted by key afterwards (bs_pc_radius_sort; t >= +0, keys distinct), so no result depends on the order of arrival.
// Not built here: BVHs, a fused pinhole kernel.
#include <math.h>

#include <algorithm>

#include "common.h"
#include "pc_grid.h"
#include "triangle.h"

namespace bs {
namespace {

constexpr int MS_THREADS = 256, MS_RAYS = 64, MS_WAVES = MS_THREADS / 64, MS_TILE = 256;      // tile: 256 triangles = 768 records = 12 KB

// ---- rays ----------------------------------------------------------------------------------------------------------------------------------
struct MsRay {
    float ox, oy, oz;           // the origin's kx, ky, kz components
    float Sx, Sy, Sz;
    int kx, ky, kz;
    bool ok;
};

__device__ __forceinline__ float ms_pick(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

__device__ __forceinline__ MsRay ms_ray(const float* __restrict__ ray) {
    MsRay r;
    const float o0 = ray[0], o1 = ray[1], o2 = ray[2], d0 = ray[3], d1 = ray[4], d2 = ray[5];
    r.ok = pc_finite(o0) && pc_finite(o1) && pc_finite(o2) && pc_finite(d0) && pc_finite(d1) && pc_finite(d2) &&
           (d0 != 0.0f || d1 != 0.0f || d2 != 0.0f);
    int kz = 0;
    float m = fabsf(d0);
    if (fabsf(d1) > m) { kz = 1; m = fabsf(d1); }
    if (fabsf(d2) > m) kz = 2;
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const float dz = r.ok ? ms_pick(d0, d1, d2, kz) : 1.0f;
    if (dz < 0.0f) { const int s = kx; kx = ky; ky = s; }
    r.kx = kx; r.ky = ky; r.kz = kz;
    r.ox = ms_pick(o0, o1, o2, kx); r.oy = ms_pick(o0, o1, o2, ky); r.oz = ms_pick(o0, o1, o2, kz);
    r.Sx = __fdiv_rn(ms_pick(d0, d1, d2, kx), dz);
    r.Sy = __fdiv_rn(ms_pick(d0, d1, d2, ky), dz);
    r.Sz = __fdiv_rn(1.0f, dz);
    return r;
}

// the sign of the fp64 edge value e of the edge P -> Q for a COUNT: an exact 0 takes the sign e would have with the ray moved by (eps, eps^2)
// in the sheared plane, e + eps (Qy - Py) + eps^2 (Px - Qx) -- the first non-zero of the two, compared exactly; both zero: 0
__device__ __forceinline__ int ms_tie_sign(double e, float Px, float Py, float Qx, float Qy) {
    if (e > 0.0) return 1;
    if (e < 0.0) return -1;
    if (Qy != Py) return Qy > Py ? 1 : -1;
    return Qx < Px ? 1 : (Qx > Px ? -1 : 0);
}

// TIE false: the closed predicate of the nearest hit (an edge value of 0 is inside for both triangles at the edge).  TIE true: the counting
// predicate (ms_tie_sign: exactly one of them claims the ray).  Everything else -- det, t, u, v from the unperturbed values -- is shared.
template <bool TIE = false>
__device__ __forceinline__ bool ms_ray_tri(const MsRay& r, const f32x4 a, const f32x4 b, const f32x4 c, float& t, float& u, float& v) {
    const float Akz = ms_pick(a[0], a[1], a[2], r.kz) - r.oz, Bkz = ms_pick(b[0], b[1], b[2], r.kz) - r.oz, Ckz = ms_pick(c[0], c[1], c[2], r.kz) - r.oz;
    const float Ax = (ms_pick(a[0], a[1], a[2], r.kx) - r.ox) - r.Sx * Akz, Ay = (ms_pick(a[0], a[1], a[2], r.ky) - r.oy) - r.Sy * Akz;
    const float Bx = (ms_pick(b[0], b[1], b[2], r.kx) - r.ox) - r.Sx * Bkz, By = (ms_pick(b[0], b[1], b[2], r.ky) - r.oy) - r.Sy * Bkz;
    const float Cx = (ms_pick(c[0], c[1], c[2], r.kx) - r.ox) - r.Sx * Ckz, Cy = (ms_pick(c[0], c[1], c[2], r.ky) - r.oy) - r.Sy * Ckz;
    float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    bool neg, pos;
    if (U == 0.0f || V == 0.0f || W == 0.0f) {
        const double Ud = (double)Cx * (double)By - (double)Cy * (double)Bx;
        const double Vd = (double)Ax * (double)Cy - (double)Ay * (double)Cx;
        const double Wd = (double)Bx * (double)Ay - (double)By * (double)Ax;
        if (TIE) {
            const int su = ms_tie_sign(Ud, Bx, By, Cx, Cy), sv = ms_tie_sign(Vd, Cx, Cy, Ax, Ay), sw = ms_tie_sign(Wd, Ax, Ay, Bx, By);
            neg = su < 0 || sv < 0 || sw < 0;
            pos = su > 0 || sv > 0 || sw > 0;
        } else {
            neg = Ud < 0.0 || Vd < 0.0 || Wd < 0.0;
            pos = Ud > 0.0 || Vd > 0.0 || Wd > 0.0;
        }
        U = (float)Ud; V = (float)Vd; W = (float)Wd;
    } else {
        neg = U < 0.0f || V < 0.0f || W < 0.0f;
        pos = U > 0.0f || V > 0.0f || W > 0.0f;
    }
    if (neg && pos) return false;
    const float det = (U + V) + W;
    if (det == 0.0f) return false;
    // edge-on triangles are left out: with |det| below 2^-12 of the products it is made of, t would be rounding noise (see the bound below)
    const float prod = ((fabsf(Cx * By) + fabsf(Cy * Bx)) + (fabsf(Ax * Cy) + fabsf(Ay * Cx))) + (fabsf(Bx * Ay) + fabsf(By * Ax));
    if (!(fabsf(det) >= prod * 2.44140625e-04f)) return false;
    const float Az = r.Sz * Akz, Bz = r.Sz * Bkz, Cz = r.Sz * Ckz;
    t = __fdiv_rn((U * Az + V * Bz) + W * Cz, det);
    if (!(t >= 0.0f && t < INFINITY)) return false;       // (false for NaN)
    if (t == 0.0f) t = 0.0f;                              // -0 -> +0: the key below orders by the bits
    u = __fdiv_rn(V, det);
    v = __fdiv_rn(W, det);
    return true;
}

// ---- closest point -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ms_dot(const float (&a)[3], const float (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the closest point pt of the triangle to p, its (u, v), and d2
__device__ __forceinline__ float ms_closest(const f32x4 a, const f32x4 b, const f32x4 c, float px, float py, float pz, float (&pt)[3], float& u,
                                            float& v) {
    const float p[3] = {px, py, pz};
    float ab[3], ac[3], bc[3], ap[3], bp[3], cp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; bc[k] = c[k] - b[k];
        ap[k] = p[k] - a[k]; bp[k] = p[k] - b[k]; cp[k] = p[k] - c[k];
    }
    const float d1 = ms_dot(ab, ap), d2 = ms_dot(ac, ap), d3 = ms_dot(ab, bp), d4 = ms_dot(ac, bp), d5 = ms_dot(ab, cp), d6 = ms_dot(ac, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4, e43 = d4 - d3, e56 = d5 - d6;
    if (d1 <= 0.0f && d2 <= 0.0f) {
        u = 0.0f; v = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) pt[k] = a[k];
    } else if (d3 >= 0.0f && d4 <= d3) {
        u = 1.0f; v = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) pt[k] = b[k];
    } else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
        const float w = __fdiv_rn(d1, d1 - d3);
        u = w; v = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) pt[k] = a[k] + w * ab[k];
    } else if (d6 >= 0.0f && d5 <= d6) {
        u = 0.0f; v = 1.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) pt[k] = c[k];
    } else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
        const float w = __fdiv_rn(d2, d2 - d6);
        u = 0.0f; v = w;
#pragma unroll
        for (int k = 0; k < 3; ++k) pt[k] = a[k] + w * ac[k];
    } else if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) {
        const float w = __fdiv_rn(e43, e43 + e56);
        u = 1.0f - w; v = w;
#pragma unroll
        for (int k = 0; k < 3; ++k) pt[k] = b[k] + w * bc[k];
    } else {
        const float den = __fdiv_rn(1.0f, (va + vb) + vc);
        u = vb * den; v = vc * den;
#pragma unroll
        for (int k = 0; k < 3; ++k) pt[k] = (a[k] + u * ab[k]) + v * ac[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {                          // into the triangle's box (a NaN stays one): what the grid's bound stands on
        const float lo = fminf(fminf(a[k], b[k]), c[k]), hi = fmaxf(fmaxf(a[k], b[k]), c[k]);
        pt[k] = pt[k] < lo ? lo : (pt[k] > hi ? hi : pt[k]);
    }
    const float dx = p[0] - pt[0], dy = p[1] - pt[1], dz = p[2] - pt[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// ---- build ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MS_THREADS) ms_records_kernel(const float* __restrict__ vertices, int64_t n_vertices,
                                                                const int32_t* __restrict__ triangles, int64_t n_triangles,
                                                                f32x4* __restrict__ records, int32_t* __restrict__ kept) {
    const int64_t i = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= n_triangles) return;
    f32x4 p[3];
    bool keep = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t j = triangles[3 * i + k];
        const bool in = j >= 0 && j < n_vertices;
        keep = keep && in;
        const int64_t jj = in ? j : 0;                     // (never read outside the array)
        p[k] = f32x4{vertices[3 * jj], vertices[3 * jj + 1], vertices[3 * jj + 2], 0.0f};
    }
    float n[3];
    keep = tri_cross(p[0], p[1], p[2], n) && keep;
    p[0][3] = __int_as_float(keep ? (int32_t)i : -1);
    records[3 * i] = p[0];
    records[3 * i + 1] = p[1];
    records[3 * i + 2] = p[2];
    const unsigned long long b = __ballot(keep);           // one atomic per wave
    if (b && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)b) - 1)) atomicAdd(kept, (int32_t)__popcll(b));
}

// ---- brute force ---------------------------------------------------------------------------------------------------------------------------
// RAYS true: `in` holds rays [*, 6] and the key's high word is t; false: query points [*, 3] and d2
template <bool RAYS>
__global__ void __launch_bounds__(MS_THREADS) ms_brute_kernel(const f32x4* __restrict__ records, int64_t n_triangles, const float* __restrict__ in,
                                                              int64_t n_rows, int64_t m, const int32_t* __restrict__ list, int64_t chunk_len,
                                                              unsigned long long* __restrict__ keys) {
    __shared__ f32x4 tile[3 * MS_TILE];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t q = (int64_t)blockIdx.x * MS_RAYS + lane;
    bool valid = q < m;
    MsRay ray = {};
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (valid) {
        const int64_t si = list ? (int64_t)list[q] : q;
        valid = si >= 0 && si < n_rows;                     // (a listed row outside the array is no query)
    }
    if (valid) {
        const int64_t si = list ? (int64_t)list[q] : q;
        if (RAYS) {
            ray = ms_ray(in + 6 * si);
            valid = ray.ok;
        } else {
            px = in[3 * si]; py = in[3 * si + 1]; pz = in[3 * si + 2];
            valid = pc_finite(px) && pc_finite(py) && pc_finite(pz);
        }
    }
    const int64_t t0 = (int64_t)blockIdx.y * chunk_len, t1 = t0 + chunk_len < n_triangles ? t0 + chunk_len : n_triangles;
    float best = INFINITY;
    int32_t bi = PC_NONE;
    for (int64_t base = t0; base < t1; base += MS_TILE) {
        __syncthreads();
        const int cnt = t1 - base < MS_TILE ? (int)(t1 - base) : MS_TILE;
        for (int k = t; k < 3 * cnt; k += MS_THREADS) tile[k] = records[3 * base + k];
        __syncthreads();
        for (int j = w; j < cnt; j += MS_WAVES) {
            const f32x4 a = tile[3 * j], b = tile[3 * j + 1], c = tile[3 * j + 2];
            const int32_t id = __float_as_int(a[3]);
            if (id < 0 || !valid) continue;                 // (id is the same in every lane)
            float val, u, v;
            bool hit;
            if (RAYS) {
                hit = ms_ray_tri(ray, a, b, c, val, u, v);
            } else {
                float pt[3];
                val = ms_closest(a, b, c, px, py, pz, pt, u, v);
                hit = true;
            }
            if (hit && (val < best || (val == best && id < bi))) { best = val; bi = id; }
        }
    }
    if (valid && bi != PC_NONE)
        atomicMin(&keys[q], ((unsigned long long)__float_as_uint(best) << 32) | (unsigned long long)(uint32_t)bi);
}

// the geometry of global triangle gi: the last g with geom_start[g] <= gi (geom_start int32 [n_geom + 1], ascending, [0] = 0)
__device__ __forceinline__ int ms_geometry(const int32_t* __restrict__ geom_start, int n_geom, int32_t gi) {
    int lo = 0, hi = n_geom - 1;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = (lo + hi + 1) >> 1;
        if (geom_start[mid] <= gi) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct MsCastOut { float* t_hit; int32_t* geometry_ids; int32_t* primitive_ids; float* uvs; float* normals; };
struct MsClosestOut { float* points; float* distance; int32_t* geometry_ids; int32_t* primitive_ids; float* uvs; };

// row si of the outputs from the winning key (~0: none): the winner is evaluated again, the same function and the same bits
__device__ __forceinline__ void ms_cast_write(const f32x4* __restrict__ records, int64_t n_triangles, unsigned long long key,
                                              const float* __restrict__ rays, int64_t si, const int32_t* __restrict__ geom_start, int32_t n_geom,
                                              const MsCastOut& o) {
    float t = INFINITY, u = 0.0f, v = 0.0f, n[3] = {0.0f, 0.0f, 0.0f};
    int32_t geom = -1, prim = -1;
    const int64_t gi = (int64_t)(key & 0xffffffffull);
    if (key != ~0ull && gi < n_triangles) {
        const f32x4 a = records[3 * gi], b = records[3 * gi + 1], c = records[3 * gi + 2];
        const MsRay ray = ms_ray(rays + 6 * si);
        if (ray.ok && ms_ray_tri(ray, a, b, c, t, u, v)) {
            geom = ms_geometry(geom_start, n_geom, (int32_t)gi);
            prim = (int32_t)gi - geom_start[geom];
            tri_unit_normal(a, b, c, n);
        } else {
            t = INFINITY; u = 0.0f; v = 0.0f;
        }
    }
    o.t_hit[si] = t;
    o.geometry_ids[si] = geom;
    o.primitive_ids[si] = prim;
    o.uvs[2 * si] = u; o.uvs[2 * si + 1] = v;
    o.normals[3 * si] = n[0]; o.normals[3 * si + 1] = n[1]; o.normals[3 * si + 2] = n[2];
}

__device__ __forceinline__ void ms_closest_write(const f32x4* __restrict__ records, int64_t n_triangles, unsigned long long key,
                                                 const float* __restrict__ query, int64_t si, float max_distance,
                                                 const int32_t* __restrict__ geom_start, int32_t n_geom, const MsClosestOut& o) {
    const float px = query[3 * si], py = query[3 * si + 1], pz = query[3 * si + 2];
    const float nan = __builtin_nanf("");
    float pt[3] = {nan, nan, nan}, d = INFINITY, u = 0.0f, v = 0.0f;
    int32_t geom = -1, prim = -1;
    if (!(pc_finite(px) && pc_finite(py) && pc_finite(pz))) {
        d = nan;
    } else {
        const int64_t gi = (int64_t)(key & 0xffffffffull);
        if (key != ~0ull && gi < n_triangles) {
            float cpt[3], cu, cv;
            const float dd = sqrtf(ms_closest(records[3 * gi], records[3 * gi + 1], records[3 * gi + 2], px, py, pz, cpt, cu, cv));
            if (!(dd > max_distance)) {
                d = dd; u = cu; v = cv;
                pt[0] = cpt[0]; pt[1] = cpt[1]; pt[2] = cpt[2];
                geom = ms_geometry(geom_start, n_geom, (int32_t)gi);
                prim = (int32_t)gi - geom_start[geom];
            }
        }
    }
    o.points[3 * si] = pt[0]; o.points[3 * si + 1] = pt[1]; o.points[3 * si + 2] = pt[2];
    o.distance[si] = d;
    o.geometry_ids[si] = geom;
    o.primitive_ids[si] = prim;
    o.uvs[2 * si] = u; o.uvs[2 * si + 1] = v;
}

__global__ void __launch_bounds__(MS_THREADS) ms_cast_finish_kernel(const f32x4* __restrict__ records, int64_t n_triangles,
                                                                    const unsigned long long* __restrict__ keys, const float* __restrict__ rays,
                                                                    int64_t n_rows, int64_t m, const int32_t* __restrict__ list,
                                                                    const int32_t* __restrict__ geom_start, int32_t n_geom, MsCastOut o) {
    const int64_t q = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (q >= m) return;
    const int64_t si = list ? (int64_t)list[q] : q;
    if (si < 0 || si >= n_rows) return;
    ms_cast_write(records, n_triangles, keys[q], rays, si, geom_start, n_geom, o);
}

__global__ void __launch_bounds__(MS_THREADS) ms_closest_finish_kernel(const f32x4* __restrict__ records, int64_t n_triangles,
                                                                       const unsigned long long* __restrict__ keys, const float* __restrict__ query,
                                                                       int64_t n_rows, int64_t m, const int32_t* __restrict__ list, float max_distance,
                                                                       const int32_t* __restrict__ geom_start, int32_t n_geom, MsClosestOut o) {
    const int64_t q = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (q >= m) return;
    const int64_t si = list ? (int64_t)list[q] : q;
    if (si < 0 || si >= n_rows) return;
    ms_closest_write(records, n_triangles, keys[q], query, si, max_distance, geom_start, n_geom, o);
}

// ---- the grid ------------------------------------------------------------------------------------------------------------------------------
// (ms_cell_range, the cells of one axis a kept triangle is referenced from, is in triangle.h: mesh_solid.hip walks the same grid)

// SCATTER false: counts[cell] += 1 for every cell the triangle's padded box overlaps.  SCATTER true: `counts` is the cursor (a copy of the
// exclusive scan) and the triangle's index goes to its slot.  The loops run over the triangle's own cell range, inside the grid.
template <bool SCATTER>
__global__ void __launch_bounds__(MS_THREADS) ms_grid_kernel(const f32x4* __restrict__ records, int64_t n_triangles, PcGrid g, float pad,
                                                             int32_t* __restrict__ counts, int64_t n_refs, int32_t* __restrict__ refs) {
    const int64_t i = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= n_triangles) return;
    const f32x4 a = records[3 * i], b = records[3 * i + 1], c = records[3 * i + 2];
    if (__float_as_int(a[3]) < 0) return;
    int c0[3], c1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) ms_cell_range(a[k], b[k], c[k], pad, g.lo[k], g.h, g.n[k], c0[k], c1[k]);
    for (int z = c0[2]; z <= c1[2]; ++z)
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int x = c0[0]; x <= c1[0]; ++x) {
                const int32_t pos = atomicAdd(&counts[(z * g.n[1] + y) * g.n[0] + x], 1);
                if (SCATTER) {
                    if (pos >= 0 && pos < n_refs) refs[pos] = (int32_t)i;
                }
            }
}

// the triangles of one cell against the ray: the running minimum of (t, index)
__device__ __forceinline__ void ms_cast_cell(const f32x4* __restrict__ records, int64_t n_triangles, const int32_t* __restrict__ refs,
                                             const int32_t* __restrict__ cell_start, int cell, const MsRay& ray, float& best, int32_t& bi) {
    const int32_t e = cell_start[cell + 1];
    for (int32_t k = cell_start[cell]; k < e; ++k) {
        const int32_t id = refs[k];
        if (id < 0 || id >= n_triangles) continue;
        float t, u, v;
        if (ms_ray_tri(ray, records[3 * (int64_t)id], records[3 * (int64_t)id + 1], records[3 * (int64_t)id + 2], t, u, v) &&
            (t < best || (t == best && id < bi))) { best = t; bi = id; }
    }
}

// One thread per ray: the walk of the bound at the top of the file.  o_limit: the largest |origin coordinate| the padding covers.
__global__ void __launch_bounds__(MS_THREADS) ms_cast_grid_kernel(const f32x4* __restrict__ records, int64_t n_triangles,
                                                                  const int32_t* __restrict__ refs, const int32_t* __restrict__ cell_start, PcGrid g,
                                                                  float pad, float o_limit, float slack_ext, const float* __restrict__ rays, int64_t m,
                                                                  const int32_t* __restrict__ geom_start, int32_t n_geom, MsCastOut out,
                                                                  int32_t* __restrict__ fb_list, int32_t* __restrict__ fb_count) {
    const int64_t i = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= m) return;
    const MsRay ray = ms_ray(rays + 6 * i);
    if (!ray.ok) { ms_cast_write(records, n_triangles, ~0ull, rays, i, geom_start, n_geom, out); return; }
    const float ox = rays[6 * i], oy = rays[6 * i + 1], oz = rays[6 * i + 2], dx = rays[6 * i + 3], dy = rays[6 * i + 4], dz = rays[6 * i + 5];
    // a ray the padding does not cover -- an origin far from the box, a direction component outside 2^-60 .. 2^60 -- goes to brute force
    const float adx = fabsf(dx), ady = fabsf(dy), adz = fabsf(dz);
    const bool dir_ok = (dx == 0.0f || (adx >= 8.673617e-19f && adx <= 1.1529215e+18f)) && (dy == 0.0f || (ady >= 8.673617e-19f && ady <= 1.1529215e+18f)) &&
                        (dz == 0.0f || (adz >= 8.673617e-19f && adz <= 1.1529215e+18f));
    if (!dir_ok || fabsf(ox) > o_limit || fabsf(oy) > o_limit || fabsf(oz) > o_limit) {
        fb_list[atomicAdd(fb_count, 1)] = (int32_t)i;
        return;
    }
    // the line against the box grown by the padding: no part of it inside, or all of it behind the origin, is a miss
    float t_in = 0.0f, t_out = INFINITY;
    bool miss = false;
    const float ix = dx != 0.0f ? __fdiv_rn(1.0f, dx) : 0.0f, iy = dy != 0.0f ? __fdiv_rn(1.0f, dy) : 0.0f, iz = dz != 0.0f ? __fdiv_rn(1.0f, dz) : 0.0f;
#define MS_SLAB(o_, d_, inv_, a_)                                                                       \
    if (d_ == 0.0f) {                                                                                   \
        miss = miss || o_ < g.lo[a_] - pad || o_ > g.hi[a_] + pad;                                      \
    } else {                                                                                            \
        const float ta = ((g.lo[a_] - pad) - o_) * inv_, tb = ((g.hi[a_] + pad) - o_) * inv_;           \
        t_in = fmaxf(t_in, fminf(ta, tb));                                                              \
        t_out = fminf(t_out, fmaxf(ta, tb));                                                            \
    }
    MS_SLAB(ox, dx, ix, 0)
    MS_SLAB(oy, dy, iy, 1)
    MS_SLAB(oz, dz, iz, 2)
#undef MS_SLAB
    float best = INFINITY;
    int32_t bi = PC_NONE;
    if (!miss && t_in <= t_out) {
        const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
        int cx = pc_cell(ox + t_in * dx, g.lo[0], g.h, nx), cy = pc_cell(oy + t_in * dy, g.lo[1], g.h, ny), cz = pc_cell(oz + t_in * dz, g.lo[2], g.h, nz);
        const int sx = dx > 0.0f ? 1 : (dx < 0.0f ? -1 : 0), sy = dy > 0.0f ? 1 : (dy < 0.0f ? -1 : 0), sz = dz > 0.0f ? 1 : (dz < 0.0f ? -1 : 0);
        // the stop's slack in t: 2^-10 of the box's extent along the dominant axis (the error of t: the conditioning rule) and the padding
        const float slack = (slack_ext + pad) * fabsf(ray.Sz) * 1.01f;
        const int steps = nx + ny + nz + 3;
        for (int k = 0; k < steps; ++k) {
            ms_cast_cell(records, n_triangles, refs, cell_start, (cz * ny + cy) * nx + cx, ray, best, bi);
            // each axis' next boundary from the cell index, never accumulated; an axis the ray does not move along never steps
            const float tx = sx ? ((g.lo[0] + (float)(cx + (sx > 0)) * g.h) - ox) * ix : INFINITY;
            const float ty = sy ? ((g.lo[1] + (float)(cy + (sy > 0)) * g.h) - oy) * iy : INFINITY;
            const float tz = sz ? ((g.lo[2] + (float)(cz + (sz > 0)) * g.h) - oz) * iz : INFINITY;
            const float t_exit = fminf(fminf(tx, ty), tz);
            if (best < t_exit - slack) break;                      // strictly: everything unvisited is at or beyond t_exit - slack
            if (tx <= ty && tx <= tz) { cx += sx; if (cx < 0 || cx >= nx) break; }
            else if (ty <= tz) { cy += sy; if (cy < 0 || cy >= ny) break; }
            else { if (!sz) break; cz += sz; if (cz < 0 || cz >= nz) break; }
        }
    }
    const unsigned long long key = bi == PC_NONE ? ~0ull : (((unsigned long long)__float_as_uint(best) << 32) | (unsigned long long)(uint32_t)bi);
    ms_cast_write(records, n_triangles, key, rays, i, geom_start, n_geom, out);
}

// ---- every hit of a ray: counts, occlusion, lists ---------------------------------------------------------------------------------------------
// MODE: BS_MESH_HITS_COUNT  out[ray] = the hits of the counting predicate with tnear <= t <= tfar
//       BS_MESH_HITS_ANY    out[ray] = 1 when the CLOSED predicate has a hit with tnear <= t <= tfar (what cast_rays would find), else 0
//       BS_MESH_HITS_FILL   the keys (t bits << 32 | global index) of COUNT's hits into keys [row_start[ray], row_start[ray + 1])
struct MsHitsOut {
    int32_t* out;
    const int64_t* row_start;
    int64_t total;
    unsigned long long* keys;
    float tnear, tfar;
};

template <int MODE>
__device__ __forceinline__ bool ms_hits_test(const MsRay& ray, const f32x4 a, const f32x4 b, const f32x4 c, const MsHitsOut& o, float& t) {
    float u, v;
    return ms_ray_tri<MODE != BS_MESH_HITS_ANY>(ray, a, b, c, t, u, v) && t >= o.tnear && t <= o.tfar;
}

// the segment of ray `si` in keys: [b, b + cap), cap 0 for bounds that are not 0 <= b <= e <= total
__device__ __forceinline__ void ms_hits_row(const MsHitsOut& o, int64_t si, int64_t& b, int64_t& cap) {
    b = o.row_start[si];
    const int64_t e = o.row_start[si + 1];
    cap = (b >= 0 && e >= b && e <= o.total) ? e - b : 0;
}

// One thread per ray: ms_cast_grid_kernel's start, no early stop (ANY: at its first hit), and every hit exactly once -- a triangle is
// tested only in the first visited cell of its cell box (the file header, "Counting").  `last`: the axis just stepped, -1 in the start cell.
template <int MODE>
__global__ void __launch_bounds__(MS_THREADS) ms_hits_grid_kernel(const f32x4* __restrict__ records, int64_t n_triangles,
                                                                  const int32_t* __restrict__ refs, const int32_t* __restrict__ cell_start, PcGrid g,
                                                                  float pad, float o_limit, const float* __restrict__ rays, int64_t m, MsHitsOut o,
                                                                  int32_t* __restrict__ fb_list, int32_t* __restrict__ fb_count) {
    const int64_t i = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= m) return;
    if (MODE != BS_MESH_HITS_FILL) o.out[i] = 0;                   // (a ray on the list: the brute-force launch adds to it)
    const MsRay ray = ms_ray(rays + 6 * i);
    if (!ray.ok) return;
    const float ox = rays[6 * i], oy = rays[6 * i + 1], oz = rays[6 * i + 2], dx = rays[6 * i + 3], dy = rays[6 * i + 4], dz = rays[6 * i + 5];
    const float adx = fabsf(dx), ady = fabsf(dy), adz = fabsf(dz);
    const bool dir_ok = (dx == 0.0f || (adx >= 8.673617e-19f && adx <= 1.1529215e+18f)) && (dy == 0.0f || (ady >= 8.673617e-19f && ady <= 1.1529215e+18f)) &&
                        (dz == 0.0f || (adz >= 8.673617e-19f && adz <= 1.1529215e+18f));
    if (!dir_ok || fabsf(ox) > o_limit || fabsf(oy) > o_limit || fabsf(oz) > o_limit) {
        fb_list[atomicAdd(fb_count, 1)] = (int32_t)i;
        return;
    }
    float t_in = 0.0f, t_out = INFINITY;
    bool miss = false;
    const float ix = dx != 0.0f ? __fdiv_rn(1.0f, dx) : 0.0f, iy = dy != 0.0f ? __fdiv_rn(1.0f, dy) : 0.0f, iz = dz != 0.0f ? __fdiv_rn(1.0f, dz) : 0.0f;
#define MS_SLAB(o_, d_, inv_, a_)                                                                       \
    if (d_ == 0.0f) {                                                                                   \
        miss = miss || o_ < g.lo[a_] - pad || o_ > g.hi[a_] + pad;                                      \
    } else {                                                                                            \
        const float ta = ((g.lo[a_] - pad) - o_) * inv_, tb = ((g.hi[a_] + pad) - o_) * inv_;           \
        t_in = fmaxf(t_in, fminf(ta, tb));                                                              \
        t_out = fminf(t_out, fmaxf(ta, tb));                                                            \
    }
    MS_SLAB(ox, dx, ix, 0)
    MS_SLAB(oy, dy, iy, 1)
    MS_SLAB(oz, dz, iz, 2)
#undef MS_SLAB
    int32_t n = 0;
    int64_t row = 0, cap = 0;
    if (MODE == BS_MESH_HITS_FILL) ms_hits_row(o, i, row, cap);
    if (!miss && t_in <= t_out) {
        const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
        int cx = pc_cell(ox + t_in * dx, g.lo[0], g.h, nx), cy = pc_cell(oy + t_in * dy, g.lo[1], g.h, ny), cz = pc_cell(oz + t_in * dz, g.lo[2], g.h, nz);
        const int sx = dx > 0.0f ? 1 : (dx < 0.0f ? -1 : 0), sy = dy > 0.0f ? 1 : (dy < 0.0f ? -1 : 0), sz = dz > 0.0f ? 1 : (dz < 0.0f ? -1 : 0);
        const int steps = nx + ny + nz + 3;
        int last = -1;
        for (int k = 0; k < steps; ++k) {
            // the cell before this one differs in `last` alone: a triangle whose range on that axis holds it was met in an earlier cell
            const int prev = last == 0 ? cx - sx : (last == 1 ? cy - sy : cz - sz);
            const float lo_l = ms_pick(g.lo[0], g.lo[1], g.lo[2], last);
            const int n_l = last == 0 ? nx : (last == 1 ? ny : nz);
            const int cell = (cz * ny + cy) * nx + cx;
            const int32_t e = cell_start[cell + 1];
            for (int32_t r = cell_start[cell]; r < e; ++r) {
                const int32_t id = refs[r];
                if (id < 0 || id >= n_triangles) continue;
                const f32x4 a = records[3 * (int64_t)id], b = records[3 * (int64_t)id + 1], c = records[3 * (int64_t)id + 2];
                if (last >= 0) {
                    int c0, c1;
                    ms_cell_range(ms_pick(a[0], a[1], a[2], last), ms_pick(b[0], b[1], b[2], last), ms_pick(c[0], c[1], c[2], last), pad, lo_l, g.h, n_l,
                                  c0, c1);
                    if (prev >= c0 && prev <= c1) continue;
                }
                float t;
                if (!ms_hits_test<MODE>(ray, a, b, c, o, t)) continue;
                if (MODE == BS_MESH_HITS_FILL && n < cap) o.keys[row + n] = ((unsigned long long)__float_as_uint(t) << 32) | (unsigned long long)(uint32_t)id;
                ++n;
            }
            if (MODE == BS_MESH_HITS_ANY && n) break;
            const float tx = sx ? ((g.lo[0] + (float)(cx + (sx > 0)) * g.h) - ox) * ix : INFINITY;
            const float ty = sy ? ((g.lo[1] + (float)(cy + (sy > 0)) * g.h) - oy) * iy : INFINITY;
            const float tz = sz ? ((g.lo[2] + (float)(cz + (sz > 0)) * g.h) - oz) * iz : INFINITY;
            if (tx <= ty && tx <= tz) { if (!sx) break; last = 0; cx += sx; if (cx < 0 || cx >= nx) break; }
            else if (ty <= tz) { if (!sy) break; last = 1; cy += sy; if (cy < 0 || cy >= ny) break; }
            else { if (!sz) break; last = 2; cz += sz; if (cz < 0 || cz >= nz) break; }
        }
    }
    if (MODE == BS_MESH_HITS_COUNT) o.out[i] = n;
    if (MODE == BS_MESH_HITS_ANY) o.out[i] = n ? 1 : 0;
}

// The rays of `list` (or all) against every triangle, ms_brute_kernel's block: a pair (ray, triangle) is met by exactly one wave of one
// block, so its hit is counted once.  COUNT adds the block's count (integer atomicAdd), ANY sets the flag (atomicOr), FILL takes a slot
// from the ray's cursor (integer atomicAdd; cursor int32 [m], zeroed): the order of arrival is not fixed and the rows are sorted afterwards.
template <int MODE>
__global__ void __launch_bounds__(MS_THREADS) ms_hits_brute_kernel(const f32x4* __restrict__ records, int64_t n_triangles, const float* __restrict__ rays,
                                                                   int64_t n_rows, int64_t m, const int32_t* __restrict__ list, int64_t chunk_len,
                                                                   MsHitsOut o, int32_t* __restrict__ cursor) {
    __shared__ f32x4 tile[3 * MS_TILE];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t q = (int64_t)blockIdx.x * MS_RAYS + lane;
    bool valid = q < m;
    int64_t si = 0;
    if (valid) {
        si = list ? (int64_t)list[q] : q;
        valid = si >= 0 && si < n_rows;                     // (a listed row outside the array is no query)
        if (!valid) si = 0;
    }
    MsRay ray = {};
    if (valid) {
        ray = ms_ray(rays + 6 * si);
        valid = ray.ok;
    }
    int64_t row = 0, cap = 0;
    if (MODE == BS_MESH_HITS_FILL && valid) ms_hits_row(o, si, row, cap);
    const int64_t t0 = (int64_t)blockIdx.y * chunk_len, t1 = t0 + chunk_len < n_triangles ? t0 + chunk_len : n_triangles;
    int32_t n = 0;
    for (int64_t base = t0; base < t1; base += MS_TILE) {
        __syncthreads();
        const int cnt = t1 - base < MS_TILE ? (int)(t1 - base) : MS_TILE;
        for (int k = t; k < 3 * cnt; k += MS_THREADS) tile[k] = records[3 * base + k];
        __syncthreads();
        for (int j = w; j < cnt; j += MS_WAVES) {
            const f32x4 a = tile[3 * j], b = tile[3 * j + 1], c = tile[3 * j + 2];
            const int32_t id = __float_as_int(a[3]);
            if (id < 0 || !valid) continue;                 // (id is the same in every lane)
            if (MODE == BS_MESH_HITS_ANY && n) continue;
            float th;
            if (!ms_hits_test<MODE>(ray, a, b, c, o, th)) continue;
            if (MODE == BS_MESH_HITS_FILL) {
                const int64_t pos = atomicAdd(&cursor[q], 1);
                if (pos >= 0 && pos < cap) o.keys[row + pos] = ((unsigned long long)__float_as_uint(th) << 32) | (unsigned long long)(uint32_t)id;
            }
            ++n;
        }
    }
    if (valid && n) {
        if (MODE == BS_MESH_HITS_COUNT) atomicAdd(&o.out[si], n);
        if (MODE == BS_MESH_HITS_ANY) atomicOr(&o.out[si], 1);
    }
}

// row j of a sorted list: the triangle of the key against ray ray_ids[j] again (the counting predicate, the same bits) for t, uv and ids
__global__ void __launch_bounds__(MS_THREADS) ms_hits_unpack_kernel(const f32x4* __restrict__ records, int64_t n_triangles, const float* __restrict__ rays,
                                                                    int64_t n_rows, const unsigned long long* __restrict__ keys,
                                                                    const int64_t* __restrict__ ray_ids, int64_t total,
                                                                    const int32_t* __restrict__ geom_start, int32_t n_geom, float* __restrict__ t_hit,
                                                                    int32_t* __restrict__ geometry_ids, int32_t* __restrict__ primitive_ids,
                                                                    float* __restrict__ uvs) {
    const int64_t j = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (j >= total) return;
    const int64_t gi = (int64_t)(keys[j] & 0xffffffffull), si = ray_ids[j];
    float t = INFINITY, u = 0.0f, v = 0.0f;
    int32_t geom = -1, prim = -1;
    if (gi < n_triangles && si >= 0 && si < n_rows) {
        const MsRay ray = ms_ray(rays + 6 * si);
        if (ray.ok && ms_ray_tri<true>(ray, records[3 * gi], records[3 * gi + 1], records[3 * gi + 2], t, u, v)) {
            geom = ms_geometry(geom_start, n_geom, (int32_t)gi);
            prim = (int32_t)gi - geom_start[geom];
        } else {
            t = INFINITY; u = 0.0f; v = 0.0f;
        }
    }
    t_hit[j] = t;
    geometry_ids[j] = geom;
    primitive_ids[j] = prim;
    uvs[2 * j] = u; uvs[2 * j + 1] = v;
}

// The sink of pc_walk over triangle references: the minimum of (d2, index)
struct MsClosestSink {
    const f32x4* __restrict__ records;
    int64_t n_triangles;
    float px, py, pz, best;
    int32_t bi;
    __device__ __forceinline__ void add(const int32_t id) {
        if (id < 0 || id >= n_triangles) return;
        float pt[3], u, v;
        const float d2 = ms_closest(records[3 * (int64_t)id], records[3 * (int64_t)id + 1], records[3 * (int64_t)id + 2], px, py, pz, pt, u, v);
        if (d2 < best || (d2 == best && id < bi)) { best = d2; bi = id; }
    }
    __device__ __forceinline__ bool bounded(float lb2) const { return best < lb2; }
};

__global__ void __launch_bounds__(MS_THREADS) ms_closest_grid_kernel(const f32x4* __restrict__ records, int64_t n_triangles,
                                                                     const int32_t* __restrict__ refs, const int32_t* __restrict__ cell_start, PcGrid g,
                                                                     const float* __restrict__ query, int64_t m, float max_distance, int32_t shell_cap,
                                                                     const int32_t* __restrict__ geom_start, int32_t n_geom, MsClosestOut out,
                                                                     int32_t* __restrict__ fb_list, int32_t* __restrict__ fb_count) {
    const int64_t i = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= m) return;
    const float px = query[3 * i], py = query[3 * i + 1], pz = query[3 * i + 2];
    if (!(pc_finite(px) && pc_finite(py) && pc_finite(pz))) { ms_closest_write(records, n_triangles, ~0ull, query, i, max_distance, geom_start, n_geom, out); return; }
    MsClosestSink sink{records, n_triangles, px, py, pz, INFINITY, PC_NONE};
    if (!pc_walk(refs, cell_start, g, px, py, pz, max_distance, shell_cap, sink)) {          // the brute-force kernel finishes this one
        fb_list[atomicAdd(fb_count, 1)] = (int32_t)i;
        return;
    }
    const unsigned long long key =
        sink.bi == PC_NONE ? ~0ull : (((unsigned long long)__float_as_uint(sink.best) << 32) | (unsigned long long)(uint32_t)sink.bi);
    ms_closest_write(records, n_triangles, key, query, i, max_distance, geom_start, n_geom, out);
}

// ---- sampling ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MS_THREADS) ms_area_kernel(const f32x4* __restrict__ records, int64_t n_triangles, double* __restrict__ area,
                                                             unsigned long long* __restrict__ top) {
    const int64_t i = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= n_triangles) return;
    const f32x4 a = records[3 * i];
    double s = 0.0;
    if (__float_as_int(a[3]) >= 0) {
        double n[3];
        tri_cross64(a, records[3 * i + 1], records[3 * i + 2], n);
        s = tri_area64(n);
    }
    area[i] = s;
    if (s > 0.0) atomicMax(top, (unsigned long long)__double_as_longlong(s));       // (a kept triangle's area is finite)
}

__global__ void __launch_bounds__(MS_THREADS) ms_weight_kernel(const double* __restrict__ area, int64_t n_triangles,
                                                               const unsigned long long* __restrict__ top, int64_t* __restrict__ weights) {
    const int64_t i = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= n_triangles) return;
    const double mx = __longlong_as_double((long long)*top);
    int64_t w = 0;
    if (mx > 0.0 && mx < (double)INFINITY) w = (int64_t)floor(area[i] / mx * 1099511627776.0);       // 2^40
    weights[i] = w;
}

__device__ __forceinline__ uint64_t ms_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void __launch_bounds__(MS_THREADS) ms_sample_kernel(const f32x4* __restrict__ records, int64_t n_triangles, const int64_t* __restrict__ cum,
                                                               const int32_t* __restrict__ triangles, const float* __restrict__ vertex_colors,
                                                               int64_t n_vertices, uint64_t seed, uint64_t first, int64_t n,
                                                               float* __restrict__ points, float* __restrict__ colors, float* __restrict__ normals,
                                                               int32_t* __restrict__ index) {
    const int64_t k = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (k >= n) return;
    const uint64_t total = (uint64_t)cum[n_triangles - 1], s0 = ms_mix(seed), i = first + (uint64_t)k;
    const uint64_t h0 = ms_mix(s0 + (3 * i + 1) * 0x9E3779B97F4A7C15ull), h1 = ms_mix(s0 + (3 * i + 2) * 0x9E3779B97F4A7C15ull),
                   h2 = ms_mix(s0 + (3 * i + 3) * 0x9E3779B97F4A7C15ull);
    const uint64_t r = __umul64hi(h0, total);                      // < total
    int64_t lo = 0, hi = n_triangles - 1;                          // the first row with cum > r (cum[T - 1] = total > r)
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int64_t mid = (lo + hi) >> 1;
        if ((uint64_t)cum[mid] > r) hi = mid; else lo = mid + 1;
    }
    const f32x4 a = records[3 * lo], b = records[3 * lo + 1], c = records[3 * lo + 2];
    const float r1 = (float)(uint32_t)(2 * (h1 >> 40) + 1) * 2.98023223876953125e-08f;       // 2^-25
    const float r2 = (float)(uint32_t)(2 * (h2 >> 40) + 1) * 2.98023223876953125e-08f;
    const float s = sqrtf(r1), wa = 1.0f - s, wb = s * (1.0f - r2), wc = s * r2;
#pragma unroll
    for (int d = 0; d < 3; ++d) points[3 * k + d] = (wa * a[d] + wb * b[d]) + wc * c[d];
    float nrm[3];
    tri_unit_normal(a, b, c, nrm);
#pragma unroll
    for (int d = 0; d < 3; ++d) normals[3 * k + d] = nrm[d];
    index[k] = (int32_t)lo;
    if (colors) {
        const int64_t ja = triangles[3 * lo], jb = triangles[3 * lo + 1], jc = triangles[3 * lo + 2];
        const bool in = ja >= 0 && ja < n_vertices && jb >= 0 && jb < n_vertices && jc >= 0 && jc < n_vertices;     // (true for a kept triangle)
#pragma unroll
        for (int d = 0; d < 3; ++d)
            colors[3 * k + d] = in ? (wa * vertex_colors[3 * ja + d] + wb * vertex_colors[3 * jb + d]) + wc * vertex_colors[3 * jc + d] : 0.0f;
    }
}

// the brute-force launch shared by rays and closest points: enough blocks to fill the device when the queries are few
template <bool RAYS>
void ms_launch_brute(const f32x4* records, int64_t n_triangles, const float* in, int64_t n_rows, int64_t m, const int32_t* list, unsigned long long* keys,
                     hipStream_t st) {
    const int64_t sb = cdiv64(m, MS_RAYS), tiles = cdiv64(n_triangles, MS_TILE);
    const int64_t want = std::max<int64_t>(1, cdiv64(4 * (int64_t)cu_count(), sb));
    const int64_t chunk_len = cdiv64(tiles, std::min<int64_t>(std::min<int64_t>(tiles, want), 65535)) * MS_TILE;
    const int64_t chunks = cdiv64(n_triangles, chunk_len);
    hipLaunchKernelGGL((ms_brute_kernel<RAYS>), dim3((unsigned)sb, (unsigned)chunks), dim3(MS_THREADS), 0, st, records, n_triangles, in, n_rows, m, list,
                       chunk_len, keys);
}

template <int MODE>
void ms_launch_hits_brute(const f32x4* records, int64_t n_triangles, const float* rays, int64_t n_rows, int64_t m, const int32_t* list, const MsHitsOut& o,
                          int32_t* cursor, hipStream_t st) {
    const int64_t sb = cdiv64(m, MS_RAYS), tiles = cdiv64(n_triangles, MS_TILE);
    const int64_t want = std::max<int64_t>(1, cdiv64(4 * (int64_t)cu_count(), sb));
    const int64_t chunk_len = cdiv64(tiles, std::min<int64_t>(std::min<int64_t>(tiles, want), 65535)) * MS_TILE;
    const int64_t chunks = cdiv64(n_triangles, chunk_len);
    hipLaunchKernelGGL((ms_hits_brute_kernel<MODE>), dim3((unsigned)sb, (unsigned)chunks), dim3(MS_THREADS), 0, st, records, n_triangles, rays, n_rows, m,
                       list, chunk_len, o, cursor);
}

// the sink's arguments, alike for the two launches: COUNT and ANY need out, FILL needs row_start, keys and 1 <= total < 2^31
bool ms_hits_args(const char* who, int32_t mode, float tnear, float tfar, const int32_t* out, const int64_t* row_start, int64_t total, const void* keys) {
    if (mode != BS_MESH_HITS_COUNT && mode != BS_MESH_HITS_ANY && mode != BS_MESH_HITS_FILL) { set_error("%s: unknown mode %d", who, mode); return false; }
    if (!(tnear == tnear && tfar == tfar)) { set_error("%s: tnear %g, tfar %g", who, (double)tnear, (double)tfar); return false; }
    if (mode == BS_MESH_HITS_FILL ? !(row_start && keys && total >= 1 && total < ((int64_t)1 << 31) && ((uintptr_t)keys & 7) == 0) : !out) {
        set_error("%s: mode %d needs %s", who, mode, mode == BS_MESH_HITS_FILL ? "row_start, 8-byte aligned keys and 1 <= total < 2^31" : "out");
        return false;
    }
    return true;
}

}  // namespace
}  // namespace bs

#define MS_ENTER(name)                                                                       \
    using namespace bs;                                                                       \
    if (!initialized()) { set_error(name ": call bs_init first"); return BS_ERR_NOT_INIT; }

extern "C" int bs_mesh_records(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, void* records,
                               int32_t* kept, void* stream) {
    MS_ENTER("bs_mesh_records");
    BS_REQUIRE(vertices && triangles && records && kept, "bs_mesh_records: null pointer");
    BS_REQUIRE(n_vertices >= 1 && n_vertices < ((int64_t)1 << 31) && n_triangles >= 1 && n_triangles <= BS_MESH_MAX_TRIANGLES,
               "bs_mesh_records: %lld vertices, %lld triangles (1 <= V < 2^31, 1 <= T <= %d)", (long long)n_vertices, (long long)n_triangles,
               BS_MESH_MAX_TRIANGLES);
    BS_REQUIRE(((uintptr_t)records & 15) == 0, "bs_mesh_records: records must be 16-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    BS_CHECK_HIP(hipMemsetAsync(kept, 0, 4, st));
    hipLaunchKernelGGL(ms_records_kernel, dim3((unsigned)cdiv64(n_triangles, MS_THREADS)), dim3(MS_THREADS), 0, st, vertices, n_vertices, triangles,
                       n_triangles, static_cast<f32x4*>(records), kept);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_cast_brute(const void* records, int64_t n_triangles, const float* rays, int64_t n_rows, const int32_t* list, int64_t m, void* keys,
                                  const int32_t* geom_start, int32_t n_geom, float* t_hit, int32_t* geometry_ids, int32_t* primitive_ids,
                                  float* primitive_uvs, float* primitive_normals, void* stream) {
    MS_ENTER("bs_mesh_cast_brute");
    BS_REQUIRE(rays && keys && t_hit && geometry_ids && primitive_ids && primitive_uvs && primitive_normals &&
               ((records && geom_start) || n_triangles == 0), "bs_mesh_cast_brute: null pointer");
    BS_REQUIRE(n_rows >= m && n_rows < ((int64_t)1 << 31), "bs_mesh_*_brute: %lld rows for m = %lld", (long long)n_rows, (long long)m);
    BS_REQUIRE(m >= 1 && m < ((int64_t)1 << 31) && n_triangles >= 0 && n_triangles <= BS_MESH_MAX_TRIANGLES && n_geom >= (n_triangles ? 1 : 0),
               "bs_mesh_cast_brute: m = %lld, %lld triangles, %d geometries", (long long)m, (long long)n_triangles, n_geom);
    BS_REQUIRE(((uintptr_t)records & 15) == 0 && ((uintptr_t)keys & 7) == 0, "bs_mesh_cast_brute: records must be 16-byte, keys 8-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned long long* k = static_cast<unsigned long long*>(keys);
    BS_CHECK_HIP(hipMemsetAsync(k, 0xff, (size_t)m * 8, st));
    if (n_triangles > 0) {
        ms_launch_brute<true>(static_cast<const f32x4*>(records), n_triangles, rays, n_rows, m, list, k, st);
        BS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ms_cast_finish_kernel, dim3((unsigned)cdiv64(m, MS_THREADS)), dim3(MS_THREADS), 0, st, static_cast<const f32x4*>(records),
                       n_triangles, k, rays, n_rows, m, list, geom_start, n_geom,
                       MsCastOut{t_hit, geometry_ids, primitive_ids, primitive_uvs, primitive_normals});
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_closest_brute(const void* records, int64_t n_triangles, const float* query, int64_t n_rows, const int32_t* list, int64_t m,
                                     float max_distance, void* keys, const int32_t* geom_start, int32_t n_geom, float* points, float* distance,
                                     int32_t* geometry_ids, int32_t* primitive_ids, float* primitive_uvs, void* stream) {
    MS_ENTER("bs_mesh_closest_brute");
    BS_REQUIRE(query && keys && points && distance && geometry_ids && primitive_ids && primitive_uvs &&
               ((records && geom_start) || n_triangles == 0), "bs_mesh_closest_brute: null pointer");
    BS_REQUIRE(n_rows >= m && n_rows < ((int64_t)1 << 31), "bs_mesh_*_brute: %lld rows for m = %lld", (long long)n_rows, (long long)m);
    BS_REQUIRE(m >= 1 && m < ((int64_t)1 << 31) && n_triangles >= 0 && n_triangles <= BS_MESH_MAX_TRIANGLES && n_geom >= (n_triangles ? 1 : 0),
               "bs_mesh_closest_brute: m = %lld, %lld triangles, %d geometries", (long long)m, (long long)n_triangles, n_geom);
    BS_REQUIRE(((uintptr_t)records & 15) == 0 && ((uintptr_t)keys & 7) == 0, "bs_mesh_closest_brute: records must be 16-byte, keys 8-byte aligned");
    BS_REQUIRE(!(max_distance < 0.0f) && max_distance == max_distance, "bs_mesh_closest_brute: max_distance %g", (double)max_distance);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned long long* k = static_cast<unsigned long long*>(keys);
    BS_CHECK_HIP(hipMemsetAsync(k, 0xff, (size_t)m * 8, st));
    if (n_triangles > 0) {
        ms_launch_brute<false>(static_cast<const f32x4*>(records), n_triangles, query, n_rows, m, list, k, st);
        BS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ms_closest_finish_kernel, dim3((unsigned)cdiv64(m, MS_THREADS)), dim3(MS_THREADS), 0, st, static_cast<const f32x4*>(records),
                       n_triangles, k, query, n_rows, m, list, max_distance, geom_start, n_geom,
                       MsClosestOut{points, distance, geometry_ids, primitive_ids, primitive_uvs});
    BS_CHECK_LAUNCH();
    return BS_OK;
}

// ---- the grid's entry points ---------------------------------------------------------------------------------------------------------------
namespace bs {
namespace {
bool ms_grid_args(const char* who, const void* records, int64_t n_triangles, const float* lo, const float* hi, float h, const int32_t* dims, float pad,
                  PcGrid& g) {
    if (!records || !lo || !hi || !dims) { set_error("%s: null pointer", who); return false; }
    if (n_triangles < 1 || n_triangles > BS_MESH_MAX_TRIANGLES || ((uintptr_t)records & 15) != 0 || !(pad >= 0.0f) || !isfinite(pad)) {
        set_error("%s: %lld triangles, padding %g, records 16-byte aligned", who, (long long)n_triangles, (double)pad);
        return false;
    }
    g = pc_grid(lo, hi, h, dims);
    if (!pc_grid_ok(g)) { set_error("%s: bad grid (cell size %g, %d x %d x %d cells, at most 2^24)", who, (double)h, dims[0], dims[1], dims[2]); return false; }
    return true;
}
}  // namespace
}  // namespace bs

extern "C" int bs_mesh_grid_count(const void* records, int64_t n_triangles, const float* lo, const float* hi, float cell_size, const int32_t* dims,
                                  float pad, int32_t* counts, void* stream) {
    MS_ENTER("bs_mesh_grid_count");
    PcGrid g;
    if (!counts || !ms_grid_args("bs_mesh_grid_count", records, n_triangles, lo, hi, cell_size, dims, pad, g)) {
        if (!counts) set_error("bs_mesh_grid_count: null pointer");
        return BS_ERR_INVALID;
    }
    hipLaunchKernelGGL(ms_grid_kernel<false>, dim3((unsigned)cdiv64(n_triangles, MS_THREADS)), dim3(MS_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       static_cast<const f32x4*>(records), n_triangles, g, pad, counts, (int64_t)0, (int32_t*)nullptr);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_grid_scatter(const void* records, int64_t n_triangles, const float* lo, const float* hi, float cell_size, const int32_t* dims,
                                    float pad, int32_t* cursor, int64_t n_refs, int32_t* refs, void* stream) {
    MS_ENTER("bs_mesh_grid_scatter");
    PcGrid g;
    if (!cursor || !refs || n_refs < 1 || n_refs >= ((int64_t)1 << 31) ||
        !ms_grid_args("bs_mesh_grid_scatter", records, n_triangles, lo, hi, cell_size, dims, pad, g)) {
        if (!cursor || !refs || n_refs < 1 || n_refs >= ((int64_t)1 << 31)) set_error("bs_mesh_grid_scatter: null pointer or n_refs = %lld", (long long)n_refs);
        return BS_ERR_INVALID;
    }
    hipLaunchKernelGGL(ms_grid_kernel<true>, dim3((unsigned)cdiv64(n_triangles, MS_THREADS)), dim3(MS_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       static_cast<const f32x4*>(records), n_triangles, g, pad, cursor, n_refs, refs);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_cast_grid(const void* records, int64_t n_triangles, const int32_t* refs, const int32_t* cell_start, const float* lo,
                                 const float* hi, float cell_size, const int32_t* dims, float pad, float origin_limit, const float* rays, int64_t m,
                                 const int32_t* geom_start, int32_t n_geom, float* t_hit, int32_t* geometry_ids, int32_t* primitive_ids,
                                 float* primitive_uvs, float* primitive_normals, int32_t* fallback_list, int32_t* fallback_count, void* stream) {
    MS_ENTER("bs_mesh_cast_grid");
    PcGrid g;
    BS_REQUIRE(refs && cell_start && rays && geom_start && t_hit && geometry_ids && primitive_ids && primitive_uvs && primitive_normals && fallback_list &&
               fallback_count, "bs_mesh_cast_grid: null pointer");
    BS_REQUIRE(m >= 1 && m < ((int64_t)1 << 31) && n_geom >= 1 && origin_limit >= 0.0f, "bs_mesh_cast_grid: m = %lld, %d geometries, origin limit %g",
               (long long)m, n_geom, (double)origin_limit);
    if (!ms_grid_args("bs_mesh_cast_grid", records, n_triangles, lo, hi, cell_size, dims, pad, g)) return BS_ERR_INVALID;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    BS_CHECK_HIP(hipMemsetAsync(fallback_count, 0, 4, st));
    const float ext = std::max(std::max(g.hi[0] - g.lo[0], g.hi[1] - g.lo[1]), g.hi[2] - g.lo[2]);
    hipLaunchKernelGGL(ms_cast_grid_kernel, dim3((unsigned)cdiv64(m, MS_THREADS)), dim3(MS_THREADS), 0, st, static_cast<const f32x4*>(records), n_triangles,
                       refs, cell_start, g, pad, origin_limit, ext * 9.765625e-04f, rays, m, geom_start, n_geom,
                       MsCastOut{t_hit, geometry_ids, primitive_ids, primitive_uvs, primitive_normals}, fallback_list, fallback_count);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_closest_grid(const void* records, int64_t n_triangles, const int32_t* refs, const int32_t* cell_start, const float* lo,
                                    const float* hi, float cell_size, const int32_t* dims, float pad, const float* query, int64_t m, float max_distance,
                                    int32_t shell_cap, const int32_t* geom_start, int32_t n_geom, float* points, float* distance, int32_t* geometry_ids,
                                    int32_t* primitive_ids, float* primitive_uvs, int32_t* fallback_list, int32_t* fallback_count, void* stream) {
    MS_ENTER("bs_mesh_closest_grid");
    PcGrid g;
    BS_REQUIRE(refs && cell_start && query && geom_start && points && distance && geometry_ids && primitive_ids && primitive_uvs && fallback_list &&
               fallback_count, "bs_mesh_closest_grid: null pointer");
    BS_REQUIRE(m >= 1 && m < ((int64_t)1 << 31) && n_geom >= 1 && shell_cap >= 0 && !(max_distance < 0.0f) && max_distance == max_distance,
               "bs_mesh_closest_grid: m = %lld, %d geometries, shell_cap %d, max_distance %g", (long long)m, n_geom, shell_cap, (double)max_distance);
    if (!ms_grid_args("bs_mesh_closest_grid", records, n_triangles, lo, hi, cell_size, dims, pad, g)) return BS_ERR_INVALID;
    // the walk's slack is written for targets inside [lo, hi]; a padded box reaches 2 pad further (the cell function still uses lo and h)
#pragma unroll
    for (int a = 0; a < 3; ++a) g.hi[a] += 2.0f * pad;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    BS_CHECK_HIP(hipMemsetAsync(fallback_count, 0, 4, st));
    hipLaunchKernelGGL(ms_closest_grid_kernel, dim3((unsigned)cdiv64(m, MS_THREADS)), dim3(MS_THREADS), 0, st, static_cast<const f32x4*>(records), n_triangles,
                       refs, cell_start, g, query, m, max_distance, shell_cap, geom_start, n_geom,
                       MsClosestOut{points, distance, geometry_ids, primitive_ids, primitive_uvs}, fallback_list, fallback_count);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_sample_weights(const void* records, int64_t n_triangles, double* area, void* top, int64_t* weights, void* stream) {
    MS_ENTER("bs_mesh_sample_weights");
    BS_REQUIRE(records && area && top && weights, "bs_mesh_sample_weights: null pointer");
    BS_REQUIRE(n_triangles >= 1 && n_triangles <= BS_MESH_MAX_SAMPLED_TRIANGLES, "bs_mesh_sample_weights: %lld triangles (1 <= T <= 2^22)",
               (long long)n_triangles);
    BS_REQUIRE(((uintptr_t)records & 15) == 0 && ((uintptr_t)top & 7) == 0, "bs_mesh_sample_weights: records must be 16-byte, top 8-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    BS_CHECK_HIP(hipMemsetAsync(top, 0, 8, st));
    const dim3 grid((unsigned)cdiv64(n_triangles, MS_THREADS));
    hipLaunchKernelGGL(ms_area_kernel, grid, dim3(MS_THREADS), 0, st, static_cast<const f32x4*>(records), n_triangles, area,
                       static_cast<unsigned long long*>(top));
    BS_CHECK_LAUNCH();
    hipLaunchKernelGGL(ms_weight_kernel, grid, dim3(MS_THREADS), 0, st, area, n_triangles, static_cast<const unsigned long long*>(top), weights);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_sample(const void* records, int64_t n_triangles, const int64_t* cum, const int32_t* triangles, const float* vertex_colors,
                              int64_t n_vertices, uint64_t seed, uint64_t first, int64_t n, float* points, float* colors, float* normals,
                              int32_t* index, void* stream) {
    MS_ENTER("bs_mesh_sample");
    BS_REQUIRE(records && cum && points && normals && index && ((triangles && vertex_colors) || !colors) && (colors || !vertex_colors),
               "bs_mesh_sample: null pointer (colors goes with vertex_colors and triangles)");
    BS_REQUIRE(n_triangles >= 1 && n_triangles <= BS_MESH_MAX_SAMPLED_TRIANGLES && n >= 1 && n < ((int64_t)1 << 31) && n_vertices >= 1,
               "bs_mesh_sample: %lld triangles (1 <= T <= 2^22), n = %lld (1 <= n < 2^31), %lld vertices", (long long)n_triangles, (long long)n,
               (long long)n_vertices);
    BS_REQUIRE(((uintptr_t)records & 15) == 0, "bs_mesh_sample: records must be 16-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ms_sample_kernel, dim3((unsigned)cdiv64(n, MS_THREADS)), dim3(MS_THREADS), 0, st, static_cast<const f32x4*>(records),
                       n_triangles, cum, triangles, vertex_colors, n_vertices, seed, first, n, points, colors, normals, index);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

// ---- every hit of a ray --------------------------------------------------------------------------------------------------------------------
extern "C" int bs_mesh_hits_grid(const void* records, int64_t n_triangles, const int32_t* refs, const int32_t* cell_start, const float* lo,
                                 const float* hi, float cell_size, const int32_t* dims, float pad, float origin_limit, const float* rays, int64_t m,
                                 int32_t mode, float tnear, float tfar, int32_t* out, const int64_t* row_start, int64_t total, void* keys,
                                 int32_t* fallback_list, int32_t* fallback_count, void* stream) {
    MS_ENTER("bs_mesh_hits_grid");
    PcGrid g;
    BS_REQUIRE(refs && cell_start && rays && fallback_list && fallback_count, "bs_mesh_hits_grid: null pointer");
    BS_REQUIRE(m >= 1 && m < ((int64_t)1 << 31) && origin_limit >= 0.0f, "bs_mesh_hits_grid: m = %lld, origin limit %g", (long long)m,
               (double)origin_limit);
    if (!ms_hits_args("bs_mesh_hits_grid", mode, tnear, tfar, out, row_start, total, keys)) return BS_ERR_INVALID;
    if (!ms_grid_args("bs_mesh_hits_grid", records, n_triangles, lo, hi, cell_size, dims, pad, g)) return BS_ERR_INVALID;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    BS_CHECK_HIP(hipMemsetAsync(fallback_count, 0, 4, st));
    const MsHitsOut o{out, row_start, total, static_cast<unsigned long long*>(keys), tnear, tfar};
    const dim3 grid((unsigned)cdiv64(m, MS_THREADS)), block(MS_THREADS);
    const f32x4* rec = static_cast<const f32x4*>(records);
#define MS_HITS_GRID(MODE_)                                                                                                                    \
    hipLaunchKernelGGL(ms_hits_grid_kernel<MODE_>, grid, block, 0, st, rec, n_triangles, refs, cell_start, g, pad, origin_limit, rays, m, o, \
                       fallback_list, fallback_count)
    if (mode == BS_MESH_HITS_COUNT) MS_HITS_GRID(BS_MESH_HITS_COUNT);
    else if (mode == BS_MESH_HITS_ANY) MS_HITS_GRID(BS_MESH_HITS_ANY);
    else MS_HITS_GRID(BS_MESH_HITS_FILL);
#undef MS_HITS_GRID
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_hits_brute(const void* records, int64_t n_triangles, const float* rays, int64_t n_rows, const int32_t* list, int64_t m,
                                  int32_t mode, float tnear, float tfar, int32_t* out, const int64_t* row_start, int64_t total, void* keys,
                                  int32_t* cursor, void* stream) {
    MS_ENTER("bs_mesh_hits_brute");
    BS_REQUIRE(rays && (records || n_triangles == 0), "bs_mesh_hits_brute: null pointer");
    BS_REQUIRE(n_rows >= m && n_rows < ((int64_t)1 << 31), "bs_mesh_*_brute: %lld rows for m = %lld", (long long)n_rows, (long long)m);
    BS_REQUIRE(m >= 1 && n_triangles >= 0 && n_triangles <= BS_MESH_MAX_TRIANGLES, "bs_mesh_hits_brute: m = %lld, %lld triangles", (long long)m,
               (long long)n_triangles);
    BS_REQUIRE(((uintptr_t)records & 15) == 0, "bs_mesh_hits_brute: records must be 16-byte aligned");
    if (!ms_hits_args("bs_mesh_hits_brute", mode, tnear, tfar, out, row_start, total, keys)) return BS_ERR_INVALID;
    BS_REQUIRE(mode != BS_MESH_HITS_FILL || cursor, "bs_mesh_hits_brute: mode %d needs cursor", mode);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // without a list every row is this call's; with one, bs_mesh_hits_grid has zeroed the listed rows
    if (mode != BS_MESH_HITS_FILL && !list) BS_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)m * 4, st));
    if (mode == BS_MESH_HITS_FILL) BS_CHECK_HIP(hipMemsetAsync(cursor, 0, (size_t)m * 4, st));
    if (n_triangles > 0) {
        const MsHitsOut o{out, row_start, total, static_cast<unsigned long long*>(keys), tnear, tfar};
        const f32x4* rec = static_cast<const f32x4*>(records);
        if (mode == BS_MESH_HITS_COUNT) ms_launch_hits_brute<BS_MESH_HITS_COUNT>(rec, n_triangles, rays, n_rows, m, list, o, cursor, st);
        else if (mode == BS_MESH_HITS_ANY) ms_launch_hits_brute<BS_MESH_HITS_ANY>(rec, n_triangles, rays, n_rows, m, list, o, cursor, st);
        else ms_launch_hits_brute<BS_MESH_HITS_FILL>(rec, n_triangles, rays, n_rows, m, list, o, cursor, st);
        BS_CHECK_LAUNCH();
    }
    return BS_OK;
}

extern "C" int bs_mesh_hits_unpack(const void* records, int64_t n_triangles, const float* rays, int64_t n_rows, const void* keys, const int64_t* ray_ids,
                                   int64_t total, const int32_t* geom_start, int32_t n_geom, float* t_hit, int32_t* geometry_ids,
                                   int32_t* primitive_ids, float* primitive_uvs, void* stream) {
    MS_ENTER("bs_mesh_hits_unpack");
    BS_REQUIRE(records && rays && keys && ray_ids && geom_start && t_hit && geometry_ids && primitive_ids && primitive_uvs,
               "bs_mesh_hits_unpack: null pointer");
    BS_REQUIRE(n_rows >= 1 && n_rows < ((int64_t)1 << 31) && total >= 1 && total < ((int64_t)1 << 31) && n_triangles >= 1 &&
               n_triangles <= BS_MESH_MAX_TRIANGLES && n_geom >= 1, "bs_mesh_hits_unpack: %lld rays, total = %lld, %lld triangles, %d geometries",
               (long long)n_rows, (long long)total, (long long)n_triangles, n_geom);
    BS_REQUIRE(((uintptr_t)records & 15) == 0 && ((uintptr_t)keys & 7) == 0, "bs_mesh_hits_unpack: records must be 16-byte, keys 8-byte aligned");
    hipLaunchKernelGGL(ms_hits_unpack_kernel, dim3((unsigned)cdiv64(total, MS_THREADS)), dim3(MS_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       static_cast<const f32x4*>(records), n_triangles, rays, n_rows, static_cast<const unsigned long long*>(keys), ray_ids, total,
                       geom_start, n_geom, t_hit, geometry_ids, primitive_ids, primitive_uvs);
    BS_CHECK_LAUNCH();
    return BS_OK;
}
