// Is this mesh a solid (bs_mesh_fan_*, bs_mesh_solid_records, bs_mesh_pairs_*, bs_mesh_signed_volume; include/bodyslam_hip.h): the roles of
// Open3D's TriangleMesh.get_non_manifold_vertices, get_self_intersecting_triangles, is_intersecting, is_watertight and get_volume.  Restated
// from Open3D's documented meaning; parity with Open3D is UNPINNED.  The statement is tests/_mesh_solid_ref.py, DESIGN section 3.26 the
// argument.  Integer atomics only; every decision is a sign of a fixed-order fp64 expression or an exact fp32 comparison, so every result is
// the same in every run and for every grid.
//
//   fan_hook      the elements are the 3 T corners 3 t + c.  One thread per half-edge h = 3 t + c (a = tri[t][c] -> b = tri[t][(c + 1) % 3]) of
//                 edge e with first triangle u: the corner of a in t is hooked to the corner of a in u, and the corner of b likewise, by
//                 union_min.h -- cc_hook's rule over corners.  An edge of three or more triangles joins them all through its first triangle.
//   fan_compress  parent[x] = root(x).  The host repeats (hook, compress) until a hook reports no change: at most 3 T rounds report one.
//   fan_count     count[v] += 1 for every root corner of a valid triangle at v: a vertex is non-manifold iff its count exceeds 1.
//   solid_records the scene's records (three f32x4 per triangle) with the three vertex rows in the w lanes; a[3] = -1 for a triangle that is
//                 not KEPT (triangle.h), which is all the grid build (bs_mesh_grid_count / _scatter) reads of it.
//   pairs_grid    one thread per query triangle walks the cells of its own padded cell box (ms_cell_range, the build's expression).  A pair
//                 is tested only in the cell whose index per axis is max(lo_i, lo_j) of the two cell ranges: both boxes hold that cell
//                 exactly when the ranges overlap on every axis -- which they do when the fp32 boxes overlap, the cell function being
//                 monotone --, so each pair is met once, without flags or atomics.  A query triangle whose box has more than cell_cap cells
//                 goes onto the fallback list.  Self mode: the thread of i tests j > i, and only pairs without a common vertex row.
//   pairs_brute   ms_hits_brute_kernel's layout: 64 query triangles across the lanes, the other mesh streamed through LDS tiles read at
//                 wave-uniform addresses, each pair in exactly one wave of one block.
//   The predicate (so_tri_tri): closed fp32 boxes overlap, then Guigue & Devillers' test restated over the signs of orient3d -- each
//   evaluated once in canonical order: the four vertex ids sorted, fp64 differences to the lowest, det = (ux (vy wz - vz wy) + uy (vz wx -
//   vx wz)) + uz (vx wy - vy wx), sign times the parity of the sort -- and, when all three vertices of one triangle have sign 0 against
//   the other's plane, the edge-separation test over orient2d in the plane that drops the largest component of the lower triangle's normal.
//   Sinks: COUNT (a count per query triangle for the caller's scan), FILL (keys i << 32 | j into the row's segment; the caller sorts the
//   rows), ANY (one flag; a thread leaves and a block stops its tile loop once it is set).
//   signed_volume vol6[t] = a . (b x c) in fp64 over the differences to ref = v[tri[parent[t]][0]], the first vertex of the component's
//                 smallest triangle, so a component's volume depends on no other component; the caller sums with bs_mesh_segment_sum.
// Loops: the cells of a box (at most cell_cap), the references of a cell, n_triangles.  Every index read from memory is checked against
// its array before it is used.
#include <math.h>

#include <algorithm>

#include "common.h"
#include "pc_grid.h"
#include "triangle.h"
#include "union_min.h"

namespace bs {
namespace {

constexpr int SO_THREADS = 256, SO_LANES = 64, SO_WAVES = SO_THREADS / 64, SO_TILE = 256;       // tile: 256 triangles = 768 records = 12 KB

// ---- vertex fans ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SO_THREADS) fan_hook_kernel(const int32_t* __restrict__ triangles, int64_t n_triangles,
                                                              const int32_t* __restrict__ edge_of_half,
                                                              const int32_t* __restrict__ edge_first_triangle, int64_t n_edges, int32_t* parent,
                                                              int32_t* __restrict__ changed) {
    const int64_t h = (int64_t)blockIdx.x * SO_THREADS + threadIdx.x;
    if (h >= 3 * n_triangles) return;
    const int32_t e = edge_of_half[h];
    if (e < 0 || e >= n_edges) return;
    const int64_t t = h / 3;
    const int c = (int)(h - 3 * t), c1 = c == 2 ? 0 : c + 1;
    const int64_t u = edge_first_triangle[e];
    if (u < 0 || u >= n_triangles || u == t) return;
    const int32_t a = triangles[3 * t + c], b = triangles[3 * t + c1];
    const int32_t u0 = triangles[3 * u], u1 = triangles[3 * u + 1], u2 = triangles[3 * u + 2];
    const int ka = a == u0 ? 0 : (a == u1 ? 1 : (a == u2 ? 2 : -1)), kb = b == u0 ? 0 : (b == u1 ? 1 : (b == u2 ? 2 : -1));
    if (ka >= 0) cc_union(parent, (int32_t)(3 * t + c), (int32_t)(3 * u + ka), 3 * n_triangles, changed);
    if (kb >= 0) cc_union(parent, (int32_t)(3 * t + c1), (int32_t)(3 * u + kb), 3 * n_triangles, changed);
}

__global__ void __launch_bounds__(SO_THREADS) fan_compress_kernel(int32_t* parent, int64_t n_corners) {
    const int64_t x = (int64_t)blockIdx.x * SO_THREADS + threadIdx.x;
    if (x >= n_corners) return;
    cc_compress(parent, (int32_t)x, n_corners);
}

__global__ void __launch_bounds__(SO_THREADS) fan_count_kernel(const int32_t* __restrict__ triangles, int64_t n_triangles, int64_t n_vertices,
                                                               const int32_t* __restrict__ edge_of_half, const int32_t* __restrict__ parent,
                                                               int32_t* __restrict__ count) {
    const int64_t x = (int64_t)blockIdx.x * SO_THREADS + threadIdx.x;
    if (x >= 3 * n_triangles) return;
    if (edge_of_half[x] < 0 || parent[x] != (int32_t)x) return;      // (a valid triangle has all three of its half-edges)
    const int32_t v = triangles[x];
    if (v >= 0 && v < n_vertices) atomicAdd(&count[v], 1);
}

// ---- records -------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SO_THREADS) solid_records_kernel(const float* __restrict__ vertices, int64_t n_vertices,
                                                                   const int32_t* __restrict__ triangles, int64_t n_triangles,
                                                                   f32x4* __restrict__ records, int32_t* __restrict__ kept) {
    const int64_t i = (int64_t)blockIdx.x * SO_THREADS + threadIdx.x;
    bool keep = false;
    if (i < n_triangles) {
        int32_t idx[3];
        const bool valid = tri_indices(triangles, i, n_vertices, idx);
        f32x4 p[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int64_t j = valid ? idx[k] : 0;                  // (never read outside the array; n_vertices >= 1)
            p[k] = f32x4{vertices[3 * j], vertices[3 * j + 1], vertices[3 * j + 2], __int_as_float(valid ? idx[k] : -1)};
        }
        float n[3];
        keep = tri_cross(p[0], p[1], p[2], n) && valid;
        if (!keep) p[0][3] = __int_as_float(-1);
        records[3 * i] = p[0];
        records[3 * i + 1] = p[1];
        records[3 * i + 2] = p[2];
    }
    const unsigned long long b = __ballot(keep);                   // one atomic per wave (no early return: whole waves vote)
    if (b && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)b) - 1)) atomicAdd(kept, (int32_t)__popcll(b));
}

// ---- the predicate -------------------------------------------------------------------------------------------------------------------------
struct SoPoint {
    uint32_t id;                // (mesh, row): the row, with the top bit set for the second mesh
    float x, y, z;
};

__device__ __forceinline__ int so_sign(double d) { return (d > 0.0) - (d < 0.0); }

__device__ __forceinline__ void so_order(SoPoint& a, SoPoint& b, int& parity) {
    if (b.id < a.id) {
        const SoPoint t = a;
        a = b;
        b = t;
        parity = -parity;
    }
}

// the sign of det[b - a, c - a, d - a], computed once per geometric quadruple: in the order of the ids
__device__ __forceinline__ int so_orient3d(SoPoint a, SoPoint b, SoPoint c, SoPoint d) {
    int parity = 1;
    so_order(a, b, parity); so_order(c, d, parity); so_order(a, c, parity); so_order(b, d, parity); so_order(b, c, parity);
    const double ux = (double)b.x - (double)a.x, uy = (double)b.y - (double)a.y, uz = (double)b.z - (double)a.z;
    const double vx = (double)c.x - (double)a.x, vy = (double)c.y - (double)a.y, vz = (double)c.z - (double)a.z;
    const double wx = (double)d.x - (double)a.x, wy = (double)d.y - (double)a.y, wz = (double)d.z - (double)a.z;
    const double det = (ux * (vy * wz - vz * wy) + uy * (vz * wx - vx * wz)) + uz * (vx * wy - vy * wx);
    return so_sign(det) * parity;
}

__device__ __forceinline__ float so_axis(const SoPoint& p, int k) { return k == 0 ? p.x : (k == 1 ? p.y : p.z); }

__device__ __forceinline__ int so_orient2d(SoPoint a, SoPoint b, SoPoint c, int X, int Y) {
    int parity = 1;
    so_order(a, b, parity); so_order(b, c, parity); so_order(a, b, parity);
    const double ax = (double)so_axis(a, X), ay = (double)so_axis(a, Y);
    const double ux = (double)so_axis(b, X) - ax, uy = (double)so_axis(b, Y) - ay, vx = (double)so_axis(c, X) - ax, vy = (double)so_axis(c, Y) - ay;
    return so_sign(ux * vy - uy * vx) * parity;
}

__device__ __forceinline__ SoPoint so_pick(const SoPoint (&T)[3], int k) { return k == 0 ? T[0] : (k == 1 ? T[1] : T[2]); }

// the first ALONE vertex of the signs: strictly on one side with both others on the closed other side, or on the plane with both others
// strictly on one side; side: the side it lies on.  (Signs that are neither all zero nor all strictly on one side always have one.)
__device__ __forceinline__ void so_alone(int s0, int s1, int s2, int& k, int& side) {
    k = 0; side = 1;
#define SO_TRY(k_, s_, a_, b_)                                               \
    if (s_ > 0 && a_ <= 0 && b_ <= 0) { k = k_; side = 1; return; }          \
    if (s_ < 0 && a_ >= 0 && b_ >= 0) { k = k_; side = -1; return; }         \
    if (s_ == 0 && a_ * b_ > 0) { k = k_; side = -a_; return; }
    SO_TRY(0, s0, s1, s2)
    SO_TRY(1, s1, s2, s0)
    SO_TRY(2, s2, s0, s1)
#undef SO_TRY
}

// an edge line of A has all of B strictly beyond it
__device__ __forceinline__ bool so_separates(const SoPoint (&A)[3], const SoPoint (&B)[3], int X, int Y) {
    const int o = so_orient2d(A[0], A[1], A[2], X, Y);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const SoPoint a = A[k], b = A[k == 2 ? 0 : k + 1];
        if (so_orient2d(a, b, B[0], X, Y) * o < 0 && so_orient2d(a, b, B[1], X, Y) * o < 0 && so_orient2d(a, b, B[2], X, Y) * o < 0) return true;
    }
    return false;
}

__device__ __forceinline__ bool so_coplanar(const SoPoint (&T1)[3], const SoPoint (&T2)[3]) {
    const float a[3] = {T1[0].x, T1[0].y, T1[0].z}, b[3] = {T1[1].x, T1[1].y, T1[1].z}, c[3] = {T1[2].x, T1[2].y, T1[2].z};
    double n[3];
    tri_cross64(a, b, c, n);
    const double n0 = fabs(n[0]), n1 = fabs(n[1]), n2 = fabs(n[2]);
    int drop = 0;
    double best = n0;
    if (n1 > best) { drop = 1; best = n1; }
    if (n2 > best) drop = 2;
    const int X = drop == 0 ? 1 : 0, Y = drop == 2 ? 1 : 2;
    return !so_separates(T1, T2, X, Y) && !so_separates(T2, T1, X, Y);
}

// the closed triangles meet; T1 is the lower triangle, every id is distinct
__device__ __forceinline__ bool so_tri_tri(const SoPoint (&T1)[3], const SoPoint (&T2)[3]) {
    const int a0 = so_orient3d(T2[0], T2[1], T2[2], T1[0]), a1 = so_orient3d(T2[0], T2[1], T2[2], T1[1]), a2 = so_orient3d(T2[0], T2[1], T2[2], T1[2]);
    if ((a0 > 0 && a1 > 0 && a2 > 0) || (a0 < 0 && a1 < 0 && a2 < 0)) return false;
    int b0 = so_orient3d(T1[0], T1[1], T1[2], T2[0]), b1 = so_orient3d(T1[0], T1[1], T1[2], T2[1]), b2 = so_orient3d(T1[0], T1[1], T1[2], T2[2]);
    if ((b0 > 0 && b1 > 0 && b2 > 0) || (b0 < 0 && b1 < 0 && b2 < 0)) return false;
    if ((a0 == 0 && a1 == 0 && a2 == 0) || (b0 == 0 && b1 == 0 && b2 == 0)) return so_coplanar(T1, T2);
    int k, side;
    so_alone(a0, a1, a2, k, side);
    const SoPoint p1 = so_pick(T1, k);
    SoPoint q1 = so_pick(T1, k == 2 ? 0 : k + 1), r1 = so_pick(T1, k == 0 ? 2 : k - 1);
    SoPoint U[3] = {T2[0], T2[1], T2[2]};
    if (side < 0) {
        U[1] = T2[2]; U[2] = T2[1];
        const int t = b1; b1 = b2; b2 = t;
    }
    so_alone(b0, b1, b2, k, side);
    const SoPoint p2 = so_pick(U, k), q2 = so_pick(U, k == 2 ? 0 : k + 1), r2 = so_pick(U, k == 0 ? 2 : k - 1);
    if (side < 0) {
        const SoPoint t = q1; q1 = r1; r1 = t;
    }
    return so_orient3d(p1, q1, p2, q2) <= 0 && so_orient3d(p1, r1, r2, p2) <= 0;
}

// the candidate filter and the predicate for query triangle (a, b, c) and triangle (d, e, f); self: one mesh, pairs with a common vertex
// row take no part; otherwise (d, e, f) is of the second mesh
__device__ __forceinline__ bool so_pair(const f32x4 a, const f32x4 b, const f32x4 c, const f32x4 d, const f32x4 e, const f32x4 f, bool self) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float lo1 = fminf(fminf(a[k], b[k]), c[k]), hi1 = fmaxf(fmaxf(a[k], b[k]), c[k]);
        const float lo2 = fminf(fminf(d[k], e[k]), f[k]), hi2 = fmaxf(fmaxf(d[k], e[k]), f[k]);
        if (!(lo1 <= hi2 && lo2 <= hi1)) return false;
    }
    const uint32_t i0 = __float_as_uint(a[3]), i1 = __float_as_uint(b[3]), i2 = __float_as_uint(c[3]);
    uint32_t j0 = __float_as_uint(d[3]), j1 = __float_as_uint(e[3]), j2 = __float_as_uint(f[3]);
    if (self) {
        if (i0 == j0 || i0 == j1 || i0 == j2 || i1 == j0 || i1 == j1 || i1 == j2 || i2 == j0 || i2 == j1 || i2 == j2) return false;
    } else {
        j0 |= 0x80000000u; j1 |= 0x80000000u; j2 |= 0x80000000u;
    }
    const SoPoint T1[3] = {{i0, a[0], a[1], a[2]}, {i1, b[0], b[1], b[2]}, {i2, c[0], c[1], c[2]}};
    const SoPoint T2[3] = {{j0, d[0], d[1], d[2]}, {j1, e[0], e[1], e[2]}, {j2, f[0], f[1], f[2]}};
    return so_tri_tri(T1, T2);
}

// ---- the pairs -----------------------------------------------------------------------------------------------------------------------------
struct SoOut {
    int32_t* out;                       // COUNT: int32 [n_q]
    const int64_t* row_start;           // FILL: int64 [n_q + 1], keys [total]
    int64_t total;
    unsigned long long* keys;
    int32_t* any;                       // ANY: int32 [1]
};

// the segment of query triangle `si` in keys: [b, b + cap), cap 0 for bounds that are not 0 <= b <= e <= total
__device__ __forceinline__ void so_row(const SoOut& o, int64_t si, int64_t& b, int64_t& cap) {
    b = o.row_start[si];
    const int64_t e = o.row_start[si + 1];
    cap = (b >= 0 && e >= b && e <= o.total) ? e - b : 0;
}

__device__ __forceinline__ bool so_any_set(const int32_t* any) { return __hip_atomic_load(any, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0; }

template <int MODE>
__global__ void __launch_bounds__(SO_THREADS) pairs_grid_kernel(const f32x4* __restrict__ q_records, int64_t n_q, const f32x4* __restrict__ records,
                                                                int64_t n_triangles, const int32_t* __restrict__ refs, int64_t n_refs,
                                                                const int32_t* __restrict__ cell_start, PcGrid g, float pad, int self,
                                                                int64_t cell_cap, SoOut o, int32_t* __restrict__ fb_list,
                                                                int32_t* __restrict__ fb_count) {
    const int64_t i = (int64_t)blockIdx.x * SO_THREADS + threadIdx.x;
    if (i >= n_q) return;
    if (MODE == BS_MESH_PAIRS_COUNT) o.out[i] = 0;                 // (a triangle on the list: the brute-force launch adds to it)
    const f32x4 a = q_records[3 * i], b = q_records[3 * i + 1], c = q_records[3 * i + 2];
    if (__float_as_int(a[3]) < 0) return;
    if (MODE == BS_MESH_PAIRS_ANY && so_any_set(o.any)) return;
    int c0[3], c1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) ms_cell_range(a[k], b[k], c[k], pad, g.lo[k], g.h, g.n[k], c0[k], c1[k]);
    if ((int64_t)(c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1) > cell_cap) {
        const int32_t pos = atomicAdd(fb_count, 1);
        if (pos >= 0 && pos < n_q) fb_list[pos] = (int32_t)i;
        return;
    }
    int64_t row = 0, cap = 0;
    if (MODE == BS_MESH_PAIRS_FILL) so_row(o, i, row, cap);
    int32_t n = 0;
    for (int z = c0[2]; z <= c1[2]; ++z)
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int x = c0[0]; x <= c1[0]; ++x) {
                if (MODE == BS_MESH_PAIRS_ANY && so_any_set(o.any)) return;
                const int cell = (z * g.n[1] + y) * g.n[0] + x;
                int64_t rb = cell_start[cell], re = cell_start[cell + 1];
                rb = rb < 0 ? 0 : rb;
                re = re > n_refs ? n_refs : re;
                for (int64_t r = rb; r < re; ++r) {
                    const int64_t j = refs[r];
                    if (j < 0 || j >= n_triangles || (self && j <= i)) continue;
                    const f32x4 d = records[3 * j], e = records[3 * j + 1], f = records[3 * j + 2];
                    if (__float_as_int(d[3]) < 0) continue;
                    int d0, d1;                                    // the first common cell of the two boxes, axis by axis
                    ms_cell_range(d[0], e[0], f[0], pad, g.lo[0], g.h, g.n[0], d0, d1);
                    if (x != max(c0[0], d0)) continue;
                    ms_cell_range(d[1], e[1], f[1], pad, g.lo[1], g.h, g.n[1], d0, d1);
                    if (y != max(c0[1], d0)) continue;
                    ms_cell_range(d[2], e[2], f[2], pad, g.lo[2], g.h, g.n[2], d0, d1);
                    if (z != max(c0[2], d0)) continue;
                    if (!so_pair(a, b, c, d, e, f, self != 0)) continue;
                    if (MODE == BS_MESH_PAIRS_FILL && n < cap) o.keys[row + n] = ((unsigned long long)i << 32) | (unsigned long long)j;
                    ++n;
                    if (MODE == BS_MESH_PAIRS_ANY) {
                        atomicOr(o.any, 1);
                        return;
                    }
                }
            }
    if (MODE == BS_MESH_PAIRS_COUNT) o.out[i] = n;
}

// The query triangles of `list` (or all) against every triangle: a pair is met by exactly one wave of one block.  COUNT adds the block's
// count (integer atomicAdd), ANY sets the flag, FILL takes a slot from the query triangle's cursor (integer atomicAdd; cursor int32 [m],
// zeroed): the order of arrival is not fixed and the rows are sorted afterwards.
template <int MODE>
__global__ void __launch_bounds__(SO_THREADS) pairs_brute_kernel(const f32x4* __restrict__ q_records, int64_t n_q, const int32_t* __restrict__ list,
                                                                 int64_t m, const f32x4* __restrict__ records, int64_t n_triangles, int self,
                                                                 int64_t chunk_len, SoOut o, int32_t* __restrict__ cursor) {
    __shared__ f32x4 tile[3 * SO_TILE];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t q = (int64_t)blockIdx.x * SO_LANES + lane;
    bool valid = q < m;
    int64_t si = 0;
    if (valid) {
        si = list ? (int64_t)list[q] : q;
        valid = si >= 0 && si < n_q;                               // (a listed row outside the array is no query)
        if (!valid) si = 0;
    }
    f32x4 a = {}, b = {}, c = {};
    if (valid) {
        a = q_records[3 * si]; b = q_records[3 * si + 1]; c = q_records[3 * si + 2];
        valid = __float_as_int(a[3]) >= 0;
    }
    int64_t row = 0, cap = 0;
    if (MODE == BS_MESH_PAIRS_FILL && valid) so_row(o, si, row, cap);
    const int64_t t0 = (int64_t)blockIdx.y * chunk_len, t1 = t0 + chunk_len < n_triangles ? t0 + chunk_len : n_triangles;
    int32_t n = 0;
    for (int64_t base = t0; base < t1; base += SO_TILE) {
        if (MODE == BS_MESH_PAIRS_ANY) {
            if (__syncthreads_or(so_any_set(o.any) ? 1 : 0)) break;          // (the same answer in every thread of the block)
        } else {
            __syncthreads();
        }
        const int cnt = t1 - base < SO_TILE ? (int)(t1 - base) : SO_TILE;
        for (int k = t; k < 3 * cnt; k += SO_THREADS) tile[k] = records[3 * base + k];
        __syncthreads();
        for (int j = w; j < cnt; j += SO_WAVES) {
            const f32x4 d = tile[3 * j], e = tile[3 * j + 1], f = tile[3 * j + 2];
            if (__float_as_int(d[3]) < 0 || !valid) continue;      // (d is the same in every lane)
            if (self && base + j <= si) continue;
            if (MODE == BS_MESH_PAIRS_ANY && n) continue;
            if (!so_pair(a, b, c, d, e, f, self != 0)) continue;
            if (MODE == BS_MESH_PAIRS_FILL) {
                const int64_t pos = atomicAdd(&cursor[q], 1);
                if (pos >= 0 && pos < cap) o.keys[row + pos] = ((unsigned long long)si << 32) | (unsigned long long)(base + j);
            }
            ++n;
        }
        if (MODE == BS_MESH_PAIRS_ANY && n) atomicOr(o.any, 1);
    }
    if (valid && n && MODE == BS_MESH_PAIRS_COUNT) atomicAdd(&o.out[si], n);
}

// ---- volume --------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SO_THREADS) signed_volume_kernel(const float* __restrict__ vertices, int64_t n_vertices,
                                                                   const int32_t* __restrict__ triangles, int64_t n_triangles,
                                                                   const int32_t* __restrict__ parent, double* __restrict__ vol6) {
    const int64_t t = (int64_t)blockIdx.x * SO_THREADS + threadIdx.x;
    if (t >= n_triangles) return;
    double out = 0.0;
    int32_t idx[3], ridx[3];
    const int64_t r = parent[t];
    if (tri_indices(triangles, t, n_vertices, idx) && r >= 0 && r < n_triangles && tri_indices(triangles, r, n_vertices, ridx)) {
        float p[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int d = 0; d < 3; ++d) p[k][d] = vertices[3 * (int64_t)idx[k] + d];
        float n32[3];
        if (tri_cross(p[0], p[1], p[2], n32)) {
            const double rx = (double)vertices[3 * (int64_t)ridx[0]], ry = (double)vertices[3 * (int64_t)ridx[0] + 1],
                         rz = (double)vertices[3 * (int64_t)ridx[0] + 2];
            const double ax = (double)p[0][0] - rx, ay = (double)p[0][1] - ry, az = (double)p[0][2] - rz;
            const double bx = (double)p[1][0] - rx, by = (double)p[1][1] - ry, bz = (double)p[1][2] - rz;
            const double cx = (double)p[2][0] - rx, cy = (double)p[2][1] - ry, cz = (double)p[2][2] - rz;
            out = (ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz)) + az * (bx * cy - by * cx);
        }
    }
    vol6[t] = out;
}

inline bool so_count(int64_t n) { return n >= 1 && n <= (int64_t)BS_MESH_MAX_TRIANGLES; }
inline dim3 so_grid(int64_t n) { return dim3((unsigned)cdiv64(n, SO_THREADS)); }

// the sink's arguments, alike for the two launches
bool so_sink_args(const char* who, int32_t mode, const int32_t* out, const int64_t* row_start, int64_t total, const void* keys, const int32_t* any) {
    const bool ok = mode == BS_MESH_PAIRS_COUNT ? out != nullptr
                  : mode == BS_MESH_PAIRS_ANY  ? any != nullptr
                  : mode == BS_MESH_PAIRS_FILL ? (row_start && keys && total >= 1 && total < ((int64_t)1 << 31) && ((uintptr_t)keys & 7) == 0)
                                               : false;
    if (!ok) set_error("%s: mode %d needs out (COUNT), any (ANY) or row_start, 8-byte aligned keys and 1 <= total < 2^31 (FILL)", who, mode);
    return ok;
}

}  // namespace
}  // namespace bs

#define SO_ENTER(name) \
    using namespace bs; \
    if (!initialized()) { set_error(name ": call bs_init first"); return BS_ERR_NOT_INIT; } \
    hipStream_t st = reinterpret_cast<hipStream_t>(stream)

extern "C" int bs_mesh_fan_hook(const int32_t* triangles, int64_t n_triangles, const int32_t* edge_of_half, const int32_t* edge_first_triangle,
                                int64_t n_edges, int32_t* parent, int32_t* changed, void* stream) {
    SO_ENTER("bs_mesh_fan_hook");
    BS_REQUIRE(triangles && edge_of_half && parent && changed && (n_edges == 0 || edge_first_triangle), "bs_mesh_fan_hook: null pointer");
    BS_REQUIRE(so_count(n_triangles) && n_edges >= 0 && n_edges <= 3 * n_triangles, "bs_mesh_fan_hook: T = %lld, E = %lld", (long long)n_triangles,
               (long long)n_edges);
    hipLaunchKernelGGL(fan_hook_kernel, so_grid(3 * n_triangles), dim3(SO_THREADS), 0, st, triangles, n_triangles, edge_of_half, edge_first_triangle,
                       n_edges, parent, changed);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_fan_compress(int32_t* parent, int64_t n_corners, void* stream) {
    SO_ENTER("bs_mesh_fan_compress");
    BS_REQUIRE(parent && n_corners >= 3 && n_corners <= 3 * (int64_t)BS_MESH_MAX_TRIANGLES, "bs_mesh_fan_compress: parent %p, %lld corners",
               (void*)parent, (long long)n_corners);
    hipLaunchKernelGGL(fan_compress_kernel, so_grid(n_corners), dim3(SO_THREADS), 0, st, parent, n_corners);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_fan_count(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, const int32_t* edge_of_half, const int32_t* parent,
                                 int32_t* count, void* stream) {
    SO_ENTER("bs_mesh_fan_count");
    BS_REQUIRE(triangles && edge_of_half && parent && count, "bs_mesh_fan_count: null pointer");
    BS_REQUIRE(so_count(n_triangles) && n_vertices >= 1 && n_vertices < ((int64_t)1 << 31), "bs_mesh_fan_count: T = %lld, V = %lld",
               (long long)n_triangles, (long long)n_vertices);
    hipLaunchKernelGGL(fan_count_kernel, so_grid(3 * n_triangles), dim3(SO_THREADS), 0, st, triangles, n_triangles, n_vertices, edge_of_half, parent,
                       count);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_solid_records(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, void* records,
                                     int32_t* kept, void* stream) {
    SO_ENTER("bs_mesh_solid_records");
    BS_REQUIRE(vertices && triangles && records && kept, "bs_mesh_solid_records: null pointer");
    BS_REQUIRE(so_count(n_triangles) && n_vertices >= 1 && n_vertices < ((int64_t)1 << 31), "bs_mesh_solid_records: T = %lld, V = %lld",
               (long long)n_triangles, (long long)n_vertices);
    BS_REQUIRE(((uintptr_t)records & 15) == 0, "bs_mesh_solid_records: records must be 16-byte aligned");
    BS_CHECK_HIP(hipMemsetAsync(kept, 0, 4, st));
    hipLaunchKernelGGL(solid_records_kernel, so_grid(n_triangles), dim3(SO_THREADS), 0, st, vertices, n_vertices, triangles, n_triangles,
                       static_cast<f32x4*>(records), kept);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_pairs_grid(const void* q_records, int64_t n_q, const void* records, int64_t n_triangles, const int32_t* refs, int64_t n_refs,
                                  const int32_t* cell_start, const float* lo, const float* hi, float cell_size, const int32_t* dims, float pad,
                                  int32_t self, int64_t cell_cap, int32_t mode, int32_t* out, const int64_t* row_start, int64_t total, void* keys,
                                  int32_t* any, int32_t* fallback_list, int32_t* fallback_count, void* stream) {
    SO_ENTER("bs_mesh_pairs_grid");
    BS_REQUIRE(q_records && records && refs && cell_start && lo && hi && dims && fallback_list && fallback_count, "bs_mesh_pairs_grid: null pointer");
    BS_REQUIRE(so_count(n_q) && so_count(n_triangles) && n_refs >= 1 && n_refs < ((int64_t)1 << 31) && cell_cap >= 1 &&
               (!self || (q_records == records && n_q == n_triangles)),
               "bs_mesh_pairs_grid: %lld query triangles, %lld triangles, %lld references, cell cap %lld (self: one set of records)", (long long)n_q,
               (long long)n_triangles, (long long)n_refs, (long long)cell_cap);
    BS_REQUIRE((((uintptr_t)q_records | (uintptr_t)records) & 15) == 0 && pad >= 0.0f && isfinite(pad),
               "bs_mesh_pairs_grid: records must be 16-byte aligned, padding %g", (double)pad);
    const PcGrid g = pc_grid(lo, hi, cell_size, dims);
    BS_REQUIRE(pc_grid_ok(g), "bs_mesh_pairs_grid: bad grid (cell size %g, %d x %d x %d cells, at most 2^24)", (double)cell_size, dims[0], dims[1],
               dims[2]);
    if (!so_sink_args("bs_mesh_pairs_grid", mode, out, row_start, total, keys, any)) return BS_ERR_INVALID;
    BS_CHECK_HIP(hipMemsetAsync(fallback_count, 0, 4, st));
    const SoOut o{out, row_start, total, static_cast<unsigned long long*>(keys), any};
    const f32x4 *qr = static_cast<const f32x4*>(q_records), *rr = static_cast<const f32x4*>(records);
#define SO_GRID(MODE_)                                                                                                                             \
    hipLaunchKernelGGL((pairs_grid_kernel<MODE_>), so_grid(n_q), dim3(SO_THREADS), 0, st, qr, n_q, rr, n_triangles, refs, n_refs, cell_start, g, pad, \
                       (int)(self != 0), cell_cap, o, fallback_list, fallback_count)
    if (mode == BS_MESH_PAIRS_COUNT) SO_GRID(BS_MESH_PAIRS_COUNT);
    else if (mode == BS_MESH_PAIRS_ANY) SO_GRID(BS_MESH_PAIRS_ANY);
    else SO_GRID(BS_MESH_PAIRS_FILL);
#undef SO_GRID
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_pairs_brute(const void* q_records, int64_t n_q, const int32_t* list, int64_t m, const void* records, int64_t n_triangles,
                                   int32_t self, int32_t mode, int32_t* out, const int64_t* row_start, int64_t total, void* keys, int32_t* cursor,
                                   int32_t* any, void* stream) {
    SO_ENTER("bs_mesh_pairs_brute");
    BS_REQUIRE(q_records && records, "bs_mesh_pairs_brute: null pointer");
    BS_REQUIRE(so_count(n_q) && so_count(n_triangles) && m >= 1 && m <= n_q && (list || m == n_q) &&
               (!self || (q_records == records && n_q == n_triangles)),
               "bs_mesh_pairs_brute: %lld query triangles, m = %lld, %lld triangles (self: one set of records)", (long long)n_q, (long long)m,
               (long long)n_triangles);
    BS_REQUIRE((((uintptr_t)q_records | (uintptr_t)records) & 15) == 0, "bs_mesh_pairs_brute: records must be 16-byte aligned");
    if (!so_sink_args("bs_mesh_pairs_brute", mode, out, row_start, total, keys, any)) return BS_ERR_INVALID;
    BS_REQUIRE(mode != BS_MESH_PAIRS_FILL || cursor, "bs_mesh_pairs_brute: FILL needs a cursor");
    if (mode == BS_MESH_PAIRS_COUNT && !list) BS_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)n_q * 4, st));
    if (mode == BS_MESH_PAIRS_FILL) BS_CHECK_HIP(hipMemsetAsync(cursor, 0, (size_t)m * 4, st));
    const SoOut o{out, row_start, total, static_cast<unsigned long long*>(keys), any};
    const f32x4 *qr = static_cast<const f32x4*>(q_records), *rr = static_cast<const f32x4*>(records);
    // enough blocks to fill the device when the query triangles are few (ms_launch_hits_brute's rule)
    const int64_t sb = cdiv64(m, SO_LANES), tiles = cdiv64(n_triangles, SO_TILE);
    const int64_t want = std::max<int64_t>(1, cdiv64(4 * (int64_t)cu_count(), sb));
    const int64_t chunk_len = cdiv64(tiles, std::min<int64_t>(std::min<int64_t>(tiles, want), 65535)) * SO_TILE;
    const int64_t chunks = cdiv64(n_triangles, chunk_len);
#define SO_BRUTE(MODE_)                                                                                                                       \
    hipLaunchKernelGGL((pairs_brute_kernel<MODE_>), dim3((unsigned)sb, (unsigned)chunks), dim3(SO_THREADS), 0, st, qr, n_q, list, m, rr, n_triangles, \
                       (int)(self != 0), chunk_len, o, cursor)
    if (mode == BS_MESH_PAIRS_COUNT) SO_BRUTE(BS_MESH_PAIRS_COUNT);
    else if (mode == BS_MESH_PAIRS_ANY) SO_BRUTE(BS_MESH_PAIRS_ANY);
    else SO_BRUTE(BS_MESH_PAIRS_FILL);
#undef SO_BRUTE
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_signed_volume(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, const int32_t* parent,
                                     double* vol6, void* stream) {
    SO_ENTER("bs_mesh_signed_volume");
    BS_REQUIRE(vertices && triangles && parent && vol6, "bs_mesh_signed_volume: null pointer");
    BS_REQUIRE(so_count(n_triangles) && n_vertices >= 1 && n_vertices < ((int64_t)1 << 31), "bs_mesh_signed_volume: T = %lld, V = %lld",
               (long long)n_triangles, (long long)n_vertices);
    hipLaunchKernelGGL(signed_volume_kernel, so_grid(n_triangles), dim3(SO_THREADS), 0, st, vertices, n_vertices, triangles, n_triangles, parent,
                       vol6);
    BS_CHECK_LAUNCH();
    return BS_OK;
}
