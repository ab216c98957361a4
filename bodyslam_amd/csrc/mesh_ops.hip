// Mesh topology and clean-up (bs_mesh_edge_*, bs_mesh_cc_*, bs_mesh_segment_sum, bs_mesh_triangle_geometry, bs_mesh_vertex_normals,
// bs_mesh_laplacian_step, bs_mesh_orient_*; include/bodyslam_hip.h): the roles of Open3D's TriangleMesh.cluster_connected_triangles,
// get_non_manifold_edges, compute_triangle_normals, compute_vertex_normals, get_surface_area, filter_smooth_laplacian, filter_smooth_taubin,
// is_orientable and orient_triangles.  Restated from Open3D's documented meaning; parity with Open3D is UNPINNED.  The statement is
// tests/_mesh_ops_ref.py (tests/_orient_ref.py for bs_mesh_orient_*), DESIGN section 3.21 the argument (3.24 for the orientation).
//
//   edge_insert   one thread per half-edge h = 3 t + c (a = tri[t][c] -> b = tri[t][(c + 1) % 3]) of a valid triangle inserts the key
//                 min(a, b) << 32 | max(a, b) into the open-addressing table of 64-bit keys of slot_table.h (slot_insert: the table voxel.hip
//                 uses too), then three integer atomics on the slot: the minimum of h, the count, and the count of half-edges with a < b.
//                 A table without room after `slots` probes sets BS_MESH_EDGE_TABLE_FULL.
//   edge_flags    slot_table.h's flags kernel: leader[h] = first_half[slot_h], is_first[h] = (leader[h] == h); the caller's inclusive scan of is_first is the edge's rank:
//                 edges are numbered in the order of their first half-edge, whatever slot they got.
//   edge_rows     one thread per half-edge writes edge_of_half; the first half-edge of an edge writes the edge's row.
//   cc_hook       one thread per half-edge: the roots of its triangle and of its edge's first triangle; when they differ, atomicMin of the
//                 smaller root into the larger root's parent and changed = 1.  parent[x] <= x always (it starts as x and only decreases), so a
//                 root walk strictly descends: at most T steps, no spin, no retry loop.
//   cc_compress   parent[t] = root(t).  The host repeats (hook, compress) until a hook reports no change; every round that reports one turns
//                 at least one root into a non-root for good, so there are at most T such rounds.  At the fixed point every triangle of a
//                 component has the same root, and since root(x) <= x it is the component's smallest index: unique whatever the schedule.
//   cc_roots / cc_clusters   is_root flags for the caller's scan; cluster = rank of the root - 1, the sizes by integer atomics (one per distinct
//                 cluster of a wave).
//   orient_hook / _compress / _check / _flip   the winding: every edge of exactly two triangles links them with s = (edge_forward != 1) -- 0 when
//                 the two run it in opposite directions, as neighbours of one orientation do -- through union_parity.h; edges of any other
//                 count link nothing and connect nothing.  Rounds of (hook, compress) until a hook reports no change; check re-tests every
//                 link against the stored parities and marks the root of a violated one; flip swaps the last two corners of every triangle
//                 of an unmarked component whose parity to the component's smallest triangle is 1.
//   segment_sum   one wave per segment of an fp64 array, reduce.h's column_sum order: cluster areas and the surface area.
//   triangle_geometry   triangle.h, the functions mesh_scene.hip calls too: validity, the fp32 cross product with the kept rule, the unit
//                 normal, the fp64 cross product and area.
//   vertex_normals      one thread per vertex adds the fp64 cross products of its corners in ascending corner number (the caller's stable
//                 sort of the corners by vertex): the store-then-sum-per-destination form, no float atomics.
//   laplacian_step      one thread per vertex gathers its neighbours (CSR, ascending) in fp64 and writes a second buffer.
// No floating-point atomics anywhere; every index read from memory is checked against its array before it is used.
#include <math.h>

#include "common.h"
#include "pc_grid.h"
#include "reduce.h"
#include "slot_table.h"
#include "triangle.h"
#include "union_min.h"
#include "union_parity.h"

namespace bs {
namespace {

constexpr int MO_THREADS = 256;
typedef slot_key edge_key;

__global__ void __launch_bounds__(MO_THREADS) edge_insert_kernel(const int32_t* __restrict__ triangles, int64_t n_triangles, int64_t n_vertices,
                                                                 edge_key* __restrict__ keys, int32_t* __restrict__ first_half,
                                                                 int32_t* __restrict__ count, int32_t* __restrict__ forward, int64_t slots,
                                                                 int32_t* __restrict__ slot_of_half, int32_t* __restrict__ status) {
    const int64_t h = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    if (h >= 3 * n_triangles) return;
    const int64_t t = h / 3;
    const int c = (int)(h - 3 * t);
    int32_t v[3];
    int32_t found = -1;
    if (tri_indices(triangles, t, n_vertices, v)) {
        const int32_t a = v[c], b = v[c == 2 ? 0 : c + 1];
        found = slot_insert(keys, slots, ((edge_key)(a < b ? a : b) << 32) | (edge_key)(a < b ? b : a));
        if (found < 0) {
            atomicOr(&status[0], BS_MESH_EDGE_TABLE_FULL);
        } else {
            atomicMin(&first_half[found], (int32_t)h);
            atomicAdd(&count[found], 1);
            if (a < b) atomicAdd(&forward[found], 1);
        }
    } else if (c == 0) {
        atomicAdd(&status[1], 1);
    }
    slot_of_half[h] = found;
}

__global__ void __launch_bounds__(MO_THREADS) edge_rows_kernel(const int32_t* __restrict__ triangles, int64_t n_triangles,
                                                               const int32_t* __restrict__ slot_of_half, const int32_t* __restrict__ count,
                                                               const int32_t* __restrict__ forward, int64_t slots,
                                                               const int32_t* __restrict__ leader, const int32_t* __restrict__ rank,
                                                               int64_t n_edges, int32_t* __restrict__ edges, int32_t* __restrict__ edge_count,
                                                               int32_t* __restrict__ edge_forward, int32_t* __restrict__ edge_first_triangle,
                                                               int32_t* __restrict__ edge_of_half) {
    const int64_t h = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    const int64_t n_half = 3 * n_triangles;
    if (h >= n_half) return;
    const int32_t slot = slot_of_half[h], ld = leader[h];
    int32_t e = -1;
    if (slot >= 0 && slot < slots && ld >= 0 && ld < n_half) {
        const int32_t r = rank[ld] - 1;
        if (r >= 0 && r < n_edges) e = r;
    }
    edge_of_half[h] = e;
    if (e >= 0 && ld == (int32_t)h) {
        const int64_t t = h / 3;
        const int c = (int)(h - 3 * t);
        const int32_t a = triangles[3 * t + c], b = triangles[3 * t + (c == 2 ? 0 : c + 1)];
        edges[2 * (int64_t)e] = a < b ? a : b;
        edges[2 * (int64_t)e + 1] = a < b ? b : a;
        edge_count[e] = count[slot];
        edge_forward[e] = forward[slot];
        edge_first_triangle[e] = (int32_t)t;
    }
}

// ---- components (the root walk, the hook and the compression: union_min.h, shared with radius.hip) --------------------------------------------
__global__ void __launch_bounds__(MO_THREADS) cc_hook_kernel(const int32_t* __restrict__ edge_of_half,
                                                             const int32_t* __restrict__ edge_first_triangle, int64_t n_triangles,
                                                             int64_t n_edges, int32_t* parent, int32_t* __restrict__ changed) {
    const int64_t h = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    if (h >= 3 * n_triangles) return;
    const int32_t e = edge_of_half[h];
    if (e < 0 || e >= n_edges) return;
    const int32_t u = edge_first_triangle[e], t = (int32_t)(h / 3);
    if (u < 0 || u >= n_triangles || u == t) return;
    cc_union(parent, t, u, n_triangles, changed);
}

__global__ void __launch_bounds__(MO_THREADS) cc_compress_kernel(int32_t* parent, int64_t n_triangles) {
    const int64_t t = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    if (t >= n_triangles) return;
    cc_compress(parent, (int32_t)t, n_triangles);
}

__global__ void __launch_bounds__(MO_THREADS) cc_roots_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ edge_of_half,
                                                              int64_t n_triangles, int32_t* __restrict__ is_root) {
    const int64_t t = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    if (t >= n_triangles) return;
    is_root[t] = edge_of_half[3 * t] >= 0 && parent[t] == (int32_t)t ? 1 : 0;       // (a valid triangle has all three of its half-edges)
}

__global__ void __launch_bounds__(MO_THREADS) cc_clusters_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ edge_of_half,
                                                                 const int32_t* __restrict__ rank, int64_t n_triangles, int64_t n_clusters,
                                                                 int32_t* __restrict__ triangle_clusters,
                                                                 int32_t* __restrict__ cluster_n_triangles) {
    // (no early return: every lane of the wave takes part in the ballots below; the block is a whole number of waves)
    const int64_t t = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    int32_t c = -1;
    if (t < n_triangles) {
        if (edge_of_half[3 * t] >= 0) {
            const int32_t r = parent[t];
            if (r >= 0 && r < n_triangles) {
                const int32_t k = rank[r] - 1;
                if (k >= 0 && k < n_clusters) c = k;
            }
        }
        triangle_clusters[t] = c;
    }
    // one atomic per distinct cluster of the wave (integer addition is associative: the same counts): a mesh is mostly one component, and
    // half a million adds of 1 to one address took 6 ms where the rest of the labelling takes 1.  At most 64 turns, one per lane.
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(c >= 0);
    for (int turn = 0; turn < 64 && todo; ++turn) {
        const int first = __ffsll((long long)todo) - 1;
        const int32_t cf = __shfl(c, first);
        const unsigned long long same = __ballot(c == cf) & todo;
        if (lane == first) atomicAdd(&cluster_n_triangles[cf], (int32_t)__popcll(same));
        todo &= ~same;
    }
}

// ---- winding (the parity walk, the hook and the compression: union_parity.h, shared with orient.hip) -------------------------------------------
// the link of half-edge h: its triangle t and the first triangle u of its edge, when the edge has exactly two triangles and t is the other one
__device__ __forceinline__ bool orient_link(const int32_t* __restrict__ edge_of_half, const int32_t* __restrict__ edge_count,
                                            const int32_t* __restrict__ edge_forward, const int32_t* __restrict__ edge_first_triangle,
                                            int64_t n_triangles, int64_t n_edges, int64_t h, uint32_t& t, uint32_t& u, uint32_t& s) {
    if (h >= 3 * n_triangles) return false;
    const int32_t e = edge_of_half[h];
    if (e < 0 || e >= n_edges || edge_count[e] != 2) return false;
    const int32_t first = edge_first_triangle[e];
    t = (uint32_t)(h / 3);
    if (first < 0 || first >= n_triangles || (uint32_t)first == t) return false;
    u = (uint32_t)first;
    s = edge_forward[e] != 1 ? 1u : 0u;
    return true;
}

__global__ void __launch_bounds__(MO_THREADS) orient_hook_kernel(const int32_t* __restrict__ edge_of_half, const int32_t* __restrict__ edge_count,
                                                                 const int32_t* __restrict__ edge_forward,
                                                                 const int32_t* __restrict__ edge_first_triangle, int64_t n_triangles,
                                                                 int64_t n_edges, uint32_t* word, int32_t* __restrict__ changed) {
    const int64_t h = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    uint32_t t, u, s;
    if (!orient_link(edge_of_half, edge_count, edge_forward, edge_first_triangle, n_triangles, n_edges, h, t, u, s)) return;
    if (up_union(word, t, u, s, n_triangles)) *changed = 1;          // (every writer stores the same value)
}

__global__ void __launch_bounds__(MO_THREADS) orient_compress_kernel(uint32_t* word, int64_t n_triangles) {
    const int64_t t = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    if (t >= n_triangles) return;
    up_compress(word, (uint32_t)t, n_triangles);
}

// after the fixed point and a compression word[t] = root << 1 | parity to the root: a link that the parities do not satisfy marks the root
__global__ void __launch_bounds__(MO_THREADS) orient_check_kernel(const int32_t* __restrict__ edge_of_half, const int32_t* __restrict__ edge_count,
                                                                  const int32_t* __restrict__ edge_forward,
                                                                  const int32_t* __restrict__ edge_first_triangle, int64_t n_triangles,
                                                                  int64_t n_edges, const uint32_t* __restrict__ word, int32_t* __restrict__ bad) {
    const int64_t h = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    uint32_t t, u, s;
    if (!orient_link(edge_of_half, edge_count, edge_forward, edge_first_triangle, n_triangles, n_edges, h, t, u, s)) return;
    const uint32_t wt = word[t], wu = word[u], r = wt >> 1;
    if (r >= n_triangles) return;
    if ((wu >> 1) != r || ((wt ^ wu) & 1u) != s) bad[r] = 1;          // (every writer stores the same value)
}

__global__ void __launch_bounds__(MO_THREADS) orient_flip_kernel(const int32_t* __restrict__ triangles, const int32_t* __restrict__ edge_of_half,
                                                                 const uint32_t* __restrict__ word, const int32_t* __restrict__ bad,
                                                                 int64_t n_triangles, int32_t* __restrict__ out, uint8_t* __restrict__ flipped) {
    const int64_t t = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    if (t >= n_triangles) return;
    bool flip = false;
    if (edge_of_half[3 * t] >= 0) {                                  // (a valid triangle has all three of its half-edges)
        const uint32_t w = word[t], r = w >> 1;
        flip = r < n_triangles && !bad[r] && (w & 1u);
    }
    const int32_t a = triangles[3 * t], b = triangles[3 * t + 1], c = triangles[3 * t + 2];
    out[3 * t] = a; out[3 * t + 1] = flip ? c : b; out[3 * t + 2] = flip ? b : c;
    flipped[t] = flip ? 1 : 0;
}

// out[s] = the sum of values[start[s] .. start[s + 1]) by one wave, column_sum's order: lane l adds elements l, l + 64, ... in order, then
// the butterfly.  The loads of eight steps are issued together; the additions keep their order.
__global__ void __launch_bounds__(MO_THREADS) segment_sum_kernel(const double* __restrict__ values, int64_t n_values,
                                                                 const int64_t* __restrict__ start, int64_t n_segments,
                                                                 double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * (MO_THREADS / 64) + (threadIdx.x >> 6);
    if (s >= n_segments) return;                                     // (whole waves leave together)
    int64_t a = start[s], b = start[s + 1];
    a = a < 0 ? 0 : a;
    b = b > n_values ? n_values : b;
    double sum = 0.0;
    int64_t i = a + lane;
    for (; i + 7 * 64 < b; i += 8 * 64) {
        double x[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = values[i + 64 * k];
#pragma unroll
        for (int k = 0; k < 8; ++k) sum += x[k];
    }
    for (; i < b; i += 64) sum += values[i];
    sum = wave_sum(sum);
    if (lane == 0) out[s] = sum;
}

// ---- normals -------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MO_THREADS) triangle_geometry_kernel(const float* __restrict__ vertices, int64_t n_vertices,
                                                                       const int32_t* __restrict__ triangles, int64_t n_triangles,
                                                                       int32_t* __restrict__ flags, float* __restrict__ normals,
                                                                       double* __restrict__ cross, double* __restrict__ area) {
    const int64_t t = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    if (t >= n_triangles) return;
    int32_t idx[3];
    const bool valid = tri_indices(triangles, t, n_vertices, idx);
    float p[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t j = valid ? idx[k] : 0;                        // (never read outside the array; n_vertices >= 1)
#pragma unroll
        for (int a = 0; a < 3; ++a) p[k][a] = vertices[3 * j + a];
    }
    float n32[3];
    const bool kept = tri_cross(p[0], p[1], p[2], n32) && valid;
    if (flags) flags[t] = (valid ? BS_MESH_TRIANGLE_VALID : 0) | (kept ? BS_MESH_TRIANGLE_KEPT : 0);
    if (normals) {
        float u[3] = {0.0f, 0.0f, 0.0f};
        if (kept) tri_unit(n32, u);
        normals[3 * t] = u[0]; normals[3 * t + 1] = u[1]; normals[3 * t + 2] = u[2];
    }
    if (cross || area) {
        double n[3] = {0.0, 0.0, 0.0}, ar = 0.0;
        if (kept) {
            tri_cross64(p[0], p[1], p[2], n);
            ar = tri_area64(n);
        }
        if (cross) { cross[3 * t] = n[0]; cross[3 * t + 1] = n[1]; cross[3 * t + 2] = n[2]; }
        if (area) area[t] = ar;
    }
}

__global__ void __launch_bounds__(MO_THREADS) vertex_normals_kernel(const double* __restrict__ cross, int64_t n_triangles,
                                                                    const int64_t* __restrict__ corner_order,
                                                                    const int64_t* __restrict__ vertex_start, int64_t n_vertices,
                                                                    float* __restrict__ normals) {
    const int64_t v = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    if (v >= n_vertices) return;
    const int64_t n_corners = 3 * n_triangles;
    int64_t a = vertex_start[v], b = vertex_start[v + 1];
    a = a < 0 ? 0 : a;
    b = b > n_corners ? n_corners : b;
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t i = a; i < b; ++i) {
        const int64_t k = corner_order[i];
        if (k < 0 || k >= n_corners) continue;
        const int64_t t = k / 3;
        s[0] += cross[3 * t]; s[1] += cross[3 * t + 1]; s[2] += cross[3 * t + 2];
    }
    const double m = fmax(fmax(fabs(s[0]), fabs(s[1])), fabs(s[2]));
    float u[3] = {0.0f, 0.0f, 0.0f};
    if (m > 0.0) {
        const double x = s[0] / m, y = s[1] / m, z = s[2] / m;
        const double len = sqrt((x * x + y * y) + z * z);
        u[0] = (float)(x / len); u[1] = (float)(y / len); u[2] = (float)(z / len);
    }
    normals[3 * v] = u[0]; normals[3 * v + 1] = u[1]; normals[3 * v + 2] = u[2];
}

// ---- smoothing -----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MO_THREADS) laplacian_step_kernel(const float* __restrict__ in, int64_t n_vertices,
                                                                    const int64_t* __restrict__ nbr_start, const int32_t* __restrict__ nbr,
                                                                    int64_t n_nbr, double lambda, int clamp, float* __restrict__ out) {
    const int64_t v = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
    if (v >= n_vertices) return;
    int64_t a = nbr_start[v], b = nbr_start[v + 1];
    a = a < 0 ? 0 : a;
    b = b > n_nbr ? n_nbr : b;
    const float x0 = in[3 * v], x1 = in[3 * v + 1], x2 = in[3 * v + 2];
    double s[3] = {0.0, 0.0, 0.0};
    int64_t k = 0;
    for (int64_t i = a; i < b; ++i) {
        const int64_t j = nbr[i];
        if (j < 0 || j >= n_vertices) continue;
        s[0] += (double)in[3 * j]; s[1] += (double)in[3 * j + 1]; s[2] += (double)in[3 * j + 2];
        ++k;
    }
    float o[3] = {x0, x1, x2};
    if (k > 0) {
        const double c = (double)k, x[3] = {(double)x0, (double)x1, (double)x2};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double mean = s[d] / c;
            double y = x[d] + lambda * (mean - x[d]);
            if (clamp) y = y < 0.0 ? 0.0 : (y > 1.0 ? 1.0 : y);     // (a NaN stays one)
            o[d] = (float)y;
        }
    }
    out[3 * v] = o[0]; out[3 * v + 1] = o[1]; out[3 * v + 2] = o[2];
}

inline bool mo_count(int64_t n) { return n >= 1 && n <= (int64_t)BS_MESH_MAX_TRIANGLES; }
inline dim3 mo_grid(int64_t n) { return dim3((unsigned)cdiv64(n, MO_THREADS)); }

}  // namespace
}  // namespace bs

#define MO_ENTER(name) \
    using namespace bs; \
    if (!initialized()) { set_error(name ": call bs_init first"); return BS_ERR_NOT_INIT; } \
    hipStream_t st = reinterpret_cast<hipStream_t>(stream)

extern "C" int bs_mesh_edge_insert(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices, void* keys, int32_t* first_half, int32_t* count,
                                   int32_t* forward, int64_t slots, int32_t* slot_of_half, int32_t* status, void* stream) {
    MO_ENTER("bs_mesh_edge_insert");
    BS_REQUIRE(triangles && keys && first_half && count && forward && slot_of_half && status, "bs_mesh_edge_insert: null pointer");
    BS_REQUIRE(mo_count(n_triangles) && n_vertices >= 0 && n_vertices < ((int64_t)1 << 31), "bs_mesh_edge_insert: T = %lld, V = %lld",
               (long long)n_triangles, (long long)n_vertices);
    BS_REQUIRE(slots >= 1 && slots <= ((int64_t)1 << 31) && (slots & (slots - 1)) == 0, "bs_mesh_edge_insert: slots = %lld (a power of two <= 2^31)",
               (long long)slots);
    BS_REQUIRE(((uintptr_t)keys & 7) == 0, "bs_mesh_edge_insert: keys must be 8-byte aligned");
    hipLaunchKernelGGL(edge_insert_kernel, mo_grid(3 * n_triangles), dim3(MO_THREADS), 0, st, triangles, n_triangles, n_vertices,
                       static_cast<edge_key*>(keys), first_half, count, forward, slots, slot_of_half, status);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_edge_flags(const int32_t* slot_of_half, const int32_t* first_half, int64_t slots, int64_t n_half, int32_t* leader,
                                  int32_t* is_first, void* stream) {
    MO_ENTER("bs_mesh_edge_flags");
    BS_REQUIRE(slot_of_half && first_half && leader && is_first, "bs_mesh_edge_flags: null pointer");
    BS_REQUIRE(n_half >= 1 && n_half < ((int64_t)1 << 31) && slots >= 1, "bs_mesh_edge_flags: n = %lld, slots = %lld", (long long)n_half,
               (long long)slots);
    slot_flags_launch(slot_of_half, first_half, slots, n_half, leader, is_first, st);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_edge_rows(const int32_t* triangles, int64_t n_triangles, const int32_t* slot_of_half, const int32_t* count,
                                 const int32_t* forward, int64_t slots, const int32_t* leader, const int32_t* rank, int64_t n_edges, int32_t* edges,
                                 int32_t* edge_count, int32_t* edge_forward, int32_t* edge_first_triangle, int32_t* edge_of_half, void* stream) {
    MO_ENTER("bs_mesh_edge_rows");
    BS_REQUIRE(triangles && slot_of_half && count && forward && leader && rank && edge_of_half, "bs_mesh_edge_rows: null pointer");
    BS_REQUIRE(mo_count(n_triangles) && slots >= 1 && n_edges >= 0 && n_edges <= 3 * n_triangles, "bs_mesh_edge_rows: T = %lld, slots = %lld, E = %lld",
               (long long)n_triangles, (long long)slots, (long long)n_edges);
    BS_REQUIRE(n_edges == 0 || (edges && edge_count && edge_forward && edge_first_triangle), "bs_mesh_edge_rows: null edge rows");
    hipLaunchKernelGGL(edge_rows_kernel, mo_grid(3 * n_triangles), dim3(MO_THREADS), 0, st, triangles, n_triangles, slot_of_half, count, forward, slots,
                       leader, rank, n_edges, edges, edge_count, edge_forward, edge_first_triangle, edge_of_half);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_cc_hook(const int32_t* edge_of_half, const int32_t* edge_first_triangle, int64_t n_triangles, int64_t n_edges, int32_t* parent,
                               int32_t* changed, void* stream) {
    MO_ENTER("bs_mesh_cc_hook");
    BS_REQUIRE(edge_of_half && parent && changed && (n_edges == 0 || edge_first_triangle), "bs_mesh_cc_hook: null pointer");
    BS_REQUIRE(mo_count(n_triangles) && n_edges >= 0 && n_edges <= 3 * n_triangles, "bs_mesh_cc_hook: T = %lld, E = %lld", (long long)n_triangles,
               (long long)n_edges);
    hipLaunchKernelGGL(cc_hook_kernel, mo_grid(3 * n_triangles), dim3(MO_THREADS), 0, st, edge_of_half, edge_first_triangle, n_triangles, n_edges,
                       parent, changed);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_cc_compress(int32_t* parent, int64_t n_triangles, void* stream) {
    MO_ENTER("bs_mesh_cc_compress");
    BS_REQUIRE(parent && mo_count(n_triangles), "bs_mesh_cc_compress: parent %p, T = %lld", (void*)parent, (long long)n_triangles);
    hipLaunchKernelGGL(cc_compress_kernel, mo_grid(n_triangles), dim3(MO_THREADS), 0, st, parent, n_triangles);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_cc_roots(const int32_t* parent, const int32_t* edge_of_half, int64_t n_triangles, int32_t* is_root, void* stream) {
    MO_ENTER("bs_mesh_cc_roots");
    BS_REQUIRE(parent && edge_of_half && is_root && mo_count(n_triangles), "bs_mesh_cc_roots: null pointer or T = %lld", (long long)n_triangles);
    hipLaunchKernelGGL(cc_roots_kernel, mo_grid(n_triangles), dim3(MO_THREADS), 0, st, parent, edge_of_half, n_triangles, is_root);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_cc_clusters(const int32_t* parent, const int32_t* edge_of_half, const int32_t* rank, int64_t n_triangles, int64_t n_clusters,
                                   int32_t* triangle_clusters, int32_t* cluster_n_triangles, void* stream) {
    MO_ENTER("bs_mesh_cc_clusters");
    BS_REQUIRE(parent && edge_of_half && rank && triangle_clusters && (n_clusters == 0 || cluster_n_triangles), "bs_mesh_cc_clusters: null pointer");
    BS_REQUIRE(mo_count(n_triangles) && n_clusters >= 0 && n_clusters <= n_triangles, "bs_mesh_cc_clusters: T = %lld, C = %lld", (long long)n_triangles,
               (long long)n_clusters);
    hipLaunchKernelGGL(cc_clusters_kernel, mo_grid(n_triangles), dim3(MO_THREADS), 0, st, parent, edge_of_half, rank, n_triangles, n_clusters,
                       triangle_clusters, cluster_n_triangles);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_orient_hook(const int32_t* edge_of_half, const int32_t* edge_count, const int32_t* edge_forward,
                                  const int32_t* edge_first_triangle, int64_t n_triangles, int64_t n_edges, uint32_t* word, int32_t* changed,
                                  void* stream) {
    MO_ENTER("bs_mesh_orient_hook");
    BS_REQUIRE(edge_of_half && word && changed && (n_edges == 0 || (edge_count && edge_forward && edge_first_triangle)),
               "bs_mesh_orient_hook: null pointer");
    BS_REQUIRE(mo_count(n_triangles) && n_edges >= 0 && n_edges <= 3 * n_triangles, "bs_mesh_orient_hook: T = %lld, E = %lld", (long long)n_triangles,
               (long long)n_edges);
    hipLaunchKernelGGL(orient_hook_kernel, mo_grid(3 * n_triangles), dim3(MO_THREADS), 0, st, edge_of_half, edge_count, edge_forward,
                       edge_first_triangle, n_triangles, n_edges, word, changed);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_orient_compress(uint32_t* word, int64_t n_triangles, void* stream) {
    MO_ENTER("bs_mesh_orient_compress");
    BS_REQUIRE(word && mo_count(n_triangles), "bs_mesh_orient_compress: word %p, T = %lld", (void*)word, (long long)n_triangles);
    hipLaunchKernelGGL(orient_compress_kernel, mo_grid(n_triangles), dim3(MO_THREADS), 0, st, word, n_triangles);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_orient_check(const int32_t* edge_of_half, const int32_t* edge_count, const int32_t* edge_forward,
                                   const int32_t* edge_first_triangle, int64_t n_triangles, int64_t n_edges, const uint32_t* word, int32_t* bad,
                                   void* stream) {
    MO_ENTER("bs_mesh_orient_check");
    BS_REQUIRE(edge_of_half && word && bad && (n_edges == 0 || (edge_count && edge_forward && edge_first_triangle)),
               "bs_mesh_orient_check: null pointer");
    BS_REQUIRE(mo_count(n_triangles) && n_edges >= 0 && n_edges <= 3 * n_triangles, "bs_mesh_orient_check: T = %lld, E = %lld", (long long)n_triangles,
               (long long)n_edges);
    hipLaunchKernelGGL(orient_check_kernel, mo_grid(3 * n_triangles), dim3(MO_THREADS), 0, st, edge_of_half, edge_count, edge_forward,
                       edge_first_triangle, n_triangles, n_edges, word, bad);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_orient_flip(const int32_t* triangles, const int32_t* edge_of_half, const uint32_t* word, const int32_t* bad, int64_t n_triangles,
                                  int32_t* out, uint8_t* flipped, void* stream) {
    MO_ENTER("bs_mesh_orient_flip");
    BS_REQUIRE(triangles && edge_of_half && word && bad && out && flipped && out != triangles, "bs_mesh_orient_flip: null pointer, or out == triangles");
    BS_REQUIRE(mo_count(n_triangles), "bs_mesh_orient_flip: T = %lld", (long long)n_triangles);
    hipLaunchKernelGGL(orient_flip_kernel, mo_grid(n_triangles), dim3(MO_THREADS), 0, st, triangles, edge_of_half, word, bad, n_triangles, out, flipped);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_segment_sum(const double* values, int64_t n_values, const int64_t* start, int64_t n_segments, double* out, void* stream) {
    MO_ENTER("bs_mesh_segment_sum");
    BS_REQUIRE(values && start && out, "bs_mesh_segment_sum: null pointer");
    BS_REQUIRE(n_values >= 1 && n_segments >= 1 && n_segments < ((int64_t)1 << 31), "bs_mesh_segment_sum: n = %lld, segments = %lld",
               (long long)n_values, (long long)n_segments);
    hipLaunchKernelGGL(segment_sum_kernel, dim3((unsigned)cdiv64(n_segments, MO_THREADS / 64)), dim3(MO_THREADS), 0, st, values, n_values, start,
                       n_segments, out);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_triangle_geometry(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, int32_t* flags,
                                         float* normals, double* cross, double* area, void* stream) {
    MO_ENTER("bs_mesh_triangle_geometry");
    BS_REQUIRE(vertices && triangles, "bs_mesh_triangle_geometry: null pointer");
    BS_REQUIRE(mo_count(n_triangles) && n_vertices >= 1 && n_vertices < ((int64_t)1 << 31), "bs_mesh_triangle_geometry: T = %lld, V = %lld",
               (long long)n_triangles, (long long)n_vertices);
    hipLaunchKernelGGL(triangle_geometry_kernel, mo_grid(n_triangles), dim3(MO_THREADS), 0, st, vertices, n_vertices, triangles, n_triangles, flags,
                       normals, cross, area);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_vertex_normals(const double* cross, int64_t n_triangles, const int64_t* corner_order, const int64_t* vertex_start,
                                      int64_t n_vertices, float* normals, void* stream) {
    MO_ENTER("bs_mesh_vertex_normals");
    BS_REQUIRE(cross && corner_order && vertex_start && normals, "bs_mesh_vertex_normals: null pointer");
    BS_REQUIRE(mo_count(n_triangles) && n_vertices >= 1 && n_vertices < ((int64_t)1 << 31), "bs_mesh_vertex_normals: T = %lld, V = %lld",
               (long long)n_triangles, (long long)n_vertices);
    hipLaunchKernelGGL(vertex_normals_kernel, mo_grid(n_vertices), dim3(MO_THREADS), 0, st, cross, n_triangles, corner_order, vertex_start, n_vertices,
                       normals);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_mesh_laplacian_step(const float* in, int64_t n_vertices, const int64_t* nbr_start, const int32_t* nbr, int64_t n_nbr, double lambda,
                                      int32_t clamp, float* out, void* stream) {
    MO_ENTER("bs_mesh_laplacian_step");
    BS_REQUIRE(in && nbr_start && out && in != out && (n_nbr == 0 || nbr), "bs_mesh_laplacian_step: null pointer, or in == out");
    BS_REQUIRE(n_vertices >= 1 && n_vertices < ((int64_t)1 << 31) && n_nbr >= 0, "bs_mesh_laplacian_step: V = %lld, neighbours = %lld",
               (long long)n_vertices, (long long)n_nbr);
    BS_REQUIRE(isfinite(lambda), "bs_mesh_laplacian_step: lambda %g", lambda);
    hipLaunchKernelGGL(laplacian_step_kernel, mo_grid(n_vertices), dim3(MO_THREADS), 0, st, in, n_vertices, nbr_start, nbr, n_nbr, lambda,
                       (int)(clamp != 0), out);
    BS_CHECK_LAUNCH();
    return BS_OK;
}
