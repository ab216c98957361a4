// Radius search on the grid: neighbour counts and lists, and the DBSCAN clusters that stand on them (bs_pc_radius_count / _fill / _sort /
// _unpack, bs_pc_dbscan_hook / _compress / _roots / _labels; include/bodyslam_hip.h): the roles of Open3D's
// KDTreeFlann.search_radius_vector_3d, PointCloud.remove_radius_outlier and PointCloud.cluster_dbscan.  Restated from Open3D's documented
// meaning; parity with Open3D is UNPINNED.  The statement is tests/_radius_ref.py, DESIGN section 3.22 the argument.
//
// Everything here is knn.hip's hybrid search without the cap on the list: the same grid, the same 16-byte records, the same fp32 arithmetic
// d2 = (dx * dx + dy * dy) + dz * dz, the same cut-off (pc_grid.h: knn_d2_cutoff -- "sqrtf(d2) <= radius" as one comparison, a target at
// exactly the radius is in), the same walk (pc_grid.h: pc_walk, max_distance = radius, no shell cap) with other sinks.
//   The bound: a sink here never says "bounded", so the walk ends on pc_walk's own two rules -- every cell has been seen, or
//   lb * 0.9999 > radius, where lb is a true lower bound on the distance of everything unvisited (derived at the top of pointcloud.hip):
//   the computed d2 of an unvisited target is >= fl(lb * lb) > cut-off, so nothing unvisited is a neighbour.  A source far outside the
//   target's box leaves after the first shells; the cell size changes how many records are looked at, never which ones pass.
//   count   the sink counts.
//   fill    the sink writes the 64-bit keys (d2 bits << 32 | original index) into the row's segment [row_start[i], row_start[i + 1]) in walk
//           order; a row whose segment is malformed or too short writes nothing beyond it and sets a status bit.
//   sort    one wave per row, ascending keys = ascending (d2, index): d2 >= 0, so the key order IS the lexicographic order (pc_brute_kernel's
//           trick).  The keys of a row are distinct -- the index half --, so the order is total: the result does not depend on the walk.
//           At most 64 keys: one key per lane (the rest padded with ~0, above every key), a bitonic compare-exchange network over
//           __shfl_xor, 21 exchanges.  More: rank counting into the second buffer, out[number of keys below mine] = mine with the lanes
//           striding the row -- c * c / 64 comparisons per lane, on reads every lane shares.  No LDS.
//   DBSCAN  core = count >= min_points.  hook: one thread per core point walks its neighbourhood and hooks itself to every core neighbour of
//           LOWER index (every edge is seen from its upper end) with union_min.h's union by minimum, the device functions of
//           bs_mesh_cc_hook / _compress.  The neighbourhood is walked again every round: memory stays O(n) whatever eps is.  labels: a core
//           point takes rank[root] - 1; another finite point walks once more for the minimum over its core neighbours.
// No floating-point atomics, no LDS; every index read from memory is checked before it addresses anything.
#include <math.h>

#include "common.h"
#include "pc_grid.h"
#include "union_min.h"

namespace bs {
namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_WAVE = 64;
typedef unsigned long long rs_key;
constexpr rs_key RS_PAD = ~0ull;

__device__ __forceinline__ float rs_d2(const f32x4 t, float sx, float sy, float sz) {
    const float dx = sx - t[0], dy = sy - t[1], dz = sz - t[2];
    return (dx * dx + dy * dy) + dz * dz;
}

struct RsCountSink {
    float sx, sy, sz, d2_max;
    int32_t n;
    __device__ __forceinline__ void add(const f32x4 t) { n += rs_d2(t, sx, sy, sz) <= d2_max ? 1 : 0; }
    __device__ __forceinline__ bool bounded(float) const { return false; }               // every neighbour is wanted: the radius rule ends the walk
};

struct RsFillSink {
    float sx, sy, sz, d2_max;
    rs_key* __restrict__ out;
    int64_t cap, n;
    __device__ __forceinline__ void add(const f32x4 t) {
        const float d2 = rs_d2(t, sx, sy, sz);
        if (!(d2 <= d2_max)) return;
        if (n < cap) out[n] = ((rs_key)__float_as_uint(d2) << 32) | (rs_key)(uint32_t)__float_as_int(t[3]);
        ++n;
    }
    __device__ __forceinline__ bool bounded(float) const { return false; }
};

__device__ __forceinline__ bool rs_source(const float* __restrict__ src, int64_t i, float& sx, float& sy, float& sz) {
    sx = src[3 * i]; sy = src[3 * i + 1]; sz = src[3 * i + 2];
    return pc_finite(sx) && pc_finite(sy) && pc_finite(sz);
}

__global__ void __launch_bounds__(RS_THREADS) pc_radius_count_kernel(const f32x4* __restrict__ records, const int32_t* __restrict__ cell_start,
                                                                     PcGrid g, const float* __restrict__ src, int64_t m, float radius,
                                                                     float d2_max, int32_t* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= m) return;
    float sx, sy, sz;
    int32_t n = 0;
    if (rs_source(src, i, sx, sy, sz)) {
        RsCountSink sink{sx, sy, sz, d2_max, 0};
        pc_walk(records, cell_start, g, sx, sy, sz, radius, 0x7fffffff, sink);
        n = sink.n;
    }
    count[i] = n;
}

__global__ void __launch_bounds__(RS_THREADS) pc_radius_fill_kernel(const f32x4* __restrict__ records, const int32_t* __restrict__ cell_start,
                                                                    PcGrid g, const float* __restrict__ src, int64_t m, float radius,
                                                                    float d2_max, const int64_t* __restrict__ row_start, int64_t total,
                                                                    rs_key* __restrict__ keys, int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= m) return;
    const int64_t b = row_start[i], e = row_start[i + 1];
    if (b < 0 || e < b || e > total) { atomicOr(status, BS_PC_RADIUS_OVERRUN); return; }
    float sx, sy, sz;
    int64_t n = 0;
    if (rs_source(src, i, sx, sy, sz)) {
        RsFillSink sink{sx, sy, sz, d2_max, keys + b, e - b, 0};
        pc_walk(records, cell_start, g, sx, sy, sz, radius, 0x7fffffff, sink);
        n = sink.n;
    }
    if (n > e - b) atomicOr(status, BS_PC_RADIUS_OVERRUN);
}

// one wave per row; no lane leaves before the shuffles: the row's bounds are the same in every lane of the wave
__global__ void __launch_bounds__(RS_THREADS) pc_radius_sort_kernel(const rs_key* __restrict__ keys, const int64_t* __restrict__ row_start,
                                                                    int64_t m, int64_t total, rs_key* __restrict__ out) {
    const int lane = threadIdx.x & (RS_WAVE - 1);
    const int64_t row = (int64_t)blockIdx.x * (RS_THREADS / RS_WAVE) + (threadIdx.x / RS_WAVE);
    if (row >= m) return;                                                               // (a whole wave)
    const int64_t b = row_start[row], e = row_start[row + 1];
    if (b < 0 || e < b || e > total) return;
    const int64_t c = e - b;
    if (c <= RS_WAVE) {
        rs_key key = lane < c ? keys[b + lane] : RS_PAD;
#pragma unroll
        for (int k = 2; k <= RS_WAVE; k <<= 1) {
#pragma unroll
            for (int j = k >> 1; j > 0; j >>= 1) {
                const rs_key other = __shfl_xor(key, j, RS_WAVE);
                const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);           // the lower lane of an ascending pair, the upper of a descending
                const rs_key lo = key < other ? key : other, hi = key < other ? other : key;
                key = keep_min ? lo : hi;
            }
        }
        if (lane < c) out[b + lane] = key;
        return;
    }
    for (int64_t j = lane; j < c; j += RS_WAVE) {
        const rs_key mine = keys[b + j];
        int64_t below = 0;
        for (int64_t t = 0; t < c; ++t) below += keys[b + t] < mine ? 1 : 0;            // <= c - 1: inside the row whatever the keys are
        out[b + below] = mine;
    }
}

__global__ void __launch_bounds__(RS_THREADS) pc_radius_unpack_kernel(const rs_key* __restrict__ keys, int64_t total, int32_t* __restrict__ index,
                                                                      float* __restrict__ d2) {
    const int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= total) return;
    const rs_key key = keys[i];
    index[i] = (int32_t)(uint32_t)(key & 0xffffffffull);
    d2[i] = __uint_as_float((uint32_t)(key >> 32));
}

// ---- DBSCAN ----------------------------------------------------------------------------------------------------------------------------------
struct DbHookSink {
    float sx, sy, sz, d2_max;
    int32_t i, min_points;
    int64_t n;
    const int32_t* __restrict__ count;
    int32_t* parent;
    int32_t* __restrict__ changed;
    __device__ __forceinline__ void add(const f32x4 t) {
        if (!(rs_d2(t, sx, sy, sz) <= d2_max)) return;
        const int32_t j = __float_as_int(t[3]);
        if (j < 0 || j >= i) return;                                                    // the edge's upper end hooks it; i < n
        if (count[j] < min_points) return;
        cc_union(parent, i, j, n, changed);
    }
    __device__ __forceinline__ bool bounded(float) const { return false; }
};

struct DbLabelSink {
    float sx, sy, sz, d2_max;
    int32_t min_points, best;
    int64_t n, n_clusters;
    const int32_t* __restrict__ count;
    const int32_t* __restrict__ parent;
    const int32_t* __restrict__ rank;
    __device__ __forceinline__ void add(const f32x4 t) {
        if (!(rs_d2(t, sx, sy, sz) <= d2_max)) return;
        const int32_t j = __float_as_int(t[3]);
        if (j < 0 || j >= n) return;
        if (count[j] < min_points) return;
        const int32_t r = parent[j];
        if (r < 0 || r >= n) return;
        const int32_t k = rank[r] - 1;
        if (k >= 0 && k < n_clusters && k < best) best = k;
    }
    __device__ __forceinline__ bool bounded(float) const { return false; }
};

__global__ void __launch_bounds__(RS_THREADS) pc_dbscan_hook_kernel(const f32x4* __restrict__ records, const int32_t* __restrict__ cell_start,
                                                                    PcGrid g, const float* __restrict__ pts, int64_t n, float eps, float d2_max,
                                                                    const int32_t* __restrict__ count, int32_t min_points, int32_t* parent,
                                                                    int32_t* __restrict__ changed) {
    const int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= n) return;
    if (count[i] < min_points) return;
    float sx, sy, sz;
    if (!rs_source(pts, i, sx, sy, sz)) return;
    DbHookSink sink{sx, sy, sz, d2_max, (int32_t)i, min_points, n, count, parent, changed};
    pc_walk(records, cell_start, g, sx, sy, sz, eps, 0x7fffffff, sink);
}

__global__ void __launch_bounds__(RS_THREADS) pc_dbscan_compress_kernel(int32_t* parent, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= n) return;
    cc_compress(parent, (int32_t)i, n);
}

__global__ void __launch_bounds__(RS_THREADS) pc_dbscan_roots_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ count,
                                                                     int32_t min_points, int64_t n, int32_t* __restrict__ is_root) {
    const int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= n) return;
    is_root[i] = count[i] >= min_points && parent[i] == (int32_t)i ? 1 : 0;
}

__global__ void __launch_bounds__(RS_THREADS) pc_dbscan_labels_kernel(const f32x4* __restrict__ records, const int32_t* __restrict__ cell_start,
                                                                      PcGrid g, const float* __restrict__ pts, int64_t n, float eps, float d2_max,
                                                                      const int32_t* __restrict__ count, int32_t min_points,
                                                                      const int32_t* __restrict__ parent, const int32_t* __restrict__ rank,
                                                                      int64_t n_clusters, int32_t* __restrict__ labels) {
    const int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= n) return;
    float sx, sy, sz;
    int32_t label = -1;
    if (rs_source(pts, i, sx, sy, sz)) {
        if (count[i] >= min_points) {
            const int32_t r = parent[i];
            if (r >= 0 && r < n) {
                const int32_t k = rank[r] - 1;
                if (k >= 0 && k < n_clusters) label = k;
            }
        } else {
            DbLabelSink sink{sx, sy, sz, d2_max, min_points, PC_NONE, n, n_clusters, count, parent, rank};
            pc_walk(records, cell_start, g, sx, sy, sz, eps, 0x7fffffff, sink);
            if (sink.best != PC_NONE) label = sink.best;
        }
    }
    labels[i] = label;
}

inline bool rs_count(int64_t n) { return n >= 1 && n < ((int64_t)1 << 31); }
inline dim3 rs_grid(int64_t n) { return dim3((unsigned)cdiv64(n, RS_THREADS)); }

}  // namespace
}  // namespace bs

#define RS_ENTER(name)                                                                 \
    using namespace bs;                                                                \
    if (!initialized()) { set_error(name ": call bs_init first"); return BS_ERR_NOT_INIT; } \
    hipStream_t st = reinterpret_cast<hipStream_t>(stream)

// the arguments every walk shares: the index, its grid, the radius
#define RS_INDEX(name, radius)                                                                                                                     \
    BS_REQUIRE(records && cell_start && lo && hi && dims, name ": null pointer");                                                                   \
    BS_REQUIRE(n_records >= 0 && n_records < ((int64_t)1 << 31), name ": n_records = %lld", (long long)n_records);                                  \
    BS_REQUIRE(((uintptr_t)records & 15) == 0, name ": records must be 16-byte aligned");                                                           \
    BS_REQUIRE(radius > 0.0f && radius < INFINITY, name ": radius %g (positive and finite)", (double)radius);                                       \
    const PcGrid g = pc_grid(lo, hi, cell_size, dims);                                                                                              \
    BS_REQUIRE(pc_grid_ok(g), name ": bad grid (cell size %g, %d x %d x %d cells, at most 2^24)", (double)cell_size, dims[0], dims[1], dims[2]);    \
    const float d2_max = knn_d2_cutoff(radius);                                                                                                     \
    const f32x4* rec = static_cast<const f32x4*>(records)

extern "C" int bs_pc_radius_count(const void* records, const int32_t* cell_start, int64_t n_records, const float* lo, const float* hi, float cell_size,
                                  const int32_t* dims, const float* source, int64_t m, float radius, int32_t* count, void* stream) {
    RS_ENTER("bs_pc_radius_count");
    RS_INDEX("bs_pc_radius_count", radius);
    BS_REQUIRE(source && count && rs_count(m), "bs_pc_radius_count: null pointer or m = %lld (1 <= m < 2^31)", (long long)m);
    hipLaunchKernelGGL(pc_radius_count_kernel, rs_grid(m), dim3(RS_THREADS), 0, st, rec, cell_start, g, source, m, radius, d2_max, count);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_radius_fill(const void* records, const int32_t* cell_start, int64_t n_records, const float* lo, const float* hi, float cell_size,
                                 const int32_t* dims, const float* source, int64_t m, float radius, const int64_t* row_start, int64_t total,
                                 void* keys, int32_t* status, void* stream) {
    RS_ENTER("bs_pc_radius_fill");
    RS_INDEX("bs_pc_radius_fill", radius);
    BS_REQUIRE(source && row_start && keys && status && rs_count(m), "bs_pc_radius_fill: null pointer or m = %lld (1 <= m < 2^31)", (long long)m);
    BS_REQUIRE(rs_count(total), "bs_pc_radius_fill: total = %lld (1 <= total < 2^31)", (long long)total);
    BS_REQUIRE(((uintptr_t)keys & 7) == 0, "bs_pc_radius_fill: keys must be 8-byte aligned");
    hipLaunchKernelGGL(pc_radius_fill_kernel, rs_grid(m), dim3(RS_THREADS), 0, st, rec, cell_start, g, source, m, radius, d2_max, row_start, total,
                       static_cast<rs_key*>(keys), status);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_radius_sort(const void* keys, const int64_t* row_start, int64_t m, int64_t total, void* keys_out, void* stream) {
    RS_ENTER("bs_pc_radius_sort");
    BS_REQUIRE(keys && row_start && keys_out && keys != keys_out, "bs_pc_radius_sort: null pointer, or keys_out is keys");
    BS_REQUIRE(rs_count(m) && rs_count(total), "bs_pc_radius_sort: m = %lld, total = %lld (1 <= . < 2^31)", (long long)m, (long long)total);
    BS_REQUIRE((((uintptr_t)keys | (uintptr_t)keys_out) & 7) == 0, "bs_pc_radius_sort: keys must be 8-byte aligned");
    hipLaunchKernelGGL(pc_radius_sort_kernel, dim3((unsigned)cdiv64(m, RS_THREADS / RS_WAVE)), dim3(RS_THREADS), 0, st,
                       static_cast<const rs_key*>(keys), row_start, m, total, static_cast<rs_key*>(keys_out));
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_radius_unpack(const void* keys, int64_t total, int32_t* index, float* d2, void* stream) {
    RS_ENTER("bs_pc_radius_unpack");
    BS_REQUIRE(keys && index && d2 && rs_count(total), "bs_pc_radius_unpack: null pointer or total = %lld (1 <= total < 2^31)", (long long)total);
    BS_REQUIRE(((uintptr_t)keys & 7) == 0, "bs_pc_radius_unpack: keys must be 8-byte aligned");
    hipLaunchKernelGGL(pc_radius_unpack_kernel, rs_grid(total), dim3(RS_THREADS), 0, st, static_cast<const rs_key*>(keys), total, index, d2);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_dbscan_hook(const void* records, const int32_t* cell_start, int64_t n_records, const float* lo, const float* hi, float cell_size,
                                 const int32_t* dims, const float* points, int64_t n, float eps, const int32_t* count, int32_t min_points,
                                 int32_t* parent, int32_t* changed, void* stream) {
    RS_ENTER("bs_pc_dbscan_hook");
    RS_INDEX("bs_pc_dbscan_hook", eps);
    BS_REQUIRE(points && count && parent && changed && rs_count(n), "bs_pc_dbscan_hook: null pointer or n = %lld (1 <= n < 2^31)", (long long)n);
    BS_REQUIRE(min_points >= 1, "bs_pc_dbscan_hook: min_points = %d (>= 1)", min_points);
    hipLaunchKernelGGL(pc_dbscan_hook_kernel, rs_grid(n), dim3(RS_THREADS), 0, st, rec, cell_start, g, points, n, eps, d2_max, count, min_points, parent,
                       changed);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_dbscan_compress(int32_t* parent, int64_t n, void* stream) {
    RS_ENTER("bs_pc_dbscan_compress");
    BS_REQUIRE(parent && rs_count(n), "bs_pc_dbscan_compress: parent %p, n = %lld", (void*)parent, (long long)n);
    hipLaunchKernelGGL(pc_dbscan_compress_kernel, rs_grid(n), dim3(RS_THREADS), 0, st, parent, n);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_dbscan_roots(const int32_t* parent, const int32_t* count, int32_t min_points, int64_t n, int32_t* is_root, void* stream) {
    RS_ENTER("bs_pc_dbscan_roots");
    BS_REQUIRE(parent && count && is_root && rs_count(n), "bs_pc_dbscan_roots: null pointer or n = %lld", (long long)n);
    BS_REQUIRE(min_points >= 1, "bs_pc_dbscan_roots: min_points = %d (>= 1)", min_points);
    hipLaunchKernelGGL(pc_dbscan_roots_kernel, rs_grid(n), dim3(RS_THREADS), 0, st, parent, count, min_points, n, is_root);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_dbscan_labels(const void* records, const int32_t* cell_start, int64_t n_records, const float* lo, const float* hi,
                                   float cell_size, const int32_t* dims, const float* points, int64_t n, float eps, const int32_t* count,
                                   int32_t min_points, const int32_t* parent, const int32_t* rank, int64_t n_clusters, int32_t* labels,
                                   void* stream) {
    RS_ENTER("bs_pc_dbscan_labels");
    RS_INDEX("bs_pc_dbscan_labels", eps);
    BS_REQUIRE(points && count && parent && rank && labels && rs_count(n), "bs_pc_dbscan_labels: null pointer or n = %lld (1 <= n < 2^31)",
               (long long)n);
    BS_REQUIRE(min_points >= 1 && n_clusters >= 0 && n_clusters <= n, "bs_pc_dbscan_labels: min_points = %d, clusters = %lld", min_points,
               (long long)n_clusters);
    hipLaunchKernelGGL(pc_dbscan_labels_kernel, rs_grid(n), dim3(RS_THREADS), 0, st, rec, cell_start, g, points, n, eps, d2_max, count, min_points,
                       parent, rank, n_clusters, labels);
    BS_CHECK_LAUNCH();
    return BS_OK;
}
