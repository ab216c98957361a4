// k nearest neighbours on the grid, normal estimation and the mean neighbour distance of the statistical outlier removal (bs_pc_query_knn,
// bs_pc_normals, bs_pc_knn_mean_distance; include/bodyslam_hip.h): the roles of Open3D's KDTreeFlann.search_knn_vector_3d /
// search_hybrid_vector_3d, PointCloud.estimate_normals (the reference calls it at BodySLAM_not_refactored/3DM/mapping_module.py:184) and
// PointCloud.remove_statistical_outlier (mapping_module.py:87).  Restated from Open3D's documented meaning; parity with Open3D is
// UNPINNED.  The statement is tests/_knn_ref.py.
//
// The query extends pointcloud.hip's from "the minimum" to "the k smallest under the same total order": the same grid, the same 16-byte
// records, the same fp32 arithmetic d2 = (dx * dx + dy * dy) + dz * dz, the same walk over the Chebyshev shells (pc_grid.h: pc_walk, the
// device function bs_pc_query_grid and bs_icp_step run) with another sink.
//   The bound (derived at the top of pointcloud.hip) with its one changed line: lb is a true lower bound of |dx| of every unvisited target,
//   so its computed d2 is >= fl(lb * lb); the search stops once the list is FULL and its WORST d2 < lb * lb -- strictly: an equal d2
//   with a lower index must not hide behind the bound.  It also stops when every cell has been seen, or when lb * 0.9999 > radius.
//   There is NO shell cap and NO brute-force fallback (as in bs_icp_step): a source far outside the target's box, or a k above the number
//   of targets within reach, walks shell after shell until one of the three rules holds -- in the worst case over the whole grid, which
//   costs time and never changes the result.
//   The list: K 64-bit keys (d2 bits << 32 | original index) in registers, ascending; d2 >= 0, so the key order IS the lexicographic order
//   of (d2, index) -- pc_brute_kernel's trick.  A candidate below the last key enters through a fully unrolled chain
//   a[j] = max(a[j - 1], min(a[j], key)): every index is a constant, so nothing goes to scratch, and nothing goes through LDS (DESIGN
//   section 7's rule for kernels that may run beside a second stream has nothing to apply to).  The capacity K is a template parameter
//   (8, 16, 32); a k below K uses the LAST k slots, the first K - k hold the key 0, which min / max leave alone: the worst kept key is
//   always a[K - 1], a constant index.  An empty slot holds ~0, whose d2 half is a NaN pattern: it compares false with the bound.
//   The radius (hybrid search) is a precomputed fp32 cut-off: the largest d2 with sqrtf(d2) <= radius, found on the host by stepping with
//   nextafterf around radius * radius; sqrtf is monotone, so d2 <= cut-off is the same predicate without a square root per candidate.
// Normals (bs_pc_normals), one thread per point, fp64: q_j = t[idx_j] - p (exact), S = sum q_j and M = sum q_j q_j^T added in list order,
// C = M / count - (S / count)(S / count)^T, svd3.h's Jacobi on C (symmetric PSD: the singular triplets are the eigenpairs), the normalised
// column of V with the smallest singular value (ties: the lowest column), the sign by the orientation mode, one rounding to fp32.
// Mean distance (bs_pc_knn_mean_distance), one thread per row: fl32((sum_j (double) sqrtf(d2_j)) / count) in list order.
// No floating-point atomics anywhere: two runs give the same bits, and the cell size changes the time only.
#include <math.h>

#include "common.h"
#include "pc_grid.h"
#include "svd3.h"

namespace bs {
namespace {

constexpr int KNN_THREADS = 256;
typedef unsigned long long knn_key;
constexpr knn_key KNN_EMPTY = ~0ull;

template <int K>
struct PcKnnSink {
    float sx, sy, sz, d2_max;
    knn_key a[K];
    __device__ __forceinline__ void init(int k) {
#pragma unroll
        for (int j = 0; j < K; ++j) a[j] = j < K - k ? 0ull : KNN_EMPTY;
    }
    __device__ __forceinline__ void add(const f32x4 t) {
        const float dx = sx - t[0], dy = sy - t[1], dz = sz - t[2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (!(d2 <= d2_max)) return;
        const knn_key key = ((knn_key)__float_as_uint(d2) << 32) | (knn_key)(uint32_t)__float_as_int(t[3]);
        if (key >= a[K - 1]) return;
#pragma unroll
        for (int j = K - 1; j > 0; --j) {
            const knn_key lo = key < a[j] ? key : a[j];
            a[j] = a[j - 1] > lo ? a[j - 1] : lo;
        }
        a[0] = key < a[0] ? key : a[0];
    }
    // the list is full and its worst d2 is strictly below the bound (an empty slot's d2 half is a NaN pattern: false)
    __device__ __forceinline__ bool bounded(float lb2) const { return __uint_as_float((uint32_t)(a[K - 1] >> 32)) < lb2; }
};

template <int K>
__global__ void __launch_bounds__(KNN_THREADS) pc_query_knn_kernel(const f32x4* __restrict__ records, const int32_t* __restrict__ cell_start,
                                                                   PcGrid g, const float* __restrict__ src, int64_t m, int k, float radius,
                                                                   float d2_max, int32_t* __restrict__ idx, float* __restrict__ d2,
                                                                   int32_t* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * KNN_THREADS + threadIdx.x;
    if (i >= m) return;
    const float sx = src[3 * i], sy = src[3 * i + 1], sz = src[3 * i + 2];
    int32_t* __restrict__ oi = idx + i * k;
    float* __restrict__ od = d2 + i * k;
    if (!(pc_finite(sx) && pc_finite(sy) && pc_finite(sz))) {
        for (int j = 0; j < k; ++j) { oi[j] = -1; od[j] = __builtin_nanf(""); }
        count[i] = 0;
        return;
    }
    PcKnnSink<K> sink;
    sink.sx = sx; sink.sy = sy; sink.sz = sz; sink.d2_max = d2_max;
    sink.init(k);
    pc_walk(records, cell_start, g, sx, sy, sz, radius, 0x7fffffff, sink);              // no cap: always runs to the end
    int32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int o = j - (K - k);
        if (o >= 0) {
            const knn_key key = sink.a[j];
            const bool ok = key != KNN_EMPTY;
            oi[o] = ok ? (int32_t)(uint32_t)(key & 0xffffffffull) : -1;
            od[o] = ok ? __uint_as_float((uint32_t)(key >> 32)) : INFINITY;
            cnt += ok ? 1 : 0;
        }
    }
    count[i] = cnt;
}

struct KnnVec { double v[3]; };

__global__ void __launch_bounds__(KNN_THREADS) pc_normals_kernel(const float* __restrict__ pts, int64_t n, const int32_t* __restrict__ idx,
                                                                 const int32_t* __restrict__ count, int k, int mode, KnnVec vec,
                                                                 float* __restrict__ normals, double* __restrict__ eig) {
    const int64_t i = (int64_t)blockIdx.x * KNN_THREADS + threadIdx.x;
    if (i >= n) return;
    const double p0 = (double)pts[3 * i], p1 = (double)pts[3 * i + 1], p2 = (double)pts[3 * i + 2];
    const int32_t* __restrict__ row = idx + i * k;
    const int cnt = min(max(count[i], 0), k);
    double S[3] = {0.0, 0.0, 0.0}, M[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                // M: xx xy xz yy yz zz
    int used = 0;
    for (int j = 0; j < cnt; ++j) {
        const int64_t t = row[j];
        if (t < 0 || t >= n) break;                                                    // (a list from bs_pc_query_knn has no such entry)
        const double q0 = (double)pts[3 * t] - p0, q1 = (double)pts[3 * t + 1] - p1, q2 = (double)pts[3 * t + 2] - p2;
        S[0] += q0; S[1] += q1; S[2] += q2;
        M[0] += q0 * q0; M[1] += q0 * q1; M[2] += q0 * q2;
        M[3] += q1 * q1; M[4] += q1 * q2; M[5] += q2 * q2;
        ++used;
    }
    double nrm[3] = {0.0, 0.0, 0.0}, ev[3] = {0.0, 0.0, 0.0};
    if (used >= 1) {
        const double c = (double)used, m0 = S[0] / c, m1 = S[1] / c, m2 = S[2] / c;
        double C[3][3], U[3][3], s[3], V[3][3];
        C[0][0] = M[0] / c - m0 * m0;
        C[0][1] = C[1][0] = M[1] / c - m0 * m1;
        C[0][2] = C[2][0] = M[2] / c - m0 * m2;
        C[1][1] = M[3] / c - m1 * m1;
        C[1][2] = C[2][1] = M[4] / c - m1 * m2;
        C[2][2] = M[5] / c - m2 * m2;
        svd3_jacobi(C, U, s, V);
        int lo = 0, hi = 0;
        if (s[1] < s[lo]) lo = 1;
        if (s[2] < s[lo]) lo = 2;
        if (s[1] > s[hi]) hi = 1;
        if (s[2] > s[hi]) hi = 2;
        const int mid = 3 - lo - hi;                                                    // (all three equal: lo = hi = 0, and mid is not a column)
        const bool ok = used >= 3 && s[hi] > 0.0 && s[hi] < INFINITY;
        ev[0] = s[lo]; ev[2] = s[hi];
        ev[1] = lo == hi ? s[0] : s[mid];
        if (ok) {
            double v0 = V[0][0], v1 = V[1][0], v2 = V[2][0];
            if (lo == 1) { v0 = V[0][1]; v1 = V[1][1]; v2 = V[2][1]; }
            if (lo == 2) { v0 = V[0][2]; v1 = V[1][2]; v2 = V[2][2]; }
            const double len = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
            v0 /= len; v1 /= len; v2 /= len;
            double dot;
            if (mode == BS_PC_ORIENT_DIRECTION) {
                dot = (v0 * vec.v[0] + v1 * vec.v[1]) + v2 * vec.v[2];
            } else if (mode == BS_PC_ORIENT_CAMERA) {
                dot = (v0 * (vec.v[0] - p0) + v1 * (vec.v[1] - p1)) + v2 * (vec.v[2] - p2);
            } else {                                                                    // the component of largest magnitude, the first on ties
                dot = v0;
                if (fabs(v1) > fabs(dot)) dot = v1;
                if (fabs(v2) > fabs(dot)) dot = v2;
            }
            if (dot < 0.0) { v0 = -v0; v1 = -v1; v2 = -v2; }
            if (fabs(v0) < INFINITY && fabs(v1) < INFINITY && fabs(v2) < INFINITY) { nrm[0] = v0; nrm[1] = v1; nrm[2] = v2; }
        }
    }
    normals[3 * i] = (float)nrm[0];
    normals[3 * i + 1] = (float)nrm[1];
    normals[3 * i + 2] = (float)nrm[2];
    if (eig) { eig[3 * i] = ev[0]; eig[3 * i + 1] = ev[1]; eig[3 * i + 2] = ev[2]; }
}

__global__ void __launch_bounds__(KNN_THREADS) pc_knn_mean_kernel(const float* __restrict__ d2, const int32_t* __restrict__ count, int64_t m, int k,
                                                                  float* __restrict__ avg) {
    const int64_t i = (int64_t)blockIdx.x * KNN_THREADS + threadIdx.x;
    if (i >= m) return;
    const int cnt = min(max(count[i], 0), k);
    double s = 0.0;
    for (int j = 0; j < cnt; ++j) s += (double)sqrtf(d2[i * k + j]);
    avg[i] = cnt ? (float)(s / (double)cnt) : __builtin_nanf("");
}

}  // namespace
}  // namespace bs

extern "C" int bs_pc_query_knn(const void* records, const int32_t* cell_start, int64_t n_records, const float* lo, const float* hi, float cell_size,
                               const int32_t* dims, const float* source, int64_t m, int32_t k, float radius, int32_t* index, float* d2,
                               int32_t* count, void* stream) {
    using namespace bs;
    if (!initialized()) { set_error("bs_pc_query_knn: call bs_init first"); return BS_ERR_NOT_INIT; }
    BS_REQUIRE(records && cell_start && lo && hi && dims && source && index && d2 && count, "bs_pc_query_knn: null pointer");
    BS_REQUIRE(m >= 1 && m < ((int64_t)1 << 31) && n_records >= 0 && n_records < ((int64_t)1 << 31), "bs_pc_query_knn: m = %lld, n_records = %lld",
               (long long)m, (long long)n_records);
    BS_REQUIRE(k >= 1 && k <= BS_PC_KNN_MAX, "bs_pc_query_knn: k = %d (1 .. %d)", k, BS_PC_KNN_MAX);
    BS_REQUIRE(((uintptr_t)records & 15) == 0, "bs_pc_query_knn: records must be 16-byte aligned");
    BS_REQUIRE(radius > 0.0f, "bs_pc_query_knn: radius %g (positive; +inf: none)", (double)radius);
    const PcGrid g = pc_grid(lo, hi, cell_size, dims);
    BS_REQUIRE(pc_grid_ok(g), "bs_pc_query_knn: bad grid (cell size %g, %d x %d x %d cells, at most 2^24)", (double)cell_size, dims[0], dims[1], dims[2]);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const float d2_max = knn_d2_cutoff(radius);
    const dim3 grid((unsigned)cdiv64(m, KNN_THREADS)), thr(KNN_THREADS);
    const f32x4* rec = static_cast<const f32x4*>(records);
#define KNN_QUERY(K) \
    hipLaunchKernelGGL((pc_query_knn_kernel<K>), grid, thr, 0, st, rec, cell_start, g, source, m, (int)k, radius, d2_max, index, d2, count)
    if (k <= 8) KNN_QUERY(8);
    else if (k <= 16) KNN_QUERY(16);
    else KNN_QUERY(32);
#undef KNN_QUERY
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_normals(const float* points, int64_t n, const int32_t* index, const int32_t* count, int32_t k, int32_t orientation,
                             const double* vector, float* normals, double* eigenvalues, void* stream) {
    using namespace bs;
    if (!initialized()) { set_error("bs_pc_normals: call bs_init first"); return BS_ERR_NOT_INIT; }
    BS_REQUIRE(points && index && count && normals, "bs_pc_normals: null pointer");
    BS_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "bs_pc_normals: n = %lld (1 <= n < 2^31)", (long long)n);
    BS_REQUIRE(k >= 1 && k <= BS_PC_KNN_MAX, "bs_pc_normals: k = %d (1 .. %d)", k, BS_PC_KNN_MAX);
    BS_REQUIRE(orientation == BS_PC_ORIENT_AXIS || orientation == BS_PC_ORIENT_DIRECTION || orientation == BS_PC_ORIENT_CAMERA,
               "bs_pc_normals: orientation %d", orientation);
    KnnVec vec = {{0.0, 0.0, 0.0}};
    if (orientation != BS_PC_ORIENT_AXIS) {
        BS_REQUIRE(vector, "bs_pc_normals: the orientation needs its vector");
        for (int a = 0; a < 3; ++a) {
            BS_REQUIRE(isfinite(vector[a]), "bs_pc_normals: the orientation vector is not finite");
            vec.v[a] = vector[a];
        }
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pc_normals_kernel, dim3((unsigned)cdiv64(n, KNN_THREADS)), dim3(KNN_THREADS), 0, st, points, n, index, count, (int)k,
                       (int)orientation, vec, normals, eigenvalues);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_knn_mean_distance(const float* d2, const int32_t* count, int64_t m, int32_t k, float* avg, void* stream) {
    using namespace bs;
    if (!initialized()) { set_error("bs_pc_knn_mean_distance: call bs_init first"); return BS_ERR_NOT_INIT; }
    BS_REQUIRE(d2 && count && avg, "bs_pc_knn_mean_distance: null pointer");
    BS_REQUIRE(m >= 1 && m < ((int64_t)1 << 31), "bs_pc_knn_mean_distance: m = %lld (1 <= m < 2^31)", (long long)m);
    BS_REQUIRE(k >= 1 && k <= BS_PC_KNN_MAX, "bs_pc_knn_mean_distance: k = %d (1 .. %d)", k, BS_PC_KNN_MAX);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pc_knn_mean_kernel, dim3((unsigned)cdiv64(m, KNN_THREADS)), dim3(KNN_THREADS), 0, st, d2, count, m, (int)k, avg);
    BS_CHECK_LAUNCH();
    return BS_OK;
}
