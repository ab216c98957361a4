// Rigid ICP registration (bs_icp_step, bs_icp_finish; include/bodyslam_hip.h): the role of Open3D's registration_icp with
// TransformationEstimationPointToPlane / PointToPoint and ICPConvergenceCriteria, and of evaluate_registration.  Restated from Open3D's
// published interface; parity with Open3D is UNPINNED.  The statement is tests/_icp_ref.py.
//
// One iteration is two launches, and the host reads nothing in between: the transform, the iteration count, the previous fitness / rmse and
// the status live in a small device state, and once a status is set both kernels return at their first instruction, so the host can
// enqueue iterations in chunks and read the state once per chunk.
//   bs_icp_step    one thread per source row: p = fl32(((a0 s0 + a1 s1) + a2 s2) + t) in fp64 rounded once (bs_pc_transform's arithmetic,
//                  T from the device state); the exact nearest target point of p by the walk over the grid's Chebyshev shells that
//                  bs_pc_query_grid runs (pc_grid.h: the same device function) -- with NO shell cap and NO brute-force fallback: the radius
//                  is mandatory, and a source searches until the bound holds, the whole grid has been seen, or lb * 0.9999 > radius, so
//                  the correspondence is the statement's for every cell size.  Valid when the fp32 distance d <= radius.  The terms in
//                  fp64, relative to c = the midpoint of the grid's box (a cloud far from the origin loses no digits):
//                    all      count, usable count, sum d^2 (d widened to fp64)
//                    plane    usable = the target normal n is finite and non-zero; r = ((p - q) . n), J = [(p - c) x n, n]; the 21 upper
//                             entries of J J^T, then J r
//                    point    usable = valid; sum (p - c), sum (q - c), sum (p - c)(q - c)^T
//                  reduced in a fixed order: the xor butterfly in the wave, the waves in order, one row of BS_ICP_PARTIAL_FIELDS doubles per
//                  block; the grid depends on m alone.  No floating-point atomics; LDS carries the four wave sums only and is read 16 bytes
//                  per lane (DESIGN section 7's rule for kernels that may run beside a second stream).
//   bs_icp_finish  one block: the rows added in an order fixed by their number (a wave per term, lanes strided over the rows, the
//                  butterfly: reduce.h); fitness = count / m, rmse = sqrt(sum d^2 / count); the log row; the stopping rule; the solve --
//                  Cholesky of the 6 x 6 normal matrix (block6.h) and T <- C exp(delta) C^-1 T, or Kabsch (rigid3.h) and T <- [R | t] T --
//                  and the status word.  One thread does the serial part: a 6 x 6 system.
#include <math.h>

#include "block6.h"
#include "common.h"
#include "pc_grid.h"
#include "reduce.h"
#include "rigid3.h"

namespace bs {
namespace {

constexpr int ICP_THREADS = 256, ICP_WAVES = ICP_THREADS / 64, ICP_ROW = BS_ICP_PARTIAL_FIELDS;
constexpr int ICP_TERMS_PLANE = 3 + 27, ICP_TERMS_POINT = 3 + 15;
// the device state (BS_ICP_STATE_FIELDS doubles, then the log)
constexpr int IS_STATUS = 0, IS_ITER = 1, IS_T = 2, IS_PREV = 14, IS_EVAL = 16, IS_TOTALS = 32;
static_assert(ICP_TERMS_PLANE <= ICP_ROW && IS_TOTALS + ICP_ROW <= BS_ICP_STATE_FIELDS && ICP_ROW % 2 == 0, "icp layout");

typedef double f64x2 __attribute__((ext_vector_type(2)));

template <bool PLANE, typename S>
__global__ void __launch_bounds__(ICP_THREADS) icp_step_kernel(const f32x4* __restrict__ records, const int32_t* __restrict__ cell_start, PcGrid g,
                                                               const float* __restrict__ target, const float* __restrict__ normals, int64_t n_target,
                                                               const S* __restrict__ src, int64_t m, float radius, int mode, double c0, double c1,
                                                               double c2, const double* __restrict__ state, double* __restrict__ partial) {
    if (mode == BS_ICP_ITERATE && state[IS_STATUS] != 0.0) return;
    constexpr int NT = PLANE ? ICP_TERMS_PLANE : ICP_TERMS_POINT;
    double v[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) v[k] = 0.0;
    const int64_t i = (int64_t)blockIdx.x * ICP_THREADS + threadIdx.x;
    if (i < m) {
        const double s0 = (double)src[3 * i], s1 = (double)src[3 * i + 1], s2 = (double)src[3 * i + 2];
        float p[3];
        affine_point_f32(state + IS_T, s0, s1, s2, p);
        const float px = p[0], py = p[1], pz = p[2];
        if (pc_finite(px) && pc_finite(py) && pc_finite(pz)) {
            float best;
            int32_t bi;
            pc_walk_shells(records, cell_start, g, px, py, pz, radius, 0x7fffffff, best, bi);          // no cap: always runs to the end
            const float d = sqrtf(best);
            if (bi >= 0 && (int64_t)bi < n_target && !(d > radius)) {                                   // (PC_NONE is above every n_target)
                v[0] = 1.0;
                v[2] = (double)d * (double)d;
                const double q0 = (double)target[3 * (int64_t)bi], q1 = (double)target[3 * (int64_t)bi + 1], q2 = (double)target[3 * (int64_t)bi + 2];
                const double a0 = (double)px - c0, a1 = (double)py - c1, a2 = (double)pz - c2;
                if (PLANE) {
                    const float nx = normals[3 * (int64_t)bi], ny = normals[3 * (int64_t)bi + 1], nz = normals[3 * (int64_t)bi + 2];
                    if (pc_finite(nx) && pc_finite(ny) && pc_finite(nz) && (nx != 0.0f || ny != 0.0f || nz != 0.0f)) {
                        const double n0 = (double)nx, n1 = (double)ny, n2 = (double)nz;
                        const double r = (((double)px - q0) * n0 + ((double)py - q1) * n1) + ((double)pz - q2) * n2;
                        const double J[6] = {a1 * n2 - a2 * n1, a2 * n0 - a0 * n2, a0 * n1 - a1 * n0, n0, n1, n2};
                        v[1] = 1.0;
                        int k = 3;
#pragma unroll
                        for (int a = 0; a < 6; ++a)
#pragma unroll
                            for (int b = a; b < 6; ++b) v[k++] = J[a] * J[b];
#pragma unroll
                        for (int a = 0; a < 6; ++a) v[24 + a] = J[a] * r;
                    }
                } else {
                    const double b[3] = {q0 - c0, q1 - c1, q2 - c2}, a[3] = {a0, a1, a2};
                    v[1] = 1.0;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        v[3 + k] = a[k];
                        v[6 + k] = b[k];
#pragma unroll
                        for (int j = 0; j < 3; ++j) v[9 + 3 * k + j] = a[k] * b[j];
                    }
                }
            }
        }
    }
    __shared__ f64x2 red[ICP_ROW][ICP_WAVES / 2];          // [term][wave], 32 bytes per term
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const double s = wave_sum(v[k]);
        if (lane == 0) reinterpret_cast<double*>(red)[k * ICP_WAVES + wave] = s;
    }
    __syncthreads();
    if (threadIdx.x < ICP_ROW) {
        double out = 0.0;
        if (threadIdx.x < NT) {
            const f64x2 lo = red[threadIdx.x][0], hi = red[threadIdx.x][1];
            out = ((lo[0] + lo[1]) + hi[0]) + hi[1];
        }
        partial[(int64_t)blockIdx.x * ICP_ROW + threadIdx.x] = out;
    }
}

// delta = -A^-1 b by Cholesky (s: the 21 upper entries of A, then b), g = exp(delta).  false: a pivot is not positive and finite
__device__ bool icp_solve_plane(const double* __restrict__ s, Rigid3& g) {
    double A[36], L[36], nb[6], d[6];
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) A[b * 6 + a] = s[k++];             // the lower triangle, which is what chol6 reads
    chol6(A, L);
    // chol6 does not stop at a bad pivot, and this test rejects what a test of each pivot p would: up to the first bad one the arithmetic is
    // the same, and p <= 0, NaN or Inf gives sqrt(p) = a zero, NaN or Inf, which fails here
    for (int j = 0; j < 6; ++j)
        if (!(L[j * 6 + j] > 0.0) || !(L[j * 6 + j] < INFINITY)) return false;
    for (int i = 0; i < 6; ++i) nb[i] = -s[21 + i];
    lsolve6(L, nb, 1, d);
    ltsolve6(L, d);
    for (int i = 0; i < 6; ++i)
        if (!(fabs(d[i]) < INFINITY)) return false;
    se3_exp(d, g);
    return true;
}

// Kabsch on the sums relative to c (s: sum p, sum q, sum p q^T; rigid3.h takes sum q p^T).  false: the second singular value is not
// positive (collinear or coincident pairs)
__device__ bool icp_solve_point(const double* __restrict__ s, double n, Rigid3& g) {
    double t[15];
    for (int i = 0; i < 6; ++i) t[i] = s[i];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) t[6 + 3 * i + j] = s[6 + 3 * j + i];
    const KabschFit f = kabsch_from_sums(t, n);
    if (!(fmin(f.da, f.db) > 0.0) || !(fmax(f.da, f.db) < INFINITY)) return false;
    g = f.g;
    return true;
}

__global__ void __launch_bounds__(ICP_THREADS) icp_finish_kernel(const double* __restrict__ partial, int nblocks, double m, int plane, int mode,
                                                                 int max_iteration, double rel_fitness, double rel_rmse, double c0, double c1,
                                                                 double c2, double* __restrict__ state) {
    if (mode == BS_ICP_ITERATE && state[IS_STATUS] != 0.0) return;
    __shared__ f64x2 tot[ICP_ROW / 2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nt = plane ? ICP_TERMS_PLANE : ICP_TERMS_POINT;
    for (int k = wave; k < ICP_ROW; k += ICP_WAVES) {
        const double s = column_sum(partial, k < nt ? nblocks : 0, ICP_ROW, k, lane);          // (a term the estimation has not: +0)
        if (lane == 0) reinterpret_cast<double*>(tot)[k] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s[ICP_ROW];
#pragma unroll
    for (int j = 0; j < ICP_ROW / 2; ++j) {
        const f64x2 u = tot[j];
        s[2 * j] = u[0];
        s[2 * j + 1] = u[1];
    }
    for (int k = 0; k < ICP_ROW; ++k) state[IS_TOTALS + k] = s[k];
    const double count = s[0], usable = s[1];
    const double fitness = count / m, rmse = count > 0.0 ? sqrt(s[2] / count) : 0.0;
    if (mode != BS_ICP_ITERATE) {
        state[IS_EVAL] = fitness; state[IS_EVAL + 1] = rmse; state[IS_EVAL + 2] = count; state[IS_EVAL + 3] = usable;
        return;
    }
    const int it = (int)state[IS_ITER];
    if (it >= max_iteration) { state[IS_STATUS] = (double)BS_ICP_MAX_ITERATION; return; }            // (not reached: the status stops the run first)
    double* row = state + BS_ICP_STATE_FIELDS + (int64_t)it * BS_ICP_LOG_FIELDS;
    row[0] = fitness; row[1] = rmse; row[2] = count; row[3] = usable;
    state[IS_ITER] = (double)(it + 1);
    if (it >= 1 && fabs(fitness - state[IS_PREV]) < rel_fitness && fabs(rmse - state[IS_PREV + 1]) < rel_rmse) {
        state[IS_STATUS] = (double)BS_ICP_CONVERGED;
        return;
    }
    state[IS_PREV] = fitness;
    state[IS_PREV + 1] = rmse;
    Rigid3 g;
    const bool ok = plane ? (usable >= 6.0 && icp_solve_plane(s + 3, g)) : (count >= 3.0 && icp_solve_point(s + 3, count, g));
    if (!ok) { state[IS_STATUS] = (double)BS_ICP_DEGENERATE; return; }
    // g acts on coordinates relative to c: x -> R (x - c) + t + c
    const double c[3] = {c0, c1, c2};
    for (int i = 0; i < 3; ++i) g.t[i] = (g.t[i] + c[i]) - ((g.r[i * 3] * c[0] + g.r[i * 3 + 1] * c[1]) + g.r[i * 3 + 2] * c[2]);
    left_apply(g, state + IS_T);
    if (it + 1 >= max_iteration) state[IS_STATUS] = (double)BS_ICP_MAX_ITERATION;
}

}  // namespace
}  // namespace bs

extern "C" int bs_icp_step(const void* records, const int32_t* cell_start, int64_t n_records, const float* lo, const float* hi, float cell_size,
                           const int32_t* dims, const float* target, const float* normals, int64_t n_target, const void* source, int32_t dtype,
                           int64_t m, float max_distance, int32_t estimation, int32_t mode, const double* state, double* partial, void* stream) {
    using namespace bs;
    if (!initialized()) { set_error("bs_icp_step: call bs_init first"); return BS_ERR_NOT_INIT; }
    BS_REQUIRE(records && cell_start && lo && hi && dims && target && source && state && partial, "bs_icp_step: null pointer");
    BS_REQUIRE(estimation == BS_ICP_POINT_TO_POINT || estimation == BS_ICP_POINT_TO_PLANE, "bs_icp_step: estimation %d", estimation);
    BS_REQUIRE(estimation == BS_ICP_POINT_TO_POINT || normals, "bs_icp_step: point-to-plane needs the target's normals");
    BS_REQUIRE(mode == BS_ICP_ITERATE || mode == BS_ICP_EVALUATE, "bs_icp_step: mode %d", mode);
    BS_REQUIRE(dtype == BS_F32 || dtype == BS_F64, "bs_icp_step: dtype %d (BS_F32 or BS_F64)", dtype);
    BS_REQUIRE(m >= 1 && m < ((int64_t)1 << 31) && n_records >= 0 && n_records <= n_target && n_target >= 1 && n_target < ((int64_t)1 << 31),
               "bs_icp_step: m = %lld, n_records = %lld, n_target = %lld", (long long)m, (long long)n_records, (long long)n_target);
    BS_REQUIRE(((uintptr_t)records & 15) == 0 && ((uintptr_t)state & 15) == 0 && ((uintptr_t)partial & 15) == 0,
               "bs_icp_step: records, state and partial must be 16-byte aligned");
    BS_REQUIRE(max_distance > 0.0f && max_distance < INFINITY, "bs_icp_step: max_distance %g (a positive finite radius is mandatory)", (double)max_distance);
    const PcGrid g = pc_grid(lo, hi, cell_size, dims);
    BS_REQUIRE(pc_grid_ok(g), "bs_icp_step: bad grid (cell size %g, %d x %d x %d cells, at most 2^24)", (double)cell_size, dims[0], dims[1], dims[2]);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const double c0 = ((double)lo[0] + (double)hi[0]) * 0.5, c1 = ((double)lo[1] + (double)hi[1]) * 0.5, c2 = ((double)lo[2] + (double)hi[2]) * 0.5;
    const dim3 grid((unsigned)cdiv64(m, ICP_THREADS)), thr(ICP_THREADS);
    const f32x4* rec = static_cast<const f32x4*>(records);
#define ICP_STEP(PLANE, S)                                                                                                                  \
    hipLaunchKernelGGL((icp_step_kernel<PLANE, S>), grid, thr, 0, st, rec, cell_start, g, target, normals, n_target, static_cast<const S*>(source), \
                       m, max_distance, (int)mode, c0, c1, c2, state, partial)
    if (estimation == BS_ICP_POINT_TO_PLANE) {
        if (dtype == BS_F32) ICP_STEP(true, float); else ICP_STEP(true, double);
    } else {
        if (dtype == BS_F32) ICP_STEP(false, float); else ICP_STEP(false, double);
    }
#undef ICP_STEP
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_icp_finish(const double* partial, int64_t m, const float* lo, const float* hi, int32_t estimation, int32_t mode,
                             int32_t max_iteration, double relative_fitness, double relative_rmse, double* state, void* stream) {
    using namespace bs;
    if (!initialized()) { set_error("bs_icp_finish: call bs_init first"); return BS_ERR_NOT_INIT; }
    BS_REQUIRE(partial && lo && hi && state, "bs_icp_finish: null pointer");
    BS_REQUIRE(estimation == BS_ICP_POINT_TO_POINT || estimation == BS_ICP_POINT_TO_PLANE, "bs_icp_finish: estimation %d", estimation);
    BS_REQUIRE(mode == BS_ICP_ITERATE || mode == BS_ICP_EVALUATE, "bs_icp_finish: mode %d", mode);
    BS_REQUIRE(m >= 1 && m < ((int64_t)1 << 31), "bs_icp_finish: m = %lld (1 <= m < 2^31)", (long long)m);
    BS_REQUIRE(max_iteration >= 1 && max_iteration <= BS_ICP_MAX_ITERATIONS, "bs_icp_finish: max_iteration %d (1 .. %d)", max_iteration, BS_ICP_MAX_ITERATIONS);
    BS_REQUIRE(relative_fitness == relative_fitness && relative_rmse == relative_rmse, "bs_icp_finish: NaN criterion");
    BS_REQUIRE(((uintptr_t)state & 15) == 0 && ((uintptr_t)partial & 15) == 0, "bs_icp_finish: state and partial must be 16-byte aligned");
    for (int a = 0; a < 3; ++a) BS_REQUIRE(isfinite(lo[a]) && isfinite(hi[a]), "bs_icp_finish: bounds not finite");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const double c0 = ((double)lo[0] + (double)hi[0]) * 0.5, c1 = ((double)lo[1] + (double)hi[1]) * 0.5, c2 = ((double)lo[2] + (double)hi[2]) * 0.5;
    hipLaunchKernelGGL(icp_finish_kernel, dim3(1), dim3(ICP_THREADS), 0, st, partial, (int)cdiv64(m, ICP_THREADS), (double)m,
                       (int)(estimation == BS_ICP_POINT_TO_PLANE), (int)mode, (int)max_iteration, relative_fitness, relative_rmse, c0, c1, c2, state);
    BS_CHECK_LAUNCH();
    return BS_OK;
}
