// Trajectory evaluation with the reference's MPEM metrics (bs_similarity_fit, bs_trajectory_metrics; include/bodyslam_hip.h), fp64.
//   estimate_similarity_transformation   BodySLAM_not_refactored/3DM/slam_utils.py:138-169 (Umeyama; evo's umeyama_alignment is the same arithmetic)
//   MPEM_Metrics.compute_pose_metrics    BodySLAM_not_refactored/EVALUATION/evaluation_metrics.py:136-165 (evo: align_origin, align, APE / RPE)
//   TrainingLoss.compute_scale_factor / compute_ARE_and_ATE / compute_RRE_and_RTE   BodySLAM_not_refactored/MPEM/training_utils.py:473-585
//
// bs_similarity_fit: four launches on the caller's stream.
//   sim_pass<0>   grid of at most SIM_GRID blocks: per block the sums of both point sets                      -> partial1 [blocks, 6]
//   sim_means     one block: the partials in block order, / n                                               -> mean [6]
//   sim_pass<1>   the same grid: sum |x - mx|^2 and sum (y - my)(x - mx)^T around those means                -> partial2 [blocks, 10]
//   sim_finish    one block: the partials in block order, the 3x3 SVD (svd3.h), R, s, t                      -> out [16]
// A thread takes 48 bytes of each set at a time -- four fp32 points or two fp64 points, three 16-byte loads -- in a grid-stride loop whose
// shape depends on n alone; sums go thread -> wave (butterfly shuffles) -> block (waves in order, through LDS) -> grid (blocks in order).
// No atomics: the same input gives the same bits in every run.
//
// bs_trajectory_metrics: one launch, one block per trajectory pair, which walks its poses in strided loops (any length).  A block reads
// its own poses only, so a pair's record has the same bits alone or at any place of any batch.
#include <math.h>

#include "common.h"
#include "reduce.h"
#include "rigid3.h"

namespace bs {
namespace {

constexpr int TE_THREADS = 256;
constexpr int TE_WAVES = TE_THREADS / 64;
constexpr int SIM_GRID = 1024;    // blocks of a pass (four per CU); each walks its groups in a fixed order: deterministic partials
constexpr double TE_EPS = 2.220446049250313e-16;    // np.finfo(np.float64).eps
constexpr double TE_DEG = 57.29577951308232;        // 180 / pi

// reduce.h's block_sum for minima (v[0 .. K-1]) and maxima (v[K .. 2K-1]); NaN never enters (callers feed finite errors or the neutral +-inf)
template <int K>
__device__ __forceinline__ void block_minmax(double (&v)[2 * K], double* lds) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            v[k] = fmin(v[k], __shfl_xor(v[k], d, 64));
            v[K + k] = fmax(v[K + k], __shfl_xor(v[K + k], d, 64));
        }
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 2 * K; ++k) lds[w * 2 * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2 * K; ++k) {
        double a = lds[k];
#pragma unroll
        for (int i = 1; i < TE_WAVES; ++i) a = k < K ? fmin(a, lds[i * 2 * K + k]) : fmax(a, lds[i * 2 * K + k]);
        v[k] = a;
    }
}

// ---- Umeyama from the moments -----------------------------------------------------------------------------------------------------------
struct SimFit {
    double R[9], s, t[3], sigma_x;
    int rank;     // singular values of Sxy above eps
};
// mx, my: the means; sigma_x = mean |x - mx|^2; Sxy = mean (y - my)(x - mx)^T.  with_scale = false: s = 1 (evo's align without
// correct_scale).  S = diag(1, 1, -1) on the smallest singular direction when det(Sxy) < 0, as the reference writes it (slam_utils.py:160-162);
// for full rank that is evo's det(U) det(V) < 0.  With exactly two singular values above eps (a planar point set) det(Sxy) is the sign of
// round-off and the Jacobi's third column of U is not determined by Sxy: the column is completed to a right-handed basis and evo's rule
// applies, so R is the proper rotation.  Fewer than two: R is meaningless and the callers report the fit as degenerate.
__device__ void sim_solve(const double (&mx)[3], const double (&my)[3], double sigma_x, const double (&Sxy)[3][3], bool with_scale, SimFit& f) {
    double U[3][3], V[3][3], d[3];
    svd3_jacobi(Sxy, U, d, V);
    const int kmin = svd3_smallest(d);
    f.rank = (d[0] > TE_EPS) + (d[1] > TE_EPS) + (d[2] > TE_EPS);
    bool flip;
    if (f.rank == 3) {
        flip = det3(Sxy) < 0.0;
    } else {
        svd3_complete_column(U, kmin);                          // u_kmin = u_a x u_b gives det(U) = +1
        flip = det3(U) * det3(V) < 0.0;
    }
    double S[3] = {1.0, 1.0, 1.0};
    if (flip) S[kmin] = -1.0;
    svd3_usvt(U, S, V, f.R);
    const double tr = (d[0] * S[0] + d[1] * S[1]) + d[2] * S[2];          // tr(D S)
    f.s = with_scale ? tr / sigma_x : 1.0;
    f.sigma_x = sigma_x;
    for (int i = 0; i < 3; ++i) f.t[i] = my[i] - f.s * ((f.R[i * 3] * mx[0] + f.R[i * 3 + 1] * mx[1]) + f.R[i * 3 + 2] * mx[2]);
}

// ---- bs_similarity_fit ------------------------------------------------------------------------------------------------------------------
typedef double f64x2 __attribute__((ext_vector_type(2)));
template <typename T> struct SimGroup;
template <> struct SimGroup<float> { static constexpr int PTS = 4; typedef f32x4 vec; };
template <> struct SimGroup<double> { static constexpr int PTS = 2; typedef f64x2 vec; };

// group g of a set: points PTS * g .. PTS * g + PTS - 1, 48 bytes.  VEC: the set is 16-byte aligned, three 16-byte loads.
template <typename T, bool VEC>
__device__ __forceinline__ void sim_load(const T* __restrict__ p, int64_t g, double (&o)[SimGroup<T>::PTS * 3]) {
    constexpr int E = SimGroup<T>::PTS * 3, L = 16 / (int)sizeof(T);
    const T* q = p + g * E;
    if (VEC) {
        typedef typename SimGroup<T>::vec vec;
        const vec a = reinterpret_cast<const vec*>(q)[0], b = reinterpret_cast<const vec*>(q)[1], c = reinterpret_cast<const vec*>(q)[2];
#pragma unroll
        for (int k = 0; k < L; ++k) {
            o[k] = (double)a[k];
            o[L + k] = (double)b[k];
            o[2 * L + k] = (double)c[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < E; ++k) o[k] = (double)q[k];
    }
}

// PASS 0: acc[0..2] += x, acc[3..5] += y.  PASS 1: acc[0] += |x - mx|^2, acc[1 + 3 i + j] += (y - my)_i (x - mx)_j
template <int PASS>
__device__ __forceinline__ void sim_point(const double* x, const double* y, const double (&m)[6], double (&acc)[PASS ? 10 : 6]) {
    if (PASS == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            acc[k] += x[k];
            acc[3 + k] += y[k];
        }
    } else {
        const double xc[3] = {x[0] - m[0], x[1] - m[1], x[2] - m[2]};
        const double yc[3] = {y[0] - m[3], y[1] - m[4], y[2] - m[5]};
        acc[0] += (xc[0] * xc[0] + xc[1] * xc[1]) + xc[2] * xc[2];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[1 + 3 * i + j] += yc[i] * xc[j];
    }
}

template <typename T, bool VEC, int PASS>
__global__ void __launch_bounds__(TE_THREADS) sim_pass_kernel(const T* __restrict__ src, const T* __restrict__ dst, int64_t n,
                                                              const double* __restrict__ mean, double* __restrict__ partial) {
    constexpr int K = PASS ? 10 : 6, PTS = SimGroup<T>::PTS;
    __shared__ double lds[TE_WAVES * K];
    double m[6] = {0, 0, 0, 0, 0, 0};
    if (PASS) {
#pragma unroll
        for (int k = 0; k < 6; ++k) m[k] = mean[k];
    }
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    const int64_t groups = n / PTS, stride = (int64_t)gridDim.x * TE_THREADS;
#pragma unroll 2
    for (int64_t g = (int64_t)blockIdx.x * TE_THREADS + threadIdx.x; g < groups; g += stride) {
        double x[PTS * 3], y[PTS * 3];
        sim_load<T, VEC>(src, g, x);
        sim_load<T, VEC>(dst, g, y);
#pragma unroll
        for (int q = 0; q < PTS; ++q) sim_point<PASS>(x + 3 * q, y + 3 * q, m, acc);
    }
    // the tail (n % PTS points), one per thread of block 0
    const int64_t tail = groups * PTS + threadIdx.x;
    if (blockIdx.x == 0 && tail < n) {
        const double x[3] = {(double)src[3 * tail], (double)src[3 * tail + 1], (double)src[3 * tail + 2]};
        const double y[3] = {(double)dst[3 * tail], (double)dst[3 * tail + 1], (double)dst[3 * tail + 2]};
        sim_point<PASS>(x, y, m, acc);
    }
    block_sum<K, TE_WAVES>(acc, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) partial[(int64_t)blockIdx.x * K + k] = acc[k];
    }
}

// column k of partial [blocks, K], the blocks in order
__device__ __forceinline__ double sim_column(const double* __restrict__ partial, int blocks, int K, int k) {
    double a = 0.0;
    for (int b = 0; b < blocks; ++b) a += partial[(int64_t)b * K + k];
    return a;
}

__global__ void __launch_bounds__(64) sim_means_kernel(const double* __restrict__ partial1, int blocks, int64_t n, double* __restrict__ mean) {
    const int k = threadIdx.x;
    if (k < 6) mean[k] = sim_column(partial1, blocks, 6, k) / (double)n;
}

__global__ void __launch_bounds__(64) sim_finish_kernel(const double* __restrict__ partial2, int blocks, int64_t n, const double* __restrict__ mean,
                                                        double* __restrict__ out) {
    __shared__ double tot[10];
    const int k = threadIdx.x;
    if (k < 10) tot[k] = sim_column(partial2, blocks, 10, k) / (double)n;
    __syncthreads();
    if (k != 0) return;
    const double mx[3] = {mean[0], mean[1], mean[2]}, my[3] = {mean[3], mean[4], mean[5]};
    double Sxy[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Sxy[i][j] = tot[1 + 3 * i + j];
    SimFit f;
    sim_solve(mx, my, tot[0], Sxy, true, f);
    for (int i = 0; i < 9; ++i) out[i] = f.R[i];
    out[9] = f.s;
    out[10] = f.t[0]; out[11] = f.t[1]; out[12] = f.t[2];
    out[13] = f.sigma_x;
    out[14] = (double)f.rank;
    out[15] = (double)n;
}

struct SimLayout {
    static constexpr size_t mean = 0;                                   // 8 doubles (6 used)
    static constexpr size_t partial1 = 8 * sizeof(double);              // [SIM_GRID, 6]
    static constexpr size_t partial2 = partial1 + (size_t)SIM_GRID * 6 * sizeof(double);   // [SIM_GRID, 10]
    static constexpr size_t total = partial2 + (size_t)SIM_GRID * 10 * sizeof(double);
};
static_assert(SimLayout::total == BS_SIMILARITY_FIT_WORKSPACE_BYTES, "BS_SIMILARITY_FIT_WORKSPACE_BYTES");

template <typename T>
int sim_launch(const T* src, const T* dst, int64_t n, char* ws, double* out, hipStream_t st) {
    double* mean = reinterpret_cast<double*>(ws + SimLayout::mean);
    double* p1 = reinterpret_cast<double*>(ws + SimLayout::partial1);
    double* p2 = reinterpret_cast<double*>(ws + SimLayout::partial2);
    const int64_t groups = n / SimGroup<T>::PTS;
    const int64_t want = cdiv64(groups, (int64_t)TE_THREADS * 2);       // two groups per thread before the grid grows
    const int blocks = (int)(want < 1 ? 1 : (want > SIM_GRID ? SIM_GRID : want));
    const bool vec = ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0;
    if (vec) hipLaunchKernelGGL((sim_pass_kernel<T, true, 0>), dim3(blocks), dim3(TE_THREADS), 0, st, src, dst, n, (const double*)mean, p1);
    else hipLaunchKernelGGL((sim_pass_kernel<T, false, 0>), dim3(blocks), dim3(TE_THREADS), 0, st, src, dst, n, (const double*)mean, p1);
    BS_CHECK_LAUNCH();
    hipLaunchKernelGGL(sim_means_kernel, dim3(1), dim3(64), 0, st, (const double*)p1, blocks, n, mean);
    BS_CHECK_LAUNCH();
    if (vec) hipLaunchKernelGGL((sim_pass_kernel<T, true, 1>), dim3(blocks), dim3(TE_THREADS), 0, st, src, dst, n, (const double*)mean, p2);
    else hipLaunchKernelGGL((sim_pass_kernel<T, false, 1>), dim3(blocks), dim3(TE_THREADS), 0, st, src, dst, n, (const double*)mean, p2);
    BS_CHECK_LAUNCH();
    hipLaunchKernelGGL(sim_finish_kernel, dim3(1), dim3(64), 0, st, (const double*)p2, blocks, n, (const double*)mean, out);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

// ---- bs_trajectory_metrics --------------------------------------------------------------------------------------------------------------
// evo's lie.se3_inverse: [R^T | -R^T t] (the rotation block is taken as a rotation)
__device__ __forceinline__ Rigid3 aff_inv_se3(const Rigid3& a) {
    Rigid3 c;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) c.r[i * 3 + j] = a.r[j * 3 + i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) c.t[i] = -((c.r[i * 3] * a.t[0] + c.r[i * 3 + 1] * a.t[1]) + c.r[i * 3 + 2] * a.t[2]);
    return c;
}
// np.linalg.inv of an affine 4x4: [A^-1 | -A^-1 t], A^-1 by the adjugate (the training protocol inverts whatever block it is given)
__device__ __forceinline__ Rigid3 aff_inv_general(const Rigid3& a) {
    const double* m = a.r;
    Rigid3 c;
    c.r[0] = m[4] * m[8] - m[5] * m[7];
    c.r[1] = m[2] * m[7] - m[1] * m[8];
    c.r[2] = m[1] * m[5] - m[2] * m[4];
    c.r[3] = m[5] * m[6] - m[3] * m[8];
    c.r[4] = m[0] * m[8] - m[2] * m[6];
    c.r[5] = m[2] * m[3] - m[0] * m[5];
    c.r[6] = m[3] * m[7] - m[4] * m[6];
    c.r[7] = m[1] * m[6] - m[0] * m[7];
    c.r[8] = m[0] * m[4] - m[1] * m[3];
    const double det = (m[0] * c.r[0] + m[1] * c.r[3]) + m[2] * c.r[6];
#pragma unroll
    for (int i = 0; i < 9; ++i) c.r[i] /= det;
#pragma unroll
    for (int i = 0; i < 3; ++i) c.t[i] = -((c.r[i * 3] * a.t[0] + c.r[i * 3 + 1] * a.t[1]) + c.r[i * 3 + 2] * a.t[2]);
    return c;
}
// arccos(clip((tr - 1) / 2, -1, 1)) of a (R^T b) or of (a b^T)
__device__ __forceinline__ double angle_of_trace(double tr) { return acos(fmin(fmax((tr - 1.0) / 2.0, -1.0), 1.0)); }
__device__ __forceinline__ double trace_abT(const double* a, const double* b) {      // tr(a b^T) = sum a_ij b_ij
    double tr = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) tr += (a[i * 3] * b[i * 3] + a[i * 3 + 1] * b[i * 3 + 1]) + a[i * 3 + 2] * b[i * 3 + 2];
    return tr;
}
__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

struct TrajAlign {        // pose i of the prediction as evaluated: (R, t) o scale_s(O o P_i)
    Rigid3 O, A;                // (the top three rows of a 4 x 4 pose; the bottom row is taken as [0 0 0 1])
    double s;
};
__device__ __forceinline__ Rigid3 traj_aligned(const TrajAlign& al, const double* __restrict__ pred, int64_t i) {
    Rigid3 x = rigid3_compose(al.O, rigid3_load(pred + i * 16));
    x.t[0] *= al.s; x.t[1] *= al.s; x.t[2] *= al.s;
    return rigid3_compose(al.A, x);
}

// the four errors of index i: err[0] ATE, err[1] ARE (both when i < n), err[2] RTE, err[3] RRE (both when i < pairs)
__device__ __forceinline__ void traj_errors(int protocol, const TrajAlign& al, const double* __restrict__ gt, const double* __restrict__ pred,
                                            int64_t i, int64_t n, int64_t pairs, int64_t step, int64_t delta, double (&err)[4]) {
    if (protocol == BS_TRAJ_EVO) {
        if (i < n) {
            const Rigid3 q = rigid3_load(gt + i * 16), p = traj_aligned(al, pred, i);
            err[0] = norm3(q.t[0] - p.t[0], q.t[1] - p.t[1], q.t[2] - p.t[2]);
            err[1] = angle_of_trace(trace_abT(q.r, p.r)) * TE_DEG;                  // tr(Q^T P) = sum q_ij p_ij
        }
        if (i < pairs) {
            const int64_t a = i * step, b = a + delta;
            const Rigid3 qrel = rigid3_compose(aff_inv_se3(rigid3_load(gt + a * 16)), rigid3_load(gt + b * 16));
            const Rigid3 prel = rigid3_compose(aff_inv_se3(traj_aligned(al, pred, a)), traj_aligned(al, pred, b));
            const Rigid3 e = rigid3_compose(aff_inv_se3(qrel), prel);
            err[2] = norm3(e.t[0], e.t[1], e.t[2]);
            err[3] = angle_of_trace((e.r[0] + e.r[4]) + e.r[8]) * TE_DEG;
        }
    } else {
        if (i < n) {
            const Rigid3 q = rigid3_load(gt + i * 16), p = rigid3_load(pred + i * 16);
            err[0] = norm3(q.t[0] - al.s * p.t[0], q.t[1] - al.s * p.t[1], q.t[2] - al.s * p.t[2]);
            err[1] = angle_of_trace(trace_abT(q.r, p.r));
        }
        if (i < pairs) {
            const int64_t a = i * step, b = a + delta;
            const Rigid3 qrel = rigid3_compose(aff_inv_general(rigid3_load(gt + a * 16)), rigid3_load(gt + b * 16));
            const Rigid3 prel = rigid3_compose(aff_inv_general(rigid3_load(pred + a * 16)), rigid3_load(pred + b * 16));
            err[2] = norm3(qrel.t[0] - prel.t[0], qrel.t[1] - prel.t[1], qrel.t[2] - prel.t[2]);
            err[3] = angle_of_trace(trace_abT(qrel.r, prel.r));
        }
    }
}

__global__ void __launch_bounds__(TE_THREADS) traj_metrics_kernel(const double* __restrict__ gt_all, const double* __restrict__ pred_all,
                                                                  const int32_t* __restrict__ offsets, int64_t total, int32_t protocol,
                                                                  int32_t delta, int32_t flags, double* __restrict__ out) {
    __shared__ double lds[TE_WAVES * 10];
    __shared__ SimFit fit;
    const int t = threadIdx.x;
    double* o = out + (int64_t)blockIdx.x * BS_TRAJ_FIELDS;
    const int64_t o0 = offsets[blockIdx.x], o1 = offsets[blockIdx.x + 1];
    const double nan = __builtin_nan("");
    if (o0 < 0 || o1 < o0 || o1 > total) {                   // (uniform per block) offsets that leave the arrays: nothing is read
        if (t < BS_TRAJ_FIELDS) o[t] = t == 2 ? (double)BS_TRAJ_BAD_OFFSETS : (t < 2 ? 0.0 : nan);
        return;
    }
    const int64_t n = o1 - o0;
    const bool evo = protocol == BS_TRAJ_EVO;
    const bool all_pairs = !evo || (flags & BS_TRAJ_ALL_PAIRS);
    const int64_t step = all_pairs ? 1 : delta;
    // evo's id pairs: (i, i + delta) over i = 0, delta, 2 delta, ... (ceil(n / delta) - 1 of them), or over every i < n - delta
    const int64_t pairs = n <= delta ? 0 : (all_pairs ? n - delta : (n + delta - 1) / delta - 1);
    if (n < (int64_t)delta + 1) {
        if (t < BS_TRAJ_FIELDS) o[t] = t == 0 ? (double)n : (t == 1 ? 0.0 : (t == 2 ? (double)BS_TRAJ_TOO_SHORT : nan));
        return;
    }
    const double* gt = gt_all + o0 * 16;
    const double* pred = pred_all + o0 * 16;

    TrajAlign al;
    al.O = rigid3_identity();
    al.A = rigid3_identity();
    al.s = 1.0;
    int status = BS_TRAJ_OK;
    double sigma_x = 0.0, rank = 3.0;
    if (evo) {
        if (flags & BS_TRAJ_ALIGN_ORIGIN) al.O = rigid3_compose(rigid3_load(gt), aff_inv_se3(rigid3_load(pred)));
        if (flags & (BS_TRAJ_ALIGN | BS_TRAJ_CORRECT_SCALE)) {
            // the positions of the origin-aligned prediction (x) against the ground truth's (y): means, then moments about them
            double m[6] = {0, 0, 0, 0, 0, 0};
            for (int64_t i = t; i < n; i += TE_THREADS) {
                const double* p = pred + i * 16;
                const double* q = gt + i * 16;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    m[k] += ((al.O.r[k * 3] * p[3] + al.O.r[k * 3 + 1] * p[7]) + al.O.r[k * 3 + 2] * p[11]) + al.O.t[k];
                    m[3 + k] += q[4 * k + 3];
                }
            }
            block_sum<6, TE_WAVES>(m, lds);
#pragma unroll
            for (int k = 0; k < 6; ++k) m[k] /= (double)n;
            double acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int64_t i = t; i < n; i += TE_THREADS) {
                const double* p = pred + i * 16;
                const double* q = gt + i * 16;
                double x[3], y[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    x[k] = ((al.O.r[k * 3] * p[3] + al.O.r[k * 3 + 1] * p[7]) + al.O.r[k * 3 + 2] * p[11]) + al.O.t[k];
                    y[k] = q[4 * k + 3];
                }
                sim_point<1>(x, y, m, acc);
            }
            block_sum<10, TE_WAVES>(acc, lds);
            if (t == 0) {
                const double mx[3] = {m[0], m[1], m[2]}, my[3] = {m[3], m[4], m[5]};
                double Sxy[3][3];
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) Sxy[i][j] = acc[1 + 3 * i + j] / (double)n;
                sim_solve(mx, my, acc[0] / (double)n, Sxy, (flags & BS_TRAJ_CORRECT_SCALE) != 0, fit);
            }
            __syncthreads();
            sigma_x = fit.sigma_x;
            rank = (double)fit.rank;
            // evo raises where fewer than two singular values exceed eps; sigma_x = 0 divides by zero
            if (fit.rank < 2 || !(fit.sigma_x > 0.0)) status = BS_TRAJ_DEGENERATE;
            if (flags & BS_TRAJ_CORRECT_SCALE) al.s = fit.s;
            if (flags & BS_TRAJ_ALIGN) {
#pragma unroll
                for (int k = 0; k < 9; ++k) al.A.r[k] = fit.R[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) al.A.t[k] = fit.t[k];
            }
        }
    } else {
        // compute_scale_factor (training_utils.py:473-496): sum gt_t . pred_t / sum |pred_t|^2
        double a[2] = {0, 0};
        for (int64_t i = t; i < n; i += TE_THREADS) {
            const double* p = pred + i * 16;
            const double* q = gt + i * 16;
            a[0] += (q[3] * p[3] + q[7] * p[7]) + q[11] * p[11];
            const double nr = norm3(p[3], p[7], p[11]);          // np.linalg.norm(...) ** 2
            a[1] += nr * nr;
        }
        block_sum<2, TE_WAVES>(a, lds);
        al.s = a[0] / a[1];
        sigma_x = a[1];
        if (!(a[1] > 0.0)) status = BS_TRAJ_DEGENERATE;
    }
    if (status != BS_TRAJ_OK) {                               // (uniform per block)
        if (t < BS_TRAJ_FIELDS) o[t] = t == 0 ? (double)n : (t == 1 ? (double)pairs : (t == 2 ? (double)status : (t == 36 ? sigma_x : (t == 37 ? rank : nan))));
        return;
    }

    // the errors: sums and sums of squares, extrema; then the squared deviations from the means (np.std is a two-pass population std)
    double sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const double inf = __builtin_inf();
    double mm[8] = {inf, inf, inf, inf, -inf, -inf, -inf, -inf};
    for (int64_t i = t; i < n; i += TE_THREADS) {
        double e[4] = {0, 0, 0, 0};
        traj_errors(protocol, al, gt, pred, i, n, pairs, step, delta, e);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < 2 || i < pairs) {
                sum[k] += e[k];
                sum[4 + k] += e[k] * e[k];
                mm[k] = fmin(mm[k], e[k]);
                mm[4 + k] = fmax(mm[4 + k], e[k]);
            }
        }
    }
    block_sum<8, TE_WAVES>(sum, lds);
    block_minmax<4>(mm, lds);
    const double cnt[4] = {(double)n, (double)n, (double)pairs, (double)pairs};
    double mean[4], dev[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) mean[k] = sum[k] / cnt[k];
    for (int64_t i = t; i < n; i += TE_THREADS) {
        double e[4] = {0, 0, 0, 0};
        traj_errors(protocol, al, gt, pred, i, n, pairs, step, delta, e);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < 2 || i < pairs) dev[k] += (e[k] - mean[k]) * (e[k] - mean[k]);
        }
    }
    block_sum<4, TE_WAVES>(dev, lds);
    if (t == 0) {
        o[0] = (double)n;
        o[1] = (double)pairs;
        o[2] = (double)BS_TRAJ_OK;
        o[3] = al.s;
        for (int k = 0; k < 9; ++k) o[4 + k] = al.A.r[k];
        for (int k = 0; k < 3; ++k) o[13 + k] = al.A.t[k];
        for (int k = 0; k < 4; ++k) {
            double* r = o + 16 + 5 * k;
            r[0] = sqrt(sum[4 + k] / cnt[k]);
            r[1] = mean[k];
            r[2] = sqrt(dev[k] / cnt[k]);
            r[3] = mm[k];
            r[4] = mm[4 + k];
        }
        o[36] = sigma_x;
        o[37] = rank;
        o[38] = 0.0;
        o[39] = 0.0;
    }
}

}  // namespace
}  // namespace bs

extern "C" int bs_similarity_fit(const void* source, const void* target, int64_t n, int32_t dtype, void* workspace, int64_t workspace_bytes,
                                 double* out, void* stream) {
    using namespace bs;
    if (!initialized()) { set_error("bs_similarity_fit: call bs_init first"); return BS_ERR_NOT_INIT; }
    BS_REQUIRE(source && target && workspace && out, "bs_similarity_fit: null pointer");
    BS_REQUIRE(n >= 1 && n <= 2147483647LL, "bs_similarity_fit: n = %lld points (1 <= n <= 2^31 - 1)", (long long)n);
    BS_REQUIRE(dtype == BS_F32 || dtype == BS_F64, "bs_similarity_fit: dtype %d (BS_F32 or BS_F64)", dtype);
    BS_REQUIRE(workspace_bytes >= (int64_t)BS_SIMILARITY_FIT_WORKSPACE_BYTES, "bs_similarity_fit: workspace of %lld bytes, %lld needed",
               (long long)workspace_bytes, (long long)BS_SIMILARITY_FIT_WORKSPACE_BYTES);
    BS_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)out & 7) == 0, "bs_similarity_fit: workspace and out must be 8-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    if (dtype == BS_F32) {
        BS_REQUIRE(((uintptr_t)source & 3) == 0 && ((uintptr_t)target & 3) == 0, "bs_similarity_fit: misaligned fp32 points");
        return sim_launch(static_cast<const float*>(source), static_cast<const float*>(target), n, ws, out, st);
    }
    BS_REQUIRE(((uintptr_t)source & 7) == 0 && ((uintptr_t)target & 7) == 0, "bs_similarity_fit: misaligned fp64 points");
    return sim_launch(static_cast<const double*>(source), static_cast<const double*>(target), n, ws, out, st);
}

extern "C" int bs_trajectory_metrics(const double* gt, const double* pred, const int32_t* offsets, int32_t S, int64_t total_poses, int32_t protocol,
                                     int32_t delta, int32_t flags, double* out, void* stream) {
    using namespace bs;
    if (!initialized()) { set_error("bs_trajectory_metrics: call bs_init first"); return BS_ERR_NOT_INIT; }
    BS_REQUIRE(gt && pred && offsets && out, "bs_trajectory_metrics: null pointer");
    BS_REQUIRE(S >= 1, "bs_trajectory_metrics: S = %d trajectory pairs (>= 1)", S);
    BS_REQUIRE(total_poses >= 0 && total_poses <= 2147483647LL, "bs_trajectory_metrics: %lld poses in all (int32 offsets)", (long long)total_poses);
    BS_REQUIRE(protocol == BS_TRAJ_EVO || protocol == BS_TRAJ_TRAINING, "bs_trajectory_metrics: protocol %d", protocol);
    BS_REQUIRE(delta >= 1, "bs_trajectory_metrics: delta %d (>= 1)", delta);
    BS_REQUIRE((flags & ~(BS_TRAJ_ALIGN_ORIGIN | BS_TRAJ_ALIGN | BS_TRAJ_CORRECT_SCALE | BS_TRAJ_ALL_PAIRS)) == 0, "bs_trajectory_metrics: flags 0x%x", flags);
    BS_REQUIRE(((uintptr_t)gt & 7) == 0 && ((uintptr_t)pred & 7) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)offsets & 3) == 0,
               "bs_trajectory_metrics: misaligned pointer");
    hipLaunchKernelGGL(traj_metrics_kernel, dim3((unsigned)S), dim3(TE_THREADS), 0, reinterpret_cast<hipStream_t>(stream), gt, pred, offsets,
                       total_poses, protocol, delta, flags, out);
    BS_CHECK_LAUNCH();
    return BS_OK;
}
