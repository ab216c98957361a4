// Loop closure (bs_orb_lift, bs_orb_match_pairs, bs_loop_register; include/bodyslam_hip.h): one frame's ORB features against many stored
// keyframes, and a RANSAC rigid registration of the matched 3-D points that gives a pose-graph edge or says "no closure".
// The reference declares the step and never wrote it: BodySLAM_not_refactored/3DM/slam.py:30,41,42 (perform_loop_closure, num_closure,
// global_key_frame_indices) and :79-80 (a call of an undefined self._loop_closure()).  Nothing here is the reference's code.  Restated from
// publications, parity with any library UNPINNED:
//   RANSAC                Fischler & Bolles 1981; minimal sample = three correspondences
//   rigid fit             Kabsch 1976 / Arun, Huang & Blostein 1987 (the SVD of the 3 x 3 cross-covariance, proper rotation enforced as
//                         slam_utils.ensure_so3_v2 does: the sign goes to the smallest singular direction)
//   information matrix    sum G^T G with G = [ -[q]x | I3 ] over the inlier train-frame points, rotation parameters first: the form of
//                         Open3D's get_information_matrix_from_point_clouds, restated from its documentation; parity with Open3D UNPINNED
// The statement, with every choice that makes it reproducible, is tests/_loop_closure_ref.py.
//
//   bs_orb_lift           lift_kernel, one thread per keypoint: associate_depth's lookup (orb_match.h depth_at) + finite, pixel_to_3d in fp64
//   bs_orb_match_pairs    match_pairs_kernel, one block per (query frame, train frame): orb_match.h's body, the one bs_orb_match runs
//   bs_loop_register      register_kernel, one block per pair:
//     1 correspondences   the matches with distance <= max_hamming whose two points are valid, compacted in match order (block scan)
//     2 hypotheses        one thread per hypothesis h (strided): three distinct indices from a counter-based integer hash of
//                         (seed, pair, h, draw) -- loop_draw in ransac3.h, no RNG state --, Kabsch, score = #(|R p + t - q| < tau)
//     3 winner            the highest score, the lowest h among equals; a best score below 3 rejects the pair
//     4 refit             n_refit rounds of Kabsch (rigid3.h) over the current inliers + recount.  Centroids and covariance are block sums
//                         in a fixed order (thread-strided partial sums, then reduce.h's block_sum): no atomics, same bits in every run
//     5 record            T, counts, RMSE, the information matrix; the inlier mask by match row
// LDS: the correspondences as four arrays of 16-byte pairs -- source (x, y), (z, match row), target (x, y), (z, 0) -- 4 x 500 x 16 B =
// 32 000 B, + 2 000 B of inlier flags + 2 x 1 024 B for the winner + 4 x 21 x 8 B of reduction scratch: 36.7 KB.  Every gather of the
// hypothesis stage (three random correspondences per thread) and every walk over the correspondences reads 16 bytes per lane: DESIGN
// section 7's rule for a kernel that may run beside another stream's work (run_slam_loop has two streams).
// Time not measured yet (tools/loop_closure_time.py).
#include <math.h>

#include "common.h"
#include "orb_match.h"
#include "ransac3.h"
#include "reduce.h"
#include "rigid3.h"

namespace bs {
namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int LC_THREADS = ORB_THREADS;
constexpr int LC_WAVES = LC_THREADS / 64;
constexpr double LC_RANK_EPS = RANSAC3_RANK_EPS;

// ---- bs_orb_lift ------------------------------------------------------------------------------------------------------------------------
// xyz [batch, ORB_KP, 4] fp64 = (x, y, z, valid 0.0 / 1.0); rows at and behind a frame's count are zero
__global__ void __launch_bounds__(LC_THREADS) lift_kernel(const float* __restrict__ pt, const int* __restrict__ counts, const float* __restrict__ depth, int H,
                                                          int W, double fx, double fy, double cx, double cy, double* __restrict__ xyz) {
    const int k = blockIdx.x * LC_THREADS + threadIdx.x, f = blockIdx.y;
    if (k >= ORB_KP) return;
    const int n = min(counts[f * (BS_ORB_MAX_LEVELS + 1) + BS_ORB_MAX_LEVELS], ORB_KP);
    f64x2 a = {0.0, 0.0}, b = {0.0, 0.0};
    if (k < n) {
        const float u = pt[((int64_t)f * ORB_KP + k) * 2], v = pt[((int64_t)f * ORB_KP + k) * 2 + 1];
        double d = 0.0;
        if (depth_at(depth + (int64_t)f * H * W, H, W, u, v, d) && isfinite(d)) {
            a[0] = ((double)u - cx) * d / fx;            // pixel_to_3d (slam_utils.py), fp64
            a[1] = ((double)v - cy) * d / fy;
            b[0] = d;
            b[1] = 1.0;
        }
    }
    f64x2* o = reinterpret_cast<f64x2*>(xyz + ((int64_t)f * ORB_KP + k) * 4);
    o[0] = a;
    o[1] = b;
}

// ---- bs_orb_match_pairs -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(ORB_THREADS) match_pairs_kernel(const uint32_t* __restrict__ desc, const int* __restrict__ counts, int n_frames,
                                                                  const int* __restrict__ pairs, int* __restrict__ matches, int* __restrict__ mcount) {
    const int p = blockIdx.x;
    const int fq = pairs[2 * p], ft = pairs[2 * p + 1];
    if (fq < 0 || fq >= n_frames || ft < 0 || ft >= n_frames) {           // (uniform per block) a pair that leaves the arrays: nothing is read
        if (threadIdx.x == 0) mcount[p] = 0;
        return;
    }
    orb_match_pair(desc, counts, fq, ft, matches + (int64_t)p * ORB_KP * 4, mcount + p);
}

// ---- bs_loop_register -------------------------------------------------------------------------------------------------------------------
// loop_draw, loop_sample, residual2, sample_fit3: ransac3.h, shared with global_registration.hip (the same draw, the same fit, moved there as
// they stood).
// Kabsch (rigid3.h) over the three-point sample of hypothesis h, from the correspondences in LDS.  false: the second singular value of the
// sample's cross-covariance is below LC_RANK_EPS (collinear or coincident points); g is then left alone.
__device__ __forceinline__ bool lc_sample_fit(uint64_t seed, uint32_t pair, uint32_t h, int C, const f64x2* s_xy, const f64x2* s_zm, const f64x2* d_xy,
                                              const f64x2* d_zw, Rigid3& g) {
    int id[3];
    loop_sample(seed, pair, h, C, id);
    double pp[3][3], qq[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const f64x2 a0 = s_xy[id[k]], a1 = s_zm[id[k]], b0 = d_xy[id[k]], b1 = d_zw[id[k]];
        pp[k][0] = a0[0]; pp[k][1] = a0[1]; pp[k][2] = a1[0];
        qq[k][0] = b0[0]; qq[k][1] = b0[1]; qq[k][2] = b1[0];
    }
    return sample_fit3(pp, qq, g);
}

// rec [P, BS_LOOP_FIELDS] fp64: 0-15 T (row-major 4 x 4, X_train = T X_query), 16 inliers, 17 C, 18 the winning h (-1: rejected), 19 RMSE over
// the inliers, 20 status (1 accepted by the kernel, 0 rejected), 21 matches, 22-57 the information matrix (row-major 6 x 6), 58-63 zero.
// mask [P, ORB_KP] int32 by match row.
__global__ void __launch_bounds__(LC_THREADS) register_kernel(const double* __restrict__ xyz, int n_frames, const int* __restrict__ pairs,
                                                              const int* __restrict__ matches, const int* __restrict__ mcount, int max_hamming, double tau,
                                                              int n_hyp, int n_refit, int min_matches, uint64_t seed, double* __restrict__ rec,
                                                              int* __restrict__ mask) {
    __shared__ f64x2 s_xy[ORB_KP], s_zm[ORB_KP], d_xy[ORB_KP], d_zw[ORB_KP];
    __shared__ int flag[ORB_KP];
    __shared__ int red_s[LC_THREADS], red_h[LC_THREADS];
    __shared__ double red[LC_WAVES * 21];
    __shared__ int scan[LC_WAVES];
    __shared__ Rigid3 fit;
    __shared__ int fit_ok;
    const int t = threadIdx.x, p = blockIdx.x;
    double* o = rec + (int64_t)p * BS_LOOP_FIELDS;
    int* mk = mask + (int64_t)p * ORB_KP;
    for (int i = t; i < ORB_KP; i += LC_THREADS) mk[i] = 0;
    const int fq = pairs[2 * p], ft = pairs[2 * p + 1];
    const bool in_range = fq >= 0 && fq < n_frames && ft >= 0 && ft < n_frames;
    const int M = in_range ? max(min(mcount[p], ORB_KP), 0) : 0;

    // 1: the correspondences, in match order
    const f64x2* xq = reinterpret_cast<const f64x2*>(xyz + (int64_t)(in_range ? fq : 0) * ORB_KP * 4);
    const f64x2* xt = reinterpret_cast<const f64x2*>(xyz + (int64_t)(in_range ? ft : 0) * ORB_KP * 4);
    const int* mt = matches + (int64_t)p * ORB_KP * 4;
    int C = 0;
    for (int base = 0; base < M; base += LC_THREADS) {
        const int m = base + t;
        int keep = 0;
        f64x2 a0 = {0.0, 0.0}, a1 = a0, b0 = a0, b1 = a0;
        if (m < M) {
            const int q = mt[m * 4], tr = mt[m * 4 + 1], dist = mt[m * 4 + 2];
            if (dist <= max_hamming && q >= 0 && q < ORB_KP && tr >= 0 && tr < ORB_KP) {
                a0 = xq[2 * q]; a1 = xq[2 * q + 1];
                b0 = xt[2 * tr]; b1 = xt[2 * tr + 1];
                keep = (a1[1] == 1.0 && b1[1] == 1.0) ? 1 : 0;
            }
        }
        int tot;
        const int pos = C + block_excl_scan(keep, scan, tot);
        if (keep) {
            a1[1] = (double)m;
            b1[1] = 0.0;
            s_xy[pos] = a0; s_zm[pos] = a1;
            d_xy[pos] = b0; d_zw[pos] = b1;
        }
        C += tot;
    }
    __syncthreads();

    int status = 1, best_h = -1, n_in = 0;
    double rmse = 0.0;
    double info[21];
#pragma unroll
    for (int k = 0; k < 21; ++k) info[k] = 0.0;
    const double tau2 = tau * tau;
    if (C < max(3, min_matches)) status = 0;                             // (uniform per block, as every branch on status below)

    if (status) {
        // 2: the hypotheses; a thread keeps its best (the lowest h among equal scores: h ascends)
        int my_s = 0, my_h = -1;
        for (int h = t; h < n_hyp; h += LC_THREADS) {
            Rigid3 g;
            int score = 0;
            if (lc_sample_fit(seed, (uint32_t)p, (uint32_t)h, C, s_xy, s_zm, d_xy, d_zw, g)) {
                for (int j = 0; j < C; ++j) {
                    const f64x2 a0 = s_xy[j], a1 = s_zm[j], b0 = d_xy[j], b1 = d_zw[j];
                    score += residual2(g, a0[0], a0[1], a1[0], b0[0], b0[1], b1[0]) < tau2;
                }
            }
            if (score > my_s) { my_s = score; my_h = h; }
        }
        red_s[t] = my_s;
        red_h[t] = my_h;
        __syncthreads();
        // 3: the winner
        if (t == 0) {
            int bs_ = 0, bh = -1;
            for (int i = 0; i < LC_THREADS; ++i) {
                if (red_s[i] > bs_ || (red_s[i] == bs_ && bs_ > 0 && red_h[i] < bh)) { bs_ = red_s[i]; bh = red_h[i]; }
            }
            fit_ok = 0;
            Rigid3 g;
            if (bs_ >= 3 && lc_sample_fit(seed, (uint32_t)p, (uint32_t)bh, C, s_xy, s_zm, d_xy, d_zw, g)) {
                fit = g;
                fit_ok = 1;
            }
            red_h[0] = bh;
        }
        __syncthreads();
        best_h = red_h[0];
        if (!fit_ok) status = 0;
    }

    // 4: the inliers of the winner, then n_refit rounds of (Kabsch over the inliers, recount)
    for (int round = 0; status && round <= n_refit; ++round) {
        const Rigid3 g = fit;
        double cnt[1] = {0.0};
        for (int j = t; j < C; j += LC_THREADS) {
            const f64x2 a0 = s_xy[j], a1 = s_zm[j], b0 = d_xy[j], b1 = d_zw[j];
            const int in = residual2(g, a0[0], a0[1], a1[0], b0[0], b0[1], b1[0]) < tau2;
            flag[j] = in;
            cnt[0] += (double)in;
        }
        block_sum<1, LC_WAVES>(cnt, red);
        n_in = (int)cnt[0];
        if (n_in < 3) { status = 0; break; }
        if (round == n_refit) break;
        double s[15];
#pragma unroll
        for (int k = 0; k < 15; ++k) s[k] = 0.0;
        for (int j = t; j < C; j += LC_THREADS) {
            if (flag[j]) {
                const f64x2 a0 = s_xy[j], a1 = s_zm[j], b0 = d_xy[j], b1 = d_zw[j];
                const double pp[3] = {a0[0], a0[1], a1[0]}, qq[3] = {b0[0], b0[1], b1[0]};
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    s[i] += pp[i];
                    s[3 + i] += qq[i];
#pragma unroll
                    for (int k = 0; k < 3; ++k) s[6 + 3 * i + k] += qq[i] * pp[k];
                }
            }
        }
        block_sum<15, LC_WAVES>(s, red);
        if (t == 0) {
            const KabschFit f = kabsch_from_sums(s, (double)n_in);
            fit_ok = !(fmin(f.da, f.db) >= LC_RANK_EPS) ? 0 : 1;
            if (fit_ok) fit = f.g;
        }
        __syncthreads();
        if (!fit_ok) status = 0;
    }

    // 5: RMSE and the information matrix over the inliers (the upper triangle, row by row); the mask by match row
    if (status) {
        const Rigid3 g = fit;
        double s[22];
#pragma unroll
        for (int k = 0; k < 22; ++k) s[k] = 0.0;
        for (int j = t; j < C; j += LC_THREADS) {
            if (flag[j]) {
                const f64x2 a0 = s_xy[j], a1 = s_zm[j], b0 = d_xy[j], b1 = d_zw[j];
                mk[(int)a1[1]] = 1;
                s[21] += residual2(g, a0[0], a0[1], a1[0], b0[0], b0[1], b1[0]);
                const double x = b0[0], y = b0[1], z = b1[0];
                // G = [0 z -y 1 0 0; -z 0 x 0 1 0; y -x 0 0 0 1]
                s[0] += z * z + y * y;   // [0][0]
                s[1] += -(x * y);        // [0][1]
                s[2] += -(x * z);        // [0][2]
                s[4] += -z;              // [0][4]
                s[5] += y;               // [0][5]
                s[6] += z * z + x * x;   // [1][1]
                s[7] += -(y * z);        // [1][2]
                s[8] += z;               // [1][3]
                s[10] += -x;             // [1][5]
                s[11] += y * y + x * x;  // [2][2]
                s[12] += -y;             // [2][3]
                s[13] += x;              // [2][4]
                s[15] += 1.0;            // [3][3] = [4][4] = [5][5]
            }
        }
        double s21[21];
#pragma unroll
        for (int k = 0; k < 21; ++k) s21[k] = s[k];
        block_sum<21, LC_WAVES>(s21, red);
        double r1[1] = {s[21]};
        block_sum<1, LC_WAVES>(r1, red);
        rmse = sqrt(r1[0] / (double)n_in);
#pragma unroll
        for (int k = 0; k < 21; ++k) info[k] = s21[k];
        info[18] = info[15];
        info[20] = info[15];
    }

    if (t == 0) {
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) o[i * 4 + j] = status ? (i < 3 ? (j < 3 ? fit.r[i * 3 + j] : fit.t[i]) : (j == 3 ? 1.0 : 0.0)) : (i == j ? 1.0 : 0.0);
        o[16] = status ? (double)n_in : 0.0;
        o[17] = (double)C;
        o[18] = status ? (double)best_h : -1.0;
        o[19] = rmse;
        o[20] = (double)status;
        o[21] = (double)M;
        int k = 0;
        for (int i = 0; i < 6; ++i)
            for (int j = i; j < 6; ++j, ++k) {
                o[22 + i * 6 + j] = info[k];
                o[22 + j * 6 + i] = info[k];
            }
        for (int i = 58; i < BS_LOOP_FIELDS; ++i) o[i] = 0.0;
    }
}

}  // namespace
}  // namespace bs

#define LC_ENTRY(name)                                                                    \
    using namespace bs;                                                                   \
    if (!initialized()) { set_error(name ": call bs_init first"); return BS_ERR_NOT_INIT; } \
    hipStream_t st = reinterpret_cast<hipStream_t>(stream)

extern "C" int bs_orb_lift(const float* pt, const int32_t* counts, const float* depth, int32_t batch, int32_t H, int32_t W, const double* K, double* xyz,
                           void* stream) {
    LC_ENTRY("bs_orb_lift");
    BS_REQUIRE(pt && counts && depth && K && xyz, "bs_orb_lift: null pointer");
    BS_REQUIRE(batch >= 1 && batch <= 65535, "bs_orb_lift: batch %d (1 .. 65535)", batch);
    BS_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= 2147483647LL, "bs_orb_lift: depth maps of %d x %d", W, H);
    BS_REQUIRE(((uintptr_t)xyz & 15) == 0, "bs_orb_lift: xyz must be 16-byte aligned");
    BS_REQUIRE(K[0] != 0.0 && K[1] != 0.0, "bs_orb_lift: focal lengths %g, %g", K[0], K[1]);
    hipLaunchKernelGGL(lift_kernel, dim3((unsigned)((ORB_KP + LC_THREADS - 1) / LC_THREADS), (unsigned)batch), dim3(LC_THREADS), 0, st, pt, counts, depth, H, W,
                       K[0], K[1], K[2], K[3], xyz);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_orb_match_pairs(const uint32_t* desc, const int32_t* counts, int32_t n_frames, const int32_t* pairs, int32_t P, int32_t* matches,
                                  int32_t* match_counts, void* stream) {
    LC_ENTRY("bs_orb_match_pairs");
    BS_REQUIRE(desc && counts && pairs && matches && match_counts, "bs_orb_match_pairs: null pointer");
    BS_REQUIRE(n_frames >= 1, "bs_orb_match_pairs: %d frames (>= 1)", n_frames);
    BS_REQUIRE(P >= 1, "bs_orb_match_pairs: P = %d pairs (>= 1)", P);
    BS_REQUIRE(((uintptr_t)desc & 15) == 0, "bs_orb_match_pairs: descriptors must be 16-byte aligned");
    hipLaunchKernelGGL(match_pairs_kernel, dim3((unsigned)P), dim3(ORB_THREADS), 0, st, desc, counts, n_frames, pairs, matches, match_counts);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_loop_register(const double* xyz, int32_t n_frames, const int32_t* pairs, int32_t P, const int32_t* matches, const int32_t* match_counts,
                                int32_t max_hamming, double tau, int32_t n_hyp, int32_t n_refit, int32_t min_matches, uint64_t seed, double* records,
                                int32_t* mask, void* stream) {
    LC_ENTRY("bs_loop_register");
    BS_REQUIRE(xyz && pairs && matches && match_counts && records && mask, "bs_loop_register: null pointer");
    BS_REQUIRE(n_frames >= 1, "bs_loop_register: %d frames (>= 1)", n_frames);
    BS_REQUIRE(P >= 1, "bs_loop_register: P = %d pairs (>= 1)", P);
    BS_REQUIRE(tau > 0.0 && isfinite(tau), "bs_loop_register: tau %g (a positive distance)", tau);
    BS_REQUIRE(n_hyp >= 1 && n_hyp <= (1 << 20), "bs_loop_register: %d hypotheses (1 .. 2^20)", n_hyp);
    BS_REQUIRE(n_refit >= 0 && n_refit <= 64, "bs_loop_register: %d refit rounds (0 .. 64)", n_refit);
    BS_REQUIRE(min_matches >= 0 && max_hamming >= 0, "bs_loop_register: min_matches %d, max_hamming %d (>= 0)", min_matches, max_hamming);
    BS_REQUIRE(((uintptr_t)xyz & 15) == 0 && ((uintptr_t)records & 7) == 0, "bs_loop_register: xyz must be 16-byte, records 8-byte aligned");
    hipLaunchKernelGGL(register_kernel, dim3((unsigned)P), dim3(LC_THREADS), 0, st, xyz, n_frames, pairs, matches, match_counts, max_hamming, tau, n_hyp, n_refit,
                       min_matches, seed, records, mask);
    BS_CHECK_LAUNCH();
    return BS_OK;
}
