// Global registration (bs_fpfh_spfh, bs_fpfh_features, bs_feature_match, bs_gr_hypotheses / _score / _winner / _winner_fit / _refit_step /
// _refit_finish; include/bodyslam_hip.h): a pose between two clouds that share no frame, the step before ICP -- the roles of Open3D's
// compute_fpfh_feature and registration_ransac_based_on_feature_matching / _on_correspondence.  The reference only calls Open3D; nothing here
// is its code.  Restated from publications and Open3D's documented meaning, parity with Open3D UNPINNED:
//   FPFH        Rusu, Blodow & Beetz 2009 (the Darboux-frame pair features, the simplified histogram, the 1 / distance^2 weighting)
//   RANSAC      Fischler & Bolles 1981; three correspondences per sample, the edge-length and distance checkers of Open3D's documentation
//   rigid fit   Kabsch 1976 / Arun, Huang & Blostein 1987 (rigid3.h)
// The statement, with every choice that makes a result reproducible, is tests/_global_registration_ref.py; DESIGN section 3.23 the argument.
//
//   bs_fpfh_spfh      one wave per row of the CSR lists of bs_pc_radius_* (a cloud queried on itself), the lanes striding the row.  A neighbour is
//                     two 16-byte records (x, y, z, .) (nx, ny, nz, .) of a packed table.  The pair features are fp64 (fpfh_pair below, plain
//                     C++); the 33 counts come from wave ballots and population counts: integers, so the order of the row does not matter.
//                     Out: int32 [n, 36] = 33 counts, k, 0, 0 -- nine 16-byte words.
//   bs_fpfh_features  one wave per row over the SORTED lists: lane l adds the terms spfh(j) / d2 of entries l, l + 64, ... in order, then
//                     reduce.h's xor butterfly; block scaling, + spfh(i), one rounding to fp32.
//   bs_feature_match  a thread holds one source row (33 floats) in registers; the target rows pass through LDS in tiles of rows padded to 36
//                     floats and are read as 16-byte words that every lane shares (a broadcast).  Grid = source blocks x target splits; the
//                     splits merge by a 64-bit atomicMin of (distance bits << 32 | index): exact, independent of the order.
//   bs_gr_*           A  one thread per hypothesis: the draw (ransac3.h, loop closure's), the edge-length checker, the fit, the distance checker
//                     B  over the valid hypotheses only: a thread holds one transform, the correspondences pass through LDS as 16-byte words,
//                        integer partial counts merge by integer atomicAdd
//                     C  the winner by a 64-bit atomicMax of (score << 32 | ~h): the highest score, the lowest h
//                     D  refit rounds: block partials in fp64 (reduce.h block_sum), then column_sum in one wave, as icp.hip adds
// The correspondences live in global memory ([c, 6] fp64): their number is bounded by int32 only, unlike loop_closure.hip's 500 in LDS.
// No floating-point atomics; every LDS read is 16 bytes per lane; every index read from memory is checked before it
// addresses anything.  Time: tools/global_registration_time.py, profiles/global_registration_time.txt, DESIGN section 3.23.
#include <math.h>

#include "common.h"
#include "ransac3.h"
#include "reduce.h"
#include "rigid3.h"

namespace bs {
namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long gr_key;

constexpr int GR_THREADS = 256;
constexpr int GR_WAVE = 64;
constexpr int GR_WAVES = GR_THREADS / GR_WAVE;
constexpr int FPFH_BINS = 11;
constexpr int FPFH_DIM = 3 * FPFH_BINS;
constexpr int FPFH_ROW = 36;                 // a stored row: 33 values + 3, nine 16-byte words
constexpr int FPFH_WORDS = FPFH_ROW / 4;
constexpr int MT_TILE = 64;                  // target rows per LDS tile of the match: 64 x 36 x 4 B = 9 216 B
constexpr int GR_TILE = 256;                 // correspondences per LDS tile of the score: 256 x 48 B = 12 288 B
constexpr int GR_SUMS = 17;                  // count, Kabsch's 15 sums, sum of squared residuals

// ---- the pair features: plain C++ ------------------------------------------------------------------------------------------------------------
__host__ __device__ inline bool fpfh_normal_ok(const double (&n)[3]) {
    return isfinite(n[0]) && isfinite(n[1]) && isfinite(n[2]) && (n[0] != 0.0 || n[1] != 0.0 || n[2] != 0.0);
}
// floor(11 (f + 1) / 2) clipped to 0 .. 10
__host__ __device__ inline int fpfh_bin11(double f) {
    const double v = floor((11.0 * (f + 1.0)) / 2.0);
    return v < 0.0 ? 0 : (v > 10.0 ? 10 : (int)v);
}
// the bin of atan2(y, x) among eleven equal sectors of [-pi, pi], without a transcendental function: the ten inner edges are the directions
// +-(2 j + 1) pi / 11; a direction on an edge belongs to the sector above it (half-open); y >= 0 is the upper half plane
__host__ __device__ inline int fpfh_sector(double x, double y) {
    const double C[5] = {0.9594929736144975, 0.6548607339452851, 0.14231483827328512, -0.4154150130018863, -0.8412535328311811};
    const double S[5] = {0.2817325568414295, 0.7557495743542583, 0.9898214418809327, 0.9096319953545184, 0.5406408174555978};
    int n = 0;
    if (y >= 0.0) {
        n = 5;
        for (int j = 0; j < 5; ++j) n += (C[j] * y - S[j] * x >= 0.0) ? 1 : 0;
    } else {
        for (int j = 0; j < 5; ++j) n += (C[j] * y + S[j] * x >= 0.0) ? 1 : 0;
    }
    return n;
}
// the three bins (f1, f2, f3) of the pair (p1, n1), (p2, n2); false: the pair is skipped and not counted
__host__ __device__ inline bool fpfh_pair(const double (&p1)[3], const double (&n1_)[3], const double (&p2)[3], const double (&n2_)[3], int (&bin)[3]) {
    if (!fpfh_normal_ok(n1_) || !fpfh_normal_ok(n2_)) return false;
    double dp[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    const double d = sqrt((dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2]);
    if (!(d > 0.0) || !isfinite(d)) return false;
    const double a1 = ((n1_[0] * dp[0] + n1_[1] * dp[1]) + n1_[2] * dp[2]) / d;
    const double a2 = ((n2_[0] * dp[0] + n2_[1] * dp[1]) + n2_[2] * dp[2]) / d;
    const bool swap = fabs(a1) < fabs(a2);
    double n1[3], n2[3];
    for (int i = 0; i < 3; ++i) {
        n1[i] = swap ? n2_[i] : n1_[i];
        n2[i] = swap ? n1_[i] : n2_[i];
        dp[i] = swap ? -dp[i] : dp[i];
    }
    const double f3 = swap ? -a2 : a1;
    double v[3] = {dp[1] * n1[2] - dp[2] * n1[1], dp[2] * n1[0] - dp[0] * n1[2], dp[0] * n1[1] - dp[1] * n1[0]};
    const double vn = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    if (!(vn > 0.0) || !isfinite(vn)) return false;
    for (int i = 0; i < 3; ++i) v[i] = v[i] / vn;
    const double w[3] = {n1[1] * v[2] - n1[2] * v[1], n1[2] * v[0] - n1[0] * v[2], n1[0] * v[1] - n1[1] * v[0]};
    const double f2 = (v[0] * n2[0] + v[1] * n2[1]) + v[2] * n2[2];
    const double y = (w[0] * n2[0] + w[1] * n2[1]) + w[2] * n2[2];
    const double x = (n1[0] * n2[0] + n1[1] * n2[1]) + n1[2] * n2[2];
    bin[0] = fpfh_sector(x, y);
    bin[1] = fpfh_bin11(f2);
    bin[2] = fpfh_bin11(f3);
    return true;
}

// ---- bs_fpfh_spfh --------------------------------------------------------------------------------------------------------------------------
// row r of the lists belongs to point first + r.  One wave per row; no lane leaves before the ballots: the row's bounds are wave-uniform.
__global__ void __launch_bounds__(GR_THREADS) spfh_kernel(const f32x4* __restrict__ table, int64_t n, const int64_t* __restrict__ row_start,
                                                          const int32_t* __restrict__ index, const float* __restrict__ d2, int64_t m, int64_t first,
                                                          int64_t total, int32_t* __restrict__ spfh) {
    const int lane = threadIdx.x & (GR_WAVE - 1);
    const int64_t row = (int64_t)blockIdx.x * GR_WAVES + (threadIdx.x / GR_WAVE);
    if (row >= m) return;                                                               // (a whole wave)
    const int64_t i = first + row;
    int64_t b = row_start[row], e = row_start[row + 1];
    if (b < 0 || e < b || e > total) { b = 0; e = 0; }
    const f32x4 P = table[2 * i], N = table[2 * i + 1];
    const double p1[3] = {(double)P[0], (double)P[1], (double)P[2]}, n1[3] = {(double)N[0], (double)N[1], (double)N[2]};
    const bool ok1 = isfinite(p1[0]) && isfinite(p1[1]) && isfinite(p1[2]);
    int mine = 0, k = 0;
    for (int64_t base = b; base < e; base += GR_WAVE) {
        const int64_t j = base + lane;
        int bin[3] = {-1, -1, -1};
        bool counted = false;
        if (j < e && ok1) {
            const int32_t t = index[j];
            if (t >= 0 && t < n && d2[j] != 0.0f) {
                const f32x4 Q = table[2 * (int64_t)t], M = table[2 * (int64_t)t + 1];
                const double p2[3] = {(double)Q[0], (double)Q[1], (double)Q[2]}, n2[3] = {(double)M[0], (double)M[1], (double)M[2]};
                counted = fpfh_pair(p1, n1, p2, n2, bin);
            }
        }
        if (!counted) bin[0] = bin[1] = bin[2] = -1;
#pragma unroll
        for (int f = 0; f < 3; ++f) {
#pragma unroll
            for (int q = 0; q < FPFH_BINS; ++q) {
                const int c = __popcll(__ballot(bin[f] == q));
                if (lane == f * FPFH_BINS + q) mine += c;
            }
        }
        k += __popcll(__ballot(counted));
    }
    if (lane < FPFH_ROW) spfh[i * FPFH_ROW + lane] = lane < FPFH_DIM ? mine : (lane == FPFH_DIM ? k : 0);
}

// ---- bs_fpfh_features ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(GR_THREADS) fpfh_kernel(const i32x4* __restrict__ spfh, int64_t n, const int64_t* __restrict__ row_start,
                                                          const int32_t* __restrict__ index, const float* __restrict__ d2, int64_t m, int64_t first,
                                                          int64_t total, float* __restrict__ out) {
    const int lane = threadIdx.x & (GR_WAVE - 1);
    const int64_t row = (int64_t)blockIdx.x * GR_WAVES + (threadIdx.x / GR_WAVE);
    if (row >= m) return;                                                               // (a whole wave)
    const int64_t i = first + row;
    int64_t b = row_start[row], e = row_start[row + 1];
    if (b < 0 || e < b || e > total) { b = 0; e = 0; }
    double acc[FPFH_DIM];
#pragma unroll
    for (int q = 0; q < FPFH_DIM; ++q) acc[q] = 0.0;
    for (int64_t j = b + lane; j < e; j += GR_WAVE) {
        const int32_t t = index[j];
        const float dd = d2[j];
        if (t < 0 || t >= n || dd == 0.0f) continue;
        i32x4 w[FPFH_WORDS];
#pragma unroll
        for (int q = 0; q < FPFH_WORDS; ++q) w[q] = spfh[(int64_t)t * FPFH_WORDS + q];
        const int kk = w[FPFH_DIM / 4][FPFH_DIM % 4];
        if (kk <= 0) continue;
        const double kd = (double)kk, wd = (double)dd;
#pragma unroll
        for (int q = 0; q < FPFH_DIM; ++q) acc[q] += ((100.0 * (double)w[q / 4][q % 4]) / kd) / wd;
    }
#pragma unroll
    for (int q = 0; q < FPFH_DIM; ++q) acc[q] = wave_sum(acc[q]);
    i32x4 own[FPFH_WORDS];
#pragma unroll
    for (int q = 0; q < FPFH_WORDS; ++q) own[q] = spfh[i * FPFH_WORDS + q];
    const int ki = own[FPFH_DIM / 4][FPFH_DIM % 4];
    float mine = 0.0f;
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        const double* a = acc + f * FPFH_BINS;                                          // the symmetric order: mirror_fpfh commutes with it bit for bit
        const double s = (((((a[0] + a[10]) + (a[1] + a[9])) + (a[2] + a[8])) + (a[3] + a[7])) + (a[4] + a[6])) + a[5];
#pragma unroll
        for (int q = 0; q < FPFH_BINS; ++q) {
            const int c = f * FPFH_BINS + q;
            double v = acc[c];
            if (s > 0.0) v = (v * 100.0) / s;
            if (ki > 0) v = v + (100.0 * (double)own[c / 4][c % 4]) / (double)ki;
            if (lane == c) mine = ki > 0 ? (float)v : 0.0f;
        }
    }
    if (lane < FPFH_DIM) out[i * FPFH_DIM + lane] = mine;
}

// ---- bs_feature_match ----------------------------------------------------------------------------------------------------------------------
// best [m]: the caller fills it with ~0; afterwards the minimum of (distance bits << 32 | target index) over the finite target rows, for every
// finite source row
__global__ void __launch_bounds__(GR_THREADS) match_kernel(const float* __restrict__ src, int64_t m, const float* __restrict__ tgt, int64_t n,
                                                           int64_t rows_per_split, gr_key* __restrict__ best) {
    __shared__ f32x4 tile[MT_TILE * FPFH_WORDS];
    float* tile_f = reinterpret_cast<float*>(tile);
    const int t = threadIdx.x;
    const int64_t s = (int64_t)blockIdx.x * GR_THREADS + t;
    const int64_t t0 = (int64_t)blockIdx.y * rows_per_split, t1 = t0 + rows_per_split < n ? t0 + rows_per_split : n;
    float a[FPFH_DIM];
    bool ok = s < m;
#pragma unroll
    for (int q = 0; q < FPFH_DIM; ++q) {
        a[q] = s < m ? src[s * FPFH_DIM + q] : 0.0f;
        ok = ok && isfinite(a[q]);
    }
    gr_key mine = ~0ull;
    for (int64_t base = t0; base < t1; base += MT_TILE) {
        const int rows = t1 - base < MT_TILE ? (int)(t1 - base) : MT_TILE;
        __syncthreads();
        for (int e = t; e < MT_TILE * FPFH_ROW; e += GR_THREADS) {
            const int r = e / FPFH_ROW, c = e % FPFH_ROW;
            tile_f[e] = (r < rows && c < FPFH_DIM) ? tgt[(base + r) * FPFH_DIM + c] : 0.0f;
        }
        __syncthreads();
        if (t < MT_TILE) {                                                              // word 8, entry 1: 1.0 = every value of the row is finite
            bool fin = t < rows;
            f32x4 w8 = tile[t * FPFH_WORDS + FPFH_WORDS - 1];
#pragma unroll
            for (int q = 0; q < FPFH_WORDS - 1; ++q) {
                const f32x4 w = tile[t * FPFH_WORDS + q];
                fin = fin && isfinite(w[0]) && isfinite(w[1]) && isfinite(w[2]) && isfinite(w[3]);
            }
            fin = fin && isfinite(w8[0]);
            w8[1] = fin ? 1.0f : 0.0f;
            tile[t * FPFH_WORDS + FPFH_WORDS - 1] = w8;
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            f32x4 w[FPFH_WORDS];
#pragma unroll
            for (int q = 0; q < FPFH_WORDS; ++q) w[q] = tile[r * FPFH_WORDS + q];
            if (w[FPFH_WORDS - 1][1] != 1.0f) continue;                                 // (uniform: every lane reads the same row)
            float acc = 0.0f;
#pragma unroll
            for (int q = 0; q < FPFH_DIM; ++q) {
                const float d = a[q] - w[q / 4][q % 4];
                acc = acc + d * d;
            }
            const gr_key key = ((gr_key)__float_as_uint(acc) << 32) | (gr_key)(uint32_t)(base + r);
            mine = key < mine ? key : mine;
        }
    }
    if (ok && mine != ~0ull) atomicMin(best + s, mine);
}

// ---- RANSAC over correspondences in global memory ----------------------------------------------------------------------------------------------
// corr [c, 6] fp64 = (px, py, pz, qx, qy, qz), read as three 16-byte words per row
__device__ __forceinline__ void gr_load(const f64x2* __restrict__ corr, int64_t j, double (&p)[3], double (&q)[3]) {
    const f64x2 a = corr[3 * j], b = corr[3 * j + 1], c = corr[3 * j + 2];
    p[0] = a[0]; p[1] = a[1]; p[2] = b[0];
    q[0] = b[1]; q[1] = c[0]; q[2] = c[1];
}
__device__ __forceinline__ double gr_length(const double (&a)[3], const double (&b)[3]) {
    const double x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
    return sqrt((x * x + y * y) + z * z);
}
// the edge-length checker: every pair of the sample has |ps| >= s |pt| and |pt| >= s |ps|.  Plain arithmetic, before any fit.
__device__ __forceinline__ bool gr_edges_ok(const double (&p)[3][3], const double (&q)[3][3], double s_edge) {
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int b = a + 1; b < 3; ++b) {
            const double ls = gr_length(p[a], p[b]), lt = gr_length(q[a], q[b]);
            ok = ok && ls >= s_edge * lt && lt >= s_edge * ls;
        }
    }
    return ok;
}
// the whole of stage A for hypothesis h: draw, edge checker, fit with its rank test, distance checker
__device__ __forceinline__ bool gr_hypothesis(const f64x2* __restrict__ corr, int c, uint64_t seed, uint32_t h, double s_edge, double tau2, Rigid3& g) {
    int id[3];
    loop_sample(seed, 0u, h, c, id);
    double p[3][3], q[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) gr_load(corr, id[k], p[k], q[k]);
    if (!gr_edges_ok(p, q, s_edge)) return false;
    if (!sample_fit3(p, q, g)) return false;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) ok = ok && residual2(g, p[k][0], p[k][1], p[k][2], q[k][0], q[k][1], q[k][2]) < tau2;
    return ok;
}

__global__ void __launch_bounds__(GR_THREADS) gr_hypotheses_kernel(const f64x2* __restrict__ corr, int c, uint64_t seed, uint32_t h0, int count,
                                                                   double s_edge, double tau2, double* __restrict__ fits, int32_t* __restrict__ valid) {
    const int t = blockIdx.x * GR_THREADS + threadIdx.x;
    if (t >= count) return;
    Rigid3 g = rigid3_identity();
    const bool ok = gr_hypothesis(corr, c, seed, h0 + (uint32_t)t, s_edge, tau2, g);
    double* o = fits + (int64_t)t * 12;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) o[i * 4 + j] = g.r[i * 3 + j];
        o[i * 4 + 3] = g.t[i];
    }
    valid[t] = ok ? 1 : 0;
}

// grid (blocks of valid hypotheses, splits of the correspondences); score [count] zeroed by the caller
__global__ void __launch_bounds__(GR_THREADS) gr_score_kernel(const f64x2* __restrict__ corr, int c, const double* __restrict__ fits,
                                                              const int32_t* __restrict__ list, int n_valid, int count, int rows_per_split,
                                                              double tau2, int32_t* __restrict__ score) {
    __shared__ f64x2 tile[GR_TILE * 3];
    const int t = threadIdx.x;
    const int v = blockIdx.x * GR_THREADS + t;
    int hyp = v < n_valid ? list[v] : -1;
    if (hyp < 0 || hyp >= count) hyp = -1;
    Rigid3 g = rigid3_identity();
    if (hyp >= 0) g = rigid3_load(fits + (int64_t)hyp * 12);
    const int64_t lo64 = (int64_t)blockIdx.y * rows_per_split;
    const int c0 = lo64 < c ? (int)lo64 : c, c1 = lo64 + rows_per_split < c ? (int)(lo64 + rows_per_split) : c;
    int n = 0;
    for (int base = c0; base < c1; base += GR_TILE) {
        const int rows = min(GR_TILE, c1 - base);
        __syncthreads();
        for (int e = t; e < rows * 3; e += GR_THREADS) tile[e] = corr[(int64_t)base * 3 + e];
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            const f64x2 a = tile[3 * r], b = tile[3 * r + 1], d = tile[3 * r + 2];
            n += residual2(g, a[0], a[1], b[0], b[1], d[0], d[1]) < tau2 ? 1 : 0;
        }
    }
    if (hyp >= 0 && n > 0) atomicAdd(score + hyp, n);
}

// best: (score << 32 | ~h), zeroed by the caller before the first chunk; a score of zero never enters
__global__ void __launch_bounds__(GR_THREADS) gr_winner_kernel(const int32_t* __restrict__ score, int count, uint32_t h0, gr_key* __restrict__ best) {
    const int t = blockIdx.x * GR_THREADS + threadIdx.x;
    if (t >= count) return;
    const int32_t s = score[t];
    if (s > 0) atomicMax(best, ((gr_key)(uint32_t)s << 32) | (gr_key)(uint32_t)(~(h0 + (uint32_t)t)));
}

// state [BS_GR_STATE_FIELDS] fp64: 0-11 the rows of [R | t], 12 status (1 = a fit stands, 0 = degenerate), 13 inliers, 14 RMSE, 15 rounds done
__global__ void gr_winner_fit_kernel(const f64x2* __restrict__ corr, int c, uint64_t seed, uint32_t h, double s_edge, double tau2,
                                     double* __restrict__ state) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    Rigid3 g = rigid3_identity();
    const bool ok = gr_hypothesis(corr, c, seed, h, s_edge, tau2, g);
    rigid3_store(g, state);
    state[12] = ok ? 1.0 : 0.0;
    state[13] = 0.0;
    state[14] = 0.0;
    state[15] = 0.0;
}

__global__ void __launch_bounds__(GR_THREADS) gr_refit_step_kernel(const f64x2* __restrict__ corr, int c, const double* __restrict__ state, double tau2,
                                                                   int32_t* __restrict__ mask, double* __restrict__ partial) {
    __shared__ double red[GR_WAVES * GR_SUMS];
    if (state[12] != 1.0) return;                                                       // (uniform over the grid)
    const Rigid3 g = rigid3_load(state);
    const int j = blockIdx.x * GR_THREADS + threadIdx.x;
    double v[GR_SUMS];
#pragma unroll
    for (int k = 0; k < GR_SUMS; ++k) v[k] = 0.0;
    if (j < c) {
        double p[3], q[3];
        gr_load(corr, j, p, q);
        const double r2 = residual2(g, p[0], p[1], p[2], q[0], q[1], q[2]);
        const bool in = r2 < tau2;
        mask[j] = in ? 1 : 0;
        if (in) {
            double s[15];
#pragma unroll
            for (int k = 0; k < 15; ++k) s[k] = 0.0;
            kabsch_add(s, p, q);
            v[0] = 1.0;
#pragma unroll
            for (int k = 0; k < 15; ++k) v[1 + k] = s[k];
            v[16] = r2;
        }
    }
    block_sum<GR_SUMS, GR_WAVES>(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < GR_SUMS; ++k) partial[(int64_t)blockIdx.x * GR_SUMS + k] = v[k];
    }
}

// one wave: the columns of the partials in column_sum's order; final = 0: Kabsch over the inliers replaces the transform; final = 1: the
// inlier count and the RMSE of the transform as it stands
__global__ void __launch_bounds__(GR_WAVE) gr_refit_finish_kernel(const double* __restrict__ partial, int nblocks, int final, double* __restrict__ state) {
    if (state[12] != 1.0) return;
    const int lane = threadIdx.x;
    double tot[GR_SUMS];
#pragma unroll
    for (int k = 0; k < GR_SUMS; ++k) tot[k] = column_sum(partial, nblocks, GR_SUMS, k, lane);
    if (lane != 0) return;
    const double n_in = tot[0];
    state[15] = state[15] + 1.0;
    if (!(n_in >= 3.0)) { state[12] = 0.0; return; }
    if (final) {
        state[13] = n_in;
        state[14] = sqrt(tot[16] / n_in);
        return;
    }
    double s[15];
#pragma unroll
    for (int k = 0; k < 15; ++k) s[k] = tot[1 + k];
    const KabschFit f = kabsch_from_sums(s, n_in);
    if (!(fmin(f.da, f.db) >= RANSAC3_RANK_EPS)) { state[12] = 0.0; return; }
    rigid3_store(f.g, state);
}

inline bool gr_rows(int64_t n) { return n >= 1 && n < ((int64_t)1 << 31); }

}  // namespace
}  // namespace bs

#define GR_ENTER(name)                                                                 \
    using namespace bs;                                                                \
    if (!initialized()) { set_error(name ": call bs_init first"); return BS_ERR_NOT_INIT; } \
    hipStream_t st = reinterpret_cast<hipStream_t>(stream)

#define GR_LISTS(name)                                                                                                                                   \
    BS_REQUIRE(row_start && index && d2, name ": null pointer");                                                                                         \
    BS_REQUIRE(gr_rows(n) && gr_rows(m) && first >= 0 && first + m <= n, name ": n = %lld, m = %lld, first = %lld (1 <= m, first + m <= n < 2^31)",      \
               (long long)n, (long long)m, (long long)first);                                                                                            \
    BS_REQUIRE(total >= 0 && total < ((int64_t)1 << 31), name ": total = %lld (0 <= total < 2^31)", (long long)total)

extern "C" int bs_fpfh_spfh(const void* table, int64_t n, const int64_t* row_start, const int32_t* index, const float* d2, int64_t m, int64_t first,
                            int64_t total, int32_t* spfh, void* stream) {
    GR_ENTER("bs_fpfh_spfh");
    GR_LISTS("bs_fpfh_spfh");
    BS_REQUIRE(table && spfh, "bs_fpfh_spfh: null pointer");
    BS_REQUIRE((((uintptr_t)table | (uintptr_t)spfh) & 15) == 0, "bs_fpfh_spfh: table and spfh must be 16-byte aligned");
    hipLaunchKernelGGL(spfh_kernel, dim3((unsigned)cdiv64(m, GR_WAVES)), dim3(GR_THREADS), 0, st, static_cast<const f32x4*>(table), n, row_start, index, d2, m,
                       first, total, spfh);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_fpfh_features(const int32_t* spfh, int64_t n, const int64_t* row_start, const int32_t* index, const float* d2, int64_t m, int64_t first,
                                int64_t total, float* features, void* stream) {
    GR_ENTER("bs_fpfh_features");
    GR_LISTS("bs_fpfh_features");
    BS_REQUIRE(spfh && features, "bs_fpfh_features: null pointer");
    BS_REQUIRE(((uintptr_t)spfh & 15) == 0, "bs_fpfh_features: spfh must be 16-byte aligned");
    hipLaunchKernelGGL(fpfh_kernel, dim3((unsigned)cdiv64(m, GR_WAVES)), dim3(GR_THREADS), 0, st, reinterpret_cast<const i32x4*>(spfh), n, row_start, index, d2,
                       m, first, total, features);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_feature_match(const float* source, int64_t m, const float* target, int64_t n, int32_t splits, void* best, void* stream) {
    GR_ENTER("bs_feature_match");
    BS_REQUIRE(source && target && best, "bs_feature_match: null pointer");
    BS_REQUIRE(gr_rows(m) && gr_rows(n), "bs_feature_match: m = %lld, n = %lld (1 <= . < 2^31)", (long long)m, (long long)n);
    BS_REQUIRE(splits >= 1 && splits <= 65535, "bs_feature_match: %d splits (1 .. 65535)", splits);
    BS_REQUIRE(((uintptr_t)best & 7) == 0, "bs_feature_match: best must be 8-byte aligned");
    const int64_t rows_per_split = cdiv64(cdiv64(n, splits), MT_TILE) * MT_TILE;
    hipLaunchKernelGGL(match_kernel, dim3((unsigned)cdiv64(m, GR_THREADS), (unsigned)splits), dim3(GR_THREADS), 0, st, source, m, target, n, rows_per_split,
                       static_cast<gr_key*>(best));
    BS_CHECK_LAUNCH();
    return BS_OK;
}

#define GR_CORR(name)                                                                                                              \
    BS_REQUIRE(corr && c >= 3, name ": null pointer or c = %d correspondences (>= 3)", c);                                         \
    BS_REQUIRE(((uintptr_t)corr & 15) == 0, name ": corr must be 16-byte aligned");                                                \
    BS_REQUIRE(tau > 0.0 && isfinite(tau), name ": tau %g (a positive distance)", tau);                                            \
    const f64x2* cr = reinterpret_cast<const f64x2*>(corr)

extern "C" int bs_gr_hypotheses(const double* corr, int32_t c, uint64_t seed, uint32_t h0, int32_t count, double edge_length_threshold, double tau,
                                double* fits, int32_t* valid, void* stream) {
    GR_ENTER("bs_gr_hypotheses");
    GR_CORR("bs_gr_hypotheses");
    BS_REQUIRE(fits && valid, "bs_gr_hypotheses: null pointer");
    BS_REQUIRE(count >= 1 && count <= (1 << 20) && (uint64_t)h0 + (uint64_t)count <= 0x7fffffffull, "bs_gr_hypotheses: %d hypotheses from %u (1 .. 2^20, h < 2^31)",
               count, h0);
    BS_REQUIRE(edge_length_threshold > 0.0 && edge_length_threshold <= 1.0, "bs_gr_hypotheses: edge_length_threshold %g (0 < . <= 1)", edge_length_threshold);
    hipLaunchKernelGGL(gr_hypotheses_kernel, dim3((unsigned)cdiv64(count, GR_THREADS)), dim3(GR_THREADS), 0, st, cr, c, seed, h0, count, edge_length_threshold,
                       tau * tau, fits, valid);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_gr_score(const double* corr, int32_t c, const double* fits, const int32_t* list, int32_t n_valid, int32_t count, int32_t splits, double tau,
                           int32_t* score, void* stream) {
    GR_ENTER("bs_gr_score");
    GR_CORR("bs_gr_score");
    BS_REQUIRE(fits && list && score, "bs_gr_score: null pointer");
    BS_REQUIRE(count >= 1 && count <= (1 << 20) && n_valid >= 1 && n_valid <= count, "bs_gr_score: %d valid of %d hypotheses (1 <= valid <= count <= 2^20)",
               n_valid, count);
    BS_REQUIRE(splits >= 1 && splits <= 65535, "bs_gr_score: %d splits (1 .. 65535)", splits);
    const int rows_per_split = (int)(cdiv64(cdiv64(c, splits), GR_TILE) * GR_TILE);
    hipLaunchKernelGGL(gr_score_kernel, dim3((unsigned)cdiv64(n_valid, GR_THREADS), (unsigned)splits), dim3(GR_THREADS), 0, st, cr, c, fits, list, n_valid, count,
                       rows_per_split, tau * tau, score);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_gr_winner(const int32_t* score, int32_t count, uint32_t h0, void* best, void* stream) {
    GR_ENTER("bs_gr_winner");
    BS_REQUIRE(score && best && ((uintptr_t)best & 7) == 0, "bs_gr_winner: null pointer, or best is not 8-byte aligned");
    BS_REQUIRE(count >= 1 && count <= (1 << 20) && (uint64_t)h0 + (uint64_t)count <= 0x7fffffffull, "bs_gr_winner: %d hypotheses from %u", count, h0);
    hipLaunchKernelGGL(gr_winner_kernel, dim3((unsigned)cdiv64(count, GR_THREADS)), dim3(GR_THREADS), 0, st, score, count, h0, static_cast<gr_key*>(best));
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_gr_winner_fit(const double* corr, int32_t c, uint64_t seed, uint32_t h, double edge_length_threshold, double tau, double* state,
                                void* stream) {
    GR_ENTER("bs_gr_winner_fit");
    GR_CORR("bs_gr_winner_fit");
    BS_REQUIRE(state && ((uintptr_t)state & 15) == 0, "bs_gr_winner_fit: state must be 16-byte aligned");
    BS_REQUIRE(h <= 0x7fffffffu, "bs_gr_winner_fit: h = %u", h);
    BS_REQUIRE(edge_length_threshold > 0.0 && edge_length_threshold <= 1.0, "bs_gr_winner_fit: edge_length_threshold %g (0 < . <= 1)", edge_length_threshold);
    hipLaunchKernelGGL(gr_winner_fit_kernel, dim3(1), dim3(GR_WAVE), 0, st, cr, c, seed, h, edge_length_threshold, tau * tau, state);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_gr_refit_step(const double* corr, int32_t c, const double* state, double tau, int32_t* mask, double* partial, void* stream) {
    GR_ENTER("bs_gr_refit_step");
    GR_CORR("bs_gr_refit_step");
    BS_REQUIRE(state && mask && partial, "bs_gr_refit_step: null pointer");
    hipLaunchKernelGGL(gr_refit_step_kernel, dim3((unsigned)cdiv64(c, GR_THREADS)), dim3(GR_THREADS), 0, st, cr, c, state, tau * tau, mask, partial);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_gr_refit_finish(const double* partial, int32_t c, int32_t final_round, double* state, void* stream) {
    GR_ENTER("bs_gr_refit_finish");
    BS_REQUIRE(partial && state && c >= 3, "bs_gr_refit_finish: null pointer or c = %d", c);
    hipLaunchKernelGGL(gr_refit_finish_kernel, dim3(1), dim3(GR_WAVE), 0, st, partial, (int)cdiv64(c, GR_THREADS), final_round ? 1 : 0, state);
    BS_CHECK_LAUNCH();
    return BS_OK;
}
