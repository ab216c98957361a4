// Cloud-to-cloud distances for the reconstruction evaluation (bs_pc_*; include/bodyslam_hip.h): the exact nearest neighbour of every point
// of one cloud in another -- Open3D's PointCloud.compute_point_cloud_distance, which the reference calls at
// BodySLAM_not_refactored/3DM/mapping_module.py:45,48,62 -- and the statistics of a distance array.  Restated from Open3D's documented
// meaning; parity with Open3D is UNPINNED.  The statement is tests/_pointcloud_ref.py.
//
// Arithmetic (the whole feature follows from it).  For a source s and a target t, fp32: dx = s.x - t.x, dy, dz alike,
// d2 = (dx * dx + dy * dy) + dz * dz, no contraction; the neighbour is the minimum of (d2, original target index) in lexicographic order;
// the distance is sqrtf(d2), correctly rounded.  A minimum under a total order does not depend on the order of the candidates, so no
// kernel below cares in which order points land in a cell (integer atomics) or cells are visited, and the cell size changes the time only.
//
// Index: a uniform grid over the bounding box [lo, hi] of the finite target points, cell edge h.
//   cell coordinate along an axis   c(x) = (int) min(max(floorf((x - lo) / h), 0), n - 1), fp32, IEEE division: the SAME function for
//                                   targets (build) and sources (query), and monotone in x
//   default h (bodyslam_amd/pointcloud.py default_cell_size): over the k axes of positive extent, h = (product of those extents /
//                                   number of finite points)^(1 / k) -- about as many cells as points --, grown by factors of 1.25 until
//                                   nx ny nz <= 2^24, n_a = (int) floorf((hi_a - lo_a) / h) + 1; no positive extent: one cell
//   bs_pc_bounds        one launch: per axis min and max of the finite points through integer atomics on order-preserving bit patterns,
//                       and their count
//   bs_pc_grid_count    one launch: counts[cell] += 1 (integer atomics).  The exclusive scan of the counts is the caller's (torch.cumsum)
//   bs_pc_grid_scatter  one launch: record (x, y, z, bit-cast original index), 16 bytes, to cell order through a per-cell cursor
// Query (bs_pc_query_grid), one thread per source, one launch: Chebyshev shells r = 0, 1, 2, ... of cells around the source's (clamped)
// cell; every candidate is ONE 16-byte load.
//   The bound.  A target in a cell not visited after shell r differs from the source's cell by >= r + 1 along some axis.  With
//   u(x) = fl(fl(x - lo) / h) and c = clamp(floor(u)), c(t) >= c(s) + r + 1 gives u(t) - u(s) > r in every clamping case (a target is
//   clamped only downwards from n, a source outside the box only towards it), and |u(x) - (x - lo) / h| <= 2^-23 |x - lo| / h, so
//   |t - s| > r h - 2^-23 (|t - lo| + |s - lo|) along that axis.  The kernel takes slack = 2^-21 max_a((hi_a - lo_a) + |s_a - lo_a|)
//   (four times that term) and lb = (r h - slack) * 0.99999 (1e-5 against the 1e-7 of the chain's own rounding): lb is a true lower
//   bound of |dx| for every unvisited target.  fp32 subtraction, multiplication and the addition of non-negative terms are monotone, so
//   the COMPUTED d2 of such a target is >= fl(lb * lb); the search stops once best d2 < lb * lb (strictly: an equal d2 with a lower index
//   cannot hide behind the bound).  A late stop costs time, an early one would be a wrong answer.  It also stops when every cell of
//   the grid has been visited, and, with max_distance, when lb * 0.9999 > max_distance.
//   A source still searching after shell `shell_cap` (isolated points, clouds far apart before alignment) goes onto a device list.
// Brute force (bs_pc_query_brute; the fallback for that list and method = "brute"): a block per 64 sources (lane = source, in each of its
// four waves) and per chunk of targets, the chunk streamed through LDS tiles of 1024 records; wave w reads records w, w + 4, ... of a tile,
// every LDS read is one record, 16 bytes per lane (DESIGN section 7's rule for kernels that may run beside a second stream); the
// block's result goes into a 64-bit key (d2 bits << 32 | index) by an integer atomicMin -- d2 >= 0, so the key order IS the
// lexicographic order.  A second launch turns keys into (distance, index).
//
// Statistics (bs_pc_stats): count, sum, sum of squares, max, up to 8 threshold counts, and the exact median by radix selection on the
// order-preserving bit patterns, 11 + 11 + 10 bits: three passes over the array, each followed by a one-block selection (the last one
// writes the record): six launches and one memset.  fp64 sums: a thread's groups in order, the butterfly inside a wave, the waves in
// order, the blocks in order, over a grid that depends on n alone.  No floating-point atomics: the same bits in every run.
#include <math.h>

#include <algorithm>

#include "common.h"
#include "pc_grid.h"
#include "rigid3.h"

namespace bs {
namespace {

constexpr int PC_THREADS = 256;

// order-preserving map of fp32 bit patterns onto uint32 (and back)
__device__ __forceinline__ uint32_t pc_ord(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float pc_unord(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// ---- build ---------------------------------------------------------------------------------------------------------------------------------
// out[0..2] = min of ord(x, y, z), out[3..5] = min of ~ord = ~max (so one 0xff fill initialises both), out[6] = finite points
__global__ void __launch_bounds__(PC_THREADS) pc_bounds_kernel(const float* __restrict__ pts, int64_t n, uint32_t* __restrict__ out) {
    uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, cnt = 0;
    const int64_t stride = (int64_t)gridDim.x * PC_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x; i < n; i += stride) {
        const float p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        if (!(pc_finite(p[0]) && pc_finite(p[1]) && pc_finite(p[2]))) continue;
        ++cnt;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const uint32_t o = pc_ord(p[a]);
            mn[a] = min(mn[a], o);
            mx[a] = min(mx[a], ~o);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        cnt += __shfl_xor(cnt, d, 64);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            mn[a] = min(mn[a], (uint32_t)__shfl_xor(mn[a], d, 64));
            mx[a] = min(mx[a], (uint32_t)__shfl_xor(mx[a], d, 64));
        }
    }
    if ((threadIdx.x & 63) == 0 && cnt) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            atomicMin(&out[a], mn[a]);
            atomicMin(&out[3 + a], mx[a]);
        }
        atomicAdd(&out[6], cnt);
    }
}

// SCATTER false: counts[cell] += 1.  SCATTER true: `counts` is the cursor (a copy of the exclusive scan), the record goes to its slot
template <bool SCATTER>
__global__ void __launch_bounds__(PC_THREADS) pc_grid_kernel(const float* __restrict__ pts, int64_t n, PcGrid g, int32_t* __restrict__ counts,
                                                             int64_t n_records, f32x4* __restrict__ records) {
    const int64_t i = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= n) return;
    const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    if (!(pc_finite(x) && pc_finite(y) && pc_finite(z))) return;
    const int cx = pc_cell(x, g.lo[0], g.h, g.n[0]), cy = pc_cell(y, g.lo[1], g.h, g.n[1]), cz = pc_cell(z, g.lo[2], g.h, g.n[2]);
    const int cell = (cz * g.n[1] + cy) * g.n[0] + cx;
    const int32_t pos = atomicAdd(&counts[cell], 1);
    if (SCATTER) {
        if (pos >= 0 && pos < n_records) records[pos] = f32x4{x, y, z, __int_as_float((int32_t)i)};
    }
}

// ---- query ---------------------------------------------------------------------------------------------------------------------------------
// (the cell function, the candidate test and the walk over the shells: pc_grid.h, shared with icp.hip)
__global__ void __launch_bounds__(PC_THREADS) pc_query_grid_kernel(const f32x4* __restrict__ records, const int32_t* __restrict__ cell_start,
                                                                   PcGrid g, const float* __restrict__ src, int64_t m, float max_distance,
                                                                   int32_t shell_cap, float* __restrict__ dist, int32_t* __restrict__ idx,
                                                                   int32_t* __restrict__ fb_list, int32_t* __restrict__ fb_count) {
    const int64_t i = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= m) return;
    const float sx = src[3 * i], sy = src[3 * i + 1], sz = src[3 * i + 2];
    if (!(pc_finite(sx) && pc_finite(sy) && pc_finite(sz))) {
        dist[i] = __builtin_nanf("");
        idx[i] = -1;
        return;
    }
    float best;
    int32_t bi;
    if (!pc_walk_shells(records, cell_start, g, sx, sy, sz, max_distance, shell_cap, best, bi)) {     // the brute-force kernel finishes this one
        fb_list[atomicAdd(fb_count, 1)] = (int32_t)i;
        return;
    }
    float d = sqrtf(best);
    if (bi == PC_NONE || d > max_distance) { d = INFINITY; bi = -1; }
    dist[i] = d;
    idx[i] = bi;
}

constexpr int PB_SOURCES = 64, PB_WAVES = PC_THREADS / 64, PB_TILE = 1024;

__global__ void __launch_bounds__(PC_THREADS) pc_brute_kernel(const f32x4* __restrict__ records, int64_t n_records, const float* __restrict__ src,
                                                              int64_t m, const int32_t* __restrict__ list, int64_t chunk_len,
                                                              unsigned long long* __restrict__ keys) {
    __shared__ f32x4 tile[PB_TILE];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t q = (int64_t)blockIdx.x * PB_SOURCES + lane;
    const bool valid = q < m;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    if (valid) {
        const int64_t si = list ? (int64_t)list[q] : q;
        sx = src[3 * si]; sy = src[3 * si + 1]; sz = src[3 * si + 2];
    }
    const int64_t t0 = (int64_t)blockIdx.y * chunk_len, t1 = t0 + chunk_len < n_records ? t0 + chunk_len : n_records;
    float best = INFINITY;
    int32_t bi = PC_NONE;
    for (int64_t base = t0; base < t1; base += PB_TILE) {
        __syncthreads();
        const int cnt = t1 - base < PB_TILE ? (int)(t1 - base) : PB_TILE;
        for (int k = t; k < cnt; k += PC_THREADS) tile[k] = records[base + k];
        __syncthreads();
        for (int j = w; j < cnt; j += PB_WAVES) pc_candidate(tile[j], sx, sy, sz, best, bi);     // (a NaN source never compares: no update)
    }
    if (valid && bi != PC_NONE)
        atomicMin(&keys[q], ((unsigned long long)__float_as_uint(best) << 32) | (unsigned long long)(uint32_t)bi);
}

__global__ void __launch_bounds__(PC_THREADS) pc_brute_finish_kernel(const unsigned long long* __restrict__ keys, const float* __restrict__ src,
                                                                     int64_t m, const int32_t* __restrict__ list, float max_distance,
                                                                     float* __restrict__ dist, int32_t* __restrict__ idx) {
    const int64_t q = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x;
    if (q >= m) return;
    const int64_t si = list ? (int64_t)list[q] : q;
    const float sx = src[3 * si], sy = src[3 * si + 1], sz = src[3 * si + 2];
    float d;
    int32_t bi = -1;
    if (!(pc_finite(sx) && pc_finite(sy) && pc_finite(sz))) {
        d = __builtin_nanf("");
    } else {
        const unsigned long long key = keys[q];
        d = INFINITY;
        if (key != ~0ull) {
            const float dd = sqrtf(__uint_as_float((uint32_t)(key >> 32)));
            if (!(dd > max_distance)) { d = dd; bi = (int32_t)(uint32_t)(key & 0xffffffffull); }
        }
    }
    dist[si] = d;
    idx[si] = bi;
}

// s R p + t in fp64, rounded once to fp32; A = s R (12 doubles: the rows of [A | t])
struct PcAffine { double a[12]; };
template <typename T>
__global__ void __launch_bounds__(PC_THREADS) pc_transform_kernel(const T* __restrict__ src, int64_t n, PcAffine M, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= n) return;
    const double p0 = (double)src[3 * i], p1 = (double)src[3 * i + 1], p2 = (double)src[3 * i + 2];
    float o[3];
    affine_point_f32(M.a, p0, p1, p2, o);
#pragma unroll
    for (int r = 0; r < 3; ++r) out[3 * i + r] = o[r];
}

// ---- statistics ----------------------------------------------------------------------------------------------------------------------------
constexpr int PS_GRID_MAX = 1024, PS_WAVES = PC_THREADS / 64;
constexpr int PS_BINS_HI = 2048, PS_BINS_LO = 1024;      // digits of 11, 11 and 10 bits

struct PsPartial {        // per block of pass 0
    double sum, sumsq;
    uint64_t n_fin, n_inf, n_nan;
    uint64_t c[BS_PC_MAX_THRESHOLDS];
    float mx;
    uint32_t pad[5];
};
static_assert(sizeof(PsPartial) == 128, "PsPartial");
struct PsState {          // the two middle ranks floor((n - 1) / 2), floor(n / 2): the key bits found so far and the rank inside them
    uint32_t prefix[2], rank[2], n, pad[3];
};
struct PsTaus { float v[BS_PC_MAX_THRESHOLDS]; };
struct PsLayout { size_t hist0, hist1, hist2, state, partial, total; };
PsLayout ps_layout() {
    PsLayout L;
    size_t o = 0;
    L.hist0 = o; o += (size_t)PS_BINS_HI * 4;
    L.hist1 = o; o += (size_t)2 * PS_BINS_HI * 4;
    L.hist2 = o; o += (size_t)2 * PS_BINS_LO * 4;
    L.state = o; o += sizeof(PsState);
    o = (o + 127) & ~(size_t)127;
    L.partial = o; o += (size_t)PS_GRID_MAX * sizeof(PsPartial);
    L.total = o;
    return L;
}
static_assert(BS_PC_STATS_WORKSPACE_BYTES >= (PS_BINS_HI * 3 + PS_BINS_LO * 2) * 4 + 128 + PS_GRID_MAX * 128, "BS_PC_STATS_WORKSPACE_BYTES");

// group g of the array: elements 4g .. 4g+3 (in[k]: inside the array).  VEC: the array is 16-byte aligned, a whole group is one load.
// Both forms hand the same elements to the same thread in the same order.
template <bool VEC>
__device__ __forceinline__ void ps_load4(const float* __restrict__ d, int64_t n, int64_t g, float (&v)[4], bool (&in)[4]) {
    const int64_t p0 = g * 4;
    if (VEC && p0 + 3 < n) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(d + p0);
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] = a[k]; in[k] = true; }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            in[k] = p0 + k < n;
            v[k] = in[k] ? d[p0 + k] : 0.0f;
        }
    }
}

// PASS 0: the sums and the histogram of the top 11 key bits; 1: of the middle 11 bits under each rank's prefix; 2: of the low 10 bits
template <int PASS, bool VEC>
__global__ void __launch_bounds__(PC_THREADS) ps_pass_kernel(const float* __restrict__ d, int64_t n, PsTaus taus, int32_t n_tau,
                                                             const PsState* __restrict__ state, uint32_t* __restrict__ hist,
                                                             PsPartial* __restrict__ partial) {
    constexpr int BINS = PASS == 2 ? PS_BINS_LO : PS_BINS_HI, NH = PASS == 0 ? 1 : 2;
    __shared__ uint32_t h[NH * BINS];
    __shared__ double ldsd[PS_WAVES][2];
    __shared__ uint64_t ldsu[PS_WAVES][3 + BS_PC_MAX_THRESHOLDS];
    __shared__ float ldsm[PS_WAVES];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int i = t; i < NH * BINS; i += PC_THREADS) h[i] = 0;
    uint32_t pre0 = 0, pre1 = 0;
    if (PASS) { pre0 = state->prefix[0]; pre1 = state->prefix[1]; }
    __syncthreads();
    double sum = 0.0, sumsq = 0.0;
    float mx = -INFINITY;
    uint32_t n_fin = 0, n_inf = 0, n_nan = 0, c[BS_PC_MAX_THRESHOLDS];
#pragma unroll
    for (int k = 0; k < BS_PC_MAX_THRESHOLDS; ++k) c[k] = 0;
    const int64_t groups = (n + 3) / 4, stride = (int64_t)gridDim.x * PC_THREADS;
    for (int64_t g = (int64_t)blockIdx.x * PC_THREADS + t; g < groups; g += stride) {
        float v[4];
        bool in[4];
        ps_load4<VEC>(d, n, g, v, in);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!in[k]) continue;
            const float x = v[k];
            if (!pc_finite(x)) {
                if (PASS == 0) { if (x != x) ++n_nan; else ++n_inf; }
                continue;
            }
            const uint32_t key = pc_ord(x);
            if (PASS == 0) {
                ++n_fin;
                const double xd = (double)x;
                sum += xd;
                sumsq += xd * xd;
                mx = fmaxf(mx, x);
#pragma unroll
                for (int j = 0; j < BS_PC_MAX_THRESHOLDS; ++j) c[j] += (j < n_tau && x < taus.v[j]) ? 1u : 0u;
                atomicAdd(&h[key >> 21], 1u);
            } else if (PASS == 1) {
                if ((key >> 21) == pre0) atomicAdd(&h[(key >> 10) & 2047u], 1u);
                if ((key >> 21) == pre1) atomicAdd(&h[BINS + ((key >> 10) & 2047u)], 1u);
            } else {
                if ((key >> 10) == pre0) atomicAdd(&h[key & 1023u], 1u);
                if ((key >> 10) == pre1) atomicAdd(&h[BINS + (key & 1023u)], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = t; i < NH * BINS; i += PC_THREADS) {
        const uint32_t v = h[i];
        if (v) atomicAdd(&hist[i], v);
    }
    if (PASS == 0) {
        uint64_t u[3 + BS_PC_MAX_THRESHOLDS] = {n_fin, n_inf, n_nan};
#pragma unroll
        for (int k = 0; k < BS_PC_MAX_THRESHOLDS; ++k) u[3 + k] = c[k];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            sum += __shfl_xor(sum, s, 64);
            sumsq += __shfl_xor(sumsq, s, 64);
            mx = fmaxf(mx, __shfl_xor(mx, s, 64));
#pragma unroll
            for (int k = 0; k < 3 + BS_PC_MAX_THRESHOLDS; ++k) u[k] += __shfl_xor(u[k], s, 64);
        }
        if (lane == 0) {
            ldsd[w][0] = sum; ldsd[w][1] = sumsq; ldsm[w] = mx;
#pragma unroll
            for (int k = 0; k < 3 + BS_PC_MAX_THRESHOLDS; ++k) ldsu[w][k] = u[k];
        }
        __syncthreads();
        if (t == 0) {
            PsPartial q;
            q.sum = ((ldsd[0][0] + ldsd[1][0]) + ldsd[2][0]) + ldsd[3][0];
            q.sumsq = ((ldsd[0][1] + ldsd[1][1]) + ldsd[2][1]) + ldsd[3][1];
            q.mx = fmaxf(fmaxf(ldsm[0], ldsm[1]), fmaxf(ldsm[2], ldsm[3]));
            q.n_fin = ldsu[0][0] + ldsu[1][0] + ldsu[2][0] + ldsu[3][0];
            q.n_inf = ldsu[0][1] + ldsu[1][1] + ldsu[2][1] + ldsu[3][1];
            q.n_nan = ldsu[0][2] + ldsu[1][2] + ldsu[2][2] + ldsu[3][2];
            for (int k = 0; k < BS_PC_MAX_THRESHOLDS; ++k) q.c[k] = ldsu[0][3 + k] + ldsu[1][3 + k] + ldsu[2][3 + k] + ldsu[3][3 + k];
            for (int k = 0; k < 5; ++k) q.pad[k] = 0;
            partial[blockIdx.x] = q;
        }
    }
}

// one block: the bin of each middle rank.  PASS 0 sets the ranks from the total; PASS 2 also adds the partials in block order and writes the
// record (BS_PC_STATS_FIELDS doubles, include/bodyslam_hip.h)
template <int PASS>
__global__ void __launch_bounds__(PC_THREADS) ps_select_kernel(const uint32_t* __restrict__ hist, PsState* __restrict__ state,
                                                               const PsPartial* __restrict__ partial, int32_t blocks, int64_t n, int32_t n_tau,
                                                               double* __restrict__ out) {
    constexpr int BINS = PASS == 2 ? PS_BINS_LO : PS_BINS_HI, PER = BINS / PC_THREADS, BITS = PASS == 2 ? 10 : 11;
    __shared__ uint32_t tot[PC_THREADS];
    __shared__ PsState s;
    const int t = threadIdx.x;
    if (t == 0) {
        if (PASS == 0) { s.prefix[0] = s.prefix[1] = 0; s.rank[0] = s.rank[1] = 0; s.n = 0; s.pad[0] = s.pad[1] = s.pad[2] = 0; }
        else s = *state;
    }
    __syncthreads();
    const PsState in = s;
    __syncthreads();
    for (int r = 0; r < 2; ++r) {
        const uint32_t* hr = hist + (PASS == 0 ? 0 : r * BINS);
        uint32_t v[PER], mine = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) { v[k] = hr[t * PER + k]; mine += v[k]; }
        tot[t] = mine;
        __syncthreads();
        uint32_t excl = 0, total = 0;
        for (int i = 0; i < PC_THREADS; ++i) {          // (256 LDS reads per thread, three times per call: nothing next to a pass over the data)
            const uint32_t u = tot[i];
            if (i < t) excl += u;
            total += u;
        }
        uint32_t rank = in.rank[r];
        if (PASS == 0) {
            rank = total ? (r == 0 ? (total - 1) / 2 : total / 2) : 0;
            if (t == 0 && r == 0) s.n = total;
        }
        if (total) {
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                if (excl <= rank && rank < excl + v[k]) {
                    s.prefix[r] = (in.prefix[r] << BITS) | (uint32_t)(t * PER + k);
                    s.rank[r] = rank - excl;
                }
                excl += v[k];
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        if (PASS < 2) {
            *state = s;
        } else {
            double sum = 0.0, sumsq = 0.0;
            float mx = -INFINITY;
            uint64_t n_fin = 0, n_inf = 0, n_nan = 0, c[BS_PC_MAX_THRESHOLDS];
            for (int k = 0; k < BS_PC_MAX_THRESHOLDS; ++k) c[k] = 0;
            for (int b = 0; b < blocks; ++b) {
                const PsPartial q = partial[b];
                sum += q.sum; sumsq += q.sumsq; mx = fmaxf(mx, q.mx);
                n_fin += q.n_fin; n_inf += q.n_inf; n_nan += q.n_nan;
                for (int k = 0; k < BS_PC_MAX_THRESHOLDS; ++k) c[k] += q.c[k];
            }
            const double nan = __builtin_nan("");
            out[0] = (double)n;
            out[1] = (double)n_fin;
            out[2] = (double)n_inf;
            out[3] = (double)n_nan;
            out[4] = sum;
            out[5] = sumsq;
            out[6] = n_fin ? (double)mx : nan;
            out[7] = n_fin ? ((double)pc_unord(s.prefix[0]) + (double)pc_unord(s.prefix[1])) / 2.0 : nan;
            for (int k = 0; k < BS_PC_MAX_THRESHOLDS; ++k) out[8 + k] = k < n_tau ? (double)c[k] : 0.0;
            for (int k = 8 + BS_PC_MAX_THRESHOLDS; k < BS_PC_STATS_FIELDS; ++k) out[k] = 0.0;
        }
    }
}

}  // namespace
}  // namespace bs

extern "C" int bs_pc_bounds(const float* points, int64_t n, uint32_t* out, void* stream) {
    using namespace bs;
    if (!initialized()) { set_error("bs_pc_bounds: call bs_init first"); return BS_ERR_NOT_INIT; }
    BS_REQUIRE(points && out, "bs_pc_bounds: null pointer");
    BS_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "bs_pc_bounds: n = %lld (1 <= n < 2^31)", (long long)n);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    BS_CHECK_HIP(hipMemsetAsync(out, 0xff, 24, st));
    BS_CHECK_HIP(hipMemsetAsync(out + 6, 0, 8, st));
    const int blocks = (int)std::min<int64_t>(cdiv64(n, PC_THREADS), 4 * (int64_t)cu_count());
    hipLaunchKernelGGL(pc_bounds_kernel, dim3(blocks), dim3(PC_THREADS), 0, st, points, n, out);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_grid_count(const float* points, int64_t n, const float* lo, const float* hi, float cell_size, const int32_t* dims,
                                int32_t* counts, void* stream) {
    using namespace bs;
    if (!initialized()) { set_error("bs_pc_grid_count: call bs_init first"); return BS_ERR_NOT_INIT; }
    BS_REQUIRE(points && lo && hi && dims && counts, "bs_pc_grid_count: null pointer");
    BS_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "bs_pc_grid_count: n = %lld (1 <= n < 2^31)", (long long)n);
    const PcGrid g = pc_grid(lo, hi, cell_size, dims);
    BS_REQUIRE(pc_grid_ok(g), "bs_pc_grid_count: bad grid (cell size %g, %d x %d x %d cells, at most 2^24)", (double)cell_size, dims[0], dims[1], dims[2]);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pc_grid_kernel<false>, dim3((unsigned)cdiv64(n, PC_THREADS)), dim3(PC_THREADS), 0, st, points, n, g, counts, (int64_t)0,
                       (f32x4*)nullptr);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_grid_scatter(const float* points, int64_t n, const float* lo, const float* hi, float cell_size, const int32_t* dims,
                                  int32_t* cursor, int64_t n_records, void* records, void* stream) {
    using namespace bs;
    if (!initialized()) { set_error("bs_pc_grid_scatter: call bs_init first"); return BS_ERR_NOT_INIT; }
    BS_REQUIRE(points && lo && hi && dims && cursor && records, "bs_pc_grid_scatter: null pointer");
    BS_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && n_records >= 0 && n_records <= n, "bs_pc_grid_scatter: n = %lld, n_records = %lld", (long long)n,
               (long long)n_records);
    BS_REQUIRE(((uintptr_t)records & 15) == 0, "bs_pc_grid_scatter: records must be 16-byte aligned");
    const PcGrid g = pc_grid(lo, hi, cell_size, dims);
    BS_REQUIRE(pc_grid_ok(g), "bs_pc_grid_scatter: bad grid (cell size %g, %d x %d x %d cells, at most 2^24)", (double)cell_size, dims[0], dims[1], dims[2]);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pc_grid_kernel<true>, dim3((unsigned)cdiv64(n, PC_THREADS)), dim3(PC_THREADS), 0, st, points, n, g, cursor, n_records,
                       static_cast<f32x4*>(records));
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_query_grid(const void* records, const int32_t* cell_start, int64_t n_records, const float* lo, const float* hi, float cell_size,
                                const int32_t* dims, const float* source, int64_t m, float max_distance, int32_t shell_cap, float* dist,
                                int32_t* index, int32_t* fallback_list, int32_t* fallback_count, void* stream) {
    using namespace bs;
    if (!initialized()) { set_error("bs_pc_query_grid: call bs_init first"); return BS_ERR_NOT_INIT; }
    BS_REQUIRE(records && cell_start && lo && hi && dims && source && dist && index && fallback_list && fallback_count, "bs_pc_query_grid: null pointer");
    BS_REQUIRE(m >= 1 && m < ((int64_t)1 << 31) && n_records >= 0 && n_records < ((int64_t)1 << 31), "bs_pc_query_grid: m = %lld, n_records = %lld",
               (long long)m, (long long)n_records);
    BS_REQUIRE(((uintptr_t)records & 15) == 0, "bs_pc_query_grid: records must be 16-byte aligned");
    BS_REQUIRE(shell_cap >= 0 && !(max_distance < 0.0f) && max_distance == max_distance, "bs_pc_query_grid: shell_cap %d, max_distance %g", shell_cap,
               (double)max_distance);
    const PcGrid g = pc_grid(lo, hi, cell_size, dims);
    BS_REQUIRE(pc_grid_ok(g), "bs_pc_query_grid: bad grid (cell size %g, %d x %d x %d cells, at most 2^24)", (double)cell_size, dims[0], dims[1], dims[2]);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    BS_CHECK_HIP(hipMemsetAsync(fallback_count, 0, 4, st));
    hipLaunchKernelGGL(pc_query_grid_kernel, dim3((unsigned)cdiv64(m, PC_THREADS)), dim3(PC_THREADS), 0, st, static_cast<const f32x4*>(records),
                       cell_start, g, source, m, max_distance, shell_cap, dist, index, fallback_list, fallback_count);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_query_brute(const void* records, int64_t n_records, const float* source, const int32_t* list, int64_t m, float max_distance,
                                 void* keys, float* dist, int32_t* index, void* stream) {
    using namespace bs;
    if (!initialized()) { set_error("bs_pc_query_brute: call bs_init first"); return BS_ERR_NOT_INIT; }
    BS_REQUIRE(source && keys && dist && index && (records || n_records == 0), "bs_pc_query_brute: null pointer");
    BS_REQUIRE(m >= 1 && m < ((int64_t)1 << 31) && n_records >= 0 && n_records < ((int64_t)1 << 31), "bs_pc_query_brute: m = %lld, n_records = %lld",
               (long long)m, (long long)n_records);
    BS_REQUIRE(((uintptr_t)records & 15) == 0 && ((uintptr_t)keys & 7) == 0, "bs_pc_query_brute: records must be 16-byte, keys 8-byte aligned");
    BS_REQUIRE(!(max_distance < 0.0f) && max_distance == max_distance, "bs_pc_query_brute: max_distance %g", (double)max_distance);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned long long* k = static_cast<unsigned long long*>(keys);
    BS_CHECK_HIP(hipMemsetAsync(k, 0xff, (size_t)m * 8, st));
    if (n_records > 0) {
        // enough blocks to fill the device (four per CU) when the sources are few: the targets are cut into chunks of whole tiles
        const int64_t sb = cdiv64(m, PB_SOURCES), tiles = cdiv64(n_records, PB_TILE);
        const int64_t want = std::max<int64_t>(1, cdiv64(4 * (int64_t)cu_count(), sb));
        const int64_t chunk_len = cdiv64(tiles, std::min<int64_t>(std::min<int64_t>(tiles, want), 65535)) * PB_TILE;
        const int64_t chunks = cdiv64(n_records, chunk_len);
        hipLaunchKernelGGL(pc_brute_kernel, dim3((unsigned)sb, (unsigned)chunks), dim3(PC_THREADS), 0, st, static_cast<const f32x4*>(records), n_records,
                           source, m, list, chunk_len, k);
        BS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(pc_brute_finish_kernel, dim3((unsigned)cdiv64(m, PC_THREADS)), dim3(PC_THREADS), 0, st, k, source, m, list, max_distance, dist, index);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_transform(const void* source, int32_t dtype, int64_t n, const double* affine, float* out, void* stream) {
    using namespace bs;
    if (!initialized()) { set_error("bs_pc_transform: call bs_init first"); return BS_ERR_NOT_INIT; }
    BS_REQUIRE(source && affine && out, "bs_pc_transform: null pointer");
    BS_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "bs_pc_transform: n = %lld (1 <= n < 2^31)", (long long)n);
    BS_REQUIRE(dtype == BS_F32 || dtype == BS_F64, "bs_pc_transform: dtype %d (BS_F32 or BS_F64)", dtype);
    PcAffine M;
    for (int i = 0; i < 12; ++i) M.a[i] = affine[i];
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)cdiv64(n, PC_THREADS));
    if (dtype == BS_F32) hipLaunchKernelGGL(pc_transform_kernel<float>, grid, dim3(PC_THREADS), 0, st, static_cast<const float*>(source), n, M, out);
    else hipLaunchKernelGGL(pc_transform_kernel<double>, grid, dim3(PC_THREADS), 0, st, static_cast<const double*>(source), n, M, out);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_stats(const float* dist, int64_t n, const float* thresholds, int32_t n_thresholds, void* workspace, int64_t workspace_bytes,
                           double* out, void* stream) {
    using namespace bs;
    if (!initialized()) { set_error("bs_pc_stats: call bs_init first"); return BS_ERR_NOT_INIT; }
    BS_REQUIRE(dist && workspace && out && (thresholds || n_thresholds == 0), "bs_pc_stats: null pointer");
    BS_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "bs_pc_stats: n = %lld (1 <= n < 2^31)", (long long)n);
    BS_REQUIRE(n_thresholds >= 0 && n_thresholds <= BS_PC_MAX_THRESHOLDS, "bs_pc_stats: %d thresholds (at most %d)", n_thresholds, BS_PC_MAX_THRESHOLDS);
    const PsLayout L = ps_layout();
    BS_REQUIRE(workspace_bytes >= (int64_t)L.total, "bs_pc_stats: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)L.total);
    BS_REQUIRE(((uintptr_t)workspace & 127) == 0, "bs_pc_stats: workspace must be 128-byte aligned");
    PsTaus taus;
    for (int k = 0; k < BS_PC_MAX_THRESHOLDS; ++k) taus.v[k] = k < n_thresholds ? thresholds[k] : 0.0f;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    uint32_t* hist0 = reinterpret_cast<uint32_t*>(ws + L.hist0);
    uint32_t* hist1 = reinterpret_cast<uint32_t*>(ws + L.hist1);
    uint32_t* hist2 = reinterpret_cast<uint32_t*>(ws + L.hist2);
    PsState* state = reinterpret_cast<PsState*>(ws + L.state);
    PsPartial* partial = reinterpret_cast<PsPartial*>(ws + L.partial);
    BS_CHECK_HIP(hipMemsetAsync(ws, 0, L.state, st));             // the three histograms
    const int blocks = (int)std::min<int64_t>(cdiv64(cdiv64(n, 4), PC_THREADS), PS_GRID_MAX);        // depends on n alone
    const bool vec = ((uintptr_t)dist & 15) == 0;
    const dim3 grid(blocks), one(1), thr(PC_THREADS);
#define PS_PASS(P, H)                                                                                                        \
    do {                                                                                                                     \
        if (vec) hipLaunchKernelGGL((ps_pass_kernel<P, true>), grid, thr, 0, st, dist, n, taus, n_thresholds, state, H, partial);  \
        else hipLaunchKernelGGL((ps_pass_kernel<P, false>), grid, thr, 0, st, dist, n, taus, n_thresholds, state, H, partial);     \
        BS_CHECK_LAUNCH();                                                                                                   \
        hipLaunchKernelGGL((ps_select_kernel<P>), one, thr, 0, st, H, state, partial, blocks, n, n_thresholds, out);          \
        BS_CHECK_LAUNCH();                                                                                                   \
    } while (0)
    PS_PASS(0, hist0);
    PS_PASS(1, hist1);
    PS_PASS(2, hist2);
#undef PS_PASS
    return BS_OK;
}
