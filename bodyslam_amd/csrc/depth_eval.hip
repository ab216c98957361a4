// Depth-map evaluation with the reference's MDEM protocol (bs_depth_metrics, include/bodyslam_hip.h):
// per-frame GT mask, exact medians of the masked GT and prediction, median scaling, and AbsRel / SqRel / RMSE / RMSE-log / three
// delta accuracies in fp64 (BodySLAM_not_refactored/EVALUATION/MDEM_eval.py:114-127,179-197, evaluation_metrics.py:24-102).
//
// Six launches (and one memset of the histograms) on the caller's stream, over a grid of (chunks, frames) or of frames:
//   hist_hi    histogram of the high byte of the masked GT and prediction values (integer LDS atomics, then one global atomic per
//              non-empty bin and block)
//   select_hi  per frame: the high-byte buckets that hold ranks floor((n-1)/2) and floor(n/2), by a block scan of the 256 bins
//   hist_lo    histogram of the low byte of the values inside those buckets
//   select_lo  per frame: the two order statistics -> exact medians (numpy's: the mean of the two middle values for even n), scale
//   metrics    fp64 per-pixel terms summed thread -> wave -> block into one partial per chunk of EV_CHUNK pixels
//   combine    per frame: the chunk partials summed in chunk order, the record written
// The histograms hold integer counts, so their atomics give the same counts in any order; the fp64 sums run in an order fixed by the
// pixel's place in its frame alone (the chunk size is a constant), so a frame's record has the same bits in every run, alone or at any
// position of any batch.
#include <math.h>

#include "common.h"

namespace bs {
namespace {

constexpr int EV_THREADS = 256;
constexpr int EV_VEC = 8;                                        // pixels per group: one 16-byte load of each map
constexpr int EV_ITERS = 8;                                      // groups per thread and chunk
constexpr int64_t EV_CHUNK = (int64_t)EV_THREADS * EV_VEC * EV_ITERS;   // 16384 pixels

// delta thresholds: evaluation_metrics.py:98 compares with criterion ** 2 for criterion = 1.25, 1.25 ** 2, 1.25 ** 3 -- the squares,
// 1.25^2, 1.25^4, 1.25^6, all exact in fp64 (the reference's quirk, kept)
constexpr double EV_T1 = 1.5625, EV_T2 = 2.44140625, EV_T3 = 3.814697265625;

struct EvSel {            // per frame, from select_hi: for GT (0) and prediction (1) the buckets of the two middle ranks and the ranks in them
    int32_t n;            // masked pixels
    int32_t bucket[2][2];
    int32_t rank[2][2];
    int32_t pad;
};
struct EvStat {           // per frame, from select_lo
    double median[2];     // GT, prediction
    double scale;
    double n_mask;
};
struct EvPartial {        // per (frame, chunk), from metrics
    double abs_rel, sq_rel, sq, log_sq;
    uint32_t n_valid, n_pos, c1, c2, c3, pad[3];
};
static_assert(sizeof(EvPartial) == 64, "EvPartial");

struct EvLayout {
    int64_t chunks;
    size_t hist_hi, hist_lo, sel, stat, partial, total;          // byte offsets into the workspace
};
EvLayout ev_layout(int64_t B, int64_t N) {
    EvLayout L;
    L.chunks = cdiv64(N, EV_CHUNK);
    size_t o = 0;
    L.hist_hi = o; o += (size_t)B * 2 * 256 * 4;
    L.hist_lo = o; o += (size_t)B * 4 * 256 * 4;
    L.sel = o;     o += (size_t)B * sizeof(EvSel);
    o = (o + 63) & ~(size_t)63;
    L.stat = o;    o += (size_t)B * sizeof(EvStat);
    o = (o + 63) & ~(size_t)63;
    L.partial = o; o += (size_t)B * L.chunks * sizeof(EvPartial);
    L.total = o;
    return L;
}

// the 8 pixels of group g of a frame (pixels 8g .. 8g+7); out-of-frame pixels are reported invalid.  VEC: N % 8 == 0 and both frames
// 16-byte aligned, one 16-byte load per map.  Both forms hand the same pixels to the same thread in the same order.
template <bool VEC>
__device__ __forceinline__ void ev_load8(const uint16_t* __restrict__ gt, const uint16_t* __restrict__ pred, int64_t N, int64_t g,
                                         uint32_t (&gv)[8], uint32_t (&pv)[8], bool (&in)[8]) {
    const int64_t p0 = g * EV_VEC;
    if (VEC) {
        const bool ok = p0 < N;
        u32x4 a = {0, 0, 0, 0}, b = {0, 0, 0, 0};
        if (ok) {
            a = *reinterpret_cast<const u32x4*>(gt + p0);
            b = *reinterpret_cast<const u32x4*>(pred + p0);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            gv[2 * k] = a[k] & 0xffffu; gv[2 * k + 1] = a[k] >> 16;
            pv[2 * k] = b[k] & 0xffffu; pv[2 * k + 1] = b[k] >> 16;
            in[2 * k] = ok; in[2 * k + 1] = ok;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            in[k] = p0 + k < N;
            gv[k] = in[k] ? gt[p0 + k] : 0u;
            pv[k] = in[k] ? pred[p0 + k] : 0u;
        }
    }
}

// Depth is spatially smooth: most of a thread's 8 neighbouring values share a digit.  Equal keys in a row are merged into one LDS
// atomic (key < 0: no add).
struct RunAdd {
    int key = -1;
    uint32_t cnt = 0;
    __device__ __forceinline__ void push(uint32_t* h, int k) {
        if (k == key) { ++cnt; return; }
        if (key >= 0) atomicAdd(&h[key], cnt);
        key = k;
        cnt = k >= 0 ? 1u : 0u;
    }
    __device__ __forceinline__ void flush(uint32_t* h) {
        if (key >= 0) atomicAdd(&h[key], cnt);
        key = -1;
        cnt = 0;
    }
};

template <bool VEC>
__global__ void __launch_bounds__(EV_THREADS) ev_hist_hi_kernel(const uint16_t* __restrict__ pred, const uint16_t* __restrict__ gt, int64_t N,
                                                                uint32_t glo, uint32_t ghi, uint32_t* __restrict__ hist_hi) {
    __shared__ uint32_t h[2 * 256];
    const int t = threadIdx.x;
    const int64_t f = blockIdx.y;
    for (int i = t; i < 2 * 256; i += EV_THREADS) h[i] = 0;
    __syncthreads();
    const uint16_t* g_f = gt + f * N;
    const uint16_t* p_f = pred + f * N;
    RunAdd rg, rp;
    for (int it = 0; it < EV_ITERS; ++it) {
        const int64_t grp = (int64_t)blockIdx.x * (EV_CHUNK / EV_VEC) + it * EV_THREADS + t;
        uint32_t gv[8], pv[8];
        bool in[8];
        ev_load8<VEC>(g_f, p_f, N, grp, gv, pv, in);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool m = in[k] && gv[k] >= glo && gv[k] <= ghi;
            rg.push(h, m ? (int)(gv[k] >> 8) : -1);
            rp.push(h, m ? 256 + (int)(pv[k] >> 8) : -1);
        }
    }
    rg.flush(h);
    rp.flush(h);
    __syncthreads();
    uint32_t* out = hist_hi + f * 512;
    for (int i = t; i < 512; i += EV_THREADS) {
        const uint32_t v = h[i];
        if (v) atomicAdd(&out[i], v);
    }
}

// inclusive sum over the block's 256 threads (4 waves): wave scan by shuffles, then the wave totals
__device__ __forceinline__ uint32_t ev_block_scan(uint32_t v, uint32_t* lds4) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    __syncthreads();                                             // (lds4 may still be read by a previous scan)
    if (lane == 63) lds4[w] = v;
    __syncthreads();
    for (int i = 0; i < w; ++i) v += lds4[i];
    return v;
}

__global__ void __launch_bounds__(EV_THREADS) ev_select_hi_kernel(const uint32_t* __restrict__ hist_hi, EvSel* __restrict__ sel) {
    __shared__ uint32_t lds4[4];
    __shared__ EvSel s;
    const int t = threadIdx.x;
    const int64_t f = blockIdx.x;
    if (t == 0) {
        s.n = 0; s.pad = 0;
        for (int a = 0; a < 2; ++a)
            for (int r = 0; r < 2; ++r) { s.bucket[a][r] = -1; s.rank[a][r] = 0; }
    }
    for (int a = 0; a < 2; ++a) {
        const uint32_t v = hist_hi[f * 512 + a * 256 + t];
        const uint32_t incl = ev_block_scan(v, lds4);
        const uint32_t n = lds4[0] + lds4[1] + lds4[2] + lds4[3];
        const uint32_t excl = incl - v;
        if (a == 0 && t == 0) s.n = (int32_t)n;
        if (n > 0) {
            const uint32_t k[2] = {(n - 1) / 2, n / 2};
            for (int r = 0; r < 2; ++r)
                if (excl <= k[r] && k[r] < incl) { s.bucket[a][r] = t; s.rank[a][r] = (int32_t)(k[r] - excl); }
        }
    }
    __syncthreads();
    if (t == 0) sel[f] = s;
}

template <bool VEC>
__global__ void __launch_bounds__(EV_THREADS) ev_hist_lo_kernel(const uint16_t* __restrict__ pred, const uint16_t* __restrict__ gt, int64_t N,
                                                                uint32_t glo, uint32_t ghi, const EvSel* __restrict__ sel,
                                                                uint32_t* __restrict__ hist_lo) {
    __shared__ uint32_t h[4 * 256];
    const int t = threadIdx.x;
    const int64_t f = blockIdx.y;
    const EvSel s = sel[f];
    if (s.n == 0) return;                                       // (uniform per block) empty mask: no median to find
    for (int i = t; i < 4 * 256; i += EV_THREADS) h[i] = 0;
    __syncthreads();
    // slot 0: the bucket of rank floor((n-1)/2); slot 1: that of rank floor(n/2) where it is another bucket
    const int bg0 = s.bucket[0][0], bg1 = s.bucket[0][1] != bg0 ? s.bucket[0][1] : -1;
    const int bp0 = s.bucket[1][0], bp1 = s.bucket[1][1] != bp0 ? s.bucket[1][1] : -1;
    const uint16_t* g_f = gt + f * N;
    const uint16_t* p_f = pred + f * N;
    RunAdd rg, rp;
    for (int it = 0; it < EV_ITERS; ++it) {
        const int64_t grp = (int64_t)blockIdx.x * (EV_CHUNK / EV_VEC) + it * EV_THREADS + t;
        uint32_t gv[8], pv[8];
        bool in[8];
        ev_load8<VEC>(g_f, p_f, N, grp, gv, pv, in);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool m = in[k] && gv[k] >= glo && gv[k] <= ghi;
            const int dg = (int)(gv[k] >> 8), dp = (int)(pv[k] >> 8);
            const int kg = !m ? -1 : dg == bg0 ? (int)(gv[k] & 255) : dg == bg1 ? 256 + (int)(gv[k] & 255) : -1;
            const int kp = !m ? -1 : dp == bp0 ? 512 + (int)(pv[k] & 255) : dp == bp1 ? 768 + (int)(pv[k] & 255) : -1;
            rg.push(h, kg);
            rp.push(h, kp);
        }
    }
    rg.flush(h);
    rp.flush(h);
    __syncthreads();
    uint32_t* out = hist_lo + f * 1024;
    for (int i = t; i < 1024; i += EV_THREADS) {
        const uint32_t v = h[i];
        if (v) atomicAdd(&out[i], v);
    }
}

// scale_mode 0: s = median(gt) / median(pred) (MDEM_eval.py:114-127,196); 1: s = fixed_scale
__global__ void __launch_bounds__(EV_THREADS) ev_select_lo_kernel(const uint32_t* __restrict__ hist_lo, const EvSel* __restrict__ sel,
                                                                  int32_t scale_mode, double fixed_scale, EvStat* __restrict__ stat) {
    __shared__ uint32_t lds4[4];
    __shared__ uint32_t val[2][2];
    const int t = threadIdx.x;
    const int64_t f = blockIdx.x;
    const EvSel s = sel[f];
    if (t < 4) val[t >> 1][t & 1] = 0;
    if (s.n > 0) {
        for (int a = 0; a < 2; ++a)
            for (int slot = 0; slot < 2; ++slot) {
                const uint32_t v = hist_lo[f * 1024 + (a * 2 + slot) * 256 + t];
                const uint32_t incl = ev_block_scan(v, lds4);
                const uint32_t excl = incl - v;
                for (int r = 0; r < 2; ++r) {
                    // rank r lives in slot 0 unless its bucket differs from rank 0's
                    const int rs = (r == 1 && s.bucket[a][1] != s.bucket[a][0]) ? 1 : 0;
                    const uint32_t k = (uint32_t)s.rank[a][r];
                    if (rs == slot && excl <= k && k < incl) val[a][r] = ((uint32_t)s.bucket[a][r] << 8) | (uint32_t)t;
                }
            }
    }
    __syncthreads();
    if (t == 0) {
        EvStat st;
        for (int a = 0; a < 2; ++a)   // np.median: the middle value, or the mean of the two middle values (np.mean in fp64: (a + b) / 2)
            st.median[a] = s.n > 0 ? ((double)val[a][0] + (double)val[a][1]) / 2.0 : __builtin_nan("");
        st.scale = scale_mode == 1 ? fixed_scale : st.median[0] / st.median[1];
        st.n_mask = (double)s.n;
        stat[f] = st;
    }
}

template <bool VEC>
__global__ void __launch_bounds__(EV_THREADS) ev_metrics_kernel(const uint16_t* __restrict__ pred, const uint16_t* __restrict__ gt, int64_t N,
                                                                uint32_t glo, uint32_t ghi, const EvStat* __restrict__ stat, int64_t chunks,
                                                                EvPartial* __restrict__ partial) {
    __shared__ double ldsd[4][4];
    __shared__ uint32_t ldsu[4][5];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t f = blockIdx.y;
    const double s = stat[f].scale;
    const uint16_t* g_f = gt + f * N;
    const uint16_t* p_f = pred + f * N;
    double a_abs = 0.0, a_sqr = 0.0, a_sq = 0.0, a_log = 0.0;
    uint32_t n_valid = 0, n_pos = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int it = 0; it < EV_ITERS; ++it) {
        const int64_t grp = (int64_t)blockIdx.x * (EV_CHUNK / EV_VEC) + it * EV_THREADS + t;
        uint32_t gv[8], pv[8];
        bool in[8];
        ev_load8<VEC>(g_f, p_f, N, grp, gv, pv, in);
        for (int k = 0; k < 8; ++k) {
            if (!(in[k] && gv[k] >= glo && gv[k] <= ghi)) continue;
            const double g = (double)gv[k];
            const double p = s * (double)pv[k];                   // MDEM_eval.py:197
            // abs_rel_diff / squared_rel_error / rmse (evaluation_metrics.py:24-69): mask gt != 0; np.nanmean skips NaN terms, and a
            // term is NaN exactly where p is (g is finite and nonzero here)
            if (gv[k] != 0 && !__builtin_isnan(p)) {
                const double d = g - p;
                const double d2 = d * d;
                a_abs += fabs(d) / g;
                a_sqr += d2 / g;
                a_sq += d2;
                ++n_valid;
            }
            // rmse_log / accuracy (:71-102): mask gt > 0 and p > 0 (p > 0 is false for NaN).  np.log of the uint16 GT runs in fp32: the
            // correctly rounded fp32 value, widened (log(double) is within a few ulp, and every log g, g < 65536, lies over 4000 fp64 ulp
            // from an fp32 rounding boundary, so the conversion rounds it correctly); log p in fp64
            if (gv[k] != 0 && p > 0.0) {
                const double e = (double)(float)log(g) - log(p);
                a_log += e * e;
                const double r = fmax(g / p, p / g);
                c1 += r < EV_T1;
                c2 += r < EV_T2;
                c3 += r < EV_T3;
                ++n_pos;
            }
        }
    }
    // wave: a fixed butterfly; block: the waves in order
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a_abs += __shfl_xor(a_abs, d, 64);
        a_sqr += __shfl_xor(a_sqr, d, 64);
        a_sq += __shfl_xor(a_sq, d, 64);
        a_log += __shfl_xor(a_log, d, 64);
        n_valid += __shfl_xor(n_valid, d, 64);
        n_pos += __shfl_xor(n_pos, d, 64);
        c1 += __shfl_xor(c1, d, 64);
        c2 += __shfl_xor(c2, d, 64);
        c3 += __shfl_xor(c3, d, 64);
    }
    if (lane == 0) {
        ldsd[w][0] = a_abs; ldsd[w][1] = a_sqr; ldsd[w][2] = a_sq; ldsd[w][3] = a_log;
        ldsu[w][0] = n_valid; ldsu[w][1] = n_pos; ldsu[w][2] = c1; ldsu[w][3] = c2; ldsu[w][4] = c3;
    }
    __syncthreads();
    if (t == 0) {
        EvPartial q;
        q.abs_rel = ((ldsd[0][0] + ldsd[1][0]) + ldsd[2][0]) + ldsd[3][0];
        q.sq_rel = ((ldsd[0][1] + ldsd[1][1]) + ldsd[2][1]) + ldsd[3][1];
        q.sq = ((ldsd[0][2] + ldsd[1][2]) + ldsd[2][2]) + ldsd[3][2];
        q.log_sq = ((ldsd[0][3] + ldsd[1][3]) + ldsd[2][3]) + ldsd[3][3];
        q.n_valid = ldsu[0][0] + ldsu[1][0] + ldsu[2][0] + ldsu[3][0];
        q.n_pos = ldsu[0][1] + ldsu[1][1] + ldsu[2][1] + ldsu[3][1];
        q.c1 = ldsu[0][2] + ldsu[1][2] + ldsu[2][2] + ldsu[3][2];
        q.c2 = ldsu[0][3] + ldsu[1][3] + ldsu[2][3] + ldsu[3][3];
        q.c3 = ldsu[0][4] + ldsu[1][4] + ldsu[2][4] + ldsu[3][4];
        q.pad[0] = q.pad[1] = q.pad[2] = 0;
        partial[f * chunks + blockIdx.x] = q;
    }
}

// one thread per frame: the chunk partials in chunk order, then the record (BS_DEPTH_METRICS_FIELDS doubles, include/bodyslam_hip.h)
__global__ void __launch_bounds__(64) ev_combine_kernel(const EvPartial* __restrict__ partial, const EvStat* __restrict__ stat, int64_t chunks,
                                                        int32_t B, double* __restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (f >= B) return;
    double a_abs = 0.0, a_sqr = 0.0, a_sq = 0.0, a_log = 0.0;
    uint64_t n_valid = 0, n_pos = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int64_t c = 0; c < chunks; ++c) {
        const EvPartial q = partial[f * chunks + c];
        a_abs += q.abs_rel; a_sqr += q.sq_rel; a_sq += q.sq; a_log += q.log_sq;
        n_valid += q.n_valid; n_pos += q.n_pos; c1 += q.c1; c2 += q.c2; c3 += q.c3;
    }
    const EvStat st = stat[f];
    // np.nanmean over no term and the mean of an empty boolean array are NaN: 0 / 0 gives it
    const double nv = (double)n_valid, np_ = (double)n_pos;
    double* o = out + f * BS_DEPTH_METRICS_FIELDS;
    o[0] = a_abs / nv;
    o[1] = a_sqr / nv;
    o[2] = sqrt(a_sq / nv);
    o[3] = sqrt(a_log / np_);
    o[4] = (double)c1 / np_;
    o[5] = (double)c2 / np_;
    o[6] = (double)c3 / np_;
    o[7] = st.scale;
    o[8] = st.median[0];
    o[9] = st.median[1];
    o[10] = st.n_mask;
    o[11] = nv;
    o[12] = np_;
    for (int i = 13; i < BS_DEPTH_METRICS_FIELDS; ++i) o[i] = 0.0;
}

}  // namespace
}  // namespace bs

extern "C" int64_t bs_depth_metrics_workspace(int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (int64_t)bs::ev_layout(B, (int64_t)H * W).total;
}

extern "C" int bs_depth_metrics(const uint16_t* pred, const uint16_t* gt, int32_t B, int32_t H, int32_t W, double gt_lo, double gt_hi,
                                int32_t scale_mode, double scale, void* workspace, int64_t workspace_bytes, double* out, void* stream) {
    using namespace bs;
    if (!initialized()) { set_error("bs_depth_metrics: call bs_init first"); return BS_ERR_NOT_INIT; }
    BS_REQUIRE(pred && gt && workspace && out, "bs_depth_metrics: null pointer");
    BS_REQUIRE(B > 0 && H > 0 && W > 0 && B <= 65535, "bs_depth_metrics: bad shape B=%d H=%d W=%d (1 <= B <= 65535)", B, H, W);
    const int64_t N = (int64_t)H * W;
    BS_REQUIRE(N < ((int64_t)1 << 31), "bs_depth_metrics: H*W = %lld pixels per frame is too many", (long long)N);
    BS_REQUIRE(scale_mode == BS_DEPTH_SCALE_MEDIAN || scale_mode == BS_DEPTH_SCALE_FIXED, "bs_depth_metrics: bad scale_mode %d", scale_mode);
    const EvLayout L = ev_layout(B, N);
    BS_REQUIRE(workspace_bytes >= (int64_t)L.total, "bs_depth_metrics: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
               (long long)L.total);
    // the open interval gt_lo < g < gt_hi over integers g in [0, 65535] as the closed one glo <= g <= ghi (NaN bounds: nothing passes)
    uint32_t glo = 1, ghi = 0;
    if (!isnan(gt_lo) && !isnan(gt_hi)) {
        const double lo = gt_lo < 0.0 ? 0.0 : (gt_lo >= 65535.0 ? 65536.0 : floor(gt_lo) + 1.0);
        const double hi = gt_hi > 65535.0 ? 65535.0 : (gt_hi <= 0.0 ? -1.0 : ceil(gt_hi) - 1.0);
        if (lo <= hi) { glo = (uint32_t)lo; ghi = (uint32_t)hi; }
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    uint32_t* hist_hi = reinterpret_cast<uint32_t*>(ws + L.hist_hi);
    uint32_t* hist_lo = reinterpret_cast<uint32_t*>(ws + L.hist_lo);
    EvSel* sel = reinterpret_cast<EvSel*>(ws + L.sel);
    EvStat* stat = reinterpret_cast<EvStat*>(ws + L.stat);
    EvPartial* partial = reinterpret_cast<EvPartial*>(ws + L.partial);
    BS_CHECK_HIP(hipMemsetAsync(ws, 0, L.sel, st));            // both histograms
    const bool vec = N % EV_VEC == 0 && ((uintptr_t)pred & 15) == 0 && ((uintptr_t)gt & 15) == 0;
    const dim3 grid((unsigned)L.chunks, (unsigned)B);
    if (vec) hipLaunchKernelGGL(ev_hist_hi_kernel<true>, grid, dim3(EV_THREADS), 0, st, pred, gt, N, glo, ghi, hist_hi);
    else hipLaunchKernelGGL(ev_hist_hi_kernel<false>, grid, dim3(EV_THREADS), 0, st, pred, gt, N, glo, ghi, hist_hi);
    BS_CHECK_LAUNCH();
    hipLaunchKernelGGL(ev_select_hi_kernel, dim3(B), dim3(EV_THREADS), 0, st, hist_hi, sel);
    BS_CHECK_LAUNCH();
    if (vec) hipLaunchKernelGGL(ev_hist_lo_kernel<true>, grid, dim3(EV_THREADS), 0, st, pred, gt, N, glo, ghi, sel, hist_lo);
    else hipLaunchKernelGGL(ev_hist_lo_kernel<false>, grid, dim3(EV_THREADS), 0, st, pred, gt, N, glo, ghi, sel, hist_lo);
    BS_CHECK_LAUNCH();
    hipLaunchKernelGGL(ev_select_lo_kernel, dim3(B), dim3(EV_THREADS), 0, st, hist_lo, sel, scale_mode, scale, stat);
    BS_CHECK_LAUNCH();
    if (vec) hipLaunchKernelGGL(ev_metrics_kernel<true>, grid, dim3(EV_THREADS), 0, st, pred, gt, N, glo, ghi, stat, L.chunks, partial);
    else hipLaunchKernelGGL(ev_metrics_kernel<false>, grid, dim3(EV_THREADS), 0, st, pred, gt, N, glo, ghi, stat, L.chunks, partial);
    BS_CHECK_LAUNCH();
    hipLaunchKernelGGL(ev_combine_kernel, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, st, partial, stat, L.chunks, B, out);
    BS_CHECK_LAUNCH();
    return BS_OK;
}
