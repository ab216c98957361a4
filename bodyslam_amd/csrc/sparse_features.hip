// Sparse-feature scale path (bs_orb_*; include/bodyslam_hip.h): ORB keypoints and descriptors, brute-force Hamming match with cross-check,
// depth association and the mean 3-D displacement of BodySLAM_not_refactored/3DM/scaling_system.py:107-137, all on the device.
//   ORB                   Rublee, Rabaud, Konolige, Bradski 2011; FAST-9/16: Rosten & Drummond 2006; the corner measure: Harris & Stephens 1988;
//                         the test pairs: Calonder et al. 2010 (BRIEF).  Parameters are cv2.ORB_create()'s defaults.  The algorithm, with
//                         every choice that makes it reproducible bit for bit, is stated in tests/_orb_ref.py.  Parity with OpenCV: UNPINNED.
//   associate_depth, calculate_displacements, compute_scaling_factor   scaling_system.py:46-137, restated with their quirks.
//
// Every entry works on `batch` frames in one launch per stage; a frame's (or a pair's) result does not depend on the batch.
//   bs_orb_pyramid        grey_kernel, resize_kernel per level (level l is made from level l - 1), smooth_kernel over all levels
//   bs_orb_fast           fast_kernel over all levels: FAST score + 3x3 NMS + edge margin in one pass, the histogram of the kept scores
//   bs_orb_select         select_kernel, one block per frame: per level the cut of the score histogram, an ORDER-PRESERVING compaction of
//                         the score map (so nothing depends on the order atomics hand anything out in: the only atomics are the
//                         histogram's counts), the Harris response of the 2 n_l survivors, ranking by counting
//   bs_orb_describe       describe_kernel, one wave per keypoint: moments by wave reduction (integers), bin, 256 tests packed by __ballot
//   bs_orb_match          match_kernel, one block per pair of consecutive frames: both descriptor sets in LDS, read 16 bytes at a time
//   bs_orb_displacement   displacement_kernel, one block per pair: the associations as ordered compactions, fp64 positions, the sum in
//                         list order by one thread
// Images are bytes.  The kernels read them from global memory (L2-resident: a frame's pyramid is under 1 MB) and not from an LDS tile:
// DESIGN section 7's rule allows LDS gathers of 16 bytes per lane only, which a byte-granular ring or patch gather is not.
// Time not measured yet (tools/sparse_scale_time.py).
#include <math.h>

#include "common.h"
#include "orb_match.h"

namespace bs {
namespace {

constexpr int ORB_EDGE = 31;              // edge threshold: keypoints keep this distance from a level's border
constexpr int ORB_FAST_T = 20;
constexpr int ORB_HALF_PATCH = 15;
constexpr int ORB_BINS = 30;
constexpr int ORB_CAND = 256;             // 2 n_l <= ORB_CAND

struct OrbLevels {
    int n, stride;
    int W[BS_ORB_MAX_LEVELS], H[BS_ORB_MAX_LEVELS], off[BS_ORB_MAX_LEVELS], nfeat[BS_ORB_MAX_LEVELS];
    double scale[BS_ORB_MAX_LEVELS];
};

__device__ __forceinline__ int reflect101(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i;
}

// ---- grey, pyramid, smoothing ---------------------------------------------------------------------------------------------------------
// grey = (4899 R + 9617 G + 1868 B + 8192) >> 14; bgr: the colour's channel 0 is B
__global__ void __launch_bounds__(ORB_THREADS) grey_kernel(const uint8_t* __restrict__ color, int HW, int stride, int bgr, uint8_t* __restrict__ grey) {
    const int i = blockIdx.x * ORB_THREADS + threadIdx.x;
    if (i >= HW) return;
    const uint8_t* c = color + ((int64_t)blockIdx.y * HW + i) * 3;
    const int r = bgr ? c[2] : c[0], g = c[1], b = bgr ? c[0] : c[2];
    grey[(int64_t)blockIdx.y * stride + i] = (uint8_t)((4899 * r + 9617 * g + 1868 * b + 8192) >> 14);
}

// bilinear, pixel centres aligned, 11-bit weights: q = floor(((2 x + 1) Ws - Wd) 2^10 / Wd) is the source abscissa in units of 2^-11
__global__ void __launch_bounds__(ORB_THREADS) resize_kernel(uint8_t* __restrict__ pyr, int stride, int Ws, int Hs, int offs, int Wd, int Hd, int offd) {
    const int i = blockIdx.x * ORB_THREADS + threadIdx.x;
    if (i >= Wd * Hd) return;
    const int x = i % Wd, y = i / Wd;
    const int64_t qx = (((int64_t)(2 * x + 1) * Ws - Wd) * 1024) / Wd, qy = (((int64_t)(2 * y + 1) * Hs - Hd) * 1024) / Hd;     // (>= 0: Ws >= Wd)
    int x0 = (int)(qx >> 11), y0 = (int)(qy >> 11);
    const int wx = (int)(qx & 2047), wy = (int)(qy & 2047);
    x0 = min(x0, Ws - 1);
    y0 = min(y0, Hs - 1);
    const int x1 = min(x0 + 1, Ws - 1), y1 = min(y0 + 1, Hs - 1);
    uint8_t* f = pyr + (int64_t)blockIdx.y * stride;
    const uint8_t* s = f + offs;
    const int p00 = s[y0 * Ws + x0], p01 = s[y0 * Ws + x1], p10 = s[y1 * Ws + x0], p11 = s[y1 * Ws + x1];
    const int v = (2048 - wy) * ((2048 - wx) * p00 + wx * p01) + wy * ((2048 - wx) * p10 + wx * p11);      // <= 255 * 2^22
    f[offd + i] = (uint8_t)((v + (1 << 21)) >> 22);
}

// [1 6 15 20 15 6 1]^2 / 4096, reflect-101, one rounding
__global__ void __launch_bounds__(ORB_THREADS) smooth_kernel(const uint8_t* __restrict__ grey, OrbLevels lv, uint8_t* __restrict__ smooth) {
    const int l = blockIdx.y, W = lv.W[l], H = lv.H[l];
    const int i = blockIdx.x * ORB_THREADS + threadIdx.x;
    if (i >= W * H) return;
    const int x = i % W, y = i / W;
    const uint8_t* g = grey + (int64_t)blockIdx.z * lv.stride + lv.off[l];
    const int taps[7] = {1, 6, 15, 20, 15, 6, 1};
    int xs[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) xs[k] = reflect101(x + k - 3, W);
    int acc = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const uint8_t* row = g + reflect101(y + j - 3, H) * W;
        int r = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) r += taps[k] * row[xs[k]];
        acc += taps[j] * r;
    }
    smooth[(int64_t)blockIdx.z * lv.stride + lv.off[l] + i] = (uint8_t)((acc + 2048) >> 12);
}

// ---- FAST-9/16 ------------------------------------------------------------------------------------------------------------------------
// The score of a pixel: the largest threshold t at which it is still a corner (9 contiguous ring pixels all > p + t or all < p - t),
// max over the 16 arcs of the arc's smallest difference, minus one; 0 when that is below ORB_FAST_T.  The 16-bit brighter / darker
// masks decide first whether the pixel is a corner at ORB_FAST_T at all (rotate-and-AND).  Needs 3 <= x < W - 3, 3 <= y < H - 3.
__device__ __forceinline__ bool arc9(uint32_t m) {
    const uint32_t x = m | (m << 16);
    uint32_t r = x & (x >> 1);
    r &= r >> 2;
    r &= r >> 4;
    r &= x >> 8;
    return (r & 0xffffu) != 0;
}
__device__ __forceinline__ int fast_score(const uint8_t* __restrict__ g, int W, int x, int y) {
    const uint8_t* c = g + y * W + x;
    const int p = c[0];
    const int W2 = 2 * W, W3 = 3 * W;
    const int d[16] = {c[-W3] - p,     c[-W3 + 1] - p, c[-W2 + 2] - p, c[-W + 3] - p, c[3] - p,  c[W + 3] - p,  c[W2 + 2] - p,  c[W3 + 1] - p,
                       c[W3] - p,      c[W3 - 1] - p,  c[W2 - 2] - p,  c[W - 3] - p,  c[-3] - p, c[-W - 3] - p, c[-W2 - 2] - p, c[-W3 - 1] - p};
    uint32_t mb = 0, md = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        mb |= (uint32_t)(d[k] > ORB_FAST_T) << k;
        md |= (uint32_t)(d[k] < -ORB_FAST_T) << k;
    }
    if (!arc9(mb) && !arc9(md)) return 0;
    int best = 0;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        int lo = d[s], hi = d[s];
#pragma unroll
        for (int k = 1; k < 9; ++k) {
            lo = min(lo, d[(s + k) & 15]);
            hi = max(hi, d[(s + k) & 15]);
        }
        best = max(best, max(lo, -hi));
    }
    return best - 1;       // >= ORB_FAST_T here: an arc passed at ORB_FAST_T
}

// score map after NMS: the pixel's score where it is a corner, lies ORB_EDGE inside the level and beats its 8 neighbours strictly, else 0
__global__ void __launch_bounds__(ORB_THREADS) fast_kernel(const uint8_t* __restrict__ grey, OrbLevels lv, uint8_t* __restrict__ score, int* __restrict__ hist) {
    const int l = blockIdx.y, W = lv.W[l], H = lv.H[l];
    const int i = blockIdx.x * ORB_THREADS + threadIdx.x;
    if (i >= W * H) return;
    const int x = i % W, y = i / W;
    const uint8_t* g = grey + (int64_t)blockIdx.z * lv.stride + lv.off[l];
    int s = 0;
    if (x >= ORB_EDGE && x < W - ORB_EDGE && y >= ORB_EDGE && y < H - ORB_EDGE) {
        s = fast_score(g, W, x, y);
        if (s > 0) {
            bool keep = true;
            for (int dy = -1; dy <= 1 && keep; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if ((dx | dy) == 0) continue;
                    if (fast_score(g, W, x + dx, y + dy) >= s) { keep = false; break; }
                }
            if (!keep) s = 0;
        }
    }
    score[(int64_t)blockIdx.z * lv.stride + lv.off[l] + i] = (uint8_t)s;
    if (s > 0) atomicAdd(&hist[((int64_t)blockIdx.z * BS_ORB_MAX_LEVELS + l) * 256 + s], 1);      // counts: the same whatever the order
}

// ---- selection ------------------------------------------------------------------------------------------------------------------------
// Harris response of the 7x7 block around (x, y): int64 sums of 3x3 Sobel products, det - 0.04 tr^2 in fp64 (no contraction)
__device__ double harris_response(const uint8_t* __restrict__ g, int W, int x, int y) {
    int64_t a = 0, b = 0, c = 0;
    for (int dy = -3; dy <= 3; ++dy)
        for (int dx = -3; dx <= 3; ++dx) {
            const uint8_t* q = g + (y + dy) * W + (x + dx);
            const int ix = (q[-W + 1] - q[-W - 1]) + 2 * (q[1] - q[-1]) + (q[W + 1] - q[W - 1]);
            const int iy = (q[W - 1] - q[-W - 1]) + 2 * (q[W] - q[-W]) + (q[W + 1] - q[-W + 1]);
            a += ix * ix;
            b += iy * iy;
            c += ix * iy;
        }
    const double da = (double)a, db = (double)b, dc = (double)c;
    const double det = da * db - dc * dc, tr = da + db;
    return det - 0.04 * (tr * tr);
}

// one block per frame; the levels in turn.  kp [batch, ORB_KP, 8] int32 = (level, x, y, FAST score, m10, m01, bin, 0): this kernel writes
// fields 0-3, the keypoints of a level in the order (Harris response descending, row-major pixel index ascending), the levels one behind
// the other; resp [batch, ORB_KP] double; counts [batch, BS_ORB_MAX_LEVELS + 1] = keypoints per level and their sum.
__global__ void __launch_bounds__(ORB_THREADS) select_kernel(const uint8_t* __restrict__ grey, const uint8_t* __restrict__ score, const int* __restrict__ hist,
                                                             OrbLevels lv, int* __restrict__ kp, double* __restrict__ resp, int* __restrict__ counts) {
    __shared__ int h[256];
    __shared__ int scan[ORB_WAVES];
    __shared__ int cut[2];
    __shared__ int c_idx[ORB_CAND], t_idx[ORB_CAND];
    __shared__ double c_resp[ORB_CAND];
    const int t = threadIdx.x, f = blockIdx.x;
    int total_kp = 0;
    for (int l = 0; l < BS_ORB_MAX_LEVELS; ++l) {
        const int W = l < lv.n ? lv.W[l] : 0, H = l < lv.n ? lv.H[l] : 0, n = l < lv.n ? lv.nfeat[l] : 0;
        int count_l = 0;
        if (n > 0 && W > 2 * ORB_EDGE && H > 2 * ORB_EDGE) {                         // (uniform per block)
            const int size = W * H;
            const uint8_t* sc = score + (int64_t)f * lv.stride + lv.off[l];
            const uint8_t* g = grey + (int64_t)f * lv.stride + lv.off[l];
            __syncthreads();
            h[t] = hist[((int64_t)f * BS_ORB_MAX_LEVELS + l) * 256 + t];
            __syncthreads();
            if (t == 0) {
                // the cut: the largest T with #(score >= T) >= 2 n; scores above T are in, of those equal to T the lowest pixel indices
                int acc = 0, T = 0, need = 0;
                for (int s = 255; s >= 1; --s) {
                    if (acc + h[s] >= 2 * n) { T = s; need = 2 * n - acc; break; }
                    acc += h[s];
                }
                cut[0] = T;
                cut[1] = need;
            }
            __syncthreads();
            const int T = cut[0], need = cut[1];
            int n_sure = 0, n_tie = 0;
            for (int base = 0; base < size; base += ORB_THREADS * 16) {
                const int o = base + t * 16;
                u32x4 v = {0u, 0u, 0u, 0u};
                if (o < size) v = *reinterpret_cast<const u32x4*>(sc + o);              // (16-byte aligned; the slack behind a level covers the tail)
                int cs = 0, ct = 0;
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int s = (o + k < size) ? (int)((v[k >> 2] >> (8 * (k & 3))) & 255u) : 0;
                    cs += s > T;
                    ct += (T > 0 && s == T);
                }
                int tot;
                const int ex = block_excl_scan(cs | (ct << 16), scan, tot);
                int ps = n_sure + (ex & 0xffff), pt = n_tie + (ex >> 16);
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int s = (o + k < size) ? (int)((v[k >> 2] >> (8 * (k & 3))) & 255u) : 0;
                    if (s > T) {
                        if (ps < ORB_CAND) c_idx[ps] = o + k;
                        ++ps;
                    } else if (T > 0 && s == T) {
                        if (pt < need && pt < ORB_CAND) t_idx[pt] = o + k;
                        ++pt;
                    }
                }
                n_sure += tot & 0xffff;
                n_tie += tot >> 16;
            }
            __syncthreads();
            n_sure = min(n_sure, ORB_CAND);
            const int take = min(min(n_tie, need), ORB_CAND - n_sure);
            if (t < take) c_idx[n_sure + t] = t_idx[t];
            const int m = n_sure + take;
            __syncthreads();
            int my_idx = 0;
            double my_r = 0.0;
            if (t < m) {
                my_idx = c_idx[t];
                my_r = harris_response(g, W, my_idx % W, my_idx / W);
                c_resp[t] = my_r;
            }
            __syncthreads();
            if (t < m) {
                int rank = 0;
                for (int j = 0; j < m; ++j) {
                    const double r = c_resp[j];
                    rank += (r > my_r) || (r == my_r && c_idx[j] < my_idx);
                }
                if (rank < n) {
                    const int64_t k = (int64_t)f * ORB_KP + total_kp + rank;
                    int* o = kp + k * 8;
                    o[0] = l;
                    o[1] = my_idx % W;
                    o[2] = my_idx / W;
                    o[3] = sc[my_idx];
                    o[4] = o[5] = o[6] = o[7] = 0;
                    resp[k] = my_r;
                }
            }
            count_l = min(m, n);
        }
        if (t == 0) counts[f * (BS_ORB_MAX_LEVELS + 1) + l] = count_l;
        total_kp += count_l;
    }
    if (t == 0) counts[f * (BS_ORB_MAX_LEVELS + 1) + BS_ORB_MAX_LEVELS] = total_kp;
}

// ---- orientation and descriptor -------------------------------------------------------------------------------------------------------
// one wave per keypoint.  cs: 2 * ORB_BINS doubles (cos, then sin); pattern: int8 [ORB_BINS, 256, 4] read as one dword per pair
__global__ void __launch_bounds__(ORB_THREADS) describe_kernel(const uint8_t* __restrict__ grey, const uint8_t* __restrict__ smooth, OrbLevels lv,
                                                               const double* __restrict__ cs, const uint32_t* __restrict__ pattern, int* __restrict__ kp,
                                                               const int* __restrict__ counts, float* __restrict__ pt, uint32_t* __restrict__ desc) {
    const int lane = threadIdx.x & 63, f = blockIdx.y;
    const int k = blockIdx.x * ORB_WAVES + (threadIdx.x >> 6);
    if (k >= counts[f * (BS_ORB_MAX_LEVELS + 1) + BS_ORB_MAX_LEVELS]) return;      // (uniform per wave; no block barrier below)
    int* me = kp + ((int64_t)f * ORB_KP + k) * 8;
    const int l = me[0], x = me[1], y = me[2], W = lv.W[l];
    const uint8_t* g = grey + (int64_t)f * lv.stride + lv.off[l] + y * W + x;
    const uint8_t* s = smooth + (int64_t)f * lv.stride + lv.off[l] + y * W + x;
    int m10 = 0, m01 = 0;
    for (int i = lane; i < 31 * 31; i += 64) {
        const int v = i / 31 - ORB_HALF_PATCH, u = i % 31 - ORB_HALF_PATCH;
        if (u * u + v * v <= ORB_HALF_PATCH * ORB_HALF_PATCH) {
            const int I = g[v * W + u];
            m10 += u * I;
            m01 += v * I;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        m10 += __shfl_xor(m10, d, 64);
        m01 += __shfl_xor(m01, d, 64);
    }
    int bin = 0;
    double best = (double)m10 * cs[0] + (double)m01 * cs[ORB_BINS];
    for (int b = 1; b < ORB_BINS; ++b) {
        const double v = (double)m10 * cs[b] + (double)m01 * cs[ORB_BINS + b];
        if (v > best) { best = v; bin = b; }
    }
    unsigned long long bits[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t q = pattern[(bin * 256 + r * 64 + lane)];
        const int x1 = (int8_t)(q & 255u), y1 = (int8_t)((q >> 8) & 255u), x2 = (int8_t)((q >> 16) & 255u), y2 = (int8_t)(q >> 24);
        bits[r] = __ballot(s[y1 * W + x1] < s[y2 * W + x2]);
    }
    if (lane < 8) desc[((int64_t)f * ORB_KP + k) * 8 + lane] = (uint32_t)(bits[lane >> 1] >> (32 * (lane & 1)));
    if (lane == 0) {
        me[4] = m10;
        me[5] = m01;
        me[6] = bin;
        const double sc = lv.scale[l];
        pt[((int64_t)f * ORB_KP + k) * 2] = (float)((double)x * sc);
        pt[((int64_t)f * ORB_KP + k) * 2 + 1] = (float)((double)y * sc);
    }
}

// ---- match ----------------------------------------------------------------------------------------------------------------------------
// pair p: query = frame p (the previous frame), train = frame p + 1.  matches [pairs, ORB_KP, 4] int32 = (queryIdx, trainIdx, distance, 0)
// in BFMatcher(NORM_HAMMING, crossCheck = True) + stable sort by distance order; mcount [pairs].  The body is orb_match.h's, which
// bs_orb_match_pairs (loop_closure.hip) runs over an arbitrary list of pairs.
__global__ void __launch_bounds__(ORB_THREADS) match_kernel(const uint32_t* __restrict__ desc, const int* __restrict__ counts, int* __restrict__ matches,
                                                            int* __restrict__ mcount) {
    const int p = blockIdx.x;
    orb_match_pair(desc, counts, p, p + 1, matches + (int64_t)p * ORB_KP * 4, mcount + p);
}

// ---- association and displacement -----------------------------------------------------------------------------------------------------
// (associate_depth's lookup, depth_at: orb_match.h)
// out [pairs, BS_ORB_OUT_FIELDS] doubles: 0-2 the mean displacement (NaN without a usable pair), 3 keypoints of the previous frame, 4 of the
// current one, 5 matches, 6 associations of the previous frame's side, 7 of the current frame's side, 8 pairs used
__global__ void __launch_bounds__(ORB_THREADS) displacement_kernel(const float* __restrict__ pt, const int* __restrict__ counts, const int* __restrict__ matches,
                                                                   const int* __restrict__ mcount, const float* __restrict__ depth, int H, int W, double fx,
                                                                   double fy, double cx, double cy, int matched, double* __restrict__ out) {
    __shared__ int a_m[ORB_KP], b_m[ORB_KP];
    __shared__ double a_d[ORB_KP], b_d[ORB_KP];
    __shared__ double disp[ORB_KP * 3];
    __shared__ int scan[ORB_WAVES];
    const int t = threadIdx.x, p = blockIdx.x;
    const int n1 = min(counts[p * (BS_ORB_MAX_LEVELS + 1) + BS_ORB_MAX_LEVELS], ORB_KP);
    const int n2 = min(counts[(p + 1) * (BS_ORB_MAX_LEVELS + 1) + BS_ORB_MAX_LEVELS], ORB_KP);
    const int M = min(mcount[p], ORB_KP);
    const float* pt1 = pt + (int64_t)p * ORB_KP * 2;
    const float* pt2 = pt + (int64_t)(p + 1) * ORB_KP * 2;
    const float* dp1 = depth + (int64_t)p * H * W;
    const float* dp2 = depth + (int64_t)(p + 1) * H * W;
    const int* mt = matches + (int64_t)p * ORB_KP * 4;
    int nA = 0, nB = 0, nP = 0;
    for (int base = 0; base < M; base += ORB_THREADS) {
        const int i = base + t;
        bool fa = false, fb = false;
        double da = 0.0, db = 0.0;
        if (i < M) {
            const int q = mt[i * 4], tr = mt[i * 4 + 1];
            fa = depth_at(dp1, H, W, pt1[2 * q], pt1[2 * q + 1], da);
            if (matched) {
                fb = depth_at(dp2, H, W, pt2[2 * tr], pt2[2 * tr + 1], db);
            } else if (q < n2 && tr < n1) {
                // (sic) the reference's second call passes the keypoint lists swapped and the same matches: queryIdx, an index into the
                // previous frame's keypoints, picks a keypoint of the CURRENT frame for the depth lookup
                fb = depth_at(dp2, H, W, pt2[2 * q], pt2[2 * q + 1], db);
            }
        }
        int tot;
        if (matched) {
            const bool both = fa && fb;
            const int ex = block_excl_scan((int)fa | ((int)fb << 10) | ((int)both << 20), scan, tot);
            if (both) {
                const int pos = nP + (ex >> 20);
                a_m[pos] = i;
                a_d[pos] = da;
                b_m[pos] = i;
                b_d[pos] = db;
            }
            nA += tot & 1023;
            nB += (tot >> 10) & 1023;
            nP += tot >> 20;
        } else {
            const int ex = block_excl_scan((int)fa | ((int)fb << 10), scan, tot);
            if (fa) {
                a_m[nA + (ex & 1023)] = i;
                a_d[nA + (ex & 1023)] = da;
            }
            if (fb) {
                b_m[nB + ((ex >> 10) & 1023)] = i;
                b_d[nB + ((ex >> 10) & 1023)] = db;
            }
            nA += tot & 1023;
            nB += (tot >> 10) & 1023;
        }
    }
    if (!matched) nP = min(nA, nB);            // (sic) zip of the two independently filtered lists
    __syncthreads();
    for (int k = t; k < nP; k += ORB_THREADS) {
        const int q = mt[a_m[k] * 4], tr = mt[b_m[k] * 4 + 1];
        const double u1 = (double)pt1[2 * q], v1 = (double)pt1[2 * q + 1], u2 = (double)pt2[2 * tr], v2 = (double)pt2[2 * tr + 1];
        const double d1 = a_d[k], d2 = b_d[k];
        disp[3 * k] = (u2 - cx) * d2 / fx - (u1 - cx) * d1 / fx;
        disp[3 * k + 1] = (v2 - cy) * d2 / fy - (v1 - cy) * d1 / fy;
        disp[3 * k + 2] = d2 - d1;
    }
    __syncthreads();
    if (t == 0) {
        double* o = out + (int64_t)p * BS_ORB_OUT_FIELDS;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int k = 0; k < nP; ++k) {
            s0 += disp[3 * k];
            s1 += disp[3 * k + 1];
            s2 += disp[3 * k + 2];
        }
        const double nan = __builtin_nan("");
        o[0] = nP ? s0 / (double)nP : nan;
        o[1] = nP ? s1 / (double)nP : nan;
        o[2] = nP ? s2 / (double)nP : nan;
        o[3] = (double)n1;
        o[4] = (double)n2;
        o[5] = (double)M;
        o[6] = (double)nA;
        o[7] = (double)nB;
        o[8] = (double)nP;
    }
}

// levels: host int32 [n_levels, 3] = (W_l, H_l, offset_l)
int make_levels(const char* who, const int32_t* levels, int32_t n_levels, int64_t stride, int32_t H, int32_t W, OrbLevels& lv) {
    BS_REQUIRE(levels, "%s: null levels", who);
    BS_REQUIRE(n_levels >= 1 && n_levels <= BS_ORB_MAX_LEVELS, "%s: %d levels (1 .. %d)", who, n_levels, BS_ORB_MAX_LEVELS);
    BS_REQUIRE(stride > 0 && stride <= 2147483647LL && (stride & 15) == 0, "%s: frame stride %lld (a positive multiple of 16 below 2^31)", who, (long long)stride);
    BS_REQUIRE(levels[0] == W && levels[1] == H, "%s: level 0 is %d x %d, the frame %d x %d", who, levels[0], levels[1], W, H);
    int64_t end = 0;
    lv = OrbLevels{};
    lv.n = n_levels;
    lv.stride = (int)stride;
    for (int l = 0; l < n_levels; ++l) {
        const int w = levels[3 * l], h = levels[3 * l + 1], off = levels[3 * l + 2];
        BS_REQUIRE(w >= 8 && h >= 8 && w <= 16384 && h <= 16384, "%s: level %d is %d x %d (8 .. 16384)", who, l, w, h);
        BS_REQUIRE(l == 0 || (w <= lv.W[l - 1] && h <= lv.H[l - 1]), "%s: level %d is larger than level %d", who, l, l - 1);
        BS_REQUIRE(off >= end && (off & 15) == 0, "%s: level %d at offset %d (16-byte aligned, behind level %d's end %lld)", who, l, off, l - 1, (long long)end);
        end = (int64_t)off + ((int64_t)w * h + 15) / 16 * 16;
        BS_REQUIRE(end <= stride, "%s: level %d ends at %lld, the frame stride is %lld", who, l, (long long)end, (long long)stride);
        lv.W[l] = w;
        lv.H[l] = h;
        lv.off[l] = off;
    }
    return BS_OK;
}

}  // namespace
}  // namespace bs

#define ORB_ENTRY(name)                                                                   \
    using namespace bs;                                                                   \
    if (!initialized()) { set_error(name ": call bs_init first"); return BS_ERR_NOT_INIT; } \
    hipStream_t st = reinterpret_cast<hipStream_t>(stream)

extern "C" int bs_orb_pyramid(const uint8_t* color, int32_t batch, int32_t H, int32_t W, int32_t bgr, const int32_t* levels, int32_t n_levels,
                              int64_t stride, uint8_t* grey, uint8_t* smooth, void* stream) {
    ORB_ENTRY("bs_orb_pyramid");
    BS_REQUIRE(color && grey && smooth, "bs_orb_pyramid: null pointer");
    BS_REQUIRE(batch >= 1 && batch <= 65535, "bs_orb_pyramid: batch %d (1 .. 65535)", batch);
    OrbLevels lv;
    if (int e = make_levels("bs_orb_pyramid", levels, n_levels, stride, H, W, lv)) return e;
    const unsigned b = (unsigned)batch;
    hipLaunchKernelGGL(grey_kernel, dim3((unsigned)((H * W + ORB_THREADS - 1) / ORB_THREADS), b), dim3(ORB_THREADS), 0, st, color, H * W, lv.stride, bgr != 0, grey);
    BS_CHECK_LAUNCH();
    for (int l = 1; l < lv.n; ++l) {
        hipLaunchKernelGGL(resize_kernel, dim3((unsigned)((lv.W[l] * lv.H[l] + ORB_THREADS - 1) / ORB_THREADS), b), dim3(ORB_THREADS), 0, st, grey, lv.stride,
                           lv.W[l - 1], lv.H[l - 1], lv.off[l - 1], lv.W[l], lv.H[l], lv.off[l]);
        BS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(smooth_kernel, dim3((unsigned)((H * W + ORB_THREADS - 1) / ORB_THREADS), (unsigned)lv.n, b), dim3(ORB_THREADS), 0, st, grey, lv, smooth);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_orb_fast(const uint8_t* grey, int32_t batch, int32_t H, int32_t W, const int32_t* levels, int32_t n_levels, int64_t stride,
                           uint8_t* score, int32_t* hist, void* stream) {
    ORB_ENTRY("bs_orb_fast");
    BS_REQUIRE(grey && score && hist, "bs_orb_fast: null pointer");
    BS_REQUIRE(batch >= 1 && batch <= 65535, "bs_orb_fast: batch %d (1 .. 65535)", batch);
    OrbLevels lv;
    if (int e = make_levels("bs_orb_fast", levels, n_levels, stride, H, W, lv)) return e;
    BS_CHECK_HIP(hipMemsetAsync(hist, 0, (size_t)batch * BS_ORB_MAX_LEVELS * 256 * sizeof(int32_t), st));
    hipLaunchKernelGGL(fast_kernel, dim3((unsigned)((H * W + ORB_THREADS - 1) / ORB_THREADS), (unsigned)lv.n, (unsigned)batch), dim3(ORB_THREADS), 0, st, grey, lv,
                       score, hist);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_orb_select(const uint8_t* grey, const uint8_t* score, const int32_t* hist, int32_t batch, int32_t H, int32_t W, const int32_t* levels,
                             int32_t n_levels, int64_t stride, const int32_t* features_per_level, int32_t* keypoints, double* response, int32_t* counts,
                             void* stream) {
    ORB_ENTRY("bs_orb_select");
    BS_REQUIRE(grey && score && hist && features_per_level && keypoints && response && counts, "bs_orb_select: null pointer");
    BS_REQUIRE(batch >= 1, "bs_orb_select: batch %d (>= 1)", batch);
    BS_REQUIRE(((uintptr_t)score & 15) == 0, "bs_orb_select: the score map must be 16-byte aligned");
    OrbLevels lv;
    if (int e = make_levels("bs_orb_select", levels, n_levels, stride, H, W, lv)) return e;
    int total = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int n = features_per_level[l];
        BS_REQUIRE(n >= 0 && 2 * n <= ORB_CAND, "bs_orb_select: %d features at level %d (0 .. %d)", n, l, ORB_CAND / 2);
        lv.nfeat[l] = n;
        total += n;
    }
    BS_REQUIRE(total <= ORB_KP, "bs_orb_select: %d features in all (<= %d)", total, ORB_KP);
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)batch), dim3(ORB_THREADS), 0, st, grey, score, hist, lv, keypoints, response, counts);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_orb_describe(const uint8_t* grey, const uint8_t* smooth, int32_t batch, int32_t H, int32_t W, const int32_t* levels, int32_t n_levels,
                               int64_t stride, const double* level_scale, const double* cos_sin, const int8_t* pattern, int32_t* keypoints,
                               const int32_t* counts, float* pt, uint32_t* desc, void* stream) {
    ORB_ENTRY("bs_orb_describe");
    BS_REQUIRE(grey && smooth && level_scale && cos_sin && pattern && keypoints && counts && pt && desc, "bs_orb_describe: null pointer");
    BS_REQUIRE(batch >= 1 && batch <= 65535, "bs_orb_describe: batch %d (1 .. 65535)", batch);
    BS_REQUIRE(((uintptr_t)pattern & 3) == 0 && ((uintptr_t)cos_sin & 7) == 0, "bs_orb_describe: misaligned table");
    OrbLevels lv;
    if (int e = make_levels("bs_orb_describe", levels, n_levels, stride, H, W, lv)) return e;
    for (int l = 0; l < n_levels; ++l) lv.scale[l] = level_scale[l];
    hipLaunchKernelGGL(describe_kernel, dim3((unsigned)(ORB_KP / ORB_WAVES), (unsigned)batch), dim3(ORB_THREADS), 0, st, grey, smooth, lv, cos_sin,
                       reinterpret_cast<const uint32_t*>(pattern), keypoints, counts, pt, desc);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_orb_match(const uint32_t* desc, const int32_t* counts, int32_t batch, int32_t* matches, int32_t* match_counts, void* stream) {
    ORB_ENTRY("bs_orb_match");
    BS_REQUIRE(desc && counts && matches && match_counts, "bs_orb_match: null pointer");
    BS_REQUIRE(batch >= 2, "bs_orb_match: batch %d frames (>= 2: pair p is frames p, p + 1)", batch);
    BS_REQUIRE(((uintptr_t)desc & 15) == 0, "bs_orb_match: descriptors must be 16-byte aligned");
    hipLaunchKernelGGL(match_kernel, dim3((unsigned)(batch - 1)), dim3(ORB_THREADS), 0, st, desc, counts, matches, match_counts);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_orb_displacement(const float* pt, const int32_t* counts, const int32_t* matches, const int32_t* match_counts, const float* depth,
                                   int32_t batch, int32_t H, int32_t W, const double* K, int32_t mode, double* out, void* stream) {
    ORB_ENTRY("bs_orb_displacement");
    BS_REQUIRE(pt && counts && matches && match_counts && depth && K && out, "bs_orb_displacement: null pointer");
    BS_REQUIRE(batch >= 2, "bs_orb_displacement: batch %d frames (>= 2: pair p is frames p, p + 1)", batch);
    BS_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= 2147483647LL, "bs_orb_displacement: depth maps of %d x %d", W, H);
    BS_REQUIRE(mode == BS_ORB_ASSOC_REFERENCE || mode == BS_ORB_ASSOC_MATCHED, "bs_orb_displacement: mode %d", mode);
    hipLaunchKernelGGL(displacement_kernel, dim3((unsigned)(batch - 1)), dim3(ORB_THREADS), 0, st, pt, counts, matches, match_counts, depth, H, W, K[0], K[1],
                       K[2], K[3], mode == BS_ORB_ASSOC_MATCHED, out);
    BS_CHECK_LAUNCH();
    return BS_OK;
}
