// What sparse_features.hip (bs_orb_match, bs_orb_displacement) and loop_closure.hip (bs_orb_match_pairs, bs_orb_lift) share: the block scan,
// the 256-bit Hamming distance, the cross-checked match of one (query frame, train frame) pair and associate_depth's lookup.  One copy, so
// the consecutive-frame match and the match over a list of pairs run the same body and cannot drift apart.
#pragma once
#include "common.h"

namespace bs {
namespace {

constexpr int ORB_THREADS = 256;
constexpr int ORB_WAVES = ORB_THREADS / 64;
constexpr int ORB_KP = BS_ORB_MAX_FEATURES;

// exclusive prefix of v over the block's threads in thread order and the block's total (v may pack two 16-bit counters: no carry as long
// as each total stays below 65536).  lds: ORB_WAVES ints.
__device__ __forceinline__ int block_excl_scan(int v, int* lds, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < ORB_WAVES; ++i) {
        const int t = lds[i];
        if (i < w) base += t;
        tot += t;
    }
    total = tot;
    return base + inc - v;
}

__device__ __forceinline__ int hamming256(const u32x4& a0, const u32x4& a1, const u32x4& b0, const u32x4& b1) {
    const unsigned long long x0 = ((unsigned long long)(a0[1] ^ b0[1]) << 32) | (a0[0] ^ b0[0]);
    const unsigned long long x1 = ((unsigned long long)(a0[3] ^ b0[3]) << 32) | (a0[2] ^ b0[2]);
    const unsigned long long x2 = ((unsigned long long)(a1[1] ^ b1[1]) << 32) | (a1[0] ^ b1[0]);
    const unsigned long long x3 = ((unsigned long long)(a1[3] ^ b1[3]) << 32) | (a1[2] ^ b1[2]);
    return __popcll(x0) + __popcll(x1) + __popcll(x2) + __popcll(x3);
}

// The match of one pair by one block of ORB_THREADS threads: query = frame fq, train = frame ft of desc [frames, ORB_KP, 8] / counts
// [frames, BS_ORB_MAX_LEVELS + 1].  out [ORB_KP, 4] int32 = (queryIdx, trainIdx, distance, 0) in BFMatcher(NORM_HAMMING, crossCheck = True)
// + stable sort by distance order; *out_count = the number of matches.  A query maps to its lowest train index among equal distances (and
// a train to its lowest query).  LDS: 2 x 16 000 B of descriptors, read 16 bytes at a time, + 5 x 2 000 B of indices = 42 016 B.
__device__ __forceinline__ void orb_match_pair(const uint32_t* __restrict__ desc, const int* __restrict__ counts, int fq, int ft, int* __restrict__ out,
                                               int* __restrict__ out_count) {
    __shared__ u32x4 dq[ORB_KP * 2], dt[ORB_KP * 2];
    __shared__ int bt[ORB_KP], bd[ORB_KP], bq[ORB_KP], sq[ORB_KP], sd[ORB_KP];
    __shared__ int scan[ORB_WAVES];
    const int t = threadIdx.x;
    const int n1 = max(min(counts[fq * (BS_ORB_MAX_LEVELS + 1) + BS_ORB_MAX_LEVELS], ORB_KP), 0);
    const int n2 = max(min(counts[ft * (BS_ORB_MAX_LEVELS + 1) + BS_ORB_MAX_LEVELS], ORB_KP), 0);
    const u32x4* gq = reinterpret_cast<const u32x4*>(desc + (int64_t)fq * ORB_KP * 8);
    const u32x4* gt = reinterpret_cast<const u32x4*>(desc + (int64_t)ft * ORB_KP * 8);
    for (int i = t; i < 2 * n1; i += ORB_THREADS) dq[i] = gq[i];
    for (int i = t; i < 2 * n2; i += ORB_THREADS) dt[i] = gt[i];
    __syncthreads();
    for (int i = t; i < n1; i += ORB_THREADS) {             // the best train of every query, the lowest index among equals
        const u32x4 a0 = dq[2 * i], a1 = dq[2 * i + 1];
        int best = 1 << 30, arg = -1;
        for (int j = 0; j < n2; ++j) {
            const int d = hamming256(a0, a1, dt[2 * j], dt[2 * j + 1]);
            if (d < best) { best = d; arg = j; }
        }
        bt[i] = arg;
        bd[i] = best;
    }
    for (int j = t; j < n2; j += ORB_THREADS) {             // the best query of every train
        const u32x4 a0 = dt[2 * j], a1 = dt[2 * j + 1];
        int best = 1 << 30, arg = -1;
        for (int i = 0; i < n1; ++i) {
            const int d = hamming256(dq[2 * i], dq[2 * i + 1], a0, a1);
            if (d < best) { best = d; arg = i; }
        }
        bq[j] = arg;
    }
    __syncthreads();
    int M = 0;
    for (int base = 0; base < n1; base += ORB_THREADS) {    // the survivors of the cross-check in query order
        const int i = base + t;
        const int keep = (i < n1 && bt[i] >= 0 && bq[bt[i]] == i) ? 1 : 0;
        int tot;
        const int pos = M + block_excl_scan(keep, scan, tot);
        if (keep) {
            sq[pos] = i;
            sd[pos] = bd[i];
        }
        M += tot;
    }
    __syncthreads();
    for (int i = t; i < M; i += ORB_THREADS) {              // stable sort by distance: the rank by counting
        const int d = sd[i];
        int rank = 0;
        for (int j = 0; j < M; ++j) rank += (sd[j] < d) || (sd[j] == d && j < i);
        int* o = out + rank * 4;
        o[0] = sq[i];
        o[1] = bt[sq[i]];
        o[2] = d;
        o[3] = 0;
    }
    if (t == 0) *out_count = M;
}

// associate_depth's lookup (scaling_system.py:46-69): depth at (int(y), int(x)) -- truncation towards zero -- of a point inside the image
__device__ __forceinline__ bool depth_at(const float* __restrict__ depth, int H, int W, float x, float y, double& d) {
    if (!(x > -1.0f && x < (float)W && y > -1.0f && y < (float)H)) return false;
    d = (double)depth[(int)y * W + (int)x];
    return d != 0.0;
}

}  // namespace
}  // namespace bs
