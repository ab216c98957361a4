// The three-point RANSAC pieces that loop_closure.hip and global_registration.hip share: the counter-based draw, the three distinct indices,
// the residual and the Kabsch fit of one sample with its rank test.  One copy each: both files draw the same numbers and fit the same bits.
// RANSAC: Fischler & Bolles 1981; the fit: Kabsch 1976 / Arun, Huang & Blostein 1987 (rigid3.h).  The statements are
// tests/_loop_closure_ref.py and tests/_global_registration_ref.py.  Plain C++ apart from rigid3.h's fit: integer arithmetic and fp64 in a
// fixed order (the library is built with -ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#include "rigid3.h"

namespace bs {

constexpr double RANSAC3_RANK_EPS = 1e-12;  // m^2: a sample / inlier set whose (summed) cross-covariance has a second singular value below this is collinear

// splitmix64's finaliser over a counter: draw `draw` (0, 1, 2) of hypothesis h of pair `pair`; the high 32 bits are the draw
__host__ __device__ __forceinline__ uint32_t loop_draw(uint64_t seed, uint32_t pair, uint32_t h, uint32_t draw) {
    uint64_t z = (seed ^ ((uint64_t)pair * 0xD6E8FEB86659FD93ull)) + 0x9E3779B97F4A7C15ull * ((uint64_t)h * 3ull + draw + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (uint32_t)(z >> 32);
}
// three distinct indices below C (C >= 3): i0 = r0 % C, i1 = r1 % (C - 1), i2 = r2 % (C - 2), each shifted past the earlier picks
__host__ __device__ __forceinline__ void loop_sample(uint64_t seed, uint32_t pair, uint32_t h, int C, int (&idx)[3]) {
    const int i0 = (int)(loop_draw(seed, pair, h, 0) % (uint32_t)C);
    int i1 = (int)(loop_draw(seed, pair, h, 1) % (uint32_t)(C - 1));
    int i2 = (int)(loop_draw(seed, pair, h, 2) % (uint32_t)(C - 2));
    if (i1 >= i0) ++i1;
    const int lo = i0 < i1 ? i0 : i1, hi = i0 < i1 ? i1 : i0;
    if (i2 >= lo) ++i2;
    if (i2 >= hi) ++i2;
    idx[0] = i0; idx[1] = i1; idx[2] = i2;
}

// |R p + t - q|^2
__device__ __forceinline__ double residual2(const Rigid3& g, double px, double py, double pz, double qx, double qy, double qz) {
    const double ex = (((g.r[0] * px + g.r[1] * py) + g.r[2] * pz) + g.t[0]) - qx;
    const double ey = (((g.r[3] * px + g.r[4] * py) + g.r[5] * pz) + g.t[1]) - qy;
    const double ez = (((g.r[6] * px + g.r[7] * py) + g.r[8] * pz) + g.t[2]) - qz;
    return (ex * ex + ey * ey) + ez * ez;
}

// one pair (p, q) into Kabsch's sums (rigid3.h kabsch_from_sums)
__device__ __forceinline__ void kabsch_add(double (&s)[15], const double (&pp)[3], const double (&qq)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        s[i] += pp[i];
        s[3 + i] += qq[i];
#pragma unroll
        for (int j = 0; j < 3; ++j) s[6 + 3 * i + j] += qq[i] * pp[j];
    }
}

// Kabsch over a three-point sample, the pairs added in the order 0, 1, 2.  false: the second singular value of the sample's cross-covariance
// is below RANSAC3_RANK_EPS (collinear or coincident points); g is then left alone.
__device__ __forceinline__ bool sample_fit3(const double (&p)[3][3], const double (&q)[3][3], Rigid3& g) {
    double s[15];
#pragma unroll
    for (int k = 0; k < 15; ++k) s[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) kabsch_add(s, p[k], q[k]);
    const KabschFit f = kabsch_from_sums(s, 3.0);
    if (!(fmin(f.da, f.db) >= RANSAC3_RANK_EPS)) return false;
    g = f.g;
    return true;
}

}  // namespace bs
