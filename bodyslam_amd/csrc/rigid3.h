// The fp64 rigid-fit pieces the geometry kernels share, built on svd3.h: the 3 x 3 + 3 transform, the completion of an SVD to a proper
// rotation, Kabsch from sums, the SE(3) exponential and the left update of a 3 x 4 pose.  One copy each, so that "the same bits in every run"
// rests on one function, not on hand-copied ones staying alike.  The library is built with -ffp-contract=off: a result depends on the order
// of the operations alone, and every parenthesis (and every `acc = 0; acc += ...` start, which turns -0 into +0) below is part of the
// contract with the numpy statements under tests/.
#pragma once
#include "svd3.h"

namespace bs {

// x -> r x + t, r row-major: the top three rows of a 4 x 4 pose (the bottom row is taken as [0 0 0 1])
struct Rigid3 {
    double r[9], t[3];
};
__device__ __forceinline__ Rigid3 rigid3_identity() {
    Rigid3 a;
#pragma unroll
    for (int i = 0; i < 9; ++i) a.r[i] = (i % 4 == 0) ? 1.0 : 0.0;
    a.t[0] = a.t[1] = a.t[2] = 0.0;
    return a;
}
__device__ __forceinline__ Rigid3 rigid3_load(const double* __restrict__ p) {           // rows 0-2 of a row-major 4 x 4
    Rigid3 a;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) a.r[i * 3 + j] = p[i * 4 + j];
        a.t[i] = p[i * 4 + 3];
    }
    return a;
}
__device__ __forceinline__ void rigid3_store(const Rigid3& a, double* __restrict__ p) {   // rows 0-2; the bottom row is the caller's
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) p[i * 4 + j] = a.r[i * 3 + j];
        p[i * 4 + 3] = a.t[i];
    }
}
// a o b: (a.r b.r, a.r b.t + a.t)
__device__ __forceinline__ Rigid3 rigid3_compose(const Rigid3& a, const Rigid3& b) {
    Rigid3 c;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) c.r[i * 3 + j] = (a.r[i * 3] * b.r[j] + a.r[i * 3 + 1] * b.r[3 + j]) + a.r[i * 3 + 2] * b.r[6 + j];
        c.t[i] = ((a.r[i * 3] * b.t[0] + a.r[i * 3 + 1] * b.t[1]) + a.r[i * 3 + 2] * b.t[2]) + a.t[i];
    }
    return c;
}

// fl32(((a0 s0 + a1 s1) + a2 s2) + a3) per row of the row-major 3 x 4 A: fp64, rounded once
__device__ __forceinline__ void affine_point_f32(const double* __restrict__ A, double s0, double s1, double s2, float (&o)[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = (float)(((A[4 * r] * s0 + A[4 * r + 1] * s1) + A[4 * r + 2] * s2) + A[4 * r + 3]);
}

// the index of the smallest singular value; ties go to the last index, where a descending LAPACK ordering leaves the flipped direction
__device__ __forceinline__ int svd3_smallest(const double (&d)[3]) {
    int kmin = 0;
    if (d[1] <= d[kmin]) kmin = 1;
    if (d[2] <= d[kmin]) kmin = 2;
    return kmin;
}
// column kmin <- the cross product of the other two, (a, b, kmin) a cyclic order: for an orthonormal pair that makes det(M) = +1
__device__ __forceinline__ void svd3_complete_column(double (&M)[3][3], int kmin) {
    const int a = (kmin + 1) % 3, b = (kmin + 2) % 3;
    M[0][kmin] = M[1][a] * M[2][b] - M[2][a] * M[1][b];
    M[1][kmin] = M[2][a] * M[0][b] - M[0][a] * M[2][b];
    M[2][kmin] = M[0][a] * M[1][b] - M[1][a] * M[0][b];
}
// out (row-major 3 x 3) = U diag(S) V^T
__device__ __forceinline__ void svd3_usvt(const double (&U)[3][3], const double (&S)[3], const double (&V)[3][3], double* out) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double acc = 0;
            for (int k = 0; k < 3; ++k) acc += U[i][k] * S[k] * V[j][k];
            out[i * 3 + j] = acc;
        }
}

// Kabsch from the sums over n pairs (p, q): s[0..2] = sum p, s[3..5] = sum q, s[6 + 3 i + j] = sum q_i p_j.  S = sum q p^T - (sum q) mean(p)^T
// is the (summed) cross-covariance; with S = U diag(d) V^T, R = U V^T after the columns of U and V that belong to the smallest singular value
// are replaced by the cross product of the other two: for full rank that is the det sign fix on the smallest singular direction, for the
// rank 2 of a three-point sample (where the Jacobi leaves that column of U undetermined) it completes the bases.  t = mean q - R mean p.
// da, db: the two other singular values.  The fit means something only when both are positive and finite; every caller tests them by its own
// rule before it uses g (collinear or coincident points fail any of them).
struct KabschFit {
    Rigid3 g;
    double da, db;
};
__device__ inline KabschFit kabsch_from_sums(const double (&s)[15], double n) {
    double S[3][3], U[3][3], V[3][3], d[3];
    const double mp[3] = {s[0] / n, s[1] / n, s[2] / n}, mq[3] = {s[3] / n, s[4] / n, s[5] / n};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) S[i][j] = s[6 + 3 * i + j] - s[3 + i] * mp[j];
    svd3_jacobi(S, U, d, V);
    const int kmin = svd3_smallest(d);
    svd3_complete_column(U, kmin);
    svd3_complete_column(V, kmin);
    KabschFit f;
    f.da = d[(kmin + 1) % 3];
    f.db = d[(kmin + 2) % 3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) f.g.r[i * 3 + j] = (U[i][0] * V[j][0] + U[i][1] * V[j][1]) + U[i][2] * V[j][2];
    for (int i = 0; i < 3; ++i) f.g.t[i] = mq[i] - ((f.g.r[i * 3] * mp[0] + f.g.r[i * 3 + 1] * mp[1]) + f.g.r[i * 3 + 2] * mp[2]);
    return f;
}

// the SE(3) exponential of the left twist (omega = d[0:3], nu = d[3:6]); below th = 1e-12: R = I + Wx, V = I + Wx / 2 (the oracle's
// small-angle branch)
__device__ inline void se3_exp(const double (&d)[6], Rigid3& g) {
    const double wx = d[0], wy = d[1], wz = d[2];
    const double th = sqrt(wx * wx + wy * wy + wz * wz);
    const double Wx[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
    double W2[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W2[i][j] = Wx[i][0] * Wx[0][j] + Wx[i][1] * Wx[1][j] + Wx[i][2] * Wx[2][j];
    double a, b, c;
    if (th < 1e-12) {
        a = 1.0; b = 0.5; c = 0.0;
    } else {
        a = sin(th) / th;
        b = (1.0 - cos(th)) / (th * th);
        c = (th - sin(th)) / (th * th * th);
    }
    for (int i = 0; i < 3; ++i) {
        double V[3];
        for (int j = 0; j < 3; ++j) {
            const double I = i == j ? 1.0 : 0.0;
            g.r[i * 3 + j] = I + a * Wx[i][j] + (th < 1e-12 ? 0.0 : b * W2[i][j]);
            V[j] = I + b * Wx[i][j] + c * W2[i][j];
        }
        g.t[i] = V[0] * d[3] + V[1] * d[4] + V[2] * d[5];
    }
}

// T <- [g.r | g.t] T on a row-major 3 x 4
__device__ inline void left_apply(const Rigid3& g, double* T) {
    double N[12];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 4; ++j) N[4 * i + j] = (g.r[i * 3] * T[j] + g.r[i * 3 + 1] * T[4 + j]) + g.r[i * 3 + 2] * T[8 + j];
        N[4 * i + 3] += g.t[i];
    }
    for (int i = 0; i < 12; ++i) T[i] = N[i];
}

}  // namespace bs
