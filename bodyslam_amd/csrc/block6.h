// 6 x 6 blocks in fp64, row-major: the Cholesky factor and the two triangular solves the pose graph (posegraph.hip) and the point-to-plane
// ICP step (icp.hip) share.  Every sum runs over ascending k.  __host__ __device__, so a host program can run the same arithmetic.
#pragma once
#include <math.h>

namespace bs {

// A = L L^T, L lower (the lower triangle of A is read); a pivot that is not positive gives a diagonal entry that is NaN or zero, which the
// caller sees
__host__ __device__ inline void chol6(const double* A, double* L) {
    for (int i = 0; i < 36; ++i) L[i] = 0.0;
    for (int j = 0; j < 6; ++j) {
        double s = A[j * 6 + j];
        for (int k = 0; k < j; ++k) s -= L[j * 6 + k] * L[j * 6 + k];
        const double d = sqrt(s);
        L[j * 6 + j] = d;
        for (int i = j + 1; i < 6; ++i) {
            double a = A[i * 6 + j];
            for (int k = 0; k < j; ++k) a -= L[i * 6 + k] * L[j * 6 + k];
            L[i * 6 + j] = a / d;
        }
    }
}

// Y = L^-1 B, B and Y [6, cols]
__host__ __device__ inline void lsolve6(const double* L, const double* B, int cols, double* Y) {
    for (int c = 0; c < cols; ++c)
        for (int i = 0; i < 6; ++i) {
            double a = B[i * cols + c];
            for (int k = 0; k < i; ++k) a -= L[i * 6 + k] * Y[k * cols + c];
            Y[i * cols + c] = a / L[i * 6 + i];
        }
}

// x <- L^-T x, in place
__host__ __device__ inline void ltsolve6(const double* L, double* x) {
    for (int i = 5; i >= 0; --i) {
        double a = x[i];
        for (int j = i + 1; j < 6; ++j) a -= L[j * 6 + i] * x[j];
        x[i] = a / L[i * 6 + i];
    }
}

}  // namespace bs
