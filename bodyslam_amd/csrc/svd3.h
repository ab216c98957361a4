// The 3x3 SVD of every fp64 geometry kernel: a one-sided Jacobi.  One copy, so the callers cannot drift apart; the arithmetic is the pose
// chain's of old, operation for operation.  rigid3.h builds the rotations and rigid fits on it.
#pragma once
#include <math.h>

namespace bs {

// M = U diag(s) V^T.  The singular values come out in no particular order; a column of U whose singular value is exactly zero is zero.
__device__ inline void svd3_jacobi(const double (&M)[3][3], double (&U)[3][3], double (&s)[3], double (&V)[3][3]) {
    // one-sided Jacobi on the columns of A = M: A V = U S
    double A[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            A[i][j] = M[i][j];
            V[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 40; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int i = 0; i < 3; ++i) {
                    alpha += A[i][p] * A[i][p];
                    beta += A[i][q] * A[i][q];
                    gamma += A[i][p] * A[i][q];
                }
                off = fmax(off, fabs(gamma) / sqrt(alpha * beta + 1e-300));
                if (fabs(gamma) <= 1e-300) continue;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                for (int i = 0; i < 3; ++i) {
                    const double ap = A[i][p], aq = A[i][q];
                    A[i][p] = cs * ap - sn * aq;
                    A[i][q] = sn * ap + cs * aq;
                    const double vp = V[i][p], vq = V[i][q];
                    V[i][p] = cs * vp - sn * vq;
                    V[i][q] = sn * vp + cs * vq;
                }
            }
        if (off < 1e-17) break;
    }
    for (int j = 0; j < 3; ++j) {
        s[j] = sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
        const double inv = s[j] > 0 ? 1.0 / s[j] : 0.0;
        for (int i = 0; i < 3; ++i) U[i][j] = A[i][j] * inv;
    }
}

__device__ inline double det3(const double (&X)[3][3]) {
    return X[0][0] * (X[1][1] * X[2][2] - X[1][2] * X[2][1]) - X[0][1] * (X[1][0] * X[2][2] - X[1][2] * X[2][0]) +
           X[0][2] * (X[1][0] * X[2][1] - X[1][1] * X[2][0]);
}

}  // namespace bs
