// The per-lane DLT solve every triangulation kernel here shares (lt_triangulate_dlt and its backward, the algebraic tails, RANSAC's
// hypotheses, final solves and pinned starts), so that they solve the same system with the same instruction sequence: fp64 throughout.
// dlt_add_view: one view's two rows of A (multiview.py:131-132 / :159-161), w (x P[2,:] - P[r,:]), formed in fp64 from the fp32 matrix (the
// product of two fp32 values is exact in fp64; the reference rounds every step to fp32, which costs up to u32 |x P[2,:]| where the
// subtraction cancels) and rotated into the upper-triangular R of A = QR (Givens).  The solve works on R, i.e. on A itself as the
// reference's torch.svd(A) does: same right singular vectors, and the normal matrix A^T A would square A's condition number (pixel-space
// rows, far points, confidences down to 1e-5 reach kappa(A) ~ 1e8, where u64 kappa^2 exceeds what fp32 inputs can explain).
// INVARIANT callers rely on: a row of zeros (weight 0 with a finite point and matrix) leaves R untouched -- every a[k] == 0.0 takes the `continue` --
// so a view given weight 0 is, bit for bit, a view that is not there (multiview.triangulate_batch_of_points(view_mask=) masks views this way).
#pragma once
#include "lt_common.h"

namespace lt {

__device__ __forceinline__ void dlt_add_view(double (&R)[4][4], const float* __restrict__ P, const double x, const double y, const double w) {
    const double p[2] = {x, y};
    for (int r = 0; r < 2; ++r) {
        double a[4];
        for (int k = 0; k < 4; ++k) a[k] = ((double)P[8 + k] * p[r] - (double)P[4 * r + k]) * w;
        for (int k = 0; k < 4; ++k) {          // Givens: rotate the row into R
            if (a[k] == 0.0) continue;
            const double h = sqrt(R[k][k] * R[k][k] + a[k] * a[k]);
            const double cs = R[k][k] / h, sn = a[k] / h;
            R[k][k] = h;
            for (int m = k + 1; m < 4; ++m) {
                const double rk = R[k][m], am = a[m];
                R[k][m] = cs * rk + sn * am;
                a[m] = cs * am - sn * rk;
            }
        }
    }
}

// one-sided Jacobi SVD of R (its columns orthogonalised in place): right singular vectors in the columns of V, squared singular values
// (the eigenvalues of A^T A) in lam; returns the column of the smallest = the last right singular vector of A
__device__ __forceinline__ int dlt_svd(double (&U)[4][4], double (&V)[4][4], double (&lam)[4]) {
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 4; ++k) V[i][k] = i == k ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 4; ++p)
            for (int q = p + 1; q < 4; ++q) {
                double al = 0, be = 0, ga = 0;
                for (int k = 0; k < 4; ++k) { al += U[k][p] * U[k][p]; be += U[k][q] * U[k][q]; ga += U[k][p] * U[k][q]; }
                if (ga == 0.0 || !(fabs(ga) > 1e-15 * sqrt(al * be))) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                for (int k = 0; k < 4; ++k) {
                    const double up = U[k][p], uq = U[k][q];
                    U[k][p] = cs * up - sn * uq; U[k][q] = sn * up + cs * uq;
                    const double vp = V[k][p], vq = V[k][q];
                    V[k][p] = cs * vp - sn * vq; V[k][q] = sn * vp + cs * vq;
                }
            }
        if (!rotated) break;
    }
    int best = 0;
    for (int p = 0; p < 4; ++p) {
        lam[p] = U[0][p] * U[0][p] + U[1][p] * U[1][p] + U[2][p] * U[2][p] + U[3][p] * U[3][p];
        if (lam[p] < lam[best]) best = p;
    }
    return best;
}

// the DLT point from R, dehomogenised: X = v[:3] / v[3], v the last right singular vector
__device__ __forceinline__ void dlt_point(double (&R)[4][4], double (&X)[3]) {
    double V[4][4], lam[4];
    const int best = dlt_svd(R, V, lam);
    const double wv = V[3][best];
    X[0] = V[0][best] / wv; X[1] = V[1][best] / wv; X[2] = V[2][best] / wv;
}

}  // namespace lt
