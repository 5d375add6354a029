// The small dense solver shared by the polynomial-fit kernels (track_ops.hip: one fit per cycle of a track; polyfit_opt.hip: one fit per
// candidate weight vector of the weight search).  Device code only; include after wtk_kernels.h (kTrackMaxTimes / kTrackMaxCoef).
#pragma once
#include "wtk_kernels.h"

#include <cmath>

namespace wtk {

// Singular value decomposition of the n x K matrix A (n <= kTrackMaxTimes, K <= kTrackMaxCoef) by one-sided Jacobi (Hestenes)
// rotations of its COLUMNS, fp64: on return the columns of A are mutually orthogonal (A = U diag(s) as columns, s_p = |A[:,p]|)
// and V holds the accumulated rotations, so A_in = U diag(s) V^T.  Working on the matrix itself (not on the Gram matrix) keeps
// singular values down to ~eps * s_max resolved, which is what numpy's rcond = len(t) * eps needs.
// Two thresholds on the cosine |a_p . a_q| / (|a_p| |a_q|) of a column pair:
//   * a pair is ROTATED while its cosine exceeds 1e-16, i.e. down to the rounding noise of the dot product itself: at <= 16 x 8 a sweep is a few
//     hundred flops, so all 30 sweeps are the normal case, and on the degree-7 / 16-sample problems (scaled-Vandermonde condition ~1e9) the last
//     sub-eps rotations decide on which side of numpy's rcond cut-off the smallest singular value falls — stopping at a few eps (tried in round 4)
//     changed the reference's integer moves of tests/golden/polyfit_highdeg.json;
//   * CONVERGENCE is judged separately ("converged" must be distinguishable from "gave up") and in ABSOLUTE terms: the largest
//     |a_p . a_q| met in the last sweep run must be <= kJacobiConverged = 64 eps (16 samples x 4 eps) times the largest squared column norm,
//     i.e. the singular values are settled to ~eps * s_max — all a least-squares solve that drops everything below rcond * s_max can use.
//     (A relative test on the cosine cannot be met on these problems: a column of norm s_min carries the eps * s_max rounding noise of the
//     rotations that produced it, so its cosines stall near eps * s_max / s_min ~ 1e-7; tried first in round 4, it flagged the degree-7
//     goldens.)  The function returns false otherwise and the caller flags the sample instead of using the decomposition.
constexpr double kJacobiRotate = 1e-16;
constexpr double kJacobiConverged = 64.0 * 2.220446049250313e-16;
__device__ inline bool jacobi_svd_columns(double (&A)[kTrackMaxTimes][kTrackMaxCoef], double (&V)[kTrackMaxCoef][kTrackMaxCoef], int n, int K) {
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    double worst = 0.0, top = 0.0; // largest |a_p . a_q| and largest squared column norm met in the most recent sweep
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        worst = 0.0, top = 0.0;
        for (int p = 0; p < K; ++p)
            for (int q = p + 1; q < K; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int j = 0; j < n; ++j) alpha += A[j][p] * A[j][p], beta += A[j][q] * A[j][q], gamma += A[j][p] * A[j][q];
                top = fmax(top, fmax(alpha, beta));
                if (!(fabs(gamma) > kJacobiRotate * sqrt(alpha * beta)) || gamma == 0.0) continue; // orthogonal to the last bit (or a zero column)
                worst = fmax(worst, fabs(gamma));
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
                for (int j = 0; j < n; ++j) {
                    const double ap = A[j][p], aq = A[j][q];
                    A[j][p] = c * ap - sn * aq;
                    A[j][q] = sn * ap + c * aq;
                }
                for (int k = 0; k < K; ++k) {
                    const double vp = V[k][p], vq = V[k][q];
                    V[k][p] = c * vp - sn * vq;
                    V[k][q] = sn * vp + c * vq;
                }
            }
        if (!rotated) return true;
    }
    return worst <= kJacobiConverged * top;
}

} // namespace wtk
