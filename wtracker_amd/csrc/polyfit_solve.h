// The one place that knows the polynomial fit: numpy.polynomial.polynomial.polyfit(t, ., deg, w=weights) restated — weighted Vandermonde matrix with
// columns scaled to unit norm, minimum-norm least squares (numpy.linalg.lstsq = LAPACK gelsd: singular values <= rcond * s_max are treated as zero,
// rcond = len(t) * eps) — in three steps that every fitting kernel calls:
//   polyfit_factor    scl, the scaled matrix, its SVD, the squared singular values         (what depends on the sample times and the weights only)
//   polyfit_keeps     numpy's cut for one singular direction
//   polyfit_eval_axes solve for both axes' coefficients and evaluate c / scl at t_eval     (what depends on the centres)
// Callers: track_ops.hip (one fit per cycle of a track: factor + eval), polyfit_opt.hip (one fit per candidate weight vector: factor, then its own linear
// functional), replay_targets.hip (one factor per (sample set, particle) kept in scratch, one eval per (cycle, particle) over that record).  The library is built
// with -ffp-contract=off, so equal inputs give equal bits through every caller.  Device code only; kTrackMaxTimes / kTrackMaxCoef come from wtk_kernels.h.
#pragma once
#include "wtk_kernels.h"

#include <cmath>

namespace wtk {

constexpr double kF64Eps = 2.220446049250313e-16; // numpy.finfo(float64).eps

// Singular value decomposition of the n x K matrix A (n <= kTrackMaxTimes, K <= kTrackMaxCoef) by one-sided Jacobi (Hestenes)
// rotations of its COLUMNS, fp64: on return the columns of A are mutually orthogonal (A = U diag(s) as columns, s_p = |A[:,p]|)
// and V holds the accumulated rotations, so A_in = U diag(s) V^T.  Working on the matrix itself (not on the Gram matrix) keeps
// singular values down to ~eps * s_max resolved, which is what numpy's rcond = len(t) * eps needs (an eigen-decomposition of the Gram
// matrix, which round 2 used, only resolves singular-value ratios down to ~3e-7 and truncated directions numpy keeps at degree >= 4-5
// over tens of frames).
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
constexpr double kJacobiConverged = 64.0 * kF64Eps;
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

// What a fit of n samples with K coefficients is, before any data: L the scaled weighted Vandermonde matrix L[j][p] = w_j t_j^p / scl_p with its columns
// rotated orthogonal (L = U diag(s)), V the rotations, s2[e] = s_e^2.
struct PolyfitFactor {
    double scl[kTrackMaxCoef];
    double L[kTrackMaxTimes][kTrackMaxCoef];
    double V[kTrackMaxCoef][kTrackMaxCoef];
    double s2[kTrackMaxCoef], s2max;
};

// tt[0..n), ww[0..n): the times and weights of the samples that take part (the caller compacts).  False when the SVD did not converge (never seen): the
// caller reports "no fit" rather than a silently wrong one; s2 and s2max are not set then.
__device__ inline bool polyfit_factor(PolyfitFactor &f, const double *tt, const double *ww, int n, int K) {
    for (int p = 0; p < K; ++p) f.scl[p] = 0.0;
    for (int j = 0; j < n; ++j) {
        double tp = 1.0; // t^p by repeated multiplication, as numpy's vander
        for (int p = 0; p < K; ++p) {
            const double v = ww[j] * tp;
            f.scl[p] += v * v;
            tp *= tt[j];
        }
    }
    for (int p = 0; p < K; ++p) f.scl[p] = f.scl[p] > 0.0 ? sqrt(f.scl[p]) : 1.0;
    for (int j = 0; j < n; ++j) {
        double tp = 1.0;
        for (int p = 0; p < K; ++p) f.L[j][p] = ww[j] * tp / f.scl[p], tp *= tt[j];
    }
    if (!jacobi_svd_columns(f.L, f.V, n, K)) return false;
    f.s2max = 0.0;
    for (int e = 0; e < K; ++e) {
        double q = 0.0;
        for (int j = 0; j < n; ++j) q += f.L[j][e] * f.L[j][e];
        f.s2[e] = q;
        f.s2max = fmax(f.s2max, q);
    }
    return true;
}

// numpy's cut: a direction with s_e <= rcond * s_max, rcond = len(x) * finfo(float64).eps, is null space and the minimum-norm solution leaves it at zero
__device__ __forceinline__ bool polyfit_keeps(double s2e, double s2max, int n) {
    const double rcond = (double)n * kF64Eps;
    return s2e > rcond * rcond * s2max;
}

// The factor as the solve reads it, wherever it lives: PolyfitLocal over a factor in the thread's own memory, PopRecordView (replay_targets.hip) over a record in
// global scratch.  A view has L(j, e), V(q, e), s2(e), scl(q) and w(j), the compacted weight of sample j.
struct PolyfitLocal {
    const PolyfitFactor &f;
    const double *ww;
    __device__ __forceinline__ double L(int j, int e) const { return f.L[j][e]; }
    __device__ __forceinline__ double V(int q, int e) const { return f.V[q][e]; }
    __device__ __forceinline__ double s2(int e) const { return f.s2[e]; }
    __device__ __forceinline__ double scl(int q) const { return f.scl[q]; }
    __device__ __forceinline__ double w(int j) const { return ww[j]; }
};

// Coefficients of both axes from the centres px, py [n] and polyval (Horner, highest power first) of c / scl at t_eval.  The loops over the coefficients are
// unrolled to kTrackMaxCoef under q < K guards, so that cx / cy stay in registers when the factor is read from global memory; s2max is taken again from the
// s2 values in index order, which is how polyfit_factor found it.
template <typename View>
__device__ __forceinline__ void polyfit_eval_axes(const View &f, const double *px, const double *py, int n, int K, double t_eval, double &x, double &y) {
    double s2max = 0.0;
    for (int e = 0; e < K; ++e) s2max = fmax(s2max, f.s2(e));
    double cx[kTrackMaxCoef], cy[kTrackMaxCoef];
#pragma unroll
    for (int q = 0; q < kTrackMaxCoef; ++q) cx[q] = cy[q] = 0.0;
    for (int e = 0; e < K; ++e) {
        const double s2e = f.s2(e);
        if (!polyfit_keeps(s2e, s2max, n)) continue;
        double dx = 0.0, dy = 0.0; // (u_e . rhs) / s_e = (L_rot[:,e] . rhs) / s_e^2
        for (int j = 0; j < n; ++j) {
            const double l = f.L(j, e), w = f.w(j);
            dx += l * (w * px[j]), dy += l * (w * py[j]);
        }
        dx /= s2e, dy /= s2e;
#pragma unroll
        for (int q = 0; q < kTrackMaxCoef; ++q)
            if (q < K) {
                const double v = f.V(q, e);
                cx[q] += v * dx, cy[q] += v * dy;
            }
    }
    x = 0.0, y = 0.0;
#pragma unroll
    for (int q = kTrackMaxCoef - 1; q >= 0; --q)
        if (q < K) {
            const double s = f.scl(q);
            if (q == K - 1)
                x = cx[q] / s, y = cy[q] / s;
            else
                x = cx[q] / s + x * t_eval, y = cy[q] / s + y * t_eval;
        }
}

} // namespace wtk
