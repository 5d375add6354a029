"""Exact weighted least-squares polynomial extrapolation, the truth the device Polyfit kernel and numpy are both measured against.

The inputs of a fit (integer sample times, float64 weights, float64 head centres) are exact rationals, so the normal equations
(A^T A) c = A^T (w y), A[j][p] = w_j t_j^p, can be solved without any rounding in `fractions.Fraction`.  A^T A depends only on the times and
weights: for one (times, weights, degree, t_eval) the prediction is a fixed linear form  sum_j r_j y_j  of the samples, whose rational
coefficients r_j are computed once; a cycle's truth is that sum in exact arithmetic, rounded once to float64.  Full-rank problems only."""
from __future__ import annotations

from fractions import Fraction

import numpy as np
from numpy.polynomial import polynomial as poly


def exact_form(times, weights, degree: int, t_eval) -> list:
    """r_j (Fractions) with  polyval(t_eval, weighted LSQ fit through (t_j, y_j)) = sum_j r_j y_j."""
    t = [Fraction(int(v)) for v in times]
    w = [Fraction(float(v)) for v in weights]
    K = degree + 1
    assert len(t) == len(w) >= K
    G = [[sum(wj * wj * tj ** (p + q) for tj, wj in zip(t, w)) for q in range(K)] for p in range(K)]
    z = [Fraction(t_eval) ** p for p in range(K)]  # solve G z = e(t_eval); G is symmetric, so e^T G^-1 = z^T
    for c in range(K):  # Gauss-Jordan, exact
        piv = next(r for r in range(c, K) if G[r][c] != 0)  # StopIteration = rank deficient: not a problem this module is for
        G[c], G[piv], z[c], z[piv] = G[piv], G[c], z[piv], z[c]
        inv = 1 / G[c][c]
        G[c] = [v * inv for v in G[c]]
        z[c] *= inv
        for r in range(K):
            if r != c and G[r][c] != 0:
                f = G[r][c]
                G[r] = [a - f * b for a, b in zip(G[r], G[c])]
                z[r] -= f * z[c]
    return [wj * wj * sum(z[p] * tj ** p for p in range(K)) for tj, wj in zip(t, w)]


def exact_predict(form, y) -> float:
    """sum_j r_j y_j for float64 samples y, exact, rounded once."""
    return float(sum(r * Fraction(float(v)) for r, v in zip(form, y)))


def numpy_predict(times, weights, degree: int, t_eval, y) -> np.ndarray:
    """What the reference's PolyfitController computes: numpy's polyfit (scaled Vandermonde, SVD least squares) and polyval."""
    return poly.polyval(t_eval, poly.polyfit(np.asarray(times, float), np.asarray(y, float), deg=degree, w=np.asarray(weights, float)))


def scaled_singular_values(times, weights, degree: int) -> np.ndarray:
    """Singular values of the matrix numpy's polyfit hands to lstsq: the weighted Vandermonde with unit-norm columns."""
    lhs = poly.polyvander(np.asarray(times, float), degree) * np.asarray(weights, float)[:, None]
    return np.linalg.svd(lhs / np.sqrt(np.square(lhs).sum(0)), compute_uv=False)


def well_posed(times, weights, degree: int) -> bool:
    """Every singular value at least 1e3 x numpy's cut-off rcond * s_max (rcond = len(t) * eps): no direction is near truncation, so numpy
    and any other backward-stable solver answer the same full-rank problem."""
    if degree + 1 > len(times):
        return False
    s = scaled_singular_values(times, weights, degree)
    return bool(s.min() >= 1e3 * len(times) * np.finfo(float).eps * s.max())


# (times, weights) the device kernel is checked on, and the degrees at which each is well posed (test_polyfit_ref.py asserts that this is
# exactly the set `well_posed` admits among degrees 0-7: six samples cannot determine seven or eight coefficients)
TIME_SETS = {
    "six": ([-9, -6, -3, 0, 2, 4], [1, 1, 2, 3, 4, 5.0]),
    "sixteen": (list(range(-15, 1)), [1.0] * 16),
    "unsorted": ([2, -9, -20, 0, -6, -14, 4, -2, -17, -11, -4, 1, -7, -23, -1, -12], [0.5 + ((7 * j) % 16) / 4 for j in range(16)]),
}
MATRIX = [("six", d) for d in range(6)] + [("sixteen", d) for d in range(8)] + [("unsorted", d) for d in range(8)]
