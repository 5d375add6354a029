"""CPU: the exact Polyfit truth (tests/harness/polyfit_ref.py) and the matrix the device kernel is checked on."""
from fractions import Fraction

import numpy as np

from harness import polyfit_ref as pr


def test_matrix_is_exactly_the_well_posed_pairs():
    admitted = [(name, d) for name, (t, w) in pr.TIME_SETS.items() for d in range(8) if pr.well_posed(t, w, d)]
    assert admitted == pr.MATRIX and len(admitted) == 22
    for t, w in pr.TIME_SETS.values():
        assert len(t) == len(w) <= 16 and len(set(t)) == len(t)
    t, w = pr.TIME_SETS["unsorted"]
    assert t != sorted(t) and len(set(w)) > 4


def test_exact_form_reproduces_a_polynomial_and_agrees_with_numpy():
    rng = np.random.default_rng(0)
    for name, deg in pr.MATRIX:
        t, w = pr.TIME_SETS[name]
        form = pr.exact_form(t, w, deg, 12)
        # a polynomial of that degree with integer coefficients is extrapolated exactly, whatever the weights
        c = [int(v) for v in rng.integers(-3, 4, size=deg + 1)]
        y = [float(sum(ck * tj ** k for k, ck in enumerate(c))) for tj in t]
        assert sum(r * Fraction(v) for r, v in zip(form, y)) == sum(ck * 12 ** k for k, ck in enumerate(c)), (name, deg)
        # noisy samples: numpy's solve of the same problem is the same number to the 1e-6 px the ragged-track GPU test allows numpy itself
        y = 700 + np.cumsum(rng.normal(0.5, 0.3, size=len(t)))
        assert abs(pr.numpy_predict(t, w, deg, 12, y) - pr.exact_predict(form, y)) <= 1e-6, (name, deg)
