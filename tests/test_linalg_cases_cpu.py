"""tests/linalg_cases.py without a device: float64 LAPACK factorises every matrix tests/test_gpu_linalg.py hands the library (so no test there needs a skip
path), the ill-conditioned family has the condition numbers it is named after, and the mode table stays inside the sizes it was pruned from."""
import numpy as np
import pytest

import linalg_cases as LC


@pytest.mark.parametrize('c', LC.ILL_C)
@pytest.mark.parametrize('n', LC.ILL_N)
def test_lapack_factorises_the_ill_conditioned_family(n, c):
    for b in range(2):
        A = LC.ill_conditioned(n, c, b)
        assert np.array_equal(A, A.T)
        assert 0.5 * 10.0 ** c <= np.linalg.cond(A) <= 2.0 * 10.0 ** c
        r_fac, r_inv = LC.lapack_residuals(n, c, b)          # asserts info == 0 of dpotrf and dpotri
        assert 0 < r_fac <= 1e-14 and 0 < r_inv <= 1e-5


def test_lapack_factorises_the_well_conditioned_family():
    for n in sorted({m[0] for m in LC.MODES}):
        for b in range(2):
            L, Ainv, logdet = LC.well_conditioned_ref(n, b)
            assert np.isfinite(L).all() and np.isfinite(Ainv).all() and np.isfinite(logdet)


def test_mode_table():
    assert {m[0] for m in LC.MODES} == {1, 129, 300, 640, 1100, 1537}
    assert all(m[1] in (1, 2) and set(m[2:]) <= {0, 1} for m in LC.MODES) and len(set(LC.MODES)) == len(LC.MODES)
