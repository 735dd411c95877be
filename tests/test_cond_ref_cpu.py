"""The references of the posterior conditioned on extra rows (tests/cond_ref.py) checked on the CPU, in long double: the closed form of the rank-m
update against the refit on the statistics with the rows added, the properties the device's bounds lean on (S >= I, reduction >= 0), conditioning
in two halves against conditioning at once, and the condition that keeps test 1 of tests/test_gpu_condition.py sharp at its seeds."""
import numpy as np
import pytest

import cond_ref as CR
import predict_ref as R
import test_gpu_score as TG

LD = R.LD


class _Model(object):
    """test_gpu_score._model of a shape with fixed embeddings and its float64 statistics, built once per shape"""

    def __init__(self, shape, alpha_scale):
        N, M, Q, D = shape
        self.shape = shape
        self.d = d = TG._model(N, D, M, Q, 'A', seed=CR.model_seed(shape))
        d['alpha'] = d['alpha'] * alpha_scale
        self.Psi2, self.C = R.statistics(d['Z'], d['sf2'], d['alpha'], d['Y'], d['X_mu'], d['X_S'])
        self.tol = TG._tol(d, M, self.Psi2)
        self.g = (d['Z'], d['sf2'], d['alpha'], d['beta'])


@pytest.fixture(scope='module')
def models():
    made = {}

    def get(shape, alpha_scale=1.0):
        if (shape, alpha_scale) not in made:
            made[shape, alpha_scale] = _Model(shape, alpha_scale)
        return made[shape, alpha_scale]
    return get


def _rel(got, want, scale):
    return float(np.max(np.abs(got - want) / scale))


@pytest.mark.parametrize('m', CR.MS)
@pytest.mark.parametrize('shape', CR.SHAPES)
@pytest.mark.parametrize('alpha_scale', [8.0, 1.0])
def test_closed_form_is_the_refit(models, shape, m, alpha_scale):
    """mean' and var' of the two references agree, relative to max(1, |mean'|) and to sf2; S >= I; reduction >= 0.
    alpha_scale 8: the models of the device test with eight times the inverse squared lengthscale, cond(Kmm + beta Psi2) < 1e3, where two
    long-double evaluations (eps 1.1e-19) can agree to 1e-15, and must: the algebra is pinned there (measured 1e-17).
    alpha_scale 1: the models of the device test as they are, cond(Kmm + beta Psi2) = 2.4e7 and 5.3e7: the forward error of a long-double
    Cholesky solve is eps cond = 3e-12 and 6e-12 there, the two references agree to that (measured: mean 4e-13, var 5e-15), and the bound of
    test 1 on var' is below 1e-3 of the smallest var' at these seeds."""
    mo = models(shape, alpha_scale)
    N, M, Q, D = shape
    K = R.L.rbf_gram(mo.d['Z'], mo.d['sf2'], mo.d['alpha'])
    agree = 1e-15 if alpha_scale == 8.0 else float(np.finfo(LD).eps) * np.linalg.cond(K + mo.d['beta'] * mo.Psi2)
    Xc, Yc, X = CR.cond_inputs(Q, D, m, 300)
    ref = CR.cond_closed_form(*mo.g, mo.Psi2, mo.C, Xc, Yc, X)
    mean, var = CR.cond_refit(*mo.g, mo.Psi2, mo.C, Xc, Yc, X)
    em = _rel(ref['mean_c'], mean, np.maximum(1.0, np.abs(mean)))
    ev = _rel(ref['var_c'], var, LD(mo.d['sf2']))
    lam = np.linalg.eigvalsh(np.asarray(ref['S'], dtype=np.float64))[0]
    b_mean, b_var, b_red = CR.cond_bounds(ref, mo.tol, mo.d['sf2'], mo.d['beta'], M)
    vmin = float(np.min(ref['var_c']))
    print('shape %s m %d: closed form against refit mean %.3g var %.3g; smallest eigenvalue of S %.17g; reduction in [%.3g, %.3g]; bound on var\' '
          '%.3g against the smallest var\' %.3g (ratio %.3g); bound on mean\' %.3g'
          % (shape, m, em, ev, lam, float(ref['reduction'].min()), float(ref['reduction'].max()), b_var.max(), vmin, b_var.max() / vmin, b_mean.max()))
    assert em <= agree and ev <= agree, (em, ev, agree)
    assert lam >= 1.0 - 4 * m * np.finfo(float).eps          # >= 1 up to the rounding of the float64 eigenvalue routine
    assert np.all(ref['reduction'] >= 0) and np.all(ref['var_c'] <= ref['var'])
    if alpha_scale == 1.0:
        assert b_var.max() < 1e-3 * vmin


@pytest.mark.parametrize('m', [5, 129])
def test_two_halves_are_the_whole(models, m):
    """Conditioning on the first rows by way of the statistics and on the rest by the closed form is conditioning on all of them at once."""
    shape = CR.SHAPES[0]
    mo = models(shape, 8.0)
    N, M, Q, D = shape
    Xc, Yc, X = CR.cond_inputs(Q, D, m, 300)
    Z, sf2, alpha, beta = mo.g
    h = m // 2
    kc = R.L.psi1(np.asarray(Z, dtype=LD), LD(sf2), np.asarray(alpha, dtype=LD), np.asarray(Xc[:h], dtype=LD), np.zeros((h, Q), dtype=LD))
    Psi2h = np.asarray(mo.Psi2, dtype=LD) + kc.T.dot(kc)
    Ch = np.asarray(mo.C, dtype=LD) + kc.T.dot(np.asarray(Yc[:h], dtype=LD))
    whole = CR.cond_closed_form(*mo.g, mo.Psi2, mo.C, Xc, Yc, X)
    halves = CR.cond_closed_form(*mo.g, Psi2h, Ch, Xc[h:], Yc[h:], X)
    assert _rel(halves['mean_c'], whole['mean_c'], np.maximum(1.0, np.abs(whole['mean_c']))) <= 1e-15
    assert _rel(halves['var_c'], whole['var_c'], LD(sf2)) <= 1e-15


def test_a_query_on_a_conditioning_row_is_known_to_the_noise(models):
    """var' of f at a conditioning input is below 1/beta, and a duplicated row buys more than one copy of it."""
    shape = CR.SHAPES[0]
    mo = models(shape)
    N, M, Q, D = shape
    Xc, Yc, X = CR.cond_inputs(Q, D, 5, 300)
    ref = CR.cond_closed_form(*mo.g, mo.Psi2, mo.C, Xc, Yc, X)
    assert ref['var_c'][-1] < 1.0 / mo.d['beta']
    once = CR.cond_closed_form(*mo.g, mo.Psi2, mo.C, Xc[:-1], Yc[:-1], X)
    assert ref['reduction'][-1] > once['reduction'][-1]
