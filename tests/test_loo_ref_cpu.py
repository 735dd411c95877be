"""The closed form of leave-one-out / leave-block-out prediction (tests/loo_ref.py: a rank-g downdate of Kmm + beta Psi2) against brute force, one
long-double refit per block, and the closed form's handling of a block that cannot be left out.  No GPU: this pins the mathematics of gp_loo_score
independently of the device."""
import numpy as np
import pytest

import loo_ref as LR
import predict_ref as R

N, M, Q, D = 96, 12, 2, 3


def _model():
    """Inputs spread over a box with the inducing points among them, beta = 10, no duplicated or isolated point: every leverage stays below 1/2."""
    rs = np.random.RandomState(4)
    X = rs.uniform(-2.0, 2.0, size=(N, Q))
    Z = rs.uniform(-2.0, 2.0, size=(M, Q))
    sf2, alpha, beta = 1.2, np.array([0.9, 1.1]), 10.0
    Y = np.sin(X.dot(rs.randn(Q, D))) + rs.randn(N, D) / np.sqrt(beta)
    Psi2, C = R.statistics(Z, sf2, alpha, Y, X, np.zeros_like(X))
    return dict(X=X, Z=Z, sf2=sf2, alpha=alpha, beta=beta, Y=Y, Psi2=Psi2, C=C)


@pytest.fixture(scope='module')
def model():
    m = _model()
    # what float64 costs on this model: predict_ref in float64 on the float64 statistics against predict_ref in long double on the long-double
    # statistics of the same rows, at the training inputs
    m64, v64 = R.predict(m['Z'], m['sf2'], m['alpha'], m['beta'], m['Psi2'], m['C'], m['X'])
    _, m['Psi2_ld'], m['C_ld'], _ = LR.statistics_ld(m['Z'], m['sf2'], m['alpha'], m['Y'], m['X'])
    mld, vld = R.predict_ld(m['Z'], m['sf2'], m['alpha'], m['beta'], m['Psi2_ld'], m['C_ld'], m['X'])
    m['disc_mean'] = float(np.max(np.abs(m64 - mld)))
    m['disc_var'] = float(np.max(np.abs(v64 - vld)))
    return m


@pytest.mark.parametrize('block', [1, 5, 32])
def test_closed_form_is_the_refit(model, block):
    """N = 96, M = 12, Q = 2, D = 3; block 5 ends in a short block (96 = 19 x 5 + 1), block 32 is 32 | 32 | 32.
    Both sides see the same model: the long-double statistics of the rows, which the refit forms itself.  Tolerance, nothing chosen by hand: the
    measured float64-versus-long-double discrepancy of predict_ref on this model (mean 7.5e-13, variance 1.68e-14; cond(Kmm + beta Psi2) = 6.1e4)
    times the largest 1 / (1 - lambda_max(H)) of the case (1.83 at block 1, 1.84 at block 5, 3.08 at block 32).  The largest leverage (0.454) is
    asserted to stay at or below 1/2, so that a reference that drifts cannot hide.
    The closed form is evaluated in long double (loo_ref's docstring).  Evaluated in float64 on the float64 statistics it met the bound for the
    residuals at every block size (7.7e-13 / 8.1e-13 / 1.0e-12 against 1.37e-12 / 1.38e-12 / 2.31e-12) and for the variance at block 1 and 5
    (2.9e-14 against 3.1e-14) but not at block 32 (5.67e-14 against 5.18e-14): the float64 error of |b|^2 (1.3e-14) reaches [S^-1]_ii with the
    SQUARE of the amplification, which the rule's single factor does not cover.  In long double the two agree to the rounding of the returned
    float64 arrays (1e-15 / 1e-16, printed); given the float64 statistics instead, the long-double closed form moves by their rounding alone and is
    held to the same bound (8.1e-13 / 3.4e-14 at block 32)."""
    m = model
    cf = LR.loo_closed_form(m['Z'], m['sf2'], m['alpha'], m['beta'], m['Psi2_ld'], m['C_ld'], m['Y'], m['X'], block=block, include_noise=True)
    rf = LR.loo_refit(m['Z'], m['sf2'], m['alpha'], m['beta'], m['Y'], m['X'], block=block, include_noise=True)
    assert not cf['not_pd']
    assert np.max(cf['lev']) <= 0.5, np.max(cf['lev'])
    assert len(cf['lam_max']) == -(-N // block)
    amp = float(np.max(1.0 / (1.0 - cf['lam_max'])))
    err_e = float(np.max(np.abs(cf['e'] - rf['e'])))
    err_v = float(np.max(np.abs(cf['var'] - rf['var'])))
    print('block %d: disc mean %.3g var %.3g, amplification %.3g, max lev %.3g; error e %.3g var %.3g' % (block, m['disc_mean'], m['disc_var'], amp,
                                                                                                          np.max(cf['lev']), err_e, err_v))
    assert err_e <= amp * m['disc_mean']
    assert err_v <= amp * m['disc_var']
    # the float64 statistics (what a device holds) move the result by their own rounding only: the same bound
    c64 = LR.loo_closed_form(m['Z'], m['sf2'], m['alpha'], m['beta'], m['Psi2'], m['C'], m['Y'], m['X'], block=block, include_noise=True)
    e64, v64 = float(np.max(np.abs(c64['e'] - rf['e']))), float(np.max(np.abs(c64['var'] - rf['var'])))
    print('   on the float64 statistics: e %.3g var %.3g from the refit' % (e64, v64))
    assert e64 <= amp * m['disc_mean'] and v64 <= amp * m['disc_var']
    if block == 1:
        # the g = 1 form written out: e' = e / (1 - h), v' = sf2 - |a|^2 + |b|^2 / (1 - h)
        p = LR.parts_ld(m['Z'], m['sf2'], m['alpha'], m['beta'], m['Psi2_ld'], m['C_ld'], m['X'])
        a2, b2 = np.sum(p['a'] * p['a'], axis=0), np.sum(p['b'] * p['b'], axis=0)
        h = np.longdouble(m['beta']) * b2
        f = lambda x: np.asarray(x, dtype=float)          # noqa: E731
        assert np.allclose(cf['lev'], f(h), rtol=1e-15, atol=0)
        assert np.allclose(cf['e'], f((m['Y'] - p['mean']) / (1 - h)[:, None]), rtol=1e-15, atol=1e-17)
        assert np.allclose(cf['var'], f(np.longdouble(m['sf2']) - a2 + b2 / (1 - h) + 1 / np.longdouble(m['beta'])), rtol=1e-15, atol=0)


def test_scores_are_score_ref_on_the_leave_out_prediction(model):
    """rows and column sums are score_ref's on (e', v'): the mask selects what is summed and never enters H."""
    import score_ref as S
    m = model
    rs = np.random.RandomState(8)
    obs = rs.uniform(size=(N, D)) > 0.3
    obs[7] = False
    full = LR.loo_closed_form(m['Z'], m['sf2'], m['alpha'], m['beta'], m['Psi2'], m['C'], m['Y'], m['X'], block=5)
    part = LR.loo_closed_form(m['Z'], m['sf2'], m['alpha'], m['beta'], m['Psi2'], m['C'], m['Y'], m['X'], block=5, observed=obs)
    assert np.array_equal(full['e'], part['e']) and np.array_equal(full['var'], part['var'])
    want = S.score_from(full['e'], np.zeros_like(full['e']), full['var'][:, None], obs)
    assert np.array_equal(part['cols'], want['cols']) and np.array_equal(part['row_logp'], want['row_logp'])
    assert part['row_logp'][7] == 0.0 and part['row_sse'][7] == 0.0
    assert np.array_equal(part['cols'][:, 0], obs.sum(axis=0).astype(float))


def test_a_block_that_cannot_be_left_out_is_reported():
    """Statistics that do not contain the rows (here: a tenth of them) make H exceed the identity: the closed form names the blocks and leaves NaN."""
    m = _model()
    cf = LR.loo_closed_form(m['Z'], m['sf2'], m['alpha'], m['beta'], 0.1 * m['Psi2'], 0.1 * m['C'], m['Y'], m['X'], block=32)
    assert cf['not_pd'] and np.all(cf['lam_max'][cf['not_pd']] >= 1.0)
    rows = np.concatenate([LR.blocks(N, 32)[j] for j in cf['not_pd']])
    assert np.all(np.isnan(cf['e'][rows])) and np.all(np.isnan(cf['var'][rows]))
    assert 'cols' not in cf
