"""The numpy reference of held-out scoring (tests/score_ref.py) against a direct Gaussian log density of the exact GP, and its bookkeeping: masks,
rows without an observed entry, column sums.  No GPU."""
import numpy as np

import predict_ref as R
import score_ref as S


def _grid():
    """The 40-point grid of test_gpu_predictive.test_exact_gp_limit: M = N, Z = X, so the sparse posterior is the exact GP's."""
    rs = np.random.RandomState(3)
    X = np.stack(np.meshgrid(np.linspace(-3, 3, 8), np.linspace(-2, 2, 5)), -1).reshape(-1, 2)
    Y = np.sin(X.dot(rs.randn(2, 3))) + 0.1 * rs.randn(40, 3)
    sf2, alpha, beta = 1.3, np.array([0.8, 1.1]), 25.0
    Xs = rs.uniform(-3, 3, size=(13, 2))
    Ys = np.sin(Xs.dot(np.random.RandomState(3).randn(2, 3))) + 0.1 * rs.randn(13, 3)
    Psi2, C = R.statistics(X, sf2, alpha, Y, X, np.zeros_like(X))
    return X, Y, sf2, alpha, beta, Xs, Ys, Psi2, C


def test_reference_is_the_exact_gp_log_density():
    """score_ref on predict_ref against -1/2 ln(2 pi v) - e^2 / (2 v) written out from exact_gp's own mean and variance.  The two predictions agree
    to 1e-7 of max(1, |mean|) and of sf2 (the bound of test_exact_gp_limit); that is propagated through the derivatives of the density."""
    X, Y, sf2, alpha, beta, Xs, Ys, Psi2, C = _grid()
    got = S.score(X, sf2, alpha, beta, Psi2, C, Ys, Xs, None, None, include_noise=True)
    me, ve = R.exact_gp(X, Y, sf2, alpha, beta, Xs)
    e = Ys - me
    direct = -0.5 * np.log(2.0 * np.pi * ve) - e * e / (2.0 * ve)
    tol_m, tol_v = 1e-7 * max(1.0, np.max(np.abs(me))), 1e-7 * sf2
    bound = np.abs(e) / ve * tol_m + np.abs(e * e / (2 * ve ** 2) - 1 / (2 * ve)) * tol_v
    assert np.all(np.abs(got['row_logp'] - direct.sum(axis=1)) <= bound.sum(axis=1) + 1e-13)
    assert np.all(np.abs(got['cols'][:, 4] - direct.sum(axis=0)) <= bound.sum(axis=0) + 1e-13)
    assert np.all(np.abs(got['row_sse'] - (e * e).sum(axis=1)) <= (2 * np.abs(e) * tol_m).sum(axis=1) + 1e-13)
    assert np.array_equal(got['cols'][:, 0], np.full(3, 13.0))


def test_masks_and_empty_rows():
    rs = np.random.RandomState(5)
    n, D = 11, 7
    Y, mean, var = rs.randn(n, D), rs.randn(n, D), rs.uniform(0.1, 2.0, size=(n, D))
    obs = rs.uniform(size=(n, D)) > 0.3
    obs[4] = False                                  # a row with no observed entry scores 0
    Yh = np.where(obs, Y, np.nan)                   # the hidden entries are never used
    full, part = S.score_from(Y, mean, var), S.score_from(Yh, mean, var, obs)
    t = full['terms']
    assert np.all(np.isfinite(part['cols'])) and np.all(np.isfinite(part['row_logp']))
    assert part['row_logp'][4] == 0.0 and part['row_sse'][4] == 0.0 and part['row_chi2'][4] == 0.0
    for key, name in (('logp', 'row_logp'), ('e2', 'row_sse'), ('q', 'row_chi2')):
        want = np.where(obs, t[key], 0.0).sum(axis=1)
        assert np.allclose(part[name], want, rtol=1e-14, atol=1e-14)
    assert np.array_equal(part['cols'][:, 0], obs.sum(axis=0).astype(float))
    # one variance per row (deterministic inputs) is the same as that variance in every column
    a, b = S.score_from(Y, mean, var[:, :1], obs), S.score_from(Y, mean, np.repeat(var[:, :1], D, axis=1), obs)
    assert np.array_equal(a['cols'], b['cols']) and np.array_equal(a['row_logp'], b['row_logp'])


def test_column_sums_are_the_sums_of_the_terms():
    rs = np.random.RandomState(6)
    n, D = 23, 5
    Y, mean, var = rs.randn(n, D), rs.randn(n, D), rs.uniform(0.1, 2.0, size=(n, D))
    obs = rs.uniform(size=(n, D)) > 0.3
    s = S.score_from(Y, mean, var, obs)
    t = s['terms']
    for k, key in enumerate(('e', 'e2', 'q', 'logp')):
        assert np.allclose(s['cols'][:, k + 1], t[key].sum(axis=0), rtol=1e-14, atol=1e-14)
    # rows and columns add up to the same totals
    assert np.isclose(s['row_logp'].sum(), s['cols'][:, 4].sum(), rtol=1e-13)
    assert np.isclose(s['row_sse'].sum(), s['cols'][:, 2].sum(), rtol=1e-13)
    assert np.isclose(s['row_chi2'].sum(), s['cols'][:, 3].sum(), rtol=1e-13)
    m = S.summary(s['cols'])
    assert np.allclose(m['rmse'], np.sqrt(s['cols'][:, 2] / s['cols'][:, 0])) and np.allclose(m['nlpd'], -s['cols'][:, 4] / s['cols'][:, 0])
    # the density integrates to one: a check of the constant (column 0 of a unit-variance grid)
    x = np.linspace(-12, 12, 200001)[:, None]
    p = np.exp(S.score_from(x, np.zeros_like(x), np.full_like(x, 1.7))['terms']['logp'])
    assert abs(p.sum() * (x[1, 0] - x[0, 0]) - 1.0) < 1e-9


def test_cols_in_device_order_by_hand():
    """cols_in_device_order on sums whose value depends on the order: with 2^53 in one half of a segment a 1.0 survives only where it is added
    to its own half first, and the segments enter the total one by one."""
    big = 2.0 ** 53
    v = np.zeros((6, 1))
    o = np.ones((6, 1), dtype=bool)
    v[:, 0] = [big, 1.0, 1.0, -big, 1.0, 1.0]              # seg = 4: halves (big + 1 = big, 1 - big), then the segment (1 + 1)
    assert S.cols_in_device_order(v, o, seg=4)[0] == (big + (1.0 - big)) + 2.0 == 3.0
    assert S.cols_in_device_order(v, o, seg=2)[0] == 3.0   # (big + 1) + (1 - big) + (1 + 1), each segment whole before it enters: 0 + 1 + 2
    o[1] = False                                           # a hidden entry is skipped, not added as a zero of another sign or a NaN
    v[1] = np.nan
    assert S.cols_in_device_order(v, o, seg=4)[0] == 3.0
    m = S.one_entry_mask(7, 3, 4)
    assert np.array_equal(m.sum(axis=1), [1, 1, 1, 1, 0, 1, 1]) and m[5, 2] and m[6, 0]
