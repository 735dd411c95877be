"""Predictor.infer(ragged=True) without a device: one engine call for rows with several NaN patterns, the observed sets it passes, the restart
rule, the unchanged call sequence of ragged=False, and Predictor.inducing_start against a brute-force loop."""
import numpy as np

import infer_ref as I
from test_infer_cpu import _predictor


class RowsEngine(I.NumpyInferEngine):
    """NumpyInferEngine plus ShardEngine.infer_latent_rows: every row optimised by infer_ref.optimise_row over its own observed columns; the calls are
    recorded in ``rows_calls``."""
    rows_calls = []

    def infer_latent_rows(self, Y, X_mu, X_S, observed=None, xs_is_raw=False, max_iters=100, gtol=1e-5):
        assert self.state == 'ready' and not xs_is_raw
        Y, X_mu, X_S = np.atleast_2d(Y), np.atleast_2d(X_mu), np.atleast_2d(X_S)
        observed = ~np.isnan(Y) if observed is None else np.asarray(observed) != 0
        assert observed.shape == Y.shape and observed.any(axis=1).all() and np.all(np.isfinite(Y[observed]))
        type(self).rows_calls.append(dict(Y=Y.copy(), X_mu=X_mu.copy(), X_S=X_S.copy(), observed=observed.copy(), max_iters=max_iters))
        out = [I.optimise_row(self.mdl, np.nan_to_num(Y[i]), np.flatnonzero(observed[i]), X_mu[i], X_S[i], maxiter=max_iters) for i in range(Y.shape[0])]
        return (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]), np.zeros(len(out), dtype=np.int32))


def _setup():
    p = I.issue_problem()
    pred, mdl = _predictor(p, engine=RowsEngine)
    RowsEngine.rows_calls = []
    Yt = p['Yt'][:6].copy()
    Yt[:, 5:] = np.nan
    Yt[[1, 4], 2] = np.nan                # a second pattern
    Yt[3, 0] = np.nan                     # and a third
    return p, pred, mdl, Yt


def test_ragged_is_one_call_with_the_rows_own_observed_sets():
    p, pred, mdl, Yt = _setup()
    S0 = np.full((6, 2), 0.5)
    res = pred.infer(Yt, X_mu0=p['X0'][:6], X_S0=S0, iterations=200, ragged=True)
    assert len(RowsEngine.calls) == 0
    (call,) = RowsEngine.rows_calls
    assert np.array_equal(call['observed'], ~np.isnan(Yt)) and call['Y'].shape == (6, p['D'])
    assert np.array_equal(call['X_mu'], p['X0'][:6]) and np.array_equal(call['X_S'], S0) and call['max_iters'] == 200
    for i in range(6):
        c = np.flatnonzero(~np.isnan(Yt[i]))
        Li = I.objective(mdl, np.nan_to_num(Yt[i:i + 1]), c, res[0][i:i + 1], res[1][i:i + 1])[0][0]
        assert abs(Li - res[2][i]) <= 1e-9 * abs(Li)
    # mask minus the NaNs: a column outside the mask is not observed even where it holds a number
    RowsEngine.rows_calls = []
    pred.infer(p['Yt'][:6], mask=[0, 1, 2, 4], X_mu0=p['X0'][:6], X_S0=S0, iterations=5, ragged=True)
    (call,) = RowsEngine.rows_calls
    want = np.zeros((6, p['D']), dtype=bool)
    want[:, [0, 1, 2, 4]] = True
    assert np.array_equal(call['observed'], want)
    # the same optimum as the grouped path, which the same reference optimiser serves per pattern
    RowsEngine.calls = []
    ref = pred.infer(Yt, X_mu0=p['X0'][:6], X_S0=S0, iterations=200)
    assert np.allclose(ref[2], res[2], rtol=1e-9)


def test_not_ragged_is_todays_call_sequence():
    p, pred, mdl, Yt = _setup()
    pred.infer(Yt, X_mu0=p['X0'][:6], X_S0=np.full((6, 2), 0.5), iterations=20)
    assert len(RowsEngine.rows_calls) == 0
    calls = RowsEngine.calls
    assert [list(c['cols']) for c in calls] == [[0, 1, 2, 3, 4], [0, 1, 3, 4], [1, 2, 3, 4]]      # one call per pattern, in order of first occurrence
    assert [c['Y'].shape[0] for c in calls] == [3, 2, 1]
    assert np.array_equal(calls[0]['X_mu'], p['X0'][[0, 2, 5]]) and np.array_equal(calls[1]['X_mu'], p['X0'][[1, 4]])


def test_ragged_restarts_are_rows_and_the_earliest_best_is_kept():
    p, pred, mdl, Yt = _setup()
    n, R = 4, 3
    np.random.seed(7)
    res = pred.infer(Yt[:n], is_random_init=True, random_restarts=R, iterations=200, ragged=True)
    (call,) = RowsEngine.rows_calls
    np.random.seed(7)
    idx = np.random.randint(p['M'], size=(n, R + 1))
    assert np.array_equal(call['X_mu'], p['Z'][idx].reshape(-1, 2))
    assert np.array_equal(call['observed'], np.repeat(~np.isnan(Yt[:n]), R + 1, axis=0))
    assert np.array_equal(call['X_S'][::R + 1], call['X_S'][1::R + 1])
    for i in range(n):
        c = np.flatnonzero(~np.isnan(Yt[i]))
        out = [I.optimise_row(mdl, np.nan_to_num(Yt[i]), c, call['X_mu'][i * (R + 1) + k], call['X_S'][i * (R + 1) + k], maxiter=200) for k in range(R + 1)]
        Ls = [o[2] for o in out]
        assert res[2][i] == max(Ls)
        assert np.array_equal(res[0][i], out[int(np.argmax(Ls))][0])

    class Ties(RowsEngine):
        def infer_latent_rows(self, Y, X_mu, X_S, **kw):
            out = RowsEngine.infer_latent_rows(self, Y, X_mu, X_S, **kw)
            return out[0], out[1], np.zeros(len(out[2])), out[3]                   # every restart equally good
    pred._engine_cls = Ties
    RowsEngine.rows_calls = []
    np.random.seed(7)
    tie = pred.infer(Yt[:n], is_random_init=True, random_restarts=R, iterations=3, ragged=True)
    first = RowsEngine.rows_calls[0]
    want = [I.optimise_row(mdl, np.nan_to_num(Yt[i]), np.flatnonzero(~np.isnan(Yt[i])), first['X_mu'][i * (R + 1)], first['X_S'][i * (R + 1)], maxiter=3)[0]
            for i in range(n)]
    assert np.array_equal(tie[0], np.array(want))                                   # the earliest of equal maxima: each row's first start


def _brute(Y, observed, Z, Mz):
    out = np.empty((Y.shape[0], Z.shape[1]))
    for i in range(Y.shape[0]):
        best, arg = np.inf, -1
        for m in range(Z.shape[0]):
            d = 0.0
            for j in range(Y.shape[1]):
                if observed[i, j]:
                    d += (Y[i, j] - Mz[m, j]) ** 2
            if d < best:
                best, arg = d, m
        out[i] = Z[arg]
    return out


def test_inducing_start_against_brute_force():
    from gparml_amd.predict import Predictor
    rs = np.random.RandomState(2)
    M, Q, D, n = 7, 2, 5, 40
    Z = rs.randn(M, Q)
    Mz = rs.randint(-3, 4, size=(M, D)).astype(float)                               # small integers: every distance is exact, ties are ties
    Mz[5] = Mz[2]                                                                    # two inducing points predict the same outputs
    Y = rs.randint(-3, 4, size=(n, D)).astype(float)
    obs = rs.rand(n, D) < 0.6
    obs[:, 0] |= ~obs.any(axis=1)
    obs[0] = False
    obs[0, D - 1] = True                                                            # a row that observes a single column
    Y[1] = Mz[2]                                                                    # a row at distance 0 from points 2 and 5: the lower index wins
    obs[1] = True
    Yn = np.where(obs, Y, np.nan)                                                   # NaN where unobserved
    want = _brute(Y, obs, Z, Mz)
    assert np.array_equal(want[1], Z[2])
    for block in (None, 1, 7, 64):
        assert np.array_equal(Predictor.inducing_start(Yn, obs, Z, Mz, block=block), want)
    # real-valued means too
    Mz2, Y2 = rs.randn(M, D), rs.randn(n, D)
    assert np.array_equal(Predictor.inducing_start(np.where(obs, Y2, np.nan), obs, Z, Mz2), _brute(Y2, obs, Z, Mz2))


def test_start_inducing_reaches_the_engine():
    p, pred, mdl, Yt = _setup()
    import predict_ref as R
    res = pred.infer(Yt, start='inducing', X_S0=np.full((6, 2), 0.5), iterations=10, ragged=True)
    (call,) = RowsEngine.rows_calls
    Mz = R.predict(mdl.Z, mdl.sf2, mdl.alpha, mdl.beta, mdl.Psi2, mdl.C, p['Z'], None)[0]
    from gparml_amd.predict import Predictor
    assert np.array_equal(call['X_mu'], Predictor.inducing_start(Yt, ~np.isnan(Yt), p['Z'], Mz))
    assert np.array_equal(call['X_mu'], _brute(np.nan_to_num(Yt), ~np.isnan(Yt), p['Z'], Mz))
    assert res[0].shape == (6, 2)
    try:
        pred.infer(Yt, start='inducing', X_S0=np.full((6, 2), 0.5))
    except AssertionError as e:
        assert 'ragged' in str(e)
    else:
        raise AssertionError("start='inducing' without ragged=True must be refused")
