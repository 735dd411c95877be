"""Latent inference for new rows without a device: the numpy reference the GPU tests compare against (tests/infer_ref.py), its link to the
reference's collapsed bound, and the host logic of Predictor.infer / impute with an injected numpy engine."""
import os
import re

import numpy as np

import infer_ref as I
import predict_ref as R
from oracle import literal as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small_model(seed=1, M=9, Q=3, D=6, N=300):
    rng = np.random.default_rng(seed)
    Z, sf2, alpha, beta = rng.normal(size=(M, Q)), 1.3, np.array([0.7, 1.9, 0.4])[:Q], 8.0
    Xm, Xs, Y = rng.normal(size=(N, Q)), rng.uniform(0.05, 0.3, size=(N, Q)), rng.normal(size=(N, D))
    Psi2, C = R.statistics(Z, sf2, alpha, Y, Xm, Xs)
    return I.Model(Z, sf2, alpha, beta, Psi2, C), rng


def test_surfaces_exist():
    src = open(os.path.join(ROOT, 'include', 'gparml_hip.h')).read()
    from gparml_amd import _lib
    for name, nargs in (('gp_infer_objective', 11), ('gp_infer_latent', 12)):
        m = re.search(r'int\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m and len(m.group(1).split(',')) == nargs, name
        assert len(_lib.SIGNATURES[name][1]) == nargs
    from gparml_amd.engine import ShardEngine
    from gparml_amd.predict import Predictor
    from gparml_amd.resident import ResidentModel
    assert all(callable(f) for f in (ShardEngine.infer_objective, ShardEngine.infer_latent, Predictor.infer, Predictor.impute, ResidentModel.infer))


def test_reference_objective_is_the_predictive_identity_and_gradients_match_differences():
    mdl, rng = _small_model()
    Q, D = 3, 6
    n = 4
    mu, S, Y = rng.normal(size=(n, Q)), rng.uniform(0.1, 0.5, size=(n, Q)), rng.normal(size=(n, D))
    for cols in (None, [0, 2, 5]):
        Lv, gm, gs = I.objective(mdl, Y, cols, mu, S)
        ref = I.objective_via_predict(mdl, Y, cols, mu, S)
        assert np.max(np.abs(Lv - ref) / np.abs(ref)) <= 1e-12
        h = 1e-6
        for q in range(Q):
            e = np.zeros(Q)
            e[q] = h
            dm = (I.objective_via_predict(mdl, Y, cols, mu + e, S) - I.objective_via_predict(mdl, Y, cols, mu - e, S)) / (2 * h)
            ds = (I.objective_via_predict(mdl, Y, cols, mu, S + e) - I.objective_via_predict(mdl, Y, cols, mu, S - e)) / (2 * h)
            assert np.max(np.abs(gm[:, q] - dm)) <= 1e-7 * max(1.0, np.max(np.abs(dm)))
            assert np.max(np.abs(gs[:, q] - ds)) <= 1e-7 * max(1.0, np.max(np.abs(ds)))
    # the raw form: chain rule through the softplus, and unobserved columns are never read
    raw = I.softplus_inv(S)
    Ynan = Y.copy()
    Ynan[:, [1, 3, 4]] = np.nan
    Lr, gmr, gsr = I.objective(mdl, Ynan, [0, 2, 5], mu, raw, xs_is_raw=True)
    L0, gm0, gs0 = I.objective(mdl, Y, [0, 2, 5], mu, S)
    assert np.allclose(Lr, L0, rtol=1e-13) and np.allclose(gmr, gm0, rtol=1e-12) and np.allclose(gsr, gs0 * (1 - np.exp(-S)), rtol=1e-11)
    # the switches the GPU test uses to show that its bound catches a dropped term do drop something
    assert np.max(np.abs(I.objective(mdl, Y, None, mu, S, drop='kl_grad')[1] - gm)) > 1e-2
    assert np.max(np.abs(I.objective(mdl, Y, None, mu, S, drop='psi2')[0] - I.objective(mdl, Y, None, mu, S)[0])) > 1e-2


def test_frozen_bound_lies_below_the_collapsed_bound_and_the_gap_shrinks_with_N():
    """F(train + new rows, N + n) - F(train, N) >= sum_n L_n for any (mu, S): F maximises over q(u), L keeps it at the training optimum."""
    rng = np.random.default_rng(0)
    M, Q, D = 12, 2, 5
    Z, sf2, alpha, beta = rng.normal(size=(M, Q)), 1.3, np.array([0.7, 1.9]), 8.0
    Wt = rng.normal(size=(Q, D))
    n = 7
    ym, ys = rng.normal(size=(n, Q)), rng.uniform(0.05, 0.5, size=(n, Q))
    Yn = np.sin(ym.dot(Wt))

    def stats(Y, Xm, Xs):
        pt = L.PartialTermsOracle(Z, sf2, alpha, beta, M, Q, len(Y), D)
        pt.set_data(Y, Xm, Xs, True)
        return pt.get_local_statistics()

    def F(st, Ntot):
        pt = L.PartialTermsOracle(Z, sf2, alpha, beta, M, Q, Ntot, D)
        pt.set_local_statistics(st['sum_YYT'], st['sum_exp_K_mi_K_im'], st['exp_K_miY'], st['sum_exp_K_ii'], st['KL'])
        return float(pt.logmarglik())
    gaps = []
    for N in (100, 1600):
        Xm, Xs = rng.normal(size=(N, Q)), rng.uniform(0.05, 0.3, size=(N, Q))
        Y = np.sin(Xm.dot(Wt)) + rng.normal(size=(N, D)) / np.sqrt(beta)
        tr, nw = stats(Y, Xm, Xs), stats(Yn, ym, ys)
        mdl = I.Model(Z, sf2, alpha, beta, tr['sum_exp_K_mi_K_im'], tr['exp_K_miY'])
        Ln = I.objective(mdl, Yn, None, ym, ys)[0]
        gaps.append(F({k: tr[k] + nw[k] for k in tr}, N + n) - F(tr, N) - Ln.sum())
    assert gaps[0] >= -1e-8 and gaps[1] >= -1e-8, gaps
    assert gaps[1] < gaps[0], gaps


def _predictor(p, engine=I.NumpyInferEngine):
    from gparml_amd.predict import Predictor
    Psi2, C = R.statistics(p['Z'], p['sf2'], p['alpha'], p['Y'], p['X_mu'], p['X_S'])
    gs = dict(Z=p['Z'], sf2=p['sf2'], alpha=p['alpha'], beta=p['beta'])
    acc = dict(sum_YYT=np.sum(p['Y'] ** 2), sum_exp_K_mi_K_im=Psi2, sum_exp_K_miY=C, sum_exp_K_ii=p['N'] * p['sf2'], sum_KL=0.0)
    engine.calls = []
    return Predictor(gs, acc, p['N'], p['D'], engine_class=engine), I.Model(p['Z'], p['sf2'], p['alpha'], p['beta'], Psi2, C)


def test_predictor_infer_nearest_start_and_nan_pattern_grouping():
    p = I.issue_problem()
    pred, mdl = _predictor(p)
    Yt = p['Yt'][:6].copy()
    Yt[:, 5:] = np.nan                    # hidden outputs are simply missing
    Yt[[1, 4], 2] = np.nan                # two rows miss one more column: a second pattern
    res = pred.infer(Yt, training=[(p['Y'][:300], p['X_mu'][:300]), (p['Y'][300:], p['X_mu'][300:])], X_S0=np.full((6, 2), 0.5), iterations=200)
    calls = I.NumpyInferEngine.calls
    assert len(calls) == 2
    assert list(calls[0]['cols']) == [0, 1, 2, 3, 4] and calls[0]['Y'].shape[0] == 4
    assert list(calls[1]['cols']) == [0, 1, 3, 4] and calls[1]['Y'].shape[0] == 2
    # the start of the first pattern's rows: the nearest training output over columns 0-4 (the start issue_problem records)
    assert np.array_equal(calls[0]['X_mu'], p['X0'][[0, 2, 3, 5]])
    assert np.array_equal(calls[1]['X_mu'], pred.nearest_training_embeddings(Yt[[1, 4]], [(p['Y'], p['X_mu'])], 2, [0, 1, 3, 4]))
    # results land in the rows they belong to
    for i, cols in ((0, [0, 1, 2, 3, 4]), (4, [0, 1, 3, 4])):
        Li = I.objective(mdl, np.nan_to_num(Yt[i:i + 1]), cols, res[0][i:i + 1], res[1][i:i + 1])[0][0]
        assert abs(Li - res[2][i]) <= 1e-9 * abs(Li)
    # with mask: the same columns through the mask argument
    I.NumpyInferEngine.calls = []
    res2 = pred.infer(p['Yt'][:6], mask=[0, 1, 2, 3, 4], X_mu0=p['X0'][:6], X_S0=np.full((6, 2), 0.5), iterations=200)
    assert len(I.NumpyInferEngine.calls) == 1 and list(I.NumpyInferEngine.calls[0]['cols']) == [0, 1, 2, 3, 4]
    assert np.allclose(res2[2][[0, 2, 3, 5]], res[2][[0, 2, 3, 5]], rtol=1e-9)


def test_predictor_infer_restarts_are_rows_and_the_best_is_kept():
    p = I.issue_problem()
    pred, mdl = _predictor(p)
    n, R = 3, 4
    np.random.seed(7)
    res = pred.infer(p['Yt'][:n], mask=p['cols'], is_random_init=True, random_restarts=R, iterations=200)
    (call,) = I.NumpyInferEngine.calls
    assert call['Y'].shape == (n * (R + 1), p['D']) and call['X_mu'].shape == (n * (R + 1), 2)
    np.random.seed(7)
    idx = np.random.randint(p['M'], size=(n, R + 1))
    assert np.array_equal(call['X_mu'], p['Z'][idx].reshape(-1, 2))             # every row starts at random inducing points, restarts laid out as rows
    assert np.array_equal(call['Y'], np.repeat(p['Yt'][:n], R + 1, axis=0))
    assert np.array_equal(call['X_S'][::R + 1], call['X_S'][1::R + 1])           # a row's restarts share its starting variance
    assert np.all((call['X_S'] >= 0.001) & (call['X_S'] <= 1.0))
    for i in range(n):
        Ls = [I.optimise_row(mdl, p['Yt'][i], p['cols'], call['X_mu'][i * (R + 1) + k], call['X_S'][i * (R + 1) + k], maxiter=200)[2] for k in range(R + 1)]
        assert res[2][i] == max(Ls)


def test_predictor_impute_beats_the_zero_baseline_on_the_cpu():
    p = I.issue_problem()
    pred, _ = _predictor(p)
    n = 12
    mean, var, res = pred.impute(p['Yt'][:n], p['cols'], X_mu0=p['X0'][:n], X_S0=p['S0'][:n], iterations=300)
    hid = p['hidden']
    mae, base = np.abs(mean[:, hid] - p['Yt'][:n, hid]).mean(), np.abs(p['Yt'][:n, hid]).mean()
    assert mean.shape == (n, p['D']) and var.shape == (n, p['D']) and np.all(var > 0)
    assert mae < 0.5 * base, (mae, base)


def test_predictor_infer_needs_a_start():
    p = I.issue_problem()
    pred, _ = _predictor(p)
    try:
        pred.infer(p['Yt'][:2])
    except AssertionError as e:
        assert 'training' in str(e)
    else:
        raise AssertionError('no start and no error')
