"""gp_predict on the GPU: posterior predictive mean and variance at new inputs against tests/predict_ref.py (numpy)."""
import os

import numpy as np
import pytest

import predict_ref as R

pytestmark = pytest.mark.gpu


def _model(N, D, M, Q, regime, seed=0, spread=1.5):
    """Synthetic data with inducing points drawn apart from the data and a lengthscale short enough for cond(Kmm) < 1e6."""
    from oracle import factorised as Fz
    from oracle import literal as L
    d = Fz.synthetic_shard(N, D, M, Q, regime=regime, seed=seed, zseed=seed + 1, alpha_value=min(1.0, 1.0 / Q))
    rs = np.random.RandomState(seed + 7)
    d['Z'] = spread * rs.randn(M, Q)
    a = min(1.0, 1.0 / Q)
    while np.linalg.cond(L.rbf_gram(d['Z'], 1.0, np.full(Q, a))) > 1e6:
        a *= 1.5
    d['alpha'] = np.full(Q, a)
    return d


def _engine(d, N, D, M, Q):
    from gparml_amd.engine import ShardEngine
    e = ShardEngine(N, D, M, Q)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    e.phase1()
    e.global_step(sync=True)
    return e


def _ref(e, d, X_mu, X_S=None, include_noise=False):
    Psi2, C = e.download('PSI2_SUM'), e.download('PSI1TY')
    return R.predict(d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2, C, X_mu, X_S, include_noise)


def _tol(d, M, Psi2=None):
    """1e-10, or eps-level error amplified by the conditioning of Kmm (and of Kmm + beta Psi2 when given) if that is larger."""
    from oracle import literal as L
    K = L.rbf_gram(d['Z'], d['sf2'], d['alpha'])
    cond = np.linalg.cond(K)
    if Psi2 is not None:
        cond = max(cond, np.linalg.cond(K + d['beta'] * Psi2))
    return max(1e-10, 1e-16 * cond)


def _close(a, b, tol, scale, what):
    err = np.max(np.abs(a - b)) / scale
    assert err <= tol, '%s: %.3g > %.3g' % (what, err, tol)


@pytest.mark.parametrize('M,Q,D,regime', [(5, 1, 1, 'A'), (64, 2, 3, 'B'), (130, 17, 3, 'B'), (130, 10, 100, 'A'), (64, 50, 3, 'B'),
                                          (64, 70, 3, 'B'), (512, 10, 100, 'B'), (64, 3, 300, 'B')])
def test_against_numpy_reference(M, Q, D, regime):
    N = max(300, M + 100)
    d = _model(N, D, M, Q, regime, seed=M + Q + D)
    e = _engine(d, N, D, M, Q)
    rs = np.random.RandomState(11)
    n = 37
    Xt, St = rs.randn(n, Q), rs.uniform(0.05, 0.5, size=(n, Q))
    tol = _tol(d, M, e.download('PSI2_SUM'))
    for X_S in (None, St):
        for noise in (False, True):
            m, v = e.predict(Xt, X_S, include_noise=noise)
            mr, vr = _ref(e, d, Xt, X_S, noise)
            _close(m, mr, tol, max(1.0, np.max(np.abs(mr))), 'mean (%s)' % ('unc' if X_S is not None else 'det'))
            _close(v, vr, tol, d['sf2'], 'var (%s)' % ('unc' if X_S is not None else 'det'))
    e.close()


def test_exact_gp_limit():
    from gparml_amd.engine import ShardEngine
    rs = np.random.RandomState(3)
    X = np.stack(np.meshgrid(np.linspace(-3, 3, 8), np.linspace(-2, 2, 5)), -1).reshape(-1, 2)
    Y = np.sin(X.dot(rs.randn(2, 3))) + 0.1 * rs.randn(40, 3)
    sf2, alpha, beta = 1.3, np.array([0.8, 1.1]), 25.0
    e = ShardEngine(40, 3, 40, 2)
    e.upload_shard(Y, X, np.zeros_like(X))
    e.set_globals(X, sf2, alpha, beta)
    e.phase1()
    e.global_step(sync=True)
    Xs = rs.uniform(-3, 3, size=(13, 2))
    m, v = e.predict(Xs, include_noise=True)
    me, ve = R.exact_gp(X, Y, sf2, alpha, beta, Xs)
    _close(m, me, 1e-7, max(1.0, np.max(np.abs(me))), 'mean')
    _close(v, ve, 1e-7, sf2, 'var_y')
    e.close()


def test_quadrature_identity_q2():
    M, Q, D, N = 20, 2, 3, 200
    d = _model(N, D, M, Q, 'B', seed=5, spread=1.5)
    e = _engine(d, N, D, M, Q)
    rs = np.random.RandomState(8)
    mu, S = rs.randn(3, Q), rs.uniform(0.05, 0.3, size=(3, Q))
    xg, wg = np.polynomial.hermite_e.hermegauss(60)
    wg = wg / wg.sum()
    mu_u, var_u = e.predict(mu, S)
    for i in range(mu.shape[0]):
        s = np.sqrt(S[i])
        pts = np.stack(np.meshgrid(mu[i, 0] + s[0] * xg, mu[i, 1] + s[1] * xg, indexing='ij'), -1).reshape(-1, 2)
        w = np.outer(wg, wg).reshape(-1)
        m, v = e.predict(pts)
        em = w.dot(m)
        ev = w.dot(v[:, 0]) + w.dot((m - em) ** 2)
        _close(mu_u[i], em, 1e-9, 1.0, 'mean %d' % i)
        _close(var_u[i], ev, 1e-9, d['sf2'], 'var %d' % i)
    e.close()


def test_continuity_of_the_uncertain_path():
    M, Q, D, N = 70, 5, 4, 300
    d = _model(N, D, M, Q, 'A', seed=9, spread=1.5)
    e = _engine(d, N, D, M, Q)
    Xt = np.random.RandomState(2).randn(21, Q)
    m0, v0 = e.predict(Xt)
    m1, v1 = e.predict(Xt, np.full_like(Xt, 1e-14))
    _close(m1, m0, 1e-9, 1.0, 'mean')
    _close(v1, np.repeat(v0, D, axis=1), 1e-9, d['sf2'], 'var')
    e.close()


def _run_sequence(d, N, D, M, Q, predict):
    from gparml_amd.engine import ShardEngine
    e = ShardEngine(N, D, M, Q)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    e.phase1()
    e.global_step(sync=True)
    if predict:
        rs = np.random.RandomState(1)
        e.predict(rs.randn(50, Q))
        e.predict(rs.randn(50, Q), rs.uniform(0.1, 0.4, size=(50, Q)))
    e.phase2(True)
    out = e.finish()
    out['grad_X_mu'] = e.download('GRAD_X_MU')
    out['grad_X_S'] = e.download('GRAD_X_S')
    e.close()
    return out


def test_no_side_effects_and_determinism():
    from gparml_amd import _lib
    M, Q, D, N = 64, 3, 5, 500
    d = _model(N, D, M, Q, 'B', seed=13, spread=1.5)
    a = _run_sequence(d, N, D, M, Q, False)
    b = _run_sequence(d, N, D, M, Q, True)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    e = _engine(d, N, D, M, Q)
    rs = np.random.RandomState(4)
    Xt, St = rs.randn(450, Q), rs.uniform(0.1, 0.4, size=(450, Q))
    for X_S in (None, St):
        r1, r2 = e.predict(Xt, X_S), e.predict(Xt, X_S)
        assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])
    lib = _lib.load()
    lib.gp_debug_set_option(b'predict_rows', 128)
    try:
        for X_S in (None, St):
            whole = e.predict(Xt, X_S)                                   # 450 points: three chunks of 128 and one of 66
            parts = [e.predict(Xt[i:i + 128], None if X_S is None else X_S[i:i + 128]) for i in range(0, 450, 128)]
            assert np.array_equal(whole[0], np.concatenate([p[0] for p in parts]))
            assert np.array_equal(whole[1], np.concatenate([p[1] for p in parts]))
    finally:
        lib.gp_debug_set_option(b'predict_rows', 0)
    e.close()


def test_combined_statistics_predict_like_one_context():
    from gparml_amd.engine import ShardEngine
    M, Q, D, N = 40, 3, 4, 400
    d = _model(N, D, M, Q, 'B', seed=17, spread=1.5)
    one = _engine(d, N, D, M, Q)
    h = N // 2
    parts = []
    for sl in (slice(0, h), slice(h, N)):
        e = ShardEngine(h, D, M, Q)
        e.upload_shard(d['Y'][sl], d['X_mu'][sl], d['X_S'][sl])
        e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'], N_global=N)
        e.phase1()
        parts.append(e)
    parts[0].combine(parts[1], 'stats', 'add')
    parts[0].global_step(sync=True)
    rs = np.random.RandomState(6)
    Xt, St = rs.randn(30, Q), rs.uniform(0.1, 0.4, size=(30, Q))
    for X_S in (None, St):
        m1, v1 = one.predict(Xt, X_S)
        m2, v2 = parts[0].predict(Xt, X_S)
        _close(m2, m1, 1e-11, max(1.0, np.max(np.abs(m1))), 'mean')
        _close(v2, v1, 1e-11, max(1.0, np.max(np.abs(v1))), 'var')
    for e in parts + [one]:
        e.close()


def test_state_and_argument_errors():
    from gparml_amd import _lib
    from gparml_amd.engine import ShardEngine
    M, Q, D, N = 16, 2, 3, 100
    d = _model(N, D, M, Q, 'A', seed=21)
    e = ShardEngine(N, D, M, Q)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    with pytest.raises(_lib.GparmlHipError):
        e.predict(np.zeros((2, Q)))                   # no global step yet: GP_ERR_STATE
    e.phase1()
    with pytest.raises(_lib.GparmlHipError):
        e.predict(np.zeros((2, Q)))
    e.global_step(sync=True)
    with pytest.raises(AssertionError):
        e.predict(np.zeros((2, Q)), -np.ones((2, Q)))  # negative variance: GP_ERR_BAD_ARG
    with pytest.raises(AssertionError):
        e.predict(np.zeros((2, Q)), np.full((2, Q), np.nan))
    lib = _lib.load()
    assert lib.gp_predict(e.h, -1, None, None, 0, 0, None, None) == _lib.GP_ERR_BAD_ARG
    assert lib.gp_predict(e.h, 0, None, None, 0, 0, None, None) == _lib.GP_OK
    m, v = e.predict(np.zeros((0, Q)))
    assert m.shape == (0, D) and v.shape == (0, 1)
    e.close()


@pytest.mark.jitter_expected
def test_state_errors_after_failed_or_stale_steps():
    """GP_ERR_STATE after a global step that asked for the jitter retry, after the retry that failed too, and whenever the statistics changed
    since the last successful step (gp_set_local_statistics, gp_buffer_combine, gp_phase1)."""
    from gparml_amd import _lib
    from gparml_amd.engine import ShardEngine
    M, Q, D, N = 16, 2, 3, 100
    d = _model(N, D, M, Q, 'A', seed=25)
    e = _engine(d, N, D, M, Q)
    Xt = np.zeros((2, Q))
    e.predict(Xt)
    Psi2, C, sc = e.download('PSI2_SUM'), e.download('PSI1TY'), e.scalars()
    e.set_local_statistics(sc['sum_YYT'], -10.0 * np.eye(M), C, sc['sum_exp_K_ii'], sc['KL'])     # K + beta Psi2 indefinite
    with pytest.raises(_lib.GparmlHipError):
        e.predict(Xt)                                                   # new statistics, no global step on them yet
    e.global_step(sync=False)
    with pytest.raises(_lib.GparmlHipError):
        e.predict(Xt)                                                   # the step asks for the jitter retry
    with pytest.raises(_lib.JitterRetry):
        e.global_status()
    e.global_step(sync=False, jitter=2)
    with pytest.raises(_lib.GparmlHipError):
        e.predict(Xt)                                                   # the retry failed as well (GP_ERR_NOT_PD)
    e.set_local_statistics(sc['sum_YYT'], Psi2, C, sc['sum_exp_K_ii'], sc['KL'])
    e.global_step(sync=True)
    m1, _ = e.predict(Xt)
    other = _engine(d, N, D, M, Q)
    e.combine(other, 'stats', 'add')
    with pytest.raises(_lib.GparmlHipError):
        e.predict(Xt)                                                   # combined statistics, no global step on them yet
    e.global_step(sync=True)
    e.predict(Xt)
    e.phase1()
    with pytest.raises(_lib.GparmlHipError):
        e.predict(Xt)
    other.close()
    e.close()


def test_resident_scg_free_embeddings_then_predict():
    """SCG on a free-embedding GPLVM ends on an accepted step (update_X moves the resident embeddings after the last evaluation): predict at the
    returned x must recompute the statistics with the embeddings as they are, and match the numpy reference built from them."""
    from gparml_amd.driver import transform_vec
    from gparml_amd.resident import ResidentCG, ResidentModel
    from gparml_amd.scg_adapted import SCG_adapted
    from pipeline_util import load_pipeline
    g = load_pipeline('gplvm_2shards')
    M, Q, D = int(g['M']), int(g['Q']), int(g['D'])
    assert not bool(g['fixed'])
    shards = [(g['Y_%d' % i], g['call0_in_shard%d_embedding' % i], g['call0_in_shard%d_variance' % i]) for i in range(int(g['n_shards']))]
    model = ResidentModel(shards, M, Q, D, fixed_embeddings=False)
    x, flog, nfe, status = SCG_adapted(model.likelihood_and_gradient, g['call0_x'].copy(), ResidentCG(model), fixed_embeddings=False, maxiters=4,
                                       xtol=0, ftol=0, gtol=0)
    rs = np.random.RandomState(9)
    Xt, St = rs.randn(7, Q), rs.uniform(0.1, 0.4, size=(7, Q))
    res = [model.predict(x, Xt), model.predict(x, Xt, St)]
    # the reference: statistics of the resident embeddings as they are now (phase 1 at step 0 left them in the trial buffers)
    xt = transform_vec(model._pos, x)
    Z = xt[:M * Q].reshape(M, Q)
    sf2, alpha, beta = xt[M * Q], xt[M * Q + 1:M * Q + 1 + Q], xt[M * Q + 1 + Q]
    Psi2, C = np.zeros((M, M)), np.zeros((M, D))
    for (Y, _, _), e in zip(shards, model.engines):
        p2, c = R.statistics(Z, sf2, alpha, Y, e.download('X_MU_TRIAL'), e.download('X_S_TRIAL'))
        Psi2 += p2
        C += c
    for (m, v), X_S in zip(res, (None, St)):
        mr, vr = R.predict(Z, sf2, alpha, beta, Psi2, C, Xt, X_S)
        _close(m, mr, 1e-9, max(1.0, np.max(np.abs(mr))), 'mean')
        _close(v, vr, 1e-9, sf2, 'var')
    model.close()


def test_gplvm_reconstruction_on_the_fixture():
    from conftest import GOLDEN_DIR
    from gparml_amd.predict import Predictor
    z = np.load(os.path.join(GOLDEN_DIR, 'predict_gplvm_2shards.npz'))
    gs = dict(Z=z['global_Z'], sf2=z['global_sf2'], alpha=z['global_alpha'], beta=z['global_beta'])
    acc = {k: z['acc_' + k] for k in ('sum_YYT', 'sum_exp_K_mi_K_im', 'sum_exp_K_miY', 'sum_exp_K_ii', 'sum_KL')}
    p = Predictor(gs, acc, int(z['N']), int(z['D']))
    Xm, Xs = z['C_best_X_mu'], z['C_best_X_S']
    m, v = p.predict_outputs(Xm, Xs)
    f = lambda x: float(np.asarray(x).reshape(-1)[0])
    mr, vr = R.predict(z['global_Z'], f(z['global_sf2']), np.asarray(z['global_alpha']).reshape(-1), f(z['global_beta']),
                       acc['sum_exp_K_mi_K_im'], acc['sum_exp_K_miY'], Xm, Xs)
    _close(m, mr, 1e-10, max(1.0, np.max(np.abs(mr))), 'mean')
    _close(v, vr, 1e-10, f(z['global_sf2']), 'var')


def test_resident_model_predict_matches_engine():
    from gparml_amd.resident import ResidentModel
    from gparml_amd.driver import transform_back
    M, Q, D, N = 24, 2, 3, 200
    d = _model(N, D, M, Q, 'A', seed=23, spread=1.5)
    rm = ResidentModel([(d['Y'], d['X_mu'], d['X_S'])], M, Q, D, fixed_embeddings=True)
    x = np.concatenate([d['Z'].ravel(), [d['sf2']], d['alpha'], [d['beta']]])
    flat = np.array([transform_back(b, v) for b, v in zip(rm.bounds, x)])
    Xt = np.random.RandomState(3).randn(17, Q)
    m0, v0 = rm.predict(flat, Xt)                     # no evaluation yet: runs the statistics part itself
    rm.likelihood_and_gradient(flat, 0)
    m1, v1 = rm.predict(flat, Xt)                     # the last evaluation's statistics
    e = _engine(d, N, D, M, Q)
    mr, vr = _ref(e, d, Xt)
    tol = _tol(d, M)
    for m, v in ((m0, v0), (m1, v1)):
        _close(m, mr, max(tol, 1e-9), max(1.0, np.max(np.abs(mr))), 'mean')
        _close(v, vr, max(tol, 1e-9), d['sf2'], 'var')
    rm.close()
    e.close()


def test_poison_mode():
    """Every other test of this file again with every prediction buffer (and the library's other buffers) NaN-filled on allocation."""
    from gparml_amd import _lib
    lib = _lib.load()
    lib.gp_debug_set_option(b'poison_alloc', 1)
    try:
        for args in (5, 1, 1, 'A'), (64, 2, 3, 'B'), (130, 17, 3, 'B'), (130, 10, 100, 'A'), (64, 50, 3, 'B'), (64, 70, 3, 'B'), (512, 10, 100, 'B'), \
                (64, 3, 300, 'B'):
            test_against_numpy_reference(*args)
        for t in (test_exact_gp_limit, test_quadrature_identity_q2, test_continuity_of_the_uncertain_path, test_no_side_effects_and_determinism,
                  test_combined_statistics_predict_like_one_context, test_state_and_argument_errors, test_resident_scg_free_embeddings_then_predict,
                  test_gplvm_reconstruction_on_the_fixture, test_resident_model_predict_matches_engine, test_benchmark_size):
            t()
    finally:
        lib.gp_debug_set_option(b'poison_alloc', 0)


def _bench_model():
    """bench.py's configs[2] model (same generator, alpha 0.1, beta 10) at N = 4000, its statistics scaled by 250: the sums of N = 1e6 such points,
    so Kmm + beta Psi2 has the benchmark's conditioning (cond ~1e10)."""
    from gparml_amd.engine import ShardEngine
    M, Q, D, N = 512, 10, 100, 4000
    rs = np.random.RandomState(0)
    X = rs.randn(N, Q)
    Y = np.sin(X.dot(np.random.RandomState(1234).randn(Q, D))) + 0.1 * rs.randn(N, D)
    X_mu = X + 0.05 * rs.randn(N, Q)
    rz = np.random.RandomState(1)
    Z = np.random.RandomState(0).randn(4 * M, Q)[rz.permutation(4 * M)[:M]] + 0.05 * rz.randn(M, Q)
    d = dict(Z=Z, sf2=1.0, alpha=np.full(Q, 0.1), beta=10.0)
    e = ShardEngine(N, D, M, Q)
    e.upload_shard(Y, X_mu, np.zeros((N, Q)))
    e.set_globals(Z, 1.0, d['alpha'], 10.0, N_global=250 * N)
    e.phase1()
    f = 250.0
    sc = e.scalars()
    d['Psi2'], d['C'] = f * e.download('PSI2_SUM'), f * e.download('PSI1TY')
    e.set_local_statistics(f * sc['sum_YYT'], d['Psi2'], d['C'], f * sc['sum_exp_K_ii'], f * sc['KL'])
    e.global_step(sync=True)
    return e, d


def test_benchmark_size():
    """configs[2]'s model at its conditioning, n = 1e5 deterministic and 2e3 uncertain points; a row sample against the long-double reference
    (tests/predict_ref.py predict_ld, from the same float64 statistics).  The bounds are the errors DESIGN.md section 11 records, with a margin."""
    from oracle import literal as L
    e, d = _bench_model()
    M = d['Z'].shape[0]
    K = L.rbf_gram(d['Z'], d['sf2'], d['alpha'])
    cond_k, cond_a = np.linalg.cond(K), np.linalg.cond(K + d['beta'] * d['Psi2'])
    rs = np.random.RandomState(12)
    Xt = 0.05 * rs.randn(100000, 10) + rs.randn(100000, 10)
    St = rs.uniform(0.05, 0.5, size=(2000, 10))
    m, v = e.predict(Xt)
    mu, vu = e.predict(Xt[:2000], St)
    idx = rs.choice(2000, 24, replace=False)
    iu = idx[:6]
    mr, vr = R.predict_ld(d['Z'], d['sf2'], d['alpha'], d['beta'], d['Psi2'], d['C'], Xt[idx])
    mur, vur = R.predict_ld(d['Z'], d['sf2'], d['alpha'], d['beta'], d['Psi2'], d['C'], Xt[iu], St[iu])
    err = lambda a, b: float(np.max(np.abs(np.asarray(a, dtype=np.longdouble) - b)))
    errs = dict(cond_kmm=cond_k, cond_a=cond_a, mean_scale=float(np.max(np.abs(mr))), mean_det=err(m[idx], mr), var_det=err(v[idx], vr),
                mean_unc=err(mu[iu], mur), var_unc=err(vu[iu], vur), var_det_min=float(np.min(vr)), var_unc_min=float(np.min(vur)))
    print('[predict benchmark-size errors]', errs)
    out = os.environ.get('GPARML_PREDICT_ERR_OUT')
    if out:
        import json
        with open(out, 'w') as fh:
            json.dump({k: float(x) for k, x in errs.items()}, fh)
    assert cond_a > 1e9
    assert errs['mean_det'] <= TOL_BENCH['mean'] and errs['mean_unc'] <= TOL_BENCH['mean']
    assert errs['var_det'] <= TOL_BENCH['var_det'] and errs['var_unc'] <= TOL_BENCH['var_unc']
    e.close()


# measured on MI355X at cond(Kmm + beta Psi2) = 1.9e10: mean 4.5e-9 (|mean| <= 3.7), var 7.6e-13 (deterministic),
# 1.7e-9 (uncertain), sf2 = 1; the bounds are about 20x those
TOL_BENCH = dict(mean=1e-7, var_det=2e-11, var_unc=4e-8)
