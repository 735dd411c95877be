"""gp_predict_joint / gp_predict_sample on the GPU: the joint posterior covariance and coherent draws at new inputs against tests/joint_ref.py (numpy)."""
import numpy as np
import pytest

import joint_ref as J
import predict_ref as R

pytestmark = pytest.mark.gpu

# one tile and three tiles, a ragged last tile, Mp = 128 and 256 (the sign boundary after one and after two k-tiles), both sides of the staged latent
# width (32), D beyond one GEMM tile's padding
SHAPES = [(5, 1, 1, 'A', 37), (64, 2, 3, 'B', 129), (130, 17, 3, 'B', 300), (130, 10, 100, 'A', 300), (64, 70, 3, 'B', 129)]


def _model(N, D, M, Q, regime, seed=0, spread=1.5):
    """tests/test_gpu_predictive.py's model: inducing points drawn apart from the data and a lengthscale short enough for cond(Kmm) < 1e6."""
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


def _setup(M, Q, D, regime, n):
    N = max(300, M + 100)
    d = _model(N, D, M, Q, regime, seed=M + Q + D)
    e = _engine(d, N, D, M, Q)
    X = np.random.RandomState(11).randn(n, Q)
    return d, e, X


def _close(a, b, tol, scale, what):
    err = np.max(np.abs(a - b)) / scale
    print('%s: %.3g (tol %.3g)' % (what, err, tol))
    assert err <= tol, '%s: %.3g > %.3g' % (what, err, tol)


def gamma(k):
    u = 2.0 ** -53
    return k * u / (1.0 - k * u)


# Lc is read off draws of unit columns, out = mean + Lc e_j, by subtracting the returned mean.  With a plain 1 the sum mean + Lc[i][j] is rounded at the
# size of the mean, and the recovered column carries an absolute error of 2^-53 |mean| that the device's Lc does not have.  The columns are therefore
# scaled by a power of two (exact in the product): the sum is rounded at the size of 2^30 Lc[i][j], so the recovered Lc is the device's to two
# roundings of its own size, and an exact zero above the diagonal stays one.
LC_SCALE = 2.0 ** 30


def _recover_Lc(e, X, n, D, scale):
    eps = np.zeros((n, n, D))
    eps[np.arange(n), np.arange(n), 0] = scale                     # draw j: the unit column j in output 0 (all D outputs share Lc)
    draws, mean = e.predict_sample(X, n, include_noise=True, jitter=0.0, eps=eps)
    return ((draws[:, :, 0] - mean[None, :, 0]) / scale).T, draws, mean     # Lc[i][j] = draw j, point i


def _check_shape(M, Q, D, regime, n):
    """The covariance and the factor checks of one shape; returns the device's arrays (the poison test compares their bits)."""
    d, e, X = _setup(M, Q, D, regime, n)
    Psi2, C = e.download('PSI2_SUM'), e.download('PSI1TY')
    tol = J.cond_tol(d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2)
    out = []
    for noise in (False, True):
        m, c = e.predict_joint(X, include_noise=noise)
        mr, cr = J.joint(d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2, C, X, include_noise=noise)
        _close(m, mr, tol, max(1.0, np.max(np.abs(mr))), 'mean')
        _close(c, cr, tol, d['sf2'], 'cov (noise %d)' % noise)
        assert np.array_equal(c, c.T), 'cov is not symmetric bit for bit'
        _, v = e.predict(X, include_noise=noise)
        _close(np.diag(c), v[:, 0], tol, d['sf2'], 'diag(cov) against gp_predict')
        m2, c2 = e.predict_joint(X, include_noise=noise)
        assert np.array_equal(m, m2) and np.array_equal(c, c2), 'a second call gives other bits'
        out += [m, c]
    # the factor, on the noise-flag case
    cov_y = c
    Lc, draws, mean = _recover_Lc(e, X, n, D, LC_SCALE)
    assert np.array_equal(mean, m)
    assert np.all(np.triu(Lc, 1) == 0.0), 'Lc is not lower triangular'
    assert np.all(np.diag(Lc) > 0)
    res = np.max(np.abs(Lc.dot(Lc.T) - cov_y)) / np.max(np.abs(cov_y))
    Ln = np.linalg.cholesky(cov_y)
    res_np = np.max(np.abs(Ln.dot(Ln.T) - cov_y)) / np.max(np.abs(cov_y))
    print('factor residual %.3g, numpy %.3g, cond(cov_y) %.3g' % (res, res_np, np.linalg.cond(cov_y)))
    assert res <= 4.0 * res_np, (res, res_np)
    eps2 = np.random.RandomState(5).randn(2, n, D)
    draws2, mean2 = e.predict_sample(X, 2, include_noise=True, jitter=0.0, eps=eps2)
    for s in range(2):
        err, bound = np.abs(draws2[s] - (mean2 + Lc.dot(eps2[s]))), gamma(n + 2) * np.abs(Lc).dot(np.abs(eps2[s]))
        print('draw %d at %.3g of its bound' % (s, np.max(err / bound)))
        assert np.all(err <= bound), float(np.max(err / bound))
    out += [draws, draws2]
    e.close()
    return out


@pytest.mark.parametrize('M,Q,D,regime,n', SHAPES)
def test_covariance_and_factor(M, Q, D, regime, n):
    _check_shape(M, Q, D, regime, n)


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
    m, c = e.predict_joint(Xs, include_noise=True)
    me, ce = J.exact_gp_joint(X, Y, sf2, alpha, beta, Xs)
    _close(m, me, 1e-7, max(1.0, np.max(np.abs(me))), 'mean')
    _close(c, ce, 1e-7, sf2, 'cov_y')
    e.close()


def test_chunking():
    from gparml_amd import _lib
    M, Q, D, regime, n = SHAPES[2]
    d, e, X = _setup(M, Q, D, regime, n)
    tol = J.cond_tol(d['Z'], d['sf2'], d['alpha'], d['beta'], e.download('PSI2_SUM'))
    m0, c0 = e.predict_joint(X)
    lib = _lib.load()
    lib.gp_debug_set_option(b'predict_rows', 128)
    try:
        m1, c1 = e.predict_joint(X)                        # 300 points: two chunks of 128 and one of 44
        dr1, _ = e.predict_sample(X, 1, include_noise=True, seed=1)
    finally:
        lib.gp_debug_set_option(b'predict_rows', 0)
    dr0, _ = e.predict_sample(X, 1, include_noise=True, seed=1)
    _close(m1, m0, tol, max(1.0, np.max(np.abs(m0))), 'mean, chunks of 128')
    _close(c1, c0, tol, d['sf2'], 'cov, chunks of 128')
    assert np.array_equal(c1, c1.T)
    assert np.all(np.isfinite(dr1)) and dr1.shape == dr0.shape
    e.close()


def _sequence(d, N, D, M, Q, joint):
    from gparml_amd.engine import ShardEngine
    e = ShardEngine(N, D, M, Q)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    e.phase1()
    e.global_step(sync=True)
    if joint:
        rs = np.random.RandomState(1)
        e.predict_joint(rs.randn(150, Q))
        e.predict_sample(rs.randn(150, Q), 3, include_noise=True, seed=2)
    e.phase2(True)
    out = e.finish()
    out['grad_X_mu'] = e.download('GRAD_X_MU')
    out['grad_X_S'] = e.download('GRAD_X_S')
    out['predict_mean'], out['predict_var'] = e.predict(np.random.RandomState(2).randn(20, Q))
    e.close()
    return out


def test_state_and_argument_errors():
    from gparml_amd import _lib
    from gparml_amd.engine import ShardEngine
    M, Q, D, N = 16, 2, 3, 100
    d = _model(N, D, M, Q, 'A', seed=21)
    e = ShardEngine(N, D, M, Q)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    with pytest.raises(_lib.GparmlHipError):
        e.predict_joint(np.zeros((2, Q)))                 # no global step yet: GP_ERR_STATE
    e.phase1()
    e.global_step(sync=True)
    e.predict_joint(np.zeros((2, Q)))
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    with pytest.raises(_lib.GparmlHipError):
        e.predict_joint(np.zeros((2, Q)))                 # new globals, no global step on them
    with pytest.raises(_lib.GparmlHipError):
        e.predict_sample(np.zeros((2, Q)), 1)
    e.phase1()
    e.global_step(sync=True)
    m, c = e.predict_joint(np.zeros((0, Q)))
    assert m.shape == (0, D) and c.shape == (0, 0)
    dr, m = e.predict_sample(np.zeros((0, Q)), 2)
    assert dr.shape == (2, 0, D) and m.shape == (0, D)
    dr, _ = e.predict_sample(np.zeros((3, Q)), 0)
    assert dr.shape == (0, 3, D)
    lib = _lib.load()
    with pytest.raises(_lib.GparmlHipError, match='16384'):
        e.predict_joint(np.zeros((16385, Q)))             # GP_ERR_UNSUPPORTED, before anything is allocated
    with pytest.raises(_lib.GparmlHipError, match='8192'):
        e.predict_sample(np.zeros((8193, Q)), 1, eps=np.zeros((1, 8193, D)))
    bad = np.zeros((2, Q))
    bad[1, 0] = np.nan
    with pytest.raises(AssertionError):
        e.predict_joint(bad)
    with pytest.raises(AssertionError):
        e.predict_sample(np.zeros((2, Q)), 1, jitter=-1)
    assert lib.gp_predict_joint(e.h, -1, None, 0, None, None) == _lib.GP_ERR_BAD_ARG
    assert lib.gp_predict_sample(e.h, 2, None, 0, 0.0, -1, None, None, None) == _lib.GP_ERR_BAD_ARG
    e.close()


def test_no_side_effects():
    M, Q, D, N = 64, 3, 5, 500
    d = _model(N, D, M, Q, 'B', seed=13, spread=1.5)
    a = _sequence(d, N, D, M, Q, False)
    b = _sequence(d, N, D, M, Q, True)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_poison_mode():
    """One shape again with every buffer NaN-filled on allocation: identical bits."""
    from gparml_amd import _lib
    ref = _check_shape(*SHAPES[2])
    lib = _lib.load()
    lib.gp_debug_set_option(b'poison_alloc', 1)
    try:
        got = _check_shape(*SHAPES[2])
    finally:
        lib.gp_debug_set_option(b'poison_alloc', 0)
    for x, y in zip(ref, got):
        assert np.array_equal(x, y)
