"""gp_predict_grad on the GPU: the Jacobian of the predictive mean, the derivative of the variance, the expected metric tensor and its log-determinant
at new inputs against tests/grad_ref.py (numpy; the long-double form is the reference)."""
import itertools

import numpy as np
import pytest

import grad_ref as G
import joint_ref as J
import predict_ref as R
from test_gpu_joint import SHAPES, _engine, _model

pytestmark = pytest.mark.gpu

KEYS = ('jac', 'dvar', 'metric', 'logdet')
_ids = ['M%d-Q%d-D%d-%s-n%d' % s for s in SHAPES]
_CASES = {}


class _Case(object):
    """One shape: the model, an engine after its global step, the new inputs, the long-double reference and the bound of each block -- the larger of
    the project's max(1e-10, 1e-16 cond) and 8 x the worse error of the two float64 numpy forms against the long-double one (the device's M-long sums
    run in another order and chunking than numpy's)."""

    def __init__(self, M, Q, D, regime, n):
        self.shape = (M, Q, D, regime, n)
        self.N = max(300, M + 100)
        self.d = d = _model(self.N, D, M, Q, regime, seed=M + Q + D)
        self.e = _engine(d, self.N, D, M, Q)
        self.X = np.random.RandomState(11).randn(n, Q)
        self.stats = (self.e.download('PSI2_SUM'), self.e.download('PSI1TY'))
        self.keys = KEYS if Q <= 64 else KEYS[:3]
        args = (d['Z'], d['sf2'], d['alpha'], d['beta']) + self.stats + (self.X,)
        self.ref = G.grad_ld(*args)
        self.cond_tol = J.cond_tol(d['Z'], d['sf2'], d['alpha'], d['beta'], self.stats[0])
        forms = [G.grad(*args), G.grad_B(*args)]
        self.np_err = {k: [_err(f[k], self.ref[k]) for f in forms] for k in KEYS}
        self.bound = {k: max(self.cond_tol, 8.0 * max(self.np_err[k])) for k in KEYS}
        self.full = self.e.predict_grad(self.X, **{k: k in self.keys for k in KEYS})


def _err(a, b):
    b = np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(np.asarray(a, dtype=np.longdouble) - b)) / np.max(np.abs(b)))


def _case(shape):
    if shape not in _CASES:
        _CASES[shape] = _Case(*shape)
    return _CASES[shape]


@pytest.fixture(scope='module', autouse=True)
def _close_engines():
    yield
    for c in _CASES.values():
        c.e.close()
    _CASES.clear()


def _check_parity(c, got, what):
    bad = []
    for k in c.keys:
        err = _err(got[k], c.ref[k])
        print('[grad] %s %s %-7s device %.3g  numpy grad %.3g grad_B %.3g  bound %.3g (cond rule %.3g)' % (
            c.shape, what, k, err, c.np_err[k][0], c.np_err[k][1], c.bound[k], c.cond_tol))
        if not err <= c.bound[k]:
            bad.append('%s %.3g > %.3g' % (k, err, c.bound[k]))
    assert not bad, '%s %s: %s' % (c.shape, what, '; '.join(bad))


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_parity(shape):
    from gparml_amd import _lib
    c = _case(shape)
    assert sorted(c.full) == sorted(c.keys)
    _check_parity(c, c.full, 'parity')
    if shape[1] > 64:
        with pytest.raises(_lib.GparmlHipError, match='Q <= 64'):
            c.e.predict_grad(c.X)                                 # logdet beyond the device's width: GP_ERR_UNSUPPORTED
        lib = _lib.load()
        X, px = _lib.as_c(c.X)
        ld = np.empty(len(X))
        assert lib.gp_predict_grad(c.e.h, len(X), px, 0, None, None, None, ld.ctypes.data_as(_lib._dp)) == _lib.GP_ERR_UNSUPPORTED


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_structure(shape):
    c = _case(shape)
    M, Q, D, _, n = shape
    metric, jac = c.full['metric'], c.full['jac']
    assert metric.shape == (n, Q, Q) and jac.shape == (n, D, Q) and c.full['dvar'].shape == (n, Q)
    assert np.array_equal(metric, np.transpose(metric, (0, 2, 1))), 'metric is not symmetric bit for bit'
    only = c.e.predict_grad(c.X, jac=False, dvar=False, metric=True, logdet=False)
    assert sorted(only) == ['metric']
    assert np.array_equal(np.diagonal(only['metric'], axis1=1, axis2=2), np.diagonal(metric, axis1=1, axis2=2))
    # every subset of outputs gives the full call's bits; a second full call too
    for r in range(1, len(c.keys) + 1):
        for sub in itertools.combinations(c.keys, r):
            got = c.e.predict_grad(c.X, **{k: k in sub for k in KEYS})
            assert sorted(got) == sorted(sub)
            for k in sub:
                assert np.array_equal(got[k], c.full[k]), (sub, k)
    # E[J^T J] and D Cov(J) are positive semi-definite
    scale = np.max(np.abs(np.asarray(c.ref['metric'], dtype=float)))
    lo = np.min(np.linalg.eigvalsh(metric))
    lo_cov = np.min(np.linalg.eigvalsh(metric - np.einsum('idq,idr->iqr', jac, jac)))
    print('[grad] %s smallest eigenvalue: metric %.3g, metric - J^T J %.3g (scale %.3g)' % (shape, lo, lo_cov, scale))
    assert lo >= -c.bound['metric'] * scale and lo_cov >= -c.bound['metric'] * scale
    if 'logdet' in c.keys:
        ld = np.linalg.slogdet(metric)[1]
        err = np.max(np.abs(c.full['logdet'] - ld) / np.maximum(1.0, np.abs(ld)))
        print('[grad] %s logdet against slogdet of the returned metric: %.3g (bound %.3g)' % (shape, err, Q * 1e-14))
        assert err <= Q * 1e-14


@pytest.mark.parametrize('shape', [SHAPES[1], SHAPES[2], SHAPES[4]], ids=[_ids[1], _ids[2], _ids[4]])
def test_far_field(shape):
    """1e3 length scales beyond every inducing point: k = 0 exactly, so jac = dvar = 0 and metric = D sf2 diag(alpha)."""
    c = _case(shape)
    M, Q, D, _, n = shape
    far = np.max(c.d['Z'], axis=0) + 1e3 / np.sqrt(c.d['alpha'])
    X = np.stack([far, c.X[0], far])                              # beside an ordinary point
    m, _ = c.e.predict(X[[0, 2]])
    assert np.all(m == 0.0)
    got = c.e.predict_grad(X, logdet=False)
    want = D * c.d['sf2'] * c.d['alpha']
    for i in (0, 2):
        assert np.all(got['jac'][i] == 0.0) and np.all(got['dvar'][i] == 0.0)
        mi = got['metric'][i]
        assert np.all(mi[~np.eye(Q, dtype=bool)] == 0.0)
        assert np.all(np.abs(np.diag(mi) - want) <= 2 * np.spacing(want)), np.max(np.abs(np.diag(mi) - want) / np.spacing(want))
    for k in KEYS[:3]:
        assert np.array_equal(got[k][1], c.full[k][0]), k


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
    got = e.predict_grad(Xs)
    je, ve = G.exact_gp_grad(X, Y, sf2, alpha, beta, Xs)
    for what, a, b, scale in (('jac', got['jac'], je, max(1.0, np.max(np.abs(je)))), ('dvar', got['dvar'], ve, sf2)):
        err = np.max(np.abs(a - b)) / scale
        print('[grad] exact-GP limit %s: %.3g (tol 1e-7)' % (what, err))
        assert err <= 1e-7, (what, err)
    e.close()


@pytest.mark.parametrize('shape,alone', [(SHAPES[2], (0, 6, 7, 299)), (SHAPES[4], (0, 1, 128))], ids=[_ids[2], _ids[4]])
def test_rows_independent_and_chunking(shape, alone):
    """Chunks forced to 128 rows of T -- seven points of Q = 17 per chunk, a single point of Q = 70 -- the default chunking, and a point alone: the same bits."""
    from gparml_amd import _lib
    c = _case(shape)
    which = {k: k in c.keys for k in KEYS}
    lib = _lib.load()
    lib.gp_debug_set_option(b'predict_rows', 128)
    try:
        got = c.e.predict_grad(c.X, **which)
        solo = {i: c.e.predict_grad(c.X[i:i + 1], **which) for i in alone[:2]}
    finally:
        lib.gp_debug_set_option(b'predict_rows', 0)
    for i in alone[2:]:
        solo[i] = c.e.predict_grad(c.X[i:i + 1], **which)
    for k in c.keys:
        assert np.array_equal(got[k], c.full[k]), k
        for i in alone:
            assert np.array_equal(solo[i][k][0], c.full[k][i]), (k, i)


def test_translation():
    """X and Z moved together by 2^16 on a 2^-24 grid (the shift is exact): within the parity bound of the unshifted long-double reference."""
    M, Q, D, regime, n = SHAPES[2]
    N = max(300, M + 100)
    d = _model(N, D, M, Q, regime, seed=M + Q + D)
    grid = lambda a: np.round(a * 2.0 ** 24) / 2.0 ** 24
    d['Z'], d['X_mu'] = grid(d['Z']), grid(d['X_mu'])
    X = grid(np.random.RandomState(11).randn(n, Q))
    shift = 2.0 ** 16
    s = dict(d, Z=d['Z'] + shift, X_mu=d['X_mu'] + shift)
    assert np.array_equal(s['Z'] - shift, d['Z']) and np.array_equal((X + shift) - shift, X)
    e = _engine(s, N, D, M, Q)
    stats = (e.download('PSI2_SUM'), e.download('PSI1TY'))
    got = e.predict_grad(X + shift)
    e.close()
    args = (d['Z'], d['sf2'], d['alpha'], d['beta']) + stats + (X,)
    ref = G.grad_ld(*args)
    tol = J.cond_tol(d['Z'], d['sf2'], d['alpha'], d['beta'], stats[0])
    forms = [G.grad(*args), G.grad_B(*args)]
    for k in KEYS:
        bound = max(tol, 8.0 * max(_err(f[k], ref[k]) for f in forms))
        err = _err(got[k], ref[k])
        print('[grad] translation 2^16 %-7s %.3g (bound %.3g)' % (k, err, bound))
        assert err <= bound, (k, err, bound)


def test_state_and_argument_errors():
    from gparml_amd import _lib
    from gparml_amd.engine import ShardEngine
    M, Q, D, N = 16, 2, 3, 100
    d = _model(N, D, M, Q, 'A', seed=21)
    e = ShardEngine(N, D, M, Q)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    with pytest.raises(_lib.GparmlHipError):
        e.predict_grad(np.zeros((2, Q)))                    # no global step yet: GP_ERR_STATE
    e.phase1()
    e.global_step(sync=True)
    e.predict_grad(np.zeros((2, Q)))
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    with pytest.raises(_lib.GparmlHipError):
        e.predict_grad(np.zeros((2, Q)))                    # new globals, no global step on them
    e.phase1()
    e.global_step(sync=True)
    got = e.predict_grad(np.zeros((0, Q)))
    assert got['jac'].shape == (0, D, Q) and got['dvar'].shape == (0, Q) and got['metric'].shape == (0, Q, Q) and got['logdet'].shape == (0,)
    assert e.predict_grad(np.zeros((2, Q)), jac=False, dvar=False, metric=False, logdet=False) == {}
    bad = np.zeros((2, Q))
    bad[1, 0] = np.nan
    with pytest.raises(AssertionError):
        e.predict_grad(bad)
    lib = _lib.load()
    X, px = _lib.as_c(np.zeros((2, Q)))
    out = np.empty(2)
    assert lib.gp_predict_grad(e.h, -1, None, 0, None, None, None, None) == _lib.GP_ERR_BAD_ARG
    assert lib.gp_predict_grad(e.h, 2, px, 1, None, None, None, out.ctypes.data_as(_lib._dp)) == _lib.GP_ERR_BAD_ARG      # flags is reserved
    assert lib.gp_predict_grad(e.h, 2, None, 0, None, None, None, out.ctypes.data_as(_lib._dp)) == _lib.GP_ERR_BAD_ARG    # X is NULL
    e.close()


def _sequence(d, N, D, M, Q, grad):
    from gparml_amd.engine import ShardEngine
    e = ShardEngine(N, D, M, Q)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    e.phase1()
    e.global_step(sync=True)
    if grad:
        e.predict_grad(np.random.RandomState(1).randn(150, Q))
    e.phase2(True)
    out = e.finish()
    out['grad_X_mu'] = e.download('GRAD_X_MU')
    out['grad_X_S'] = e.download('GRAD_X_S')
    Xn = np.random.RandomState(2).randn(20, Q)
    out['predict_mean'], out['predict_var'] = e.predict(Xn)
    out['joint_mean'], out['joint_cov'] = e.predict_joint(Xn)
    e.close()
    return out


def test_no_side_effects():
    M, Q, D, N = 64, 3, 5, 500
    d = _model(N, D, M, Q, 'B', seed=13, spread=1.5)
    a = _sequence(d, N, D, M, Q, False)
    b = _sequence(d, N, D, M, Q, True)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_poison_mode():
    """One shape again with every buffer NaN-filled on allocation, in the default chunking and in chunks of 128 rows: identical bits."""
    from gparml_amd import _lib
    c = _case(SHAPES[2])
    lib = _lib.load()
    lib.gp_debug_set_option(b'poison_alloc', 1)
    try:
        d = c.d
        e = _engine(d, c.N, c.shape[2], c.shape[0], c.shape[1])
        got = e.predict_grad(c.X)
        lib.gp_debug_set_option(b'predict_rows', 128)
        got128 = e.predict_grad(c.X)
        e.close()
    finally:
        lib.gp_debug_set_option(b'predict_rows', 0)
        lib.gp_debug_set_option(b'poison_alloc', 0)
    for k in KEYS:
        assert np.array_equal(got[k], c.full[k]) and np.array_equal(got128[k], c.full[k]), k
