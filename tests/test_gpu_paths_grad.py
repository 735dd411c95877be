"""gp_paths_grad on the GPU: the derivatives of the pathwise posterior draws against tests/paths_grad_ref.py (numpy; the long-double form is the
reference), the determinism contract (a point's bits depend on the point, the plan, the model and its weights only), every status of the header,
and the Python wrappers."""
import itertools

import numpy as np
import pytest

import joint_ref as J
import paths_grad_ref as PG
import paths_ref as P
from test_gpu_joint import _engine, _model
from test_gpu_paths import CASES, _normals

pytestmark = pytest.mark.gpu

KEYS = ('jac', 'metric', 'grad', 'grad_rows', 'mean_jac')
_ids = ['M%d-Q%d-D%d-%s-n%d-F%d-S%d' % c for c in CASES]
_MODELS, _CASES = {}, {}
LD = np.longdouble
U = 2.0 ** -53


def _err(a, b):
    b = np.asarray(b, dtype=LD)
    return float(np.max(np.abs(np.asarray(a, dtype=LD) - b)) / np.max(np.abs(b)))


def _blocks(jac, jm, wv, wr):
    """The five outputs from a Jacobian (S, n, D, Q), in its own precision."""
    return dict(jac=jac, metric=np.einsum('sndq,sndr->snqr', jac, jac), grad=np.einsum('d,sndq->snq', wv.astype(jac.dtype), jac),
                grad_rows=np.einsum('snd,sndq->snq', wr.astype(jac.dtype), jac), mean_jac=jm)


class _Case(object):
    """One case: the shape's model and engine (shared by the cases of a shape), the new inputs, the normals, the long-double reference of every
    output and its bound -- the larger of the project's max(1e-10, 1e-16 cond) and 8 x the float64 mirror's error against the long-double one
    (the device's sums run in another order than numpy's) -- and the full call, computed once and left unchanged."""

    def __init__(self, M, Q, D, regime, n, F, S):
        self.case, self.shape = (M, Q, D, regime, n, F, S), (M, Q, D, regime, n)
        if self.shape not in _MODELS:
            N = max(300, M + 100)
            d = _model(N, D, M, Q, regime, seed=M + Q + D)
            e = _engine(d, N, D, M, Q)
            Psi2, C = e.download('PSI2_SUM'), e.download('PSI1TY')
            _MODELS[self.shape] = (d, e, np.random.RandomState(11).randn(n, Q), Psi2, C, J.cond_tol(d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2))
        d, e, X, Psi2, C, self.cond_tol = _MODELS[self.shape]
        self.d, self.e, self.X = d, e, X
        self.args = (d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2, C)
        self.omega, self.w, self.eps_u = _normals(d, M, Q, D, F, S)
        self.centre = d['Z'].mean(axis=0)
        rs = np.random.RandomState(9)
        self.wv, self.wr = rs.randn(D), rs.randn(S, n, D)
        self.ref = _blocks(*PG.draw_jac_ld(*self.args, X, self.omega, self.w, self.eps_u, self.centre), self.wv, self.wr)
        mirror = _blocks(*PG.draw_jac(*self.args, X, self.omega, self.w, self.eps_u, self.centre), self.wv, self.wr)
        self.np_err = {k: _err(mirror[k], self.ref[k]) for k in KEYS}
        self.bound = {k: max(self.cond_tol, 8.0 * self.np_err[k]) for k in KEYS}
        self.set()
        self.full = self.call(self.X)

    def set(self, zero=False):
        z = 0.0 if zero else 1.0
        self.e.paths_set(self.omega, z * self.w, z * self.eps_u, centre=self.centre)

    def call(self, X, rows=None, keys=KEYS):
        """The outputs `keys` at X (whose rows are rows `rows` of the case's X: the per-row weights follow): two calls, the second for grad_rows."""
        wr = self.wr if rows is None else self.wr[:, rows]
        out = {}
        first = [k for k in keys if k != 'grad_rows']
        if first:
            got = self.e.paths_grad(X, weights=self.wv if 'grad' in keys else None, jac='jac' in keys, metric='metric' in keys, want_mean='mean_jac' in keys)
            assert sorted(got) == sorted(first)
            out.update(got)
        if 'grad_rows' in keys:
            got = self.e.paths_grad(X, weights=wr, jac=False, metric=False)
            assert sorted(got) == ['grad']
            out['grad_rows'] = got['grad']
        return out


def _case(case):
    if case not in _CASES:
        _CASES[case] = _Case(*case)
    c = _CASES[case]
    c.set()                                                         # the engine of a shape holds one plan: this case's
    return c


@pytest.fixture(scope='module', autouse=True)
def _close_engines():
    yield
    for m in _MODELS.values():
        m[1].close()
    _MODELS.clear()
    _CASES.clear()


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_accuracy(case):
    """Each block relative to the reference block's largest absolute value, against the larger of max(1e-10, 1e-16 cond) and 8 x the float64
    mirror's error."""
    c = _case(case)
    M, Q, D, _, n, F, S = case
    assert c.full['jac'].shape == (S, n, D, Q) and c.full['metric'].shape == (S, n, Q, Q) and c.full['mean_jac'].shape == (n, D, Q)
    assert c.full['grad'].shape == (S, n, Q) and c.full['grad_rows'].shape == (S, n, Q)
    bad = []
    for k in KEYS:
        err = _err(c.full[k], c.ref[k])
        print('[paths_grad] %s %-9s device %.3g  numpy %.3g  bound %.3g (cond rule %.3g)  ratio %.3g' % (
            case, k, err, c.np_err[k], c.bound[k], c.cond_tol, err / c.bound[k]))
        if not err <= c.bound[k]:
            bad.append('%s %.3g > %.3g' % (k, err, c.bound[k]))
    assert not bad, '%s: %s' % (case, '; '.join(bad))


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_zero_normals_give_the_mean_jacobian(case):
    c = _case(case)
    try:
        c.set(zero=True)
        out = c.e.paths_grad(c.X, want_mean=True, metric=False)
    finally:
        c.set()
    for s in range(case[6]):
        assert np.array_equal(out['jac'][s], out['mean_jac']), 'draw %d: the mean\'s Jacobian plus exact zeros is not the mean\'s Jacobian' % s
    assert np.array_equal(out['mean_jac'], c.full['mean_jac']), 'mean_jac depends on the normals'
    pg = c.e.predict_grad(c.X, jac=True, dvar=False, metric=False, logdet=False)['jac']
    err = _err(out['mean_jac'], pg)
    print('[paths_grad] %s mean_jac against gp_predict_grad\'s jac: %.3g (bound %.3g)' % (case, err, c.bound['mean_jac']))
    assert err <= c.bound['mean_jac']


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_derived_outputs(case):
    """metric and grad are functions of the returned jac: a sum of D products in a fixed order is within (D + 2) 2^-53 of the exact sum of the
    absolute products (D roundings of the chain, or one product, the wave's butterfly and the adds across column groups on the plain path)."""
    c = _case(case)
    D = case[2]
    jac, metric = c.full['jac'], c.full['metric']
    assert np.array_equal(metric, np.transpose(metric, (0, 1, 3, 2))), 'metric is not symmetric bit for bit'
    jl, ja = jac.astype(LD), np.abs(jac)
    exact = _blocks(jl, None, c.wv, c.wr)
    room = dict(metric=np.einsum('sndq,sndr->snqr', ja, ja), grad=np.einsum('d,sndq->snq', np.abs(c.wv), ja),
                grad_rows=np.einsum('snd,sndq->snq', np.abs(c.wr), ja))
    for k in ('metric', 'grad', 'grad_rows'):
        diff = np.abs(c.full[k].astype(LD) - exact[k])
        worst = float(np.max(diff / ((D + 2) * U * room[k] + np.finfo(float).tiny)))
        print('[paths_grad] %s %-9s against the returned jac: %.3g of (D + 2) 2^-53 |.|' % (case, k, worst))
        assert worst <= 1.0, (k, worst)


def _same(a, b, what, keys=KEYS, rows=slice(None)):
    for k in keys:
        x = b[k][rows] if k == 'mean_jac' else b[k][:, rows]
        assert np.array_equal(a[k], x), '%s: %s' % (what, k)


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_a_points_bits_depend_on_the_point_alone(case):
    from gparml_amd import _lib
    c = _case(case)
    n = case[4]
    _same(c.call(c.X), c.full, 'a second call gives other bits')
    for i in (0, 1, n - 1):
        _same(c.call(c.X[i:i + 1], rows=slice(i, i + 1)), c.full, 'row %d alone' % i, rows=slice(i, i + 1))
    perm = np.random.RandomState(3).permutation(n)
    _same(c.call(c.X[perm], rows=perm), c.full, 'a permuted batch', rows=perm)
    lib = _lib.load()
    lib.gp_debug_set_option(b'paths_rows', 128)                     # floor(128 / Q) points per chunk: seven at Q = 17, one at Q = 70
    try:
        chunked = c.call(c.X)
    finally:
        lib.gp_debug_set_option(b'paths_rows', 0)
    _same(chunked, c.full, 'forced chunks')
    lo, hi = n // 3, 2 * n // 3
    _same(c.call(c.X[:hi], rows=slice(0, hi)), c.full, 'overlapping calls, the first', rows=slice(0, hi))
    _same(c.call(c.X[lo:], rows=slice(lo, n)), c.full, 'overlapping calls, the second', rows=slice(lo, n))
    # every subset of the outputs of one call (grad with the shared weights)
    one = ('jac', 'metric', 'grad', 'mean_jac')
    for r in range(1, len(one)):
        for sub in itertools.combinations(one, r):
            _same(c.call(c.X, keys=sub), c.full, 'the subset %s' % (sub,), keys=sub)


def _sequence(d, N, D, M, Q, with_grad):
    from gparml_amd.engine import ShardEngine
    e = ShardEngine(N, D, M, Q)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    e.phase1()
    e.global_step(sync=True)
    omega, w, eps_u = _normals(d, M, Q, D, 24, 3)
    e.paths_set(omega, w, eps_u)
    X = np.random.RandomState(1).randn(150, Q)
    out = {}
    if with_grad:
        g1 = e.paths_grad(X, weights=np.ones(D), want_mean=True)
        out['paths_eval_between'] = e.paths_eval(X)
        g2 = e.paths_grad(X, weights=np.ones(D), want_mean=True)
        for k in g1:
            assert np.array_equal(g1[k], g2[k]), 'gp_paths_eval between two gp_paths_grad calls changed %s' % k
    else:
        out['paths_eval_between'] = e.paths_eval(X)
    out['paths_eval'], out['paths_mean'] = e.paths_eval(X, want_mean=True)
    out['predict_mean'], out['predict_var'] = e.predict(np.random.RandomState(2).randn(20, Q))
    out.update(('predict_grad_' + k, v) for k, v in e.predict_grad(np.random.RandomState(2).randn(20, Q)).items())
    e.phase2(True)
    fin = e.finish()
    out.update(('finish_' + k, v) for k, v in fin.items())
    out['grad_X_mu'] = e.download('GRAD_X_MU')
    out['grad_X_S'] = e.download('GRAD_X_S')
    e.close()
    return out


def test_no_side_effects():
    M, Q, D, N = 64, 3, 5, 500
    d = _model(N, D, M, Q, 'B', seed=13, spread=1.5)
    a = _sequence(d, N, D, M, Q, False)
    b = _sequence(d, N, D, M, Q, True)
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_statuses():
    from gparml_amd import _lib
    from gparml_amd.engine import ShardEngine
    M, Q, D, N, F, S = 16, 2, 3, 100, 4, 2
    d = _model(N, D, M, Q, 'A', seed=21)
    omega, w, eps_u = _normals(d, M, Q, D, F, S)
    lib = _lib.load()
    dp = lambda a: a.ctypes.data_as(_lib._dp) if a is not None else None
    X, wv, wr = np.zeros((2, Q)), np.ones(D), np.ones((S, 2, D))
    jac, grad, metric, mj = np.empty((S, 2, D, Q)), np.empty((S, 2, Q)), np.empty((S, 2, Q, Q)), np.empty((2, D, Q))
    e = ShardEngine(N, D, M, Q)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    set_ = lambda: lib.gp_paths_set(e.h, S, F, dp(omega), None, dp(w), dp(eps_u))
    call = lambda n=2, x=X, flags=0, wt=wv, j=jac, g=grad, m=metric, mean=mj: lib.gp_paths_grad(e.h, n, dp(x), flags, dp(wt), dp(j), dp(g), dp(m), dp(mean))
    assert call() == _lib.GP_ERR_STATE                     # no global step yet
    e.phase1()
    e.global_step(sync=True)
    assert call() == _lib.GP_ERR_STATE                     # a model, no plan
    assert set_() == _lib.GP_OK
    assert call() == _lib.GP_OK
    ref = [a.copy() for a in (jac, grad, metric, mj)]
    assert call(flags=_lib.GP_PATHS_WEIGHTS_PER_ROW, wt=wr) == _lib.GP_OK
    assert call(j=None, g=None, wt=None, m=None) == _lib.GP_OK          # mean_jac alone
    nan = lambda a: np.where(np.arange(a.size).reshape(a.shape) == a.size - 1, np.nan, a)
    bad = dict(n0=call(n=0), n_negative=call(n=-1), x_null=call(x=None), x_nan=call(x=np.array([[0.0, np.nan], [0.0, 0.0]])),
               x_inf=call(x=np.array([[0.0, 0.0], [np.inf, 0.0]])), flag2=call(flags=2), flag3=call(flags=3), flag_minus=call(flags=-1),
               nothing=call(j=None, g=None, wt=None, m=None, mean=None), grad_without_weights=call(wt=None), weights_without_grad=call(g=None),
               w_nan=call(wt=nan(wv)), w_inf=call(wt=np.array([np.inf, 0.0, 0.0])), wr_nan=call(flags=1, wt=nan(wr)))
    for name, rc in bad.items():
        assert rc == _lib.GP_ERR_BAD_ARG, name
    assert b'gp_paths_grad' in lib.gp_last_error(e.h)
    assert call() == _lib.GP_OK                            # an argument error leaves the plan in place
    for a, r in zip((jac, grad, metric, mj), ref):
        assert np.array_equal(a, r)
    assert lib.gp_paths_clear(e.h) == _lib.GP_OK
    assert call() == _lib.GP_ERR_STATE                     # after gp_paths_clear
    assert set_() == _lib.GP_OK and call() == _lib.GP_OK
    e.phase1()
    assert call() == _lib.GP_ERR_STATE                     # gp_predict's own state rule
    e.global_step(sync=True)
    assert call() == _lib.GP_ERR_STATE, 'the plan survived gp_phase1 and a new global step'
    out = np.empty((S, 2, D))
    assert lib.gp_paths_eval(e.h, 2, dp(X), 0, dp(out), None) == _lib.GP_ERR_STATE, 'the stale plan was not dropped'
    assert set_() == _lib.GP_OK and call() == _lib.GP_OK
    for a, r in zip((jac, grad, metric, mj), ref):
        assert np.array_equal(a, r)                        # the same model, the same normals: the same bits
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    assert call() == _lib.GP_ERR_STATE
    with pytest.raises(_lib.GparmlHipError):
        e.paths_grad(X)
    e.close()


def _draws(N, D, M, Q, S, F, seed):
    from gparml_amd.predict import PathDraws
    d = _model(N, D, M, Q, 'A', seed=seed)
    e = _engine(d, N, D, M, Q)
    Psi2, C = e.download('PSI2_SUM'), e.download('PSI1TY')
    draws = PathDraws(e, d['Z'], d['alpha'], S, n_features=F, seed=7)
    rs = np.random.RandomState(7)                          # the documented use of the seed: omega, w, eps_u in this order
    om = rs.randn(F, Q) * np.sqrt(d['alpha'])
    w, eps_u = rs.randn(S, 2 * F, D), rs.randn(S, M, D)
    args = (d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2, C)
    return d, e, draws, args, (om, w, eps_u, draws.centre), J.cond_tol(d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2)


def test_path_draws_wrappers():
    """Shapes, the stale-token raise, and value_and_grad against the float64 mirror.  Bounds, with tol = max(1e-10, 1e-16 cond): the device and the
    mirror are each within tol max(1, max|f|) of the exact draw (tests/test_gpu_paths.py's bound) and within tol max|jac| of the exact Jacobian
    (test_accuracy's, whose cond rule decides at this conditioning), so they differ by at most twice that; the value and the gradient are sums of
    D products with the weights."""
    from gparml_amd.predict import PathDraws
    N, D, M, Q, S, F = 120, 2, 16, 2, 3, 64
    d, e, draws, args, nrm, tol = _draws(N, D, M, Q, S, F, 21)
    X = np.random.RandomState(4).randn(50, Q)
    wv, wr = np.array([0.75, -1.25]), np.random.RandomState(8).randn(S, 50, D)
    jac, met = draws.jacobian(X), draws.metric(X)
    assert jac.shape == (S, 50, D, Q) and met.shape == (S, 50, Q, Q)
    ref_f, _ = P.draws(*args, X, *nrm)
    ref_j, _ = PG.draw_jac(*args, X, *nrm)
    fs, js = 2.0 * max(1.0, np.max(np.abs(ref_f))), 2.0 * np.max(np.abs(ref_j))
    assert np.max(np.abs(jac - ref_j)) <= tol * js
    for wts, val_ref, grad_ref, wmax in ((wv, np.einsum('snd,d->sn', ref_f, wv), np.einsum('d,sndq->snq', wv, ref_j), np.sum(np.abs(wv))),
                                         (wr, np.einsum('snd,snd->sn', ref_f, wr), np.einsum('snd,sndq->snq', wr, ref_j), np.max(np.sum(np.abs(wr), axis=2)))):
        val, grad = draws.value_and_grad(X, wts)
        assert val.shape == (S, 50) and grad.shape == (S, 50, Q)
        ev, eg = np.max(np.abs(val - val_ref)), np.max(np.abs(grad - grad_ref))
        print('[paths_grad] value_and_grad: value %.3g (bound %.3g), grad %.3g (bound %.3g)' % (ev, wmax * tol * fs, eg, wmax * tol * js))
        assert ev <= wmax * tol * fs and eg <= wmax * tol * js
    second = PathDraws(e, d['Z'], d['alpha'], 2, n_features=8, seed=2)
    assert second.jacobian(X).shape == (2, 50, D, Q)
    for stale in (lambda: draws.jacobian(X), lambda: draws.metric(X), lambda: draws.value_and_grad(X, wv), lambda: draws.curve_energy(X.reshape(10, 5, Q))):
        with pytest.raises(RuntimeError):
            stale()
    second.close()
    with pytest.raises(RuntimeError):
        second.metric(X)
    e.close()


@pytest.mark.parametrize('T', [2, 5])
def test_curve_energy_on_the_sampled_surfaces(T):
    """energy[s, c] = 1/2 (T - 1) sum_t |f_s(x_{t+1}) - f_s(x_t)|^2 and its gradient, against the same sum on paths_ref.draws and the analytic
    gradient 1/2 (T - 1) sum_d w[s, t, d] jac[s, t, d, :], w = 2 (2 f_t - f_{t-1} - f_{t+1}) (one-sided at the ends; T = 2: both points are ends).
    Bounds, with every draw within e_f = 2 tol max(1, max|f|) and every Jacobian element within e_j = 2 tol max|jac| of the float64 mirror (each
    side within tol of the exact value, as in test_path_draws_wrappers): a difference df
    moves by at most 2 e_f, so a squared difference by 4 e_f |df| + 4 e_f^2, (T - 1) D of them per curve; a weight (coefficients 2, 4, 2 at
    most) moves by at most 8 e_f, so a product w x jac by 8 e_f max|jac| + max|w| e_j + 8 e_f e_j, D of them per gradient element."""
    N, D, M, Q, S, F, C = 120, 2, 16, 2, 3, 64, 7
    d, e, draws, args, nrm, tol = _draws(N, D, M, Q, S, F, 21)
    rs = np.random.RandomState(12)
    X = np.cumsum(0.3 * rs.randn(C, T, Q), axis=1) + rs.randn(C, 1, Q)
    energy, grad = draws.curve_energy(X)
    assert energy.shape == (S, C) and grad.shape == (S, C, T, Q)
    f = P.draws(*args, X.reshape(C * T, Q), *nrm)[0].reshape(S, C, T, D)
    jac = PG.draw_jac(*args, X.reshape(C * T, Q), *nrm)[0].reshape(S, C, T, D, Q)
    df = f[:, :, 1:] - f[:, :, :-1]
    half = 0.5 * (T - 1)
    e_ref = half * np.sum(df ** 2, axis=(2, 3))
    w = np.zeros_like(f)
    for t in range(T):
        if t > 0:
            w[:, :, t] += 2.0 * (f[:, :, t] - f[:, :, t - 1])
        if t < T - 1:
            w[:, :, t] += 2.0 * (f[:, :, t] - f[:, :, t + 1])
    g_ref = half * np.einsum('sctd,sctdq->sctq', w, jac)
    e_f, e_j = 2.0 * tol * max(1.0, np.max(np.abs(f))), 2.0 * tol * np.max(np.abs(jac))
    b_energy = half * (T - 1) * D * (4 * e_f * np.max(np.abs(df)) + 4 * e_f ** 2)
    b_grad = half * D * (8 * e_f * np.max(np.abs(jac)) + np.max(np.abs(w)) * e_j + 8 * e_f * e_j)
    ee, eg = np.max(np.abs(energy - e_ref)), np.max(np.abs(grad - g_ref))
    print('[paths_grad] curve_energy T = %d: energy %.3g (bound %.3g), grad %.3g (bound %.3g)' % (T, ee, b_energy, eg, b_grad))
    assert ee <= b_energy and eg <= b_grad
    draws.close()
    e.close()
