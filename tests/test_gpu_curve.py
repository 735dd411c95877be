"""gp_curve_energy on the GPU: the expected energy of discrete curves under the posterior of f, its segments and its gradient against tests/curve_ref.py
(numpy; the long-double form is the reference), and Predictor.geodesic on top of it."""
import itertools

import numpy as np
import pytest

import curve_ref as CR
import joint_ref as J
from test_gpu_joint import SHAPES, _engine, _model

pytestmark = pytest.mark.gpu

KEYS = ('energy', 'seg', 'grad')
WANT = {'energy': 'want_energy', 'seg': 'want_segments', 'grad': 'want_grad'}
N_CURVES, T_POINTS = 7, 9
_ids = ['M%d-Q%d-D%d-%s' % s[:4] for s in SHAPES]
_CASES = {}


def _err(a, b):
    b = np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(np.asarray(a, dtype=np.longdouble) - b)) / np.max(np.abs(b)))


def _call(e, X, keys=KEYS):
    return e.curve_energy(X, **{WANT[k]: k in keys for k in KEYS})


def _walks(rs, n, T, Q, alpha, step=0.3):
    """n random walks of T points from standard-normal starts, steps of ``step`` length scales per coordinate."""
    return rs.randn(n, 1, Q) + np.cumsum(step * rs.randn(n, T, Q) / np.sqrt(alpha), axis=1)


class _Reference(object):
    """The long-double reference of a set of curves and the bound of each block: the larger of the project's max(1e-10, 1e-16 cond) and 8 x the worse
    error of the two float64 numpy forms against the long-double one."""

    def __init__(self, case, X):
        self.X = X
        args = (case.d['Z'], case.d['sf2'], case.d['alpha'], case.d['beta']) + case.stats + (X,)
        self.ref = CR.curve_ld(*args)
        forms = [CR.curve(*args), CR.curve_B(*args)]
        self.np_err = {k: [_err(f[k], self.ref[k]) for f in forms] for k in KEYS}
        self.bound = {k: max(case.cond_tol, 8.0 * max(self.np_err[k])) for k in KEYS}


class _Case(object):
    """One shape: the model, an engine after its global step, seven curves of nine points and three of two, their references and the device's results."""

    def __init__(self, M, Q, D, regime, n):
        self.shape = (M, Q, D, regime)
        self.N = max(300, M + 100)
        self.d = d = _model(self.N, D, M, Q, regime, seed=M + Q + D)
        self.e = _engine(d, self.N, D, M, Q)
        self.stats = (self.e.download('PSI2_SUM'), self.e.download('PSI1TY'))
        self.cond_tol = J.cond_tol(d['Z'], d['sf2'], d['alpha'], d['beta'], self.stats[0])
        rs = np.random.RandomState(11)
        self.long = _Reference(self, _walks(rs, N_CURVES, T_POINTS, Q, d['alpha']))
        self.short = _Reference(self, _walks(rs, 3, 2, Q, d['alpha']))
        self.X = self.long.X
        self.full = _call(self.e, self.X)


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


def _check_parity(c, r, got, what):
    bad = []
    for k in KEYS:
        err = _err(got[k], r.ref[k])
        print('[curve] %s %s %-6s device %.3g  numpy curve %.3g curve_B %.3g  bound %.3g (cond rule %.3g)' % (
            c.shape, what, k, err, r.np_err[k][0], r.np_err[k][1], r.bound[k], c.cond_tol))
        if not err <= r.bound[k]:
            bad.append('%s %.3g > %.3g' % (k, err, r.bound[k]))
    assert not bad, '%s %s: %s' % (c.shape, what, '; '.join(bad))


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_parity(shape):
    c = _case(shape)
    M, Q, D, _ = c.shape
    assert sorted(c.full) == sorted(KEYS)
    assert c.full['energy'].shape == (N_CURVES,) and c.full['seg'].shape == (N_CURVES, T_POINTS - 1) and c.full['grad'].shape == (N_CURVES, T_POINTS, Q)
    _check_parity(c, c.long, c.full, 'T = %d' % T_POINTS)
    _check_parity(c, c.short, _call(c.e, c.short.X), 'T = 2')
    one = c.e.curve_energy(c.X[3], want_segments=True)                 # a single curve (T, Q): no leading axis, the same bits
    for k in KEYS:
        assert one[k].shape == c.full[k].shape[1:] and np.array_equal(one[k], c.full[k][3]), k


def test_fine_discretisation_and_a_repeated_point():
    """Adjacent points 2^-20 length scales apart: the differences of Psi1 and of the prior lose nothing (a difference of two exponentials would lose
    about six digits); a repeated point gives a zero segment exactly."""
    c = _case(SHAPES[1])
    M, Q, D, _ = c.shape
    rs = np.random.RandomState(3)
    u = rs.randn(Q)
    u /= np.sqrt(np.sum(c.d['alpha'] * u * u))                        # one length scale long
    fine = rs.randn(Q) + 2.0 ** -20 * np.arange(T_POINTS)[:, None] * u
    rep = c.X[0].copy()
    rep[4] = rep[3]
    got = _call(c.e, np.stack([fine, rep]))
    _check_parity(c, _Reference(c, fine[None]), {k: got[k][:1] for k in KEYS}, 'fine')            # the fine curve's blocks on their own scale
    _check_parity(c, _Reference(c, rep[None]), {k: got[k][1:] for k in KEYS}, 'repeated point')
    assert got['seg'][1, 3] == 0.0 and np.all(got['seg'][1, [0, 1, 2, 4, 5, 6, 7]] > 0.0)
    assert np.all(np.isfinite(got['grad'])) and np.all(got['seg'][0] > 0.0)


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_structure(shape):
    from gparml_amd.predict import Predictor
    c = _case(shape)
    M, Q, D, _ = c.shape
    seg, energy, grad = c.full['seg'], c.full['energy'], c.full['grad']
    assert np.all(seg >= 0.0)
    # energy = 1/2 (T - 1) sum_s seg, s ascending
    for i in range(N_CURVES):
        t = 0.0
        for s in range(T_POINTS - 1):
            t += seg[i, s]
        want = 0.5 * (T_POINTS - 1) * t
        assert abs(energy[i] - want) <= 2 * np.spacing(want), (i, energy[i], want)
    # the reversed curve: the same energy within the parity bound, the reversed gradient
    rev = _call(c.e, c.X[:, ::-1])
    scale_e, scale_g = np.max(np.abs(energy)), np.max(np.abs(grad))
    err_e = np.max(np.abs(rev['energy'] - energy)) / scale_e
    err_g = np.max(np.abs(rev['grad'][:, ::-1] - grad)) / scale_g
    print('[curve] %s reversed: energy %.3g grad %.3g (bounds %.3g %.3g)' % (c.shape, err_e, err_g, c.long.bound['energy'], c.long.bound['grad']))
    assert err_e <= c.long.bound['energy'] and err_g <= c.long.bound['grad']
    # the expected length is at least the length of the posterior mean's curve
    mean, _ = c.e.predict(c.X.reshape(-1, Q))
    mean = mean.reshape(N_CURVES, T_POINTS, D)
    mean_len = np.sum(np.sqrt(np.sum((mean[:, 1:] - mean[:, :-1]) ** 2, axis=2)), axis=1)
    length = Predictor._length(seg)
    print('[curve] %s length / length of the mean curve: %s' % (c.shape, length / mean_len))
    assert np.all(length >= mean_len * (1 - c.long.bound['seg']))


@pytest.mark.parametrize('shape', [SHAPES[2], SHAPES[3], SHAPES[4]], ids=[_ids[2], _ids[3], _ids[4]])
def test_deterministic_and_independent_of_the_batch(shape):
    """A second run, a curve alone, first and last in a batch, chunks of one curve and of three, and every subset of outputs: the same bits."""
    from gparml_amd import _lib
    c = _case(shape)
    again = _call(c.e, c.X)
    for k in KEYS:
        assert np.array_equal(again[k], c.full[k]), k
    lib = _lib.load()
    other = _call(c.e, c.X[[5, 0, 6, 2, 5]])                           # curve 5 first and last, another order
    alone = {i: _call(c.e, c.X[i:i + 1]) for i in (0, 5, 6)}
    try:
        lib.gp_debug_set_option(b'curve_curves', 1)
        one = _call(c.e, c.X)
        lib.gp_debug_set_option(b'curve_curves', 3)                    # chunks of 3, 3 and 1 curves
        three = _call(c.e, c.X)
    finally:
        lib.gp_debug_set_option(b'curve_curves', 0)
    for k in KEYS:
        assert np.array_equal(one[k], c.full[k]) and np.array_equal(three[k], c.full[k]), k
        assert np.array_equal(other[k], c.full[k][[5, 0, 6, 2, 5]]), k
        for i in alone:
            assert np.array_equal(alone[i][k][0], c.full[k][i]), (k, i)
    for r in range(1, len(KEYS)):
        for sub in itertools.combinations(KEYS, r):
            got = _call(c.e, c.X, sub)
            assert sorted(got) == sorted(sub)
            for k in sub:
                assert np.array_equal(got[k], c.full[k]), (sub, k)
    assert _call(c.e, c.X, ()) == {}


def test_poison_mode():
    """One shape again with every buffer NaN-filled on allocation, in the default chunking, in chunks of one curve and for every subset of outputs."""
    from gparml_amd import _lib
    c = _case(SHAPES[2])
    lib = _lib.load()
    lib.gp_debug_set_option(b'poison_alloc', 1)
    try:
        e = _engine(c.d, c.N, c.shape[2], c.shape[0], c.shape[1])
        got = _call(e, c.X)
        subs = {sub: _call(e, c.X, sub) for r in (1, 2) for sub in itertools.combinations(KEYS, r)}
        lib.gp_debug_set_option(b'curve_curves', 1)
        got1 = _call(e, c.X)
        e.close()
    finally:
        lib.gp_debug_set_option(b'curve_curves', 0)
        lib.gp_debug_set_option(b'poison_alloc', 0)
    for k in KEYS:
        assert np.array_equal(got[k], c.full[k]) and np.array_equal(got1[k], c.full[k]), k
    for sub, g in subs.items():
        for k in sub:
            assert np.array_equal(g[k], c.full[k]), (sub, k)


def test_state_and_argument_errors():
    from gparml_amd import _lib
    from gparml_amd.engine import ShardEngine
    M, Q, D, N = 16, 2, 3, 100
    d = _model(N, D, M, Q, 'A', seed=21)
    e = ShardEngine(N, D, M, Q)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    lib = _lib.load()
    X, px = _lib.as_c(np.random.RandomState(1).randn(2, 3, Q))
    SENTINEL = -12345.0
    en, sg, gr = np.full(2, SENTINEL), np.full((2, 2), SENTINEL), np.full((2, 3, Q), SENTINEL)
    dp = lambda a: a.ctypes.data_as(_lib._dp)
    call = lambda n, T, p, flags: lib.gp_curve_energy(e.h, n, T, p, flags, dp(en), dp(sg), dp(gr))
    untouched = lambda: np.all(en == SENTINEL) and np.all(sg == SENTINEL) and np.all(gr == SENTINEL)
    assert call(2, 3, px, 0) == _lib.GP_ERR_STATE and untouched()          # no global step yet
    e.phase1()
    e.global_step(sync=True)
    assert call(2, 3, px, 0) == _lib.GP_OK and not np.any(en == SENTINEL) and not np.any(sg == SENTINEL) and not np.any(gr == SENTINEL)
    en[:], sg[:], gr[:] = SENTINEL, SENTINEL, SENTINEL
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    assert call(2, 3, px, 0) == _lib.GP_ERR_STATE and untouched()          # new globals, no global step on them
    with pytest.raises(_lib.GparmlHipError):
        e.curve_energy(X)
    e.phase1()
    e.global_step(sync=True)
    assert call(6, 1, px, 0) == _lib.GP_ERR_BAD_ARG and untouched()        # T = 1
    assert call(2, 3, px, 1) == _lib.GP_ERR_BAD_ARG and untouched()        # flags is reserved
    assert call(-1, 3, px, 0) == _lib.GP_ERR_BAD_ARG and untouched()
    assert call(2, 3, None, 0) == _lib.GP_ERR_BAD_ARG and untouched()      # X is NULL
    bad, pb = _lib.as_c(X.copy())
    bad[1, 2, 0] = np.nan
    assert call(2, 3, pb, 0) == _lib.GP_ERR_BAD_ARG and untouched()
    assert call(0, 3, px, 0) == _lib.GP_OK and untouched()                 # n_curves = 0 writes nothing
    assert call(0, 3, None, 0) == _lib.GP_OK and untouched()
    got = e.curve_energy(np.zeros((0, 3, Q)), want_segments=True)
    assert got['energy'].shape == (0,) and got['seg'].shape == (0, 2) and got['grad'].shape == (0, 3, Q)
    # a curve beyond one chunk of gp_predict (128 points when forced): GP_ERR_UNSUPPORTED
    lib.gp_debug_set_option(b'predict_rows', 128)
    try:
        long_curve, pl = _lib.as_c(np.zeros((1, 129, Q)))
        assert lib.gp_curve_energy(e.h, 1, 129, pl, 0, dp(en), None, None) == _lib.GP_ERR_UNSUPPORTED and untouched()
        assert lib.gp_curve_energy(e.h, 1, 128, pl, 0, dp(en), None, None) == _lib.GP_OK and en[0] == 0.0
    finally:
        lib.gp_debug_set_option(b'predict_rows', 0)
    e.close()


def _sequence(d, N, D, M, Q, curve):
    from gparml_amd.engine import ShardEngine
    e = ShardEngine(N, D, M, Q)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    e.phase1()
    e.global_step(sync=True)
    if curve:
        e.curve_energy(np.random.RandomState(1).randn(20, 6, Q), want_segments=True)
    e.phase2(True)
    out = e.finish()
    out['grad_X_mu'] = e.download('GRAD_X_MU')
    out['grad_X_S'] = e.download('GRAD_X_S')
    Xn = np.random.RandomState(2).randn(20, Q)
    out['predict_mean'], out['predict_var'] = e.predict(Xn)
    out['joint_mean'], out['joint_cov'] = e.predict_joint(Xn)
    g = e.predict_grad(Xn)
    out.update(('grad_' + k, v) for k, v in g.items())
    e.close()
    return out


def test_no_side_effects():
    M, Q, D, N = 64, 3, 5, 500
    d = _model(N, D, M, Q, 'B', seed=13, spread=1.5)
    a = _sequence(d, N, D, M, Q, False)
    b = _sequence(d, N, D, M, Q, True)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_geodesic():
    """Three pairs of end points at (64,2,3,B), T = 12: no energy above its straight line's, the returned energy and length are curve_energy's at the
    returned curves bit for bit, the end points keep their bits."""
    from gparml_amd.predict import Predictor, straight_curves
    c = _case(SHAPES[1])
    M, Q, D, _ = c.shape
    d = c.d
    gs = dict(Z=d['Z'], sf2=d['sf2'], alpha=d['alpha'], beta=d['beta'])
    acc = dict(sum_YYT=np.sum(d['Y'] ** 2), sum_exp_K_mi_K_im=c.stats[0], sum_exp_K_miY=c.stats[1], sum_exp_K_ii=c.N * d['sf2'], sum_KL=0.0)
    p = Predictor(gs, acc, c.N, D)
    rs = np.random.RandomState(8)
    x0, x1 = rs.randn(3, Q), rs.randn(3, Q)
    T = 12
    res = p.geodesic(x0, x1, T=T, iterations=40)
    line = p.curve_energy(straight_curves(x0, x1, T), want_grad=False)['energy']
    print('[curve] geodesic: energy %s, straight line %s, length %s, %d evaluations' % (res['energy'], line, res['length'], res['evaluations']))
    assert res['curves'].shape == (3, T, Q) and res['energy'].shape == (3,) and res['length'].shape == (3,)
    assert np.all(res['energy'] <= line)
    assert np.any(res['energy'] < line)
    assert np.array_equal(res['curves'][:, 0], x0) and np.array_equal(res['curves'][:, -1], x1)
    again = p.curve_energy(res['curves'], want_segments=True, want_grad=False)
    assert np.array_equal(again['energy'], res['energy'])
    assert np.array_equal(p.curve_length(res['curves']), res['length']) and np.array_equal(Predictor._length(again['seg']), res['length'])
    one = p.geodesic(x0[1], x1[1], T=T, iterations=3)                      # a single pair: no leading axis
    assert one['curves'].shape == (T, Q) and np.ndim(one['energy']) == 0 and one['energy'] <= line[1]
