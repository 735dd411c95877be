"""gp_paths_set / gp_paths_eval on the GPU: pathwise posterior function draws against tests/paths_ref.py (numpy), their determinism contract
(a point's bits depend on the point, the plan and the model only), every status of the header, and the Python wrappers."""
import numpy as np
import pytest

import joint_ref as J
import paths_ref as P
from test_gpu_joint import _engine, _model

pytestmark = pytest.mark.gpu

# the first three shapes of tests/test_gpu_joint.py: one row tile, three, a ragged last one; Mp = 128 and 256; Q below and beyond the 16-wide kernel
SHAPES = [(5, 1, 1, 'A', 37), (64, 2, 3, 'B', 129), (130, 17, 3, 'B', 300)]
# 2F below, at and across a 16-deep k chunk and not a multiple of 16; n_draws D of 1, 3 and 9 columns with these shapes: one column tile
DRAWS = [(1, 1), (24, 3), (100, 3)]
# Two more shapes of tests/test_gpu_joint.py, at (F, n_draws) = (24, 3).  D = 100: n_draws D = 300 columns, three column tiles of the packed operand,
# the last one ragged (44 columns, 84 of exact zeros), so that the pack, fill and scatter kernels index s D + d across tiles and the products run
# with more than one column tile.  Q = 70: the feature kernel that reads its coordinates from memory (Q > 64).
WIDE = [(130, 10, 100, 'A', 300, 24, 3), (64, 70, 3, 'B', 129, 24, 3)]
CASES = [s + f for s in SHAPES for f in DRAWS] + WIDE

_models = {}


@pytest.fixture(scope='module')
def model():
    """(d, engine, X, Psi2, C, tol) of a shape, built once and shared by the tests of this module."""
    def get(M, Q, D, regime, n):
        key = (M, Q, D, regime, n)
        if key not in _models:
            N = max(300, M + 100)
            d = _model(N, D, M, Q, regime, seed=M + Q + D)
            e = _engine(d, N, D, M, Q)
            X = np.random.RandomState(11).randn(n, Q)
            Psi2, C = e.download('PSI2_SUM'), e.download('PSI1TY')
            _models[key] = (d, e, X, Psi2, C, J.cond_tol(d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2))
        return _models[key]
    yield get
    for v in _models.values():
        v[1].close()
    _models.clear()


def _normals(d, M, Q, D, F, S, seed=5):
    rs = np.random.RandomState(seed)
    return rs.randn(F, Q) * np.sqrt(d['alpha']), rs.randn(S, 2 * F, D), rs.randn(S, M, D)


def _close(a, b, tol, scale, what):
    err = np.max(np.abs(a - b)) / scale
    print('%s: %.3g (tol %.3g, ratio %.3g)' % (what, err, tol, err / tol))
    assert err <= tol, '%s: %.3g > %.3g' % (what, err, tol)


@pytest.mark.parametrize('M,Q,D,regime,n,F,S', CASES)
def test_draws_against_the_mirror(model, M, Q, D, regime, n, F, S):
    d, e, X, Psi2, C, tol = model(M, Q, D, regime, n)
    omega, w, eps_u = _normals(d, M, Q, D, F, S)
    centre = d['Z'].mean(axis=0)
    e.paths_set(omega, w, eps_u, centre=centre)
    out, mean = e.paths_eval(X, want_mean=True)
    ref, _ = P.draws(d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2, C, X, omega, w, eps_u, centre)
    assert out.shape == (S, n, D)
    _close(out, ref, tol, max(1.0, np.max(np.abs(ref))), 'draws')
    mp, _ = e.predict(X)
    _close(mean, mp, tol, max(1.0, np.max(np.abs(mp))), 'mean against gp_predict')
    # no centre: the same functions to rounding (a phase is a difference of two points' coordinates)
    e.paths_set(omega, w, eps_u)
    ref0, _ = P.draws(d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2, C, X, omega, w, eps_u, None)
    _close(e.paths_eval(X), ref0, tol, max(1.0, np.max(np.abs(ref0))), 'draws, centre NULL')
    e.paths_clear()


@pytest.mark.parametrize('M,Q,D,regime,n,F,S', CASES)
def test_zero_normals_give_the_mean(model, M, Q, D, regime, n, F, S):
    d, e, X, Psi2, C, tol = model(M, Q, D, regime, n)
    omega, w, eps_u = _normals(d, M, Q, D, F, S)
    e.paths_set(omega, 0.0 * w, 0.0 * eps_u, centre=d['Z'].mean(axis=0))
    out, mean = e.paths_eval(X, want_mean=True)
    mp, _ = e.predict(X)
    for s in range(S):
        _close(out[s], mp, tol, max(1.0, np.max(np.abs(mp))), 'draw %d against gp_predict\'s mean' % s)
        assert np.array_equal(out[s], mean), 'mean + exact zeros is not the mean'
    e.paths_clear()


@pytest.mark.parametrize('M,Q,D,regime,n,F,S', CASES)
def test_a_points_bits_depend_on_the_point_alone(model, M, Q, D, regime, n, F, S):
    from gparml_amd import _lib
    d, e, X, Psi2, C, tol = model(M, Q, D, regime, n)
    omega, w, eps_u = _normals(d, M, Q, D, F, S)
    e.paths_set(omega, w, eps_u, centre=d['Z'].mean(axis=0))
    full, mean = e.paths_eval(X, want_mean=True)
    again, mean2 = e.paths_eval(X, want_mean=True)
    assert np.array_equal(full, again) and np.array_equal(mean, mean2), 'a second call gives other bits'
    rows = [0, 1, n - 1]
    for i in rows:
        alone, m1 = e.paths_eval(X[i:i + 1], want_mean=True)
        assert np.array_equal(alone[:, 0], full[:, i]) and np.array_equal(m1[0], mean[i]), 'row %d alone' % i
    perm = np.random.RandomState(3).permutation(n)
    shuffled = e.paths_eval(X[perm])
    assert np.array_equal(shuffled, full[:, perm]), 'a permuted batch'
    lib = _lib.load()
    lib.gp_debug_set_option(b'paths_rows', -(-n // 3))
    try:
        chunked, mc = e.paths_eval(X, want_mean=True)          # three chunks, the last one shorter (n is no multiple of 3)
    finally:
        lib.gp_debug_set_option(b'paths_rows', 0)
    assert np.array_equal(chunked[:, rows], full[:, rows]) and np.array_equal(chunked, full) and np.array_equal(mc, mean), 'three chunks'
    # two grids that share points: the same draw agrees exactly where they overlap
    lo, hi = n // 3, 2 * n // 3
    a, b = e.paths_eval(X[:hi]), e.paths_eval(X[lo:])
    assert np.array_equal(a[:, lo:], b[:, :hi - lo]) and np.array_equal(a, full[:, :hi]), 'overlapping calls'
    e.paths_clear()


def test_centre_moves_with_the_points():
    """X, Z, the training inputs and the centre shifted together describe the same functions: all on a 2^-24 grid, so every shift is exact."""
    M, Q, D, regime, n = SHAPES[1]
    F, S = 24, 3
    N = max(300, M + 100)
    grid = lambda a: np.round(a * 2.0 ** 24) / 2.0 ** 24
    d = _model(N, D, M, Q, regime, seed=M + Q + D)
    d['Z'], d['X_mu'] = grid(d['Z']), grid(d['X_mu'])
    X = grid(np.random.RandomState(11).randn(n, Q))
    omega, w, eps_u = _normals(d, M, Q, D, F, S)
    centre = grid(d['Z'].mean(axis=0) + 0.125)
    outs = []
    for t in (0.0, 37.25):
        dt = dict(d, Z=d['Z'] + t, X_mu=d['X_mu'] + t)
        e = _engine(dt, N, D, M, Q)
        if t == 0.0:
            tol = J.cond_tol(d['Z'], d['sf2'], d['alpha'], d['beta'], e.download('PSI2_SUM'))
        e.paths_set(omega, w, eps_u, centre=centre + t)
        outs.append(e.paths_eval(X + t))
        e.close()
    _close(outs[1], outs[0], tol, max(1.0, np.max(np.abs(outs[0]))), 'shifted by 37.25 against unshifted')


def _sequence(d, N, D, M, Q, paths):
    from gparml_amd.engine import ShardEngine
    e = ShardEngine(N, D, M, Q)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    e.phase1()
    e.global_step(sync=True)
    if paths:
        omega, w, eps_u = _normals(d, M, Q, D, 24, 3)
        e.paths_set(omega, w, eps_u)
        e.paths_eval(np.random.RandomState(1).randn(150, Q))
    e.phase2(True)
    out = e.finish()
    out['grad_X_mu'] = e.download('GRAD_X_MU')
    out['grad_X_S'] = e.download('GRAD_X_S')
    out['predict_mean'], out['predict_var'] = e.predict(np.random.RandomState(2).randn(20, Q))
    out['joint_mean'], out['joint_cov'] = e.predict_joint(np.random.RandomState(2).randn(20, Q))
    e.close()
    return out


def test_no_side_effects():
    M, Q, D, N = 64, 3, 5, 500
    d = _model(N, D, M, Q, 'B', seed=13, spread=1.5)
    a = _sequence(d, N, D, M, Q, False)
    b = _sequence(d, N, D, M, Q, True)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_statuses():
    from gparml_amd import _lib
    from gparml_amd.engine import ShardEngine
    M, Q, D, N, F, S = 16, 2, 3, 100, 4, 2
    d = _model(N, D, M, Q, 'A', seed=21)
    omega, w, eps_u = _normals(d, M, Q, D, F, S)
    lib = _lib.load()
    dp = lambda a: a.ctypes.data_as(_lib._dp)
    X, out = np.zeros((2, Q)), np.empty((S, 2, D))
    e = ShardEngine(N, D, M, Q)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    set_ = lambda s=S, f=F, o=omega, c=None, ww=w, ee=eps_u: lib.gp_paths_set(e.h, s, f, dp(o) if o is not None else None, dp(c) if c is not None else None,
                                                                               dp(ww) if ww is not None else None, dp(ee) if ee is not None else None)
    ev = lambda n=2, x=X, flags=0, o=out: lib.gp_paths_eval(e.h, n, dp(x) if x is not None else None, flags, dp(o) if o is not None else None, None)
    assert set_() == _lib.GP_ERR_STATE                     # no global step yet
    assert ev() == _lib.GP_ERR_STATE
    e.phase1()
    e.global_step(sync=True)
    assert ev() == _lib.GP_ERR_STATE                       # a model, no plan
    assert ev(n=0) == _lib.GP_ERR_STATE
    # argument errors of gp_paths_set, none of which leaves a plan behind
    nan = lambda a: np.where(np.arange(a.size).reshape(a.shape) == a.size - 1, np.nan, a)
    for rc in (set_(s=0), set_(f=0), set_(o=None), set_(ww=None), set_(ee=None), set_(o=nan(omega)), set_(c=np.array([0.0, np.inf])), set_(ww=nan(w)),
               set_(ee=nan(eps_u))):
        assert rc == _lib.GP_ERR_BAD_ARG
    assert ev() == _lib.GP_ERR_STATE
    # 2 GiB of packed operand: (2F rounded up to 16 + 2 Mp) rows x (n_draws D rounded up to 128) columns of doubles -- refused before anything is read
    big_S = (2 << 30) // (8 * (16 + 256)) // D + 128
    assert lib.gp_paths_set(e.h, big_S, F, dp(omega), None, dp(w), dp(eps_u)) == _lib.GP_ERR_UNSUPPORTED
    assert b'2 GiB' in lib.gp_last_error(e.h)
    assert set_() == _lib.GP_OK
    assert ev() == _lib.GP_OK
    assert ev(n=0, x=None, o=None) == _lib.GP_OK           # n = 0 writes nothing
    for rc in (ev(n=-1), ev(flags=1), ev(x=None), ev(o=None), ev(x=np.array([[0.0, np.nan], [0.0, 0.0]]))):
        assert rc == _lib.GP_ERR_BAD_ARG
    assert ev() == _lib.GP_OK                              # an argument error leaves the plan in place
    ref = out.copy()
    # every event that takes the model away drops the plan, also when a model is there again afterwards
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    assert ev() == _lib.GP_ERR_STATE
    e.phase1()
    e.global_step(sync=True)
    assert ev() == _lib.GP_ERR_STATE, 'the plan survived gp_set_globals'
    assert set_() == _lib.GP_OK and ev() == _lib.GP_OK and np.array_equal(out, ref)
    e.phase1()
    e.global_step(sync=True)
    assert ev() == _lib.GP_ERR_STATE, 'the plan survived gp_phase1 and a new global step'
    assert set_() == _lib.GP_OK and ev() == _lib.GP_OK
    e.phase1()
    assert ev() == _lib.GP_ERR_STATE                       # gp_predict's own state rule
    e.global_step(sync=True)
    assert set_() == _lib.GP_OK and ev() == _lib.GP_OK
    assert lib.gp_paths_clear(e.h) == _lib.GP_OK
    assert ev() == _lib.GP_ERR_STATE
    assert lib.gp_paths_clear(e.h) == _lib.GP_OK           # nothing to clear is not an error
    with pytest.raises(_lib.GparmlHipError):
        e.paths_eval(X)
    e.close()


def _predictor(N, D, M, Q, seed):
    from gparml_amd.predict import Predictor
    d = _model(N, D, M, Q, 'A', seed=seed)
    e = _engine(d, N, D, M, Q)
    Psi2, C = e.download('PSI2_SUM'), e.download('PSI1TY')
    e.close()
    gs = dict(Z=d['Z'], sf2=d['sf2'], alpha=d['alpha'], beta=d['beta'])
    acc = dict(sum_YYT=np.sum(d['Y'] ** 2), sum_exp_K_mi_K_im=Psi2, sum_exp_K_miY=C, sum_exp_K_ii=N * d['sf2'], sum_KL=0.0)
    return d, Psi2, C, Predictor(gs, acc, N, D)


def test_sample_paths_is_reproducible():
    N, D, M, Q = 120, 2, 16, 2
    d, Psi2, C, p = _predictor(N, D, M, Q, 21)
    X = np.random.RandomState(4).randn(50, Q)
    with p.sample_paths(3, n_features=64, seed=7) as draws:
        a = draws(X)
        fine = draws(np.concatenate([X, X[:5] + 0.01]))
        assert np.array_equal(fine[:, :50], a), 'a finer grid moved the shared points'
        omega, centre = draws.omega, draws.centre
    with p.sample_paths(3, n_features=64, seed=7) as draws:
        b = draws(X)
    with p.sample_paths(3, n_features=64, seed=8) as draws:
        c = draws(X)
    assert a.shape == (3, 50, D) and np.array_equal(a, b) and not np.array_equal(a, c)
    # the documented use of the seed: omega, w, eps_u in this order from RandomState(seed)
    rs = np.random.RandomState(7)
    om = rs.randn(64, Q) * np.sqrt(d['alpha'])
    w, eps_u = rs.randn(3, 128, D), rs.randn(3, M, D)
    assert np.array_equal(om, omega) and np.array_equal(centre, d['Z'].mean(axis=0))
    ref, _ = P.draws(d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2, C, X, om, w, eps_u, centre)
    _close(a, ref, J.cond_tol(d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2), max(1.0, np.max(np.abs(ref))), 'sample_paths against the mirror')


def test_an_engine_holds_one_set_of_draws():
    """Two PathDraws on one engine (ResidentModel.sample_paths twice): the earlier object raises instead of returning the later one's functions,
    and closing it leaves the later one alone."""
    from gparml_amd.predict import PathDraws
    N, D, M, Q = 120, 2, 16, 2
    d = _model(N, D, M, Q, 'A', seed=21)
    e = _engine(d, N, D, M, Q)
    X = np.random.RandomState(4).randn(10, Q)
    first = PathDraws(e, d['Z'], d['alpha'], 2, n_features=8, seed=1)
    a = first(X)
    second = PathDraws(e, d['Z'], d['alpha'], 3, n_features=8, seed=2)
    b = second(X)
    assert a.shape == (2, 10, D) and b.shape == (3, 10, D)
    with pytest.raises(RuntimeError):
        first(X)
    first.close()
    assert np.array_equal(second(X), b), 'closing the replaced draws cleared the current ones'
    second.close()
    with pytest.raises(RuntimeError):
        second(X)
    e.close()


def test_empirical_covariance_of_sample_paths():
    """4096 draws at 8 points: the second moment about gp_predict's mean against gp_predict_joint's cov, per output.
    Bound per element: 6 sf2 sqrt(2 / S), six standard deviations of a covariance entry estimated from S draws about the known mean
    (sqrt((c_ii c_jj + c_ij^2) / S) <= sf2 sqrt(2 / S)), plus the feature term at the F used, 6 sf2 / sqrt(2F): the bound on an element of
    K_F - K that tests/test_paths_cpu.py holds the mirror to."""
    N, D, M, Q, S, F = 120, 2, 16, 2, 4096, 1024
    d, Psi2, C, p = _predictor(N, D, M, Q, 21)
    X = np.random.RandomState(6).randn(8, Q)
    with p.sample_paths(S, n_features=F, seed=11) as draws:
        out, mean = draws(X, want_mean=True)
    _, cov = p.predict_joint(X)
    sampling, rff = 6.0 * d['sf2'] * np.sqrt(2.0 / S), 6.0 * d['sf2'] / np.sqrt(2.0 * F)
    r = out - mean[None]
    for j in range(D):
        emp = r[:, :, j].T.dot(r[:, :, j]) / S
        err = np.max(np.abs(emp - cov))
        print('output %d: max |empirical - cov| = %.3g (bound: sampling %.3g + feature term %.3g)' % (j, err, sampling, rff))
        assert err <= sampling + rff, (err, sampling + rff)
