"""gp_condition_set / gp_condition_predict / gp_condition_clear on the GPU: the posterior conditioned on extra observed rows against the
long-double closed form (tests/cond_ref.py) under derived bounds, against a refit on the device, its properties, bit identities, the untouched
evaluation state, the state and argument rules, the poison mode and the Python layer.  The models are test_gpu_score._model's at cond_ref.SHAPES,
the seeds cond_ref.model_seed and cond_ref.cond_inputs (tests/test_cond_ref_cpu.py holds them to the sharpness condition of test 1)."""
import ctypes

import numpy as np
import pytest

import cond_ref as CR
import test_gpu_score as TG

pytestmark = pytest.mark.gpu

_dp = TG._dp
BAD_ARG, NOT_PD, STATE, UNSUPPORTED = 1, 2, 5, 6


def _set(e, Xc, Yc, m=None):
    c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)        # noqa: E731
    Xc, Yc = c(Xc), c(Yc)
    return e.lib.gp_condition_set(e.h, Xc.shape[0] if m is None else m, _dp(Xc), _dp(Yc))


def _predict(e, X, flags=0, want=(1, 1, 1), n=None):
    """gp_condition_predict as the C ABI has it: (rc, mean, var, reduction), None for an output passed as NULL."""
    X = None if X is None else np.ascontiguousarray(X, dtype=np.float64)
    n = X.shape[0] if n is None else n
    out = [np.full((max(n, 0), e.D), -7.0) if want[0] else None] + [np.full(max(n, 0), -7.0) if want[k] else None for k in (1, 2)]
    rc = e.lib.gp_condition_predict(e.h, n, _dp(X), flags, _dp(out[0]), _dp(out[1]), _dp(out[2]))
    return (rc,) + tuple(out)


def _err(e):
    return e.lib.gp_last_error(e.h).decode()


class _Case(object):
    """A trained engine of one shape (fixed embeddings) and the long-double references of its cases, each built once and never changed"""

    def __init__(self, shape):
        self.shape = shape
        N, M, Q, D = shape
        self.d = d = TG._model(N, D, M, Q, 'A', seed=CR.model_seed(shape))
        self.e = TG._engine(d, N, D, M, Q)
        self.Psi2, self.C = self.e.download('PSI2_SUM'), self.e.download('PSI1TY')
        self.tol = TG._tol(d, M, self.Psi2)
        self.g = (d['Z'], d['sf2'], d['alpha'], d['beta'])
        self.refs = {}

    def ref(self, m, n):
        if (m, n) not in self.refs:
            N, M, Q, D = self.shape
            Xc, Yc, X = CR.cond_inputs(Q, D, m, n)
            r = CR.cond_closed_form(*self.g, self.Psi2, self.C, Xc, Yc, X)
            self.refs[m, n] = (Xc, Yc, X, r, CR.cond_bounds(r, self.tol, self.d['sf2'], self.d['beta'], M))
        return self.refs[m, n]


@pytest.fixture(scope='module')
def cases():
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = _Case(shape)
        return made[shape]
    yield get
    for c in made.values():
        c.e.close()


def _rows(lib, rows):
    assert lib.gp_debug_set_option(b'predict_rows', rows) == 0


def _against_closed_form(c, m, n, what):
    Xc, Yc, X, r, (b_mean, b_var, b_red) = c.ref(m, n)
    vmin = float(np.min(r['var_c']))
    print('%s: bounds mean\' %.3g var\' %.3g reduction %.3g; smallest var\' %.3g' % (what, b_mean.max(), b_var.max(), b_red.max(), vmin))
    assert b_var.max() < 1e-3 * vmin, 'the bound on var\' is not sharp at these seeds'
    assert _set(c.e, Xc, Yc) == 0, _err(c.e)
    rc, mean, var, red = _predict(c.e, X)
    assert rc == 0, _err(c.e)
    f = lambda x: np.asarray(x, dtype=np.float64)       # noqa: E731
    TG._check_close(mean, f(r['mean_c']), b_mean, what + ' mean\'')
    TG._check_close(var, f(r['var_c']), b_var, what + ' var\'')
    TG._check_close(red, f(r['reduction']), b_red, what + ' reduction')


# ---- 1. against the closed form ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', [0, 128])
@pytest.mark.parametrize('n', CR.NS)
@pytest.mark.parametrize('m', CR.MS)
@pytest.mark.parametrize('shape', CR.SHAPES)
def test_against_the_closed_form(cases, shape, m, n, rows):
    c = cases(shape)
    _rows(c.e.lib, rows)
    try:
        _against_closed_form(c, m, n, 'shape %s m %d n %d chunk %d' % (shape, m, n, rows))
    finally:
        _rows(c.e.lib, 0)


# ---- 2. against a refit on the device ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', [0, 128])
@pytest.mark.parametrize('m', [5, 129])
def test_against_a_refit_on_the_device(cases, m, rows):
    """A second engine holds the training rows followed by the conditioning rows (fixed embeddings, same globals): its gp_predict agrees with
    gp_condition_predict within the sum of both sides' bounds -- cond_bounds here, test_gpu_score._tol of the refitted model there."""
    shape = CR.SHAPES[0]
    c = cases(shape)
    N, M, Q, D = shape
    Xc, Yc, X, r, (b_mean, b_var, _) = c.ref(m, 300)
    d2 = dict(c.d)
    d2['Y'], d2['X_mu'], d2['X_S'] = np.vstack((c.d['Y'], Yc)), np.vstack((c.d['X_mu'], Xc)), np.zeros((N + m, Q))
    _rows(c.e.lib, rows)
    e2 = TG._engine(d2, N + m, D, M, Q)
    try:
        mean2, var2 = e2.predict(X)
        tol2 = TG._tol(d2, M, e2.download('PSI2_SUM'))
        assert _set(c.e, Xc, Yc) == 0, _err(c.e)
        rc, mean, var, _ = _predict(c.e, X)
        assert rc == 0, _err(c.e)
        print('m %d chunk %d: bounds mean %.3g + %.3g, var %.3g + %.3g' % (m, rows, b_mean.max(), tol2, b_var.max(), tol2 * c.d['sf2']))
        TG._check_close(mean, mean2, b_mean + tol2 * np.maximum(1.0, np.abs(mean2)), 'refit mean')
        TG._check_close(var, var2[:, 0], b_var + tol2 * c.d['sf2'], 'refit var')
    finally:
        _rows(c.e.lib, 0)
        e2.close()


# ---- 3. properties -----------------------------------------------------------------------------------------------------------------------------
def test_reduction_is_the_difference_of_the_variances(cases):
    """reduction >= 0, and var - var' == reduction bit for bit, var from a gp_predict call large enough (66 row tiles x 4 column tiles of factor
    rows > 256 tiles) to run its factor product on the 128 x 128-tile kernel, as gp_condition_predict always does."""
    shape = CR.SHAPES[1]
    c = cases(shape)
    N, M, Q, D = shape
    Xc, Yc, _ = CR.cond_inputs(Q, D, 5, 1)
    X = np.random.RandomState(3).randn(8400, Q)
    X[:5] = Xc
    assert _set(c.e, Xc, Yc) == 0, _err(c.e)
    for flags in (0, 1):
        _, var = c.e.predict(X, include_noise=bool(flags))
        rc, _, var_c, red = _predict(c.e, X, flags, want=(0, 1, 1))
        assert rc == 0, _err(c.e)
        assert np.all(red >= 0)
        assert np.array_equal(var[:, 0] - var_c, red)
    assert np.all(var_c[:5] - 1.0 / c.d['beta'] < 1.0 / c.d['beta'])


@pytest.mark.parametrize('shape', CR.SHAPES)
def test_on_a_conditioning_row_and_far_from_one(cases, shape):
    c = cases(shape)
    N, M, Q, D = shape
    Xc, Yc, X = CR.cond_inputs(Q, D, 5, 300)              # the last query is the first conditioning input
    assert _set(c.e, Xc, Yc) == 0, _err(c.e)
    rc, _, var_c, red = _predict(c.e, X)
    assert rc == 0 and var_c[-1] < 1.0 / c.d['beta'] and np.all(red >= 0)
    # a conditioning row far from every inducing point: k = 0, nothing changes beyond gp_predict's own bound
    assert _set(c.e, np.full((1, Q), 60.0), np.ones((1, D))) == 0, _err(c.e)
    rc, mean_c, var_c, red = _predict(c.e, X)
    mean, var = c.e.predict(X)
    assert rc == 0
    TG._check_close(mean_c, mean, c.tol * np.maximum(1.0, np.abs(mean)), 'far row: mean')
    TG._check_close(var_c, var[:, 0], c.tol * c.d['sf2'], 'far row: var')
    TG._check_close(red, 0.0 * red, c.tol * c.d['sf2'], 'far row: reduction')


# ---- 4. bit identity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', [5, 300])
@pytest.mark.parametrize('shape', CR.SHAPES)
def test_bit_identity(cases, shape, m):
    c = cases(shape)
    N, M, Q, D = shape
    Xc, Yc, X = CR.cond_inputs(Q, D, m, 300)
    assert _set(c.e, Xc, Yc) == 0, _err(c.e)
    a = _predict(c.e, X, 1)
    assert a[0] == 0, _err(c.e)
    same = lambda p, q, what: [np.testing.assert_array_equal(x, y, err_msg=what) for x, y in zip(p[1:], q[1:]) if x is not None and y is not None]   # noqa: E731
    same(a, _predict(c.e, X, 1), 'two runs')
    _rows(c.e.lib, 128)
    try:
        same(a, _predict(c.e, X, 1), 'chunks of 128 against the default chunk')
        assert _set(c.e, Xc, Yc) == 0, _err(c.e)          # the set itself built in chunks of 128 rows
        same(a, _predict(c.e, X, 1), 'a set built in chunks of 128')
    finally:
        _rows(c.e.lib, 0)
    assert _set(c.e, Xc, Yc) == 0, _err(c.e)
    same(a, _predict(c.e, X, 1), 'a second set of the same rows')
    one = _predict(c.e, X[17:18], 1)
    same(tuple([0] + [x[17:18] for x in a[1:]]), one, 'a row alone against the row in a batch of 300')
    for want in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1)):
        part = _predict(c.e, X, 1, want=want)
        assert part[0] == 0
        same(a, part, 'outputs %s' % (want,))


# ---- 5. the evaluation state is untouched ------------------------------------------------------------------------------------------------------
def test_evaluation_state_untouched():
    N, M, Q, D = 300, 20, 2, 3
    d = TG._model(N, D, M, Q, 'B', seed=4)
    Xc, Yc, X = CR.cond_inputs(Q, D, 129, 300)
    outs = []
    for cond in (False, True):
        e = TG._engine(d, N, D, M, Q)
        if cond:
            assert _set(e, Xc, Yc) == 0, _err(e)
            assert _predict(e, X)[0] == 0
            assert e.lib.gp_condition_clear(e.h) == 0
            assert _set(e, Xc[:5], Yc[:5]) == 0           # and one left alive under phase 2
        e.phase2(True)
        out = e.finish()
        out['grad_X_mu'], out['grad_X_S'] = e.download('GRAD_X_MU'), e.download('GRAD_X_S')
        outs.append(out)
        e.close()
    for k in outs[0]:
        np.testing.assert_array_equal(np.asarray(outs[0][k]), np.asarray(outs[1][k]), err_msg=k)


# ---- 6. state and argument rules ---------------------------------------------------------------------------------------------------------------
def test_state_and_argument_rules():
    from gparml_amd.engine import ShardEngine
    N, M, Q, D = 300, 20, 2, 3
    d = TG._model(N, D, M, Q, 'A', seed=5)
    Xc, Yc, X = CR.cond_inputs(Q, D, 5, 3)
    e = ShardEngine(N, D, M, Q)
    lib = e.lib
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    e.phase1()
    assert _set(e, Xc, Yc) == STATE and 'gp_condition_set needs a global step' in _err(e)
    assert _predict(e, X)[0] == STATE and 'gp_condition_predict needs a global step' in _err(e)
    assert lib.gp_condition_clear(e.h) == 0 and lib.gp_condition_clear(e.h) == 0
    e.global_step(sync=True)
    assert _predict(e, X)[0] == STATE and 'needs gp_condition_set on the model as it is now' in _err(e)
    assert _set(e, Xc, Yc, m=0) == BAD_ARG and 'm must be >= 1' in _err(e)
    assert lib.gp_condition_set(e.h, 5, None, _dp(Yc)) == BAD_ARG and 'NULL' in _err(e)
    assert lib.gp_condition_set(e.h, 5, _dp(Xc), None) == BAD_ARG
    big = np.zeros((1025, max(Q, D)))
    assert lib.gp_condition_set(e.h, 1025, _dp(big), _dp(big)) == UNSUPPORTED and 'limit of 1024' in _err(e)
    for bad in (np.nan, np.inf):
        Xb, Yb = Xc.copy(), Yc.copy()
        Xb[3, 1], Yb[4, 2] = bad, bad
        assert _set(e, Xb, Yc) == BAD_ARG and 'Xc is not finite' in _err(e)
        assert _set(e, Xc, Yb) == BAD_ARG and 'Yc is not finite' in _err(e)
    assert _predict(e, X)[0] == STATE                     # none of the refused calls left a set behind
    assert _set(e, Xc, Yc) == 0, _err(e)
    assert _predict(e, X)[0] == 0
    assert _predict(e, X, n=-1)[0] == BAD_ARG and 'n must be >= 0' in _err(e)
    assert _predict(e, X, flags=2)[0] == BAD_ARG and 'unknown flags' in _err(e)
    assert _predict(e, None, n=3)[0] == BAD_ARG and 'X is NULL' in _err(e)
    Xb = X.copy()
    Xb[1, 0] = np.nan
    assert _predict(e, Xb)[0] == BAD_ARG and 'X is not finite' in _err(e)
    got = _predict(e, X[:0])
    assert got[0] == 0
    rc, mean, var, red = _predict(e, X, n=0)              # n = 0 writes nothing
    assert rc == 0 and np.all(mean == -7.0) and np.all(var == -7.0) and np.all(red == -7.0)
    assert _predict(e, X, want=(0, 0, 0))[0] == 0
    # a stale set: new globals, then a global step on them -- GP_ERR_STATE until the next set
    e.set_globals(d['Z'], d['sf2'], d['alpha'] * 1.1, d['beta'])
    assert _predict(e, X)[0] == STATE and 'needs a global step' in _err(e)
    e.phase1()
    e.global_step(sync=True)
    assert _predict(e, X)[0] == STATE and 'needs gp_condition_set on the model as it is now' in _err(e)
    assert _set(e, Xc, Yc) == 0 and _predict(e, X)[0] == 0
    e.global_step(sync=True)                              # the same statistics, but another step: the set was of the one before
    assert _predict(e, X)[0] == STATE
    assert lib.gp_condition_clear(e.h) == 0 and lib.gp_condition_clear(e.h) == 0
    assert lib.gp_condition_set(None, 5, _dp(Xc), _dp(Yc)) == BAD_ARG and lib.gp_condition_clear(None) == BAD_ARG
    assert lib.gp_condition_predict(None, 0, None, 0, None, None, None) == BAD_ARG
    e.close()


def test_destroying_the_context_frees_the_set():
    """Three contexts destroyed with a set of 1024 rows and its 89 MB chunk buffer alive: the device's free memory comes back (the allocation
    ledger of tests/test_gpu_alloc.py: free memory read through a context that stays open, within its slack of 64 MB)."""
    from gparml_amd.engine import ShardEngine
    shape = CR.SHAPES[1]
    N, M, Q, D = shape
    d = TG._model(N, D, M, Q, 'A', seed=CR.model_seed(shape))
    probe = ShardEngine(128, 1, 1, 1)
    Xc, Yc, X = CR.cond_inputs(Q, D, 1024, 1)
    try:
        e = TG._engine(d, N, D, M, Q)                     # the first context of the process pays for the runtime's own pools
        e.predict(X)
        e.close()
        base = probe.memory_info()[0]
        for _ in range(3):
            e = TG._engine(d, N, D, M, Q)
            assert _set(e, Xc, Yc) == 0, _err(e)
            assert _predict(e, X)[0] == 0
            e.close()
        for _ in range(2000):                             # freed memory returns to the device asynchronously; a leak never does
            free = probe.memory_info()[0]
            if abs(free - base) <= 64 << 20:
                break
        assert abs(free - base) <= 64 << 20, (base - free) / 2.0 ** 20
    finally:
        probe.close()


# ---- 7. poison mode ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', [0, 128])
@pytest.mark.parametrize('m', CR.MS)
def test_poison_mode(m, rows):
    """The cases of test 1 at the small shape with every allocation NaN-filled: every element of V, T and the padded parts of S is written
    before it is read."""
    shape = CR.SHAPES[0]
    from gparml_amd import _lib
    lib = _lib.load()
    assert lib.gp_debug_set_option(b'poison_alloc', 1) == 0
    _rows(lib, rows)
    c = None
    try:
        c = _Case(shape)
        for n in CR.NS:
            _against_closed_form(c, m, n, 'poison: m %d n %d chunk %d' % (m, n, rows))
    finally:
        lib.gp_debug_set_option(b'poison_alloc', 0)
        _rows(lib, 0)
        if c is not None:
            c.e.close()


# ---- 8. the Python layer -----------------------------------------------------------------------------------------------------------------------
def test_python_layer(cases):
    from gparml_amd import _lib
    from gparml_amd.predict import Predictor
    shape = CR.SHAPES[0]
    c = cases(shape)
    N, M, Q, D = shape
    Xc, Yc, X = CR.cond_inputs(Q, D, 129, 300)
    assert _set(c.e, Xc, Yc) == 0
    raw = _predict(c.e, X, 1)
    c.e.condition_clear()
    with pytest.raises(_lib.GparmlHipError):
        c.e.condition_predict(X)
    c.e.condition(Xc, Yc)
    mean, var, red = c.e.condition_predict(X, include_noise=True, want_reduction=True)
    assert var.shape == (300, 1) and red.shape == (300, 1)
    assert np.array_equal(mean, raw[1]) and np.array_equal(var[:, 0], raw[2]) and np.array_equal(red[:, 0], raw[3])
    mean2, var2 = c.e.condition_predict(X, include_noise=True)
    assert np.array_equal(mean2, mean) and np.array_equal(var2, var)
    with pytest.raises(AssertionError):
        c.e.condition(Xc, Yc[:, :2])
    with pytest.raises(AssertionError):
        c.e.condition(np.full_like(Xc, np.nan), Yc)
    c.e.condition_clear()
    sc = c.e.scalars()
    p = Predictor(dict(Z=c.d['Z'], sf2=c.d['sf2'], alpha=c.d['alpha'], beta=c.d['beta']),
                  dict(sum_YYT=sc['sum_YYT'], sum_exp_K_mi_K_im=c.Psi2, sum_exp_K_miY=c.C, sum_exp_K_ii=sc['sum_exp_K_ii'], sum_KL=sc['KL']), N, D)
    eng = p._trained_engine()
    try:
        assert _set(eng, Xc, Yc) == 0
        raw = _predict(eng, X, 0)
    finally:
        eng.close()
    mean, var, red = p.predict_conditioned(X, Xc, Yc, want_reduction=True)
    assert np.array_equal(mean, raw[1]) and np.array_equal(var[:, 0], raw[2]) and np.array_equal(red[:, 0], raw[3])
