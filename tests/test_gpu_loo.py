"""gp_loo_score on the GPU: exact leave-one-out / leave-block-out scoring of the resident rows against tests/loo_ref.py (the closed form, and brute
force refits as the end-to-end truth), its determinism, the state and argument rules and the Python layer."""
import ctypes

import numpy as np
import pytest

import loo_ref as LR
import score_ref as S
import test_gpu_score as TS

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
# (N_s, M, Q, D): one chunk with a short last block; Mp = 256 and two column tiles.  Both also run in chunks of 128 rows (several chunks, chunk ends
# that are block-aligned but not segment-aligned)
SHAPES = [(300, 20, 2, 3), (520, 130, 3, 130)]
BLOCKS = [1, 2, 5, 64, 128]
_dp = TS._dp


def _loo(e, block, obs=None, flags=1, want=(1, 1, 1, 1, 1, 1)):
    """gp_loo_score as the C ABI has it: (rc, row_logp, row_sse, row_chi2, lev, var_loo, cols), None for an output passed as NULL."""
    n = e.N_s
    o = None if obs is None else np.ascontiguousarray(obs, dtype=np.uint8)
    out = [np.full(n, -7.0) if want[k] else None for k in range(5)] + [np.full((e.D, 5), -7.0) if want[5] else None]
    rc = e.lib.gp_loo_score(e.h, block, None if o is None else o.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), flags, *[_dp(a) for a in out])
    return (rc,) + tuple(out)


def _same(a, b, what):
    for k in range(1, 7):
        if a[k] is None or b[k] is None:
            continue
        assert np.array_equal(a[k], b[k], equal_nan=True), '%s: output %d differs' % (what, k)


class _Case(object):
    """A trained fixed-embedding engine of one shape, a mask, and the closed-form references per block size (built once, never changed)."""

    def __init__(self, N, M, Q, D):
        self.N, self.M, self.Q, self.D = N, M, Q, D
        self.d = d = TS._model(N, D, M, Q, 'A', seed=M + Q + D)
        self.e = TS._engine(d, N, D, M, Q)
        self.Psi2, self.C = self.e.download('PSI2_SUM'), self.e.download('PSI1TY')
        self.tol = TS._tol(d, M, self.Psi2)
        self.obs = TS._mask(np.random.RandomState(11), N, D, 5)
        self.refs = {}

    def ref(self, block):
        if block not in self.refs:
            d = self.d
            self.refs[block] = LR.loo_closed_form(d['Z'], d['sf2'], d['alpha'], d['beta'], self.Psi2, self.C, d['Y'], d['X_mu'], block=block)
        return self.refs[block]


@pytest.fixture(scope='module')
def cases():
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = _Case(*shape)
        return made[shape]
    yield get
    for c in made.values():
        c.e.close()


def _bounds(c, cf, block, noise=True):
    """Per-row bounds on e' (n, D), v' and lev from gp_predict's bound (tol relative to max(1, |mean|) for the mean, to sf2 for
    the variance and its parts), through the block's S^-1.  With amp = |S^-1|_2 = 1 / (1 - lambda_max(H)) of the row's block and g its size:
    dS is beta times the error of g x g products b_i . b_j, |dS|_2 <= g beta tol_v; d(S^-1) = S^-1 dS S^-1, so
      |de'|   <= amp sqrt(g) tol_m + amp^2 g beta tol_v |e_col|_2     (per column, |e_col|_2 over the block's rows)
      |dv'|   <= tol_v + amp^2 g beta tol_v / beta = tol_v (1 + g amp^2)
      |dlev|  <= beta tol_v."""
    d = c.d
    tol_m, tol_v = c.tol * max(1.0, np.max(np.abs(cf['mean']))), c.tol * d['sf2']
    be, bv = np.empty_like(cf['e']), np.empty(c.N)
    E = d['Y'] - cf['mean']
    for j, G in enumerate(LR.blocks(c.N, block)):
        amp, g = 1.0 / (1.0 - cf['lam_max'][j]), len(G)
        be[G] = amp * np.sqrt(g) * tol_m + amp * amp * g * d['beta'] * tol_v * np.linalg.norm(E[G], axis=0)[None, :]
        bv[G] = tol_v * (1.0 + g * amp * amp)
    return be, bv, d['beta'] * tol_v * np.ones(c.N)


def _check_against(c, got, cf, block, obs, what):
    """rows, lev, var_loo elementwise and cols against the reference's terms: the bounds of _bounds propagated through the derivatives of each term
    as tests/test_gpu_score.py does, plus its case-1 bound on the sums (c eps S)."""
    be, bv, bl = _bounds(c, cf, block)
    TS._check_close(got[4], cf['lev'], bl + 8 * EPS * cf['lev'], what + ' lev')
    TS._check_close(got[5], cf['var'], bv + 8 * EPS * np.abs(cf['var']), what + ' var_loo')
    want = S.score_from(cf['e'], np.zeros_like(cf['e']), cf['var'][:, None], obs)
    t = want['terms']
    o, e, v = t['observed'], np.abs(t['e']), t['v']
    prop = dict(logp=np.where(o, e / v * be + np.abs(e * e / (2 * v * v) - 1 / (2 * v)) * bv[:, None], 0.0), e=np.where(o, be, 0.0),
                e2=np.where(o, 2 * e * be, 0.0), q=np.where(o, 2 * e / v * be + e * e / (v * v) * bv[:, None], 0.0))
    rb, cb = TS._sum_bounds(t, 1), TS._sum_bounds(t, 0)
    for key in prop:
        rb[key] = rb[key] + prop[key].sum(axis=1)
        cb[key] = cb[key] + prop[key].sum(axis=0)
    TS._against(dict(row_logp=got[1], row_sse=got[2], row_chi2=got[3], cols=got[6]), want, rb, cb, what)


@pytest.mark.parametrize('block', BLOCKS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'N%d-M%d-Q%d-D%d' % s)
def test_against_the_closed_form(cases, shape, block):
    from gparml_amd import _lib
    c = cases(shape)
    lib = _lib.load()
    cf = c.ref(block)
    assert not cf['not_pd']
    print('largest lambda_max(H) %.4f, largest leverage %.4f' % (np.max(cf['lam_max']), np.max(cf['lev'])))
    for rows in (0, 128):
        lib.gp_debug_set_option(b'predict_rows', rows)
        try:
            for obs in (None, c.obs):
                got = _loo(c.e, block, obs)
                assert got[0] == 0, c.e.lib.gp_last_error(c.e.h)
                _check_against(c, got, cf, block, obs, 'block %d, chunk %d, masked %d' % (block, rows, obs is not None))
                if obs is not None:
                    assert got[1][5] == 0.0 and got[2][5] == 0.0 and got[3][5] == 0.0           # the row with nothing observed
        finally:
            lib.gp_debug_set_option(b'predict_rows', 0)


@pytest.mark.parametrize('block', BLOCKS)
def test_against_the_refit(cases, block):
    """The end-to-end truth at the 300-row shape: one long-double refit per block (loo_ref.loo_refit, on statistics it forms itself from the rows).
    The bounds are those of the closed form (_bounds): the refit is exact to 1e-19 cond."""
    c = cases(SHAPES[0])
    d = c.d
    cf = c.ref(block)
    rf = LR.loo_refit(d['Z'], d['sf2'], d['alpha'], d['beta'], d['Y'], d['X_mu'], block=block)
    truth = dict(cf)
    truth['e'], truth['var'] = rf['e'].astype(float), rf['var'].astype(float)
    got = _loo(c.e, block)
    assert got[0] == 0
    _check_against(c, got, truth, block, None, 'refit, block %d' % block)


@pytest.mark.parametrize('block', BLOCKS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'N%d-M%d-Q%d-D%d' % s)
def test_bit_identity(cases, shape, block):
    from gparml_amd import _lib
    c = cases(shape)
    lib = _lib.load()
    for obs in (None, c.obs):
        for fl in (0, 1):
            what = 'block %d masked %d flags %d' % (block, obs is not None, fl)
            a = _loo(c.e, block, obs, fl)
            assert a[0] == 0
            _same(a, _loo(c.e, block, obs, fl), what + ': run to run')
            lib.gp_debug_set_option(b'predict_rows', 128)
            try:
                parts = _loo(c.e, block, obs, fl)
            finally:
                lib.gp_debug_set_option(b'predict_rows', 0)
            assert parts[0] == 0
            _same(a, parts, what + ': chunks of 128 against the default chunk')
            for want in ((1, 0, 0, 0, 0, 0), (0, 1, 1, 0, 1, 0), (0, 0, 0, 0, 0, 1), (0, 0, 0, 1, 0, 1)):
                _same(a, _loo(c.e, block, obs, fl, want), '%s: outputs %s' % (what, want))
    full = _loo(c.e, block, None, 1)
    _same(full, _loo(c.e, block, np.ones((c.N, c.D), dtype=np.uint8), 1), 'NULL mask against all ones')
    # the leverage is a function of the row alone: the same bits at every block size
    assert np.array_equal(full[4], _loo(c.e, 1, None, 1)[4])
    # block = 1 written out from the outputs themselves: var_f = sf2 - |a|^2 + |b|^2 (gp_predict at the resident inputs, factors on the same
    # kernel only to rounding), |b|^2 = lev / beta: v' - var_f = |b|^2 h / (1 - h)
    if block == 1:
        d = c.d
        _, vf = c.e.predict(d['X_mu'], include_noise=True)
        h = full[4]
        extra = h / d['beta'] * h / (1.0 - h)
        assert np.all(np.abs(full[5] - (vf[:, 0] + extra)) <= 2 * c.tol * d['sf2'] + 8 * EPS * np.abs(full[5]))


@pytest.mark.parametrize('block', [1, 5, 128])
def test_column_sums_in_the_documented_order(cases, block):
    """gp_predict_score's order of the column sums, pinned independently of the library (tests/test_gpu_score.py has the same test): under a mask in
    which every row scores one entry, cols[:, 2:5] are the row outputs themselves summed by score_ref.cols_in_device_order, bit for bit -- at the
    default chunk and at chunks of 128 rows (block 5: chunks of 125, so rows wait in the window for the next chunk's)."""
    from gparml_amd import _lib
    c = cases(SHAPES[0])                                    # N = 300, D = 3
    obs = S.one_entry_mask(c.N, c.D, 200)
    lib = _lib.load()
    for rows in (0, 128):
        lib.gp_debug_set_option(b'predict_rows', rows)
        try:
            got = _loo(c.e, block, obs, 1)
        finally:
            lib.gp_debug_set_option(b'predict_rows', 0)
        assert got[0] == 0, c.e.lib.gp_last_error(c.e.h)
        S.check_cols_order(got[1], got[2], got[3], got[6], obs, 'block %d, chunk %d' % (block, rows))


def test_state_is_left_untouched():
    """gp_phase2 / gp_finish / gp_predict after gp_loo_score are bit-identical to a run without it."""
    N, M, Q, D = SHAPES[0]
    d = TS._model(N, D, M, Q, 'A', seed=3)
    outs = []
    for with_loo in (False, True):
        e = TS._engine(d, N, D, M, Q)
        if with_loo:
            for block in (1, 5):
                assert _loo(e, block)[0] == 0
        e.phase2(False)
        r = e.finish()
        m, v = e.predict(d['X_mu'][:17])
        outs.append((r['F'], r['grad_Z'], r['grad_alpha'], m, v))
        e.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_error_paths():
    from gparml_amd import _lib
    from gparml_amd.engine import ShardEngine
    N, M, Q, D = SHAPES[0]
    d = TS._model(N, D, M, Q, 'A', seed=5)
    e = ShardEngine(N, D, M, Q)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    e.phase1()
    assert _loo(e, 1)[0] == _lib.GP_ERR_STATE                      # before a global step
    e.global_step(sync=True)
    for block, fl in ((0, 1), (129, 1), (-3, 0), (1, 2), (5, 4)):
        assert _loo(e, block, None, fl)[0] == _lib.GP_ERR_BAD_ARG
    assert _loo(e, 1)[0] == 0
    with pytest.raises(AssertionError):
        e.loo(block=200)
    e.close()
    # an engine that holds statistics but no shard
    e = TS._engine(d, N, D, M, Q)
    Psi2, C, sc = e.download('PSI2_SUM'), e.download('PSI1TY'), e.scalars()
    e.close()
    g = ShardEngine(1, D, M, Q)
    g.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'], N_global=N)
    g.set_local_statistics(sc['sum_YYT'], Psi2, C, sc['sum_exp_K_ii'], sc['KL'])
    g.global_step(sync=True)
    assert _loo(g, 1)[0] == _lib.GP_ERR_STATE
    g.close()
    # embeddings of non-zero variance: not a rank-one downdate
    db = TS._model(N, D, M, Q, 'B', seed=5)
    e = TS._engine(db, N, D, M, Q)
    assert _loo(e, 1)[0] == _lib.GP_ERR_UNSUPPORTED
    assert b'rank-one' in e.lib.gp_last_error(e.h)
    e.close()


def test_near_singular_block_stays_factorisable():
    """A benign hard case: an isolated input with an inducing point on it, uploaded twice, at beta = 1e3.  Each copy has a leverage near 1/2 and the
    pair, left out together (block 2), an H with an eigenvalue near 1: S is nearly singular but factorises, and the device agrees with the closed
    form to the bound amplified by 1 / (1 - lambda_max)."""
    N, M, Q, D = 200, 12, 2, 3
    d = TS._model(N, D, M, Q, 'A', seed=9)
    far = np.array([9.0, -9.0])
    d['X_mu'][0] = d['X_mu'][1] = far
    d['Y'][1] = d['Y'][0]
    d['Z'][0] = far
    d['beta'] = 1e3
    e = TS._engine(d, N, D, M, Q)
    c = _Case.__new__(_Case)
    c.N, c.M, c.Q, c.D, c.d, c.e = N, M, Q, D, d, e
    c.Psi2, c.C = e.download('PSI2_SUM'), e.download('PSI1TY')
    c.tol = TS._tol(d, M, c.Psi2)
    cf = LR.loo_closed_form(d['Z'], d['sf2'], d['alpha'], d['beta'], c.Psi2, c.C, d['Y'], d['X_mu'], block=2)
    print('lambda_max of the pair %.6f, its leverages %.4f %.4f' % (cf['lam_max'][0], cf['lev'][0], cf['lev'][1]))
    assert 0.99 < cf['lam_max'][0] < 1.0 and not cf['not_pd']
    got = _loo(e, 2)
    assert got[0] == 0, e.lib.gp_last_error(e.h)
    _check_against(c, got, cf, 2, None, 'near-singular pair')
    e.close()


def test_python_layer_and_two_shards():
    """ShardEngine.loo returns the C entry's bits with score_summary's figures; ResidentModel.loo_training over two shards is the per-engine calls
    with the column sums added on the host; free embeddings are refused."""
    from gparml_amd.engine import ShardEngine
    from gparml_amd.resident import ResidentModel
    from gparml_amd.driver import transform_vec
    N, M, Q, D = SHAPES[0]
    d = TS._model(N, D, M, Q, 'A', seed=13)
    h = 140
    shards = [(d['Y'][:h], d['X_mu'][:h], d['X_S'][:h]), (d['Y'][h:], d['X_mu'][h:], d['X_S'][h:])]
    model = ResidentModel(shards, M, Q, D, fixed_embeddings=True)
    x = np.concatenate([d['Z'].ravel(), [d['sf2']], d['alpha'], [d['beta']]])
    x = np.where(model._pos, np.log(np.expm1(np.where(model._pos, x, 1.0))), x)
    assert np.all(np.isfinite(transform_vec(model._pos, x)))
    got = model.loo_training(block=5, flat_array=x)
    parts = [g.loo(block=5) for g in model.engines]
    raw = [_loo(g, 5) for g in model.engines]
    for k, i in (('row_logp', 1), ('row_sse', 2), ('row_chi2', 3), ('lev', 4), ('var_loo', 5)):
        assert np.array_equal(got[k], np.concatenate([p[k] for p in parts])), k
        assert np.array_equal(got[k], np.concatenate([r[i] for r in raw])), k
    assert np.array_equal(got['cols'], parts[0]['cols'] + parts[1]['cols'])
    assert np.array_equal(got['cols'], raw[0][6] + raw[1][6])
    assert np.array_equal(got['nlpd'], ShardEngine.score_summary(got['cols'])['nlpd'])
    assert got['pooled']['count'] == N * D
    assert model.loo_training(block=1, want_rows=False)['row_logp'] is None
    model.close()
    raws = np.log(np.expm1(np.full((N, Q), 0.3)))
    free = ResidentModel([(d['Y'], d['X_mu'], raws)], M, Q, D, fixed_embeddings=False)
    with pytest.raises(AssertionError):
        free.loo_training(block=1, flat_array=x)
    free.close()
