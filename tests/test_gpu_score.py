"""gp_predict_score on the GPU: held-out scoring against gp_predict's own output, against tests/score_ref.py on tests/predict_ref.py, its
determinism and invariances, the resident rows, the state and argument rules and the Python layer."""
import ctypes

import numpy as np
import pytest

import predict_ref as R
import score_ref as S

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
# (M, Q, D, regime): the smallest shapes at which each code path can go wrong (M not a multiple of 128, Q beyond the 16-wide and the 64-wide
# instantiations, several 64-lane strides and 128-column tiles with D a multiple of neither)
SHAPES = [(5, 1, 1, 'A'), (64, 2, 3, 'B'), (130, 17, 3, 'B'), (64, 70, 3, 'B'), (64, 3, 300, 'B'), (130, 10, 100, 'A')]


def _model(N, D, M, Q, regime, seed=0, spread=1.5):
    """The recipe of tests/test_gpu_predictive.py: inducing points drawn apart from the data, a lengthscale short enough for cond(Kmm) < 1e6."""
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


def _tol(d, M, Psi2=None):
    """tests/test_gpu_predictive.py's bound on mean and variance: 1e-10, or eps-level error amplified by the conditioning if that is larger."""
    from oracle import literal as L
    K = L.rbf_gram(d['Z'], d['sf2'], d['alpha'])
    cond = np.linalg.cond(K)
    if Psi2 is not None:
        cond = max(cond, np.linalg.cond(K + d['beta'] * Psi2))
    return max(1e-10, 1e-16 * cond)


def _dp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _raw(e, n, X_mu, X_S, Y, obs, flags, want=(1, 1, 1, 1)):
    """gp_predict_score as the C ABI has it: (rc, row_logp, row_sse, row_chi2, cols), None for an output passed as NULL."""
    c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)        # noqa: E731
    X_mu, X_S, Y = c(X_mu), c(X_S), c(Y)
    o = None if obs is None else np.ascontiguousarray(obs, dtype=np.uint8)
    out = [np.full(max(n, 0), -7.0) if want[k] else None for k in range(3)] + [np.full((e.D, 5), -7.0) if want[3] else None]
    rc = e.lib.gp_predict_score(e.h, n, _dp(X_mu), _dp(X_S), 0, _dp(Y), None if o is None else o.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), flags,
                                _dp(out[0]), _dp(out[1]), _dp(out[2]), _dp(out[3]))
    return (rc,) + tuple(out)


def _mask(rs, n, D, hidden_row):
    """About 30 % hidden entries and one row hidden altogether."""
    o = rs.uniform(size=(n, D)) > 0.3
    o[hidden_row] = False
    return o


class _Case(object):
    """A trained engine of one shape, 37 new rows, a mask, and the references every test of the shape shares (built once, never changed)."""

    def __init__(self, M, Q, D, regime):
        self.M, self.Q, self.D = M, Q, D
        self.N = N = max(300, M + 100)
        self.d = d = _model(N, D, M, Q, regime, seed=M + Q + D)
        self.e = _engine(d, N, D, M, Q)
        rs = np.random.RandomState(11)
        self.n = n = 37
        self.Xt, self.St = rs.randn(n, Q), rs.uniform(0.05, 0.5, size=(n, Q))
        self.Psi2, self.C = self.e.download('PSI2_SUM'), self.e.download('PSI1TY')
        self.tol = _tol(d, M, self.Psi2)
        self.ref = {unc: R.predict(d['Z'], d['sf2'], d['alpha'], d['beta'], self.Psi2, self.C, self.Xt, self.St if unc else None, False) for unc in (False, True)}
        # outputs near the prediction: the noise-free reference mean plus noise of the model's own size
        self.Y = self.ref[False][0] + rs.randn(n, D) / np.sqrt(d['beta'])
        self.obs = _mask(rs, n, D, 5)
        self.Yh = np.where(self.obs, self.Y, np.nan)          # NaN in every hidden entry


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


def _sum_bounds(t, axis):
    """The case-1 bound c eps S of the three sums along ``axis`` of the terms t (score_ref.terms): S the sum of the absolute values of what enters
    the sum -- for logp its two parts 1/2 |ln(2 pi v)| and q / 2, which may cancel --, c the number of entries plus 16: one rounding per addition
    and a few ulps for the division and the logarithm of every entry (each relative to that entry's own parts)."""
    k = t['observed'].sum(axis=axis)
    c = (k + 16) * EPS
    return dict(logp=c * (np.abs(t['half_log']) + 0.5 * t['q']).sum(axis=axis), e2=c * t['e2'].sum(axis=axis), q=c * t['q'].sum(axis=axis),
                e=c * np.abs(t['e']).sum(axis=axis))


def _check_close(got, want, bound, what):
    err = np.abs(np.asarray(got) - np.asarray(want))
    worst = np.max(err / np.maximum(bound, 1e-300)) if err.size else 0.0
    print('%s: worst error / bound = %.3g' % (what, worst))
    assert np.all(err <= bound), '%s: error %.3g of the bound' % (what, worst)


def _against(res, want, rb, cb, what):
    """rows and columns of a device result against a score_ref.score_from result, under the row bounds rb and column bounds cb"""
    _check_close(res['row_logp'], want['row_logp'], rb['logp'], what + ' row_logp')
    _check_close(res['row_sse'], want['row_sse'], rb['e2'], what + ' row_sse')
    _check_close(res['row_chi2'], want['row_chi2'], rb['q'], what + ' row_chi2')
    assert np.array_equal(res['cols'][:, 0], want['cols'][:, 0]), what + ' count'
    for k, key in ((1, 'e'), (2, 'e2'), (3, 'q'), (4, 'logp')):
        _check_close(res['cols'][:, k], want['cols'][:, k], cb[key], what + ' cols[%d]' % k)


def _variants():
    for unc in (False, True):
        for noise in (False, True):
            for masked in (False, True):
                yield unc, noise, masked


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'M%d-Q%d-D%d' % s[:3])
def test_against_gp_predict_bits(cases, shape):
    """Case 1: the formulas in numpy on the engine's own ``predict`` output.  The device scores gp_predict's bits, so the two differ only by the
    rounding of the division, the logarithm and the sums: c eps S (_sum_bounds), derived, not tuned."""
    c = cases(shape)
    for unc, noise, masked in _variants():
        m, v = c.e.predict(c.Xt, c.St if unc else None, include_noise=noise)
        Y, obs = (c.Yh, c.obs) if masked else (c.Y, None)
        res = c.e.score(Y, c.Xt, c.St if unc else None, observed=obs, include_noise=noise)
        want = S.score_from(Y, m, v, obs)
        t = want['terms']
        _against(res, want, _sum_bounds(t, 1), _sum_bounds(t, 0), 'unc=%d noise=%d masked=%d' % (unc, noise, masked))
        if masked:
            assert res['row_logp'][5] == 0.0 and res['row_sse'][5] == 0.0 and res['row_chi2'][5] == 0.0      # the row with nothing observed


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'M%d-Q%d-D%d' % s[:3])
def test_against_the_independent_reference(cases, shape):
    """Case 2: score_ref on predict_ref.  Per entry the bound of tests/test_gpu_predictive.py on mean and variance (_tol, relative to max(1, |mean|)
    and to sf2) goes through the derivatives of each term -- logp: |e| / v tol_m + |e^2 / (2 v^2) - 1 / (2 v)| tol_v; e: tol_m; e^2: 2 |e| tol_m;
    e^2 / v: 2 |e| / v tol_m + e^2 / v^2 tol_v -- summed over the entries of the row or column, plus the bound of case 1."""
    c = cases(shape)
    sf2, beta = c.d['sf2'], c.d['beta']
    for unc, noise, masked in _variants():
        mr, vr = c.ref[unc]
        vr = vr + (1.0 / beta if noise else 0.0)
        Y, obs = (c.Yh, c.obs) if masked else (c.Y, None)
        res = c.e.score(Y, c.Xt, c.St if unc else None, observed=obs, include_noise=noise)
        want = S.score_from(Y, mr, vr, obs)
        t = want['terms']
        o, e, v = t['observed'], np.abs(t['e']), t['v']
        tol_m, tol_v = c.tol * max(1.0, np.max(np.abs(mr))), c.tol * sf2
        prop = dict(logp=np.where(o, e / v * tol_m + np.abs(e * e / (2 * v * v) - 1 / (2 * v)) * tol_v, 0.0), e=np.where(o, tol_m, 0.0),
                    e2=np.where(o, 2 * e * tol_m, 0.0), q=np.where(o, 2 * e / v * tol_m + e * e / (v * v) * tol_v, 0.0))
        rb, cb = _sum_bounds(t, 1), _sum_bounds(t, 0)
        for key in prop:
            rb[key] = rb[key] + prop[key].sum(axis=1)
            cb[key] = cb[key] + prop[key].sum(axis=0)
        _against(res, want, rb, cb, 'unc=%d noise=%d masked=%d' % (unc, noise, masked))


def _same(a, b, what):
    for k in range(1, 5):
        if a[k] is None or b[k] is None:
            continue
        assert np.array_equal(a[k], b[k], equal_nan=True), '%s: output %d differs' % (what, k)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'M%d-Q%d-D%d' % s[:3])
def test_determinism_and_invariance_bit_for_bit(cases, shape):
    """Case 3, on every shape, deterministic and uncertain, with and without the noise flag, fully observed and masked.  Every launch here has at
    most 256 tiles, the side of the GEMM dispatch on which a row is invariant without condition (include/gparml_hip.h; the other side and the
    crossing: test_across_the_gemm_dispatch_threshold)."""
    from gparml_amd import _lib
    c = cases(shape)
    e, n, D, Q = c.e, c.n, c.D, c.Q
    rs = np.random.RandomState(23)
    n3 = 300
    X3, S3 = rs.randn(n3, Q), rs.uniform(0.05, 0.5, size=(n3, Q))
    Y3 = e.predict(X3)[0] + rs.randn(n3, D) / np.sqrt(c.d['beta'])
    o3 = _mask(rs, n3, D, 129)
    lib = _lib.load()
    for unc, noise, masked in _variants():
        St, fl = (c.St if unc else None), (1 if noise else 0)
        Y, obs = (c.Yh, c.obs) if masked else (c.Y, None)
        what = 'unc=%d noise=%d masked=%d' % (unc, noise, masked)
        a = _raw(e, n, c.Xt, St, Y, obs, fl)
        assert a[0] == 0
        _same(a, _raw(e, n, c.Xt, St, Y, obs, fl), what + ': two runs')
        i = 7                                                                   # a row alone, and in reversed row order
        one = _raw(e, 1, c.Xt[i:i + 1], None if St is None else St[i:i + 1], Y[i:i + 1], None if obs is None else obs[i:i + 1], fl)
        for k in (1, 2, 3):
            assert one[k][0] == a[k][i], '%s: row %d alone: output %d' % (what, i, k)
        rev = _raw(e, n, c.Xt[::-1], None if St is None else St[::-1], Y[::-1], None if obs is None else obs[::-1], fl)
        for k in (1, 2, 3):
            assert np.array_equal(rev[k][::-1], a[k]), '%s: reversed rows: output %d' % (what, k)
        for want in ((1, 0, 0, 0), (0, 1, 1, 0), (0, 0, 0, 1), (1, 0, 0, 1)):      # a subset of the outputs gives the bits of the full call
            _same(a, _raw(e, n, c.Xt, St, Y, obs, fl, want), '%s: outputs %s' % (what, want))
        # 300 rows: one chunk by default, three chunks (and three segments, the last one ragged) at predict_rows = 128
        S3u = S3 if unc else None
        Yc, oc = (np.where(o3, Y3, np.nan), o3) if masked else (Y3, None)
        whole = _raw(e, n3, X3, S3u, Yc, oc, fl)
        lib.gp_debug_set_option(b'predict_rows', 128)
        try:
            parts = _raw(e, n3, X3, S3u, Yc, oc, fl)
        finally:
            lib.gp_debug_set_option(b'predict_rows', 0)
        assert whole[0] == 0 and parts[0] == 0
        _same(whole, parts, what + ': chunks of 128 against the default chunk')
        # and the three chunks against numpy on gp_predict's output: every segment and chunk enters the totals
        m, v = e.predict(X3, S3u, include_noise=noise)
        want = S.score_from(Yc, m, v, oc)
        res = dict(row_logp=parts[1], row_sse=parts[2], row_chi2=parts[3], cols=parts[4])
        _against(res, want, _sum_bounds(want['terms'], 1), _sum_bounds(want['terms'], 0), what + ': 300 rows in three chunks')


@pytest.mark.parametrize('M,Q,D,n', [(130, 17, 3, 8320), (64, 3, 300, 11008)], ids=['factor-product-260-tiles', 'mean-product-258-tiles'])
def test_across_the_gemm_dispatch_threshold(M, Q, D, n):
    """The documented limit of row invariance (include/gparml_hip.h).  gp_predict lets the size of a launch choose the GEMM
    kernel -- the 32 x 32-tile kernel up to 256 tiles of 128 x 128, the 128 x 128-tile kernel beyond -- and the score keeps gp_predict's bits, so it
    keeps that choice.  One chunk of n rows puts a product beyond 256 tiles: (130,17,3), n = 8320: the factor product, 65 x 4 = 260 tiles
    (deterministic inputs only); (64,3,300), n = 11008: the mean product, 86 x 3 = 258 tiles (both input forms).  At predict_rows = 4096 every
    chunk is back below.  Pinned:
      on either side the score is numpy's on gp_predict's own output of the same call shape (the case-1 bound c eps S);
      on either side a row is invariant among launches of that side: reversed row order in the large chunk; a row alone and a 128-row batch
        against the chunks of 4096;
      across the sides a row agrees to rounding: the bound of tests/test_gpu_predictive.py on mean and variance (_tol), taken twice (one for each
        kernel) and propagated through the terms' derivatives as in case 2, plus the case-1 bound.  Bit equality across is NOT promised."""
    from gparml_amd import _lib
    N = 300
    d = _model(N, D, M, Q, 'B', seed=M + Q + D)
    e = _engine(d, N, D, M, Q)
    lib = _lib.load()
    rs = np.random.RandomState(29)
    X, St = rs.randn(n, Q), rs.uniform(0.05, 0.5, size=(n, Q))
    Y = e.predict(X)[0] + rs.randn(n, D) / np.sqrt(d['beta'])
    tol = _tol(d, M, e.download('PSI2_SUM'))
    for unc in ((False,) if D == 3 else (False, True)):
        S_ = St if unc else None
        sub = lambda a, sl: None if a is None else a[sl]            # noqa: E731
        big = _raw(e, n, X, S_, Y, None, 1)
        assert big[0] == 0
        m, v = e.predict(X, S_, include_noise=True)
        want = S.score_from(Y, m, v)
        t = want['terms']
        rb, cb = _sum_bounds(t, 1), _sum_bounds(t, 0)
        _against(dict(row_logp=big[1], row_sse=big[2], row_chi2=big[3], cols=big[4]), want, rb, cb, 'large chunk, unc=%d' % unc)
        rev = _raw(e, n, X[::-1], sub(S_, slice(None, None, -1)), Y[::-1], None, 1)
        for k in (1, 2, 3):
            assert np.array_equal(rev[k][::-1], big[k]), 'large chunk, reversed rows: output %d' % k
        lib.gp_debug_set_option(b'predict_rows', 4096)
        try:
            small = _raw(e, n, X, S_, Y, None, 1)
            ms, vs = e.predict(X, S_, include_noise=True)
        finally:
            lib.gp_debug_set_option(b'predict_rows', 0)
        assert small[0] == 0
        ws = S.score_from(Y, ms, vs)
        _against(dict(row_logp=small[1], row_sse=small[2], row_chi2=small[3], cols=small[4]), ws, _sum_bounds(ws['terms'], 1), _sum_bounds(ws['terms'], 0),
                 'chunks of 4096, unc=%d' % unc)
        for sl in (slice(5000, 5001), slice(4000, 4128)):            # alone, and a batch across the chunk boundary at 4096: the small side
            part = _raw(e, sl.stop - sl.start, X[sl], sub(S_, sl), Y[sl], None, 1)
            for k in (1, 2, 3):
                assert np.array_equal(part[k], small[k][sl]), 'rows %s alone against the chunks of 4096: output %d' % (sl, k)
        # across the threshold: to rounding
        ea, vv = np.abs(t['e']), t['v']
        tol_m, tol_v = 2 * tol * max(1.0, np.max(np.abs(m))), 2 * tol * d['sf2']
        prop = dict(logp=ea / vv * tol_m + np.abs(ea * ea / (2 * vv * vv) - 1 / (2 * vv)) * tol_v, e2=2 * ea * tol_m,
                    q=2 * ea / vv * tol_m + ea * ea / (vv * vv) * tol_v)
        for k, key in ((1, 'logp'), (2, 'e2'), (3, 'q')):
            _check_close(small[k], big[k], 2 * rb[key] + prop[key].sum(axis=1), 'across the threshold, unc=%d, output %d' % (unc, k))
        print('rows whose bits differ across the threshold: %d of %d (row_logp)' % (np.sum(small[1] != big[1]), n))
    e.close()


def test_resident_rows():
    """Case 4: N_s = 300, free embeddings.  The resident form equals, bit for bit, the call with the same rows passed from the host."""
    from gparml_amd import _lib
    from gparml_amd.engine import ShardEngine
    M, Q, D, N = 64, 2, 3, 300
    d = _model(N, D, M, Q, 'B', seed=31)
    e = _engine(d, N, D, M, Q)
    Xm = e.download('X_MU')
    rs = np.random.RandomState(2)
    obs = _mask(rs, N, D, 200)
    lib = _lib.load()
    for rows in (0, 128):                                   # the default chunk, then three chunks: the resident Y is read at the chunk's offset
        lib.gp_debug_set_option(b'predict_rows', rows)
        try:
            for use_S, noise, masked in _variants():
                o, fl = (obs if masked else None), (1 if noise else 0)
                res = _raw(e, N, None, None, None, o, fl | (2 if use_S else 0))
                host = _raw(e, N, Xm, d['X_S'] if use_S else None, d['Y'], o, fl)
                assert res[0] == 0 and host[0] == 0
                _same(res, host, 'resident rows, use_S=%d noise=%d masked=%d' % (use_S, noise, masked))
                _same(res, _raw(e, N, None, None, d['Y'], o, fl | (2 if use_S else 0)), 'resident inputs with a host Y')
        finally:
            lib.gp_debug_set_option(b'predict_rows', 0)
    py = e.score(None, use_resident_S=True)
    assert np.array_equal(py['row_logp'], _raw(e, N, None, None, None, None, 3)[1])
    assert _raw(e, N - 1, None, None, None, None, 1)[0] == _lib.GP_ERR_BAD_ARG               # n must be N_s
    assert _raw(e, N, None, d['X_S'], None, None, 1)[0] == _lib.GP_ERR_BAD_ARG               # X_S with the resident rows
    e.close()
    # an engine that holds statistics but no shard
    e = _engine(d, N, D, M, Q)
    Psi2, C, sc = e.download('PSI2_SUM'), e.download('PSI1TY'), e.scalars()
    e.close()
    g = ShardEngine(1, D, M, Q)
    g.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'], N_global=N)
    g.set_local_statistics(sc['sum_YYT'], Psi2, C, sc['sum_exp_K_ii'], sc['KL'])
    g.global_step(sync=True)
    assert _raw(g, 1, None, None, None, None, 1)[0] == _lib.GP_ERR_STATE
    assert _raw(g, 0, None, None, None, None, 1)[0] == _lib.GP_ERR_STATE                     # whatever n is
    assert _raw(g, 1, np.zeros((1, Q)), None, np.zeros((1, D)), None, 1)[0] == _lib.GP_OK
    g.close()


def test_column_sums_in_the_documented_order(cases):
    """The order of the column sums, pinned independently of the library: under a mask in which every row scores one entry, cols[:, 2:5] are the row
    outputs themselves summed by score_ref.cols_in_device_order, bit for bit -- host rows and resident rows, the default chunk and chunks of 128
    (300 rows: three segments, the last one ragged)."""
    from gparml_amd import _lib
    c = cases(SHAPES[1])                                    # N = 300, D = 3
    e, N = c.e, c.N
    Xm = e.download('X_MU')
    obs = S.one_entry_mask(N, c.D, 200)
    lib = _lib.load()
    for rows in (0, 128):
        lib.gp_debug_set_option(b'predict_rows', rows)
        try:
            for name, r in (('host rows', _raw(e, N, Xm, None, c.d['Y'], obs, 1)), ('resident rows', _raw(e, N, None, None, None, obs, 1))):
                assert r[0] == 0, e.lib.gp_last_error(e.h)
                S.check_cols_order(r[1], r[2], r[3], r[4], obs, '%s, chunk %d' % (name, rows))
        finally:
            lib.gp_debug_set_option(b'predict_rows', 0)


def _finish_bits(e):
    e.phase2(True)
    out = e.finish()
    return [np.asarray(out[k]) for k in sorted(out)] + [e.download('GRAD_X_MU')]


def test_state_and_arguments():
    """Case 5 (all but the non-positive variance)."""
    from gparml_amd import _lib
    from gparml_amd.engine import ShardEngine
    M, Q, D, N = 16, 2, 3, 100
    d = _model(N, D, M, Q, 'B', seed=21)
    rs = np.random.RandomState(1)
    X, St, Y = rs.randn(9, Q), rs.uniform(0.1, 0.4, size=(9, Q)), rs.randn(9, D)
    e = ShardEngine(N, D, M, Q)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    assert _raw(e, 9, X, None, Y, None, 1)[0] == _lib.GP_ERR_STATE                  # no global step yet
    e.phase1()
    assert _raw(e, 9, X, None, Y, None, 1)[0] == _lib.GP_ERR_STATE
    e.global_step(sync=True)
    good = _raw(e, 9, X, St, Y, None, 1)
    assert good[0] == _lib.GP_OK
    before = _finish_bits(e)
    Ynan = Y.copy()
    Ynan[3, 1] = np.nan
    o = np.ones((9, D), dtype=bool)
    o[3, 1] = False
    bad = [_raw(e, -1, X, None, Y, None, 1), _raw(e, 9, X, None, Y, None, 4), _raw(e, 9, X, None, Ynan, None, 1), _raw(e, 9, X, None, Y, None, 3),
           _raw(e, 9, X, None, None, None, 1), _raw(e, 9, X, -St, Y, None, 1), _raw(e, 9, np.where(X > 5, X, np.inf), None, Y, None, 1)]
    for r in bad:
        assert r[0] == _lib.GP_ERR_BAD_ARG
        assert all(np.all(a == -7.0) for a in r[1:])                               # decided before anything is launched: nothing written
    assert _raw(e, 9, X, None, Ynan, o, 1)[0] == _lib.GP_OK                         # the NaN is hidden: never read
    z = _raw(e, 0, X, None, None, None, 1)
    assert z[0] == _lib.GP_OK and np.array_equal(z[4], np.zeros((D, 5)))
    assert _raw(e, 0, None, None, None, None, 1)[0] == _lib.GP_ERR_BAD_ARG             # the resident rows: n must be N_s, n = 0 included
    with pytest.raises(AssertionError):
        e.score(Ynan, X, observed=np.ones((9, D)))
    # after all of these a valid call and phase 2 + finish give the bits they gave before
    _same(good, _raw(e, 9, X, St, Y, None, 1), 'a valid call after the refused ones')
    e.global_step(sync=True)
    for a, b in zip(before, _finish_bits(e)):
        assert np.array_equal(a, b)
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    assert _raw(e, 9, X, None, Y, None, 1)[0] == _lib.GP_ERR_STATE                  # new globals, no global step on them
    e.close()


def test_variance_that_is_not_positive():
    """Case 5, the non-positive variance: f scored without the noise at the training inputs of an M = N exact-GP model (the 40-point grid of
    test_exact_gp_limit) with beta = 1e17, where var_f ~ 1 / beta lies below the rounding of sf2 - |a|^2 + |b|^2: predict_ref gives
    var_f <= 0 for 12 of the 40 rows (checked below, on the CPU).  The rows the DEVICE's own variance puts at <= 0 are the ones that must be NaN."""
    from gparml_amd import _lib
    from gparml_amd.engine import ShardEngine
    rs = np.random.RandomState(3)
    X = np.stack(np.meshgrid(np.linspace(-3, 3, 8), np.linspace(-2, 2, 5)), -1).reshape(-1, 2)
    Y = np.sin(X.dot(rs.randn(2, 3))) + 0.1 * rs.randn(40, 3)
    sf2, alpha, beta = 1.3, np.array([0.8, 1.1]), 1e17
    Psi2, C = R.statistics(X, sf2, alpha, Y, X, np.zeros_like(X))
    assert np.any(R.predict(X, sf2, alpha, beta, Psi2, C, X, None, False)[1] <= 0)
    e = ShardEngine(40, 3, 40, 2)
    e.upload_shard(Y, X, np.zeros_like(X))
    e.set_globals(X, sf2, alpha, beta)
    e.phase1()
    e.global_step(sync=True)
    v = e.predict(X)[1][:, 0]
    badrow = ~(v > 0)
    print('device var_f <= 0 in %d of 40 rows' % badrow.sum())
    assert badrow.any() and not badrow.all()
    before = _finish_bits(e)
    e.global_step(sync=True)
    res = _raw(e, 40, X, None, Y, None, 0)
    assert res[0] == _lib.GP_ERR_NON_FINITE
    assert ('row %d)' % np.flatnonzero(badrow)[0]) in e.lib.gp_last_error(e.h).decode()
    o = np.repeat(~badrow[:, None], 3, axis=1)
    ok = _raw(e, 40, X, None, Y, o, 0)                      # the same call with those rows hidden
    assert ok[0] == _lib.GP_OK
    for k in (1, 2, 3):
        assert np.all(np.isnan(res[k][badrow])) and np.array_equal(res[k][~badrow], ok[k][~badrow])
    assert np.all(np.isnan(res[4]))                         # every column is scored in a bad row
    with pytest.raises(FloatingPointError) as err:
        e.score(Y, X, include_noise=False)
    assert np.array_equal(err.value.result['row_logp'], res[1], equal_nan=True)
    # (the noise flag does not help here: 1 / beta = 1e-17 lies below the rounding of the sum it is added to)
    for a, b in zip(before, _finish_bits(e)):
        assert np.array_equal(a, b)
    e.close()


def _stats_of(e):
    sc = e.scalars()
    return dict(sum_YYT=sc['sum_YYT'], sum_exp_K_mi_K_im=e.download('PSI2_SUM'), sum_exp_K_miY=e.download('PSI1TY'), sum_exp_K_ii=sc['sum_exp_K_ii'],
                sum_KL=sc['KL'])


def test_python_layer():
    """Case 6."""
    from gparml_amd.driver import transform_vec
    from gparml_amd.engine import ShardEngine
    from gparml_amd.predict import Predictor
    from gparml_amd.resident import ResidentModel
    M, Q, D, N = 20, 2, 6, 200
    d = _model(N, D, M, Q, 'B', seed=41)
    e = _engine(d, N, D, M, Q)
    rs = np.random.RandomState(4)
    n = 12
    Xt, St = rs.randn(n, Q), rs.uniform(0.05, 0.3, size=(n, Q))
    Yt = e.predict(Xt)[0] + rs.randn(n, D) / np.sqrt(d['beta'])
    Yt[2, 4] = np.nan
    # Predictor.score is ShardEngine.score on the same statistics
    p = Predictor(dict(Z=d['Z'], sf2=d['sf2'], alpha=d['alpha'], beta=d['beta']), _stats_of(e), N, D)
    a, b = p.score(Yt, Xt, St), e.score(Yt, Xt, St)
    for k in ('row_logp', 'row_sse', 'row_chi2', 'cols'):
        assert np.array_equal(a[k], b[k]), k
    # the figures of the dict are those derived from the sums
    s = S.summary(b['cols'])
    for k in ('count', 'bias', 'rmse', 'chi2_mean', 'nlpd'):
        assert np.array_equal(b[k], s[k], equal_nan=True), k
    tot = b['cols'].sum(axis=0)
    assert b['pooled']['nlpd'] == -tot[4] / tot[0] and b['pooled']['rmse'] == np.sqrt(tot[2] / tot[0]) and b['pooled']['count'] == n * D - 1
    # impute_score scores exactly the entries that were hidden and are known
    mask = [0, 2, 3]
    sc, res = p.impute_score(Yt, mask, X_mu0=Xt, X_S0=St, iterations=3)
    hidden = np.ones((n, D), dtype=bool)
    hidden[:, mask] = False
    hidden &= ~np.isnan(Yt)
    assert np.array_equal(sc['count'], hidden.sum(axis=0).astype(float)) and sc['pooled']['count'] == hidden.sum()
    assert np.array_equal(sc['row_logp'], e.score(Yt, res[0], res[1], observed=hidden)['row_logp'])
    e.close()
    # ResidentModel.score_training on two shards against one engine that holds both shards' rows and the same reduced statistics
    h = N // 2
    raw = np.log(np.expm1(d['X_S']))                                                # free embeddings live in softplus-inverse space
    shards = [(d['Y'][:h], d['X_mu'][:h], raw[:h]), (d['Y'][h:], d['X_mu'][h:], raw[h:])]
    model = ResidentModel(shards, M, Q, D, fixed_embeddings=False)
    x = np.concatenate([d['Z'].ravel(), [d['sf2']], d['alpha'], [d['beta']]])
    x = np.where(model._pos, np.log(np.expm1(np.where(model._pos, x, 1.0))), x)     # the optimiser's vector: softplus-inverse of the positive entries
    xt = transform_vec(model._pos, x)
    Z, sf2, alpha, beta = xt[:M * Q].reshape(M, Q), xt[M * Q], xt[M * Q + 1:M * Q + 1 + Q], xt[M * Q + 1 + Q]
    for use_S in (True, False):
        got = model.score_training(use_S=use_S, flat_array=x)
        one = ShardEngine(N, D, M, Q)
        one.upload_shard(d['Y'], d['X_mu'], raw, xs_is_raw=True)
        one.set_globals(Z, sf2, alpha, beta, N_global=N)
        one.combine(model.engines[0], 'stats', 'copy')          # the reduced statistics of the two shards, bit for bit
        one.global_step(sync=True)
        want = one.score(None, use_resident_S=use_S)
        one.close()
        for k in ('row_logp', 'row_sse', 'row_chi2'):
            assert np.array_equal(got[k], want[k]), k           # a row's bits depend on the row and the model only
        # the shards' column sums are added on the host: the case-1 bound on the terms
        eng = model.engines[0]
        X_all = np.concatenate([g.download('X_MU') for g in model.engines])
        m, v = eng.predict(X_all, np.log1p(np.exp(raw)) if use_S else None, include_noise=True)
        t = S.score_from(d['Y'], m, v)['terms']
        cb = _sum_bounds(t, 0)
        assert np.array_equal(got['cols'][:, 0], want['cols'][:, 0])
        for k, key in ((1, 'e'), (2, 'e2'), (3, 'q'), (4, 'logp')):
            _check_close(got['cols'][:, k], want['cols'][:, k], cb[key], 'score_training cols[%d]' % k)
        assert np.array_equal(got['nlpd'], S.summary(got['cols'])['nlpd'])
    model.close()
