"""gp_nearest_rows_masked (csrc/nearest.hip, nn_search_kernel<true>): the nearest training row of new rows that each observe their own columns,
through the C ABI, ShardEngine.nearest_rows(observed=), init.nearest_start(observed=) and Predictor.infer(ragged=True, nearest='device').

Shapes: D in {1, 21, 37} (less than one 16-column tile, a ragged second tile, more than two tiles), n in {1, 17, 37} (no multiples of the 16 new
rows of a workgroup), n_train in {1, 255, 700} (no multiples of the 256-row tile), resident rows and host rows.  Every test runs at the default
chunking and with the "nearest_rows" option at 16 (chunks of 16 new rows and of 256 host rows: several on both sides).

Exact everywhere but in one test: integer data makes every sum exact in any order, and everything about determinism is bit for bit.  Normal data
against numpy (test_normal_data_against_numpy): both sides add the same k non-negative terms, each rounded once, so each is within (k + 2) u of
the exact sum, u = 2^-53 -- the bounds there."""
import ctypes

import numpy as np
import pytest

from nearest_masked_util import masked_nearest, masked_sqdist, random_masks
from nearest_util import sqdist_cols

pytestmark = pytest.mark.gpu

Q = 3
DS, NS, NTS = (1, 21, 37), (1, 17, 37), (1, 255, 700)
SHAPES = [(D, N) for D in DS for N in NTS]
IDS = ['D%d_N%d' % s for s in SHAPES]
U = 2.0 ** -53


def _set_rows(k):
    from gparml_amd import _lib
    assert _lib.load().gp_debug_set_option(b'nearest_rows', k) == 0


def _chunkings(fn):
    """fn(rows) at the default chunking and at 16; the option is back at 0 afterwards."""
    out = []
    for rows in (0, 16):
        _set_rows(rows)
        try:
            out.append(fn(rows))
        finally:
            _set_rows(0)
    return out


def _engine(Yt, Xt, M=4):
    from gparml_amd.engine import ShardEngine
    eng = ShardEngine(Yt.shape[0], Yt.shape[1], M, Xt.shape[1])
    eng.upload_shard(Yt, Xt, np.zeros(Xt.shape))
    return eng


def _case(D, N, n, integer, seed=0):
    rs = np.random.RandomState(seed + 1000 * D + 7 * N + n)
    draw = (lambda *s: rs.randint(-8, 9, size=s).astype(float)) if integer else rs.randn
    Yt, Ys = draw(N, D), draw(n, D)
    return Yt, rs.randn(N, Q), Ys, random_masks(rs, n, D), rs


def _both(eng, Yt, Ys, obs):
    """(resident result, host-rows result) of one masked call each."""
    return eng.nearest_rows(Ys, observed=obs), eng.nearest_rows(Ys, observed=obs, Y_train=Yt)


def _same(a, b):
    return all((u is None and v is None) or np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize('D,N', SHAPES, ids=IDS)
def test_exact_parity_on_integer_data(D, N):
    """Integers in [-8, 8]: dist2 and index equal numpy's exactly, with many true ties: the lowest index wins."""
    for n in NS:
        Yt, Xt, Ys, obs, _ = _case(D, N, n, True)
        if N > 20:
            Yt[N // 2] = Yt[2]                    # a duplicate row in another lane (and tile, at 700)
            Ys[0] = Yt[2]
        d2, idx = masked_nearest(Ys, Yt, obs)
        eng = _engine(Yt, Xt)
        try:
            def run(rows):
                res, host = _both(eng, Yt, np.where(obs, Ys, np.nan), obs)
                assert np.array_equal(res[0], d2) and np.array_equal(res[1], idx), (n, rows)
                assert np.array_equal(res[2], Xt[idx]) and host[2] is None, (n, rows)
                assert np.array_equal(host[0], d2) and np.array_equal(host[1], idx), (n, rows)
                assert eng.nearest_rows(Ys, observed=obs, want_x=False)[2] is None
            _chunkings(run)
        finally:
            eng.close()


@pytest.mark.parametrize('D,N,other', [(21, 255, 9), (37, 255, 9), (21, 700, 600), (37, 700, 600)], ids=['D21_lanes', 'D37_lanes', 'D21_tiles', 'D37_tiles'])
def test_a_masked_column_does_not_count(D, N, other):
    """Rows 3 and ``other`` equal the new row on its observed columns and differ wildly on its hidden ones; every other row is far away."""
    rs = np.random.RandomState(D + N)
    obs = np.zeros((3, D), dtype=bool)
    obs[0, ::3] = True                            # the row under test: columns 0, 3, 6, ...
    obs[1] = True
    obs[2, 1::2] = True
    Ys = rs.randn(3, D)
    Yt = 100.0 + rs.randn(N, D)
    Xt = rs.randn(N, Q)
    for r, wild in ((3, 1e6), (other, -1e6)):
        Yt[r] = np.where(obs[0], Ys[0], wild)
    Yn = np.where(obs, Ys, np.nan)
    eng = _engine(Yt, Xt)
    try:
        def run(rows):
            for out in _both(eng, Yt, Yn, obs):
                assert out[1][0] == 3 and out[0][0] == 0.0, (rows, out[0][0], out[1][0])
                assert out[1][1] not in (3, other) and out[0][1] > 0.0
            # with row 3 moved away the other one is found, at zero as well
            moved = Yt.copy()
            moved[3] += 50.0
            out = eng.nearest_rows(Yn, observed=obs, Y_train=moved)
            assert out[1][0] == other and out[0][0] == 0.0, rows
        _chunkings(run)
    finally:
        eng.close()


@pytest.mark.parametrize('D,N', SHAPES, ids=IDS)
def test_nan_in_every_unobserved_entry(D, N):
    for n in NS:
        Yt, Xt, Ys, obs, _ = _case(D, N, n, False, seed=1)
        eng = _engine(Yt, Xt)
        try:
            def run(rows):
                zeros, nans = _both(eng, Yt, np.where(obs, Ys, 0.0), obs), _both(eng, Yt, np.where(obs, Ys, np.nan), obs)
                assert _same(zeros[0], nans[0]) and _same(zeros[1], nans[1]), (n, rows)
                assert np.all(np.isfinite(nans[0][0])) and nans[0][1].min() >= 0 and nans[0][1].max() < N
            _chunkings(run)
        finally:
            eng.close()


@pytest.mark.parametrize('D,N', SHAPES, ids=IDS)
def test_one_shared_pattern_is_the_column_list_entry(D, N):
    """All rows with one pattern: the bits of gp_nearest_rows with cols = that pattern; all ones: the bits of cols=None.  Normal data."""
    for n in NS:
        Yt, Xt, Ys, obs, rs = _case(D, N, n, False, seed=2)
        patterns = [np.ones(D, dtype=bool)] + ([obs[-1], np.arange(D) % 16 == 5, np.arange(D) >= D - 2] if D > 1 else [])
        eng = _engine(Yt, Xt)
        try:
            def run(rows):
                for k, pat in enumerate(patterns):
                    o = np.tile(pat, (n, 1))
                    cols = None if k == 0 else np.flatnonzero(pat)
                    Yn = np.where(o, Ys, np.nan)
                    res, host = _both(eng, Yt, Yn, o)
                    assert _same(res, eng.nearest_rows(Yn, cols=cols)), (n, k, rows)
                    assert _same(host, eng.nearest_rows(Yn, cols=cols, Y_train=Yt)), (n, k, rows)
            _chunkings(run)
        finally:
            eng.close()


@pytest.mark.parametrize('D,N', SHAPES, ids=IDS)
def test_a_row_does_not_depend_on_the_others(D, N):
    """Alone, in the batch, permuted, chunked, host rows and resident rows: the same bits."""
    n = NS[-1]
    Yt, Xt, Ys, obs, rs = _case(D, N, n, False, seed=3)
    Yn = np.where(obs, Ys, np.nan)
    eng = _engine(Yt, Xt)
    try:
        res, host = _both(eng, Yt, Yn, obs)
        assert np.array_equal(res[0], host[0]) and np.array_equal(res[1], host[1])
        perm = rs.permutation(n)

        def run(rows):
            for out in _both(eng, Yt, Yn, obs):
                assert np.array_equal(out[0], res[0]) and np.array_equal(out[1], res[1]), rows
            out = eng.nearest_rows(Yn[perm], observed=obs[perm])
            assert _same(out, [r[perm] for r in res]), rows
            for m in NS[:2]:                                                       # the first rows as a smaller batch
                assert _same(eng.nearest_rows(Yn[:m], observed=obs[:m]), [r[:m] for r in res]), (rows, m)
            for i in range(n):
                one = eng.nearest_rows(Yn[i], observed=obs[i], Y_train=Yt if i % 2 else None)
                assert one[0][0] == res[0][i] and one[1][0] == res[1][i], (rows, i)
        _chunkings(run)
    finally:
        eng.close()


@pytest.mark.parametrize('D,N', SHAPES, ids=IDS)
def test_normal_data_against_numpy(D, N):
    """No case excluded.  For the device's index i of a row with k observed columns: |dist2 - ref[i]| <= (k + 2) u ref[i] and
    ref[i] <= (1 + 2 (k + 2) u) min_r ref[r]."""
    for n in NS:
        Yt, Xt, Ys, obs, _ = _case(D, N, n, False, seed=4)
        ref = masked_sqdist(Ys, Yt, obs)
        k = obs.sum(axis=1)
        eng = _engine(Yt, Xt)
        try:
            def run(rows):
                for d2, idx, _x in _both(eng, Yt, np.where(obs, Ys, np.nan), obs):
                    assert idx.min() >= 0 and idx.max() < N
                    chosen = ref[np.arange(n), idx]
                    err = np.abs(d2 - chosen) / np.where(chosen > 0, chosen, 1.0)
                    excess = chosen / np.where(ref.min(axis=1) > 0, ref.min(axis=1), 1.0) - 1.0
                    print('D=%d N=%d n=%d rows=%d: dist2 error %.2e of %.2e, index excess %.2e' % (D, N, n, rows, err.max(), (k.max() + 2) * U, excess.max()))
                    assert np.all(np.abs(d2 - chosen) <= (k + 2) * U * chosen), (n, rows)
                    assert np.all(chosen <= (1.0 + 2.0 * (k + 2) * U) * ref.min(axis=1)), (n, rows)
            _chunkings(run)
        finally:
            eng.close()


def test_errors_and_edges():
    from gparml_amd import _lib
    from gparml_amd.engine import ShardEngine
    lib = _lib.load()
    N, D, n = 50, 4, 3
    rs = np.random.RandomState(9)
    Yt, Xt, Ys = rs.randn(N, D), rs.randn(N, Q), rs.randn(n, D)
    obs = np.array([[1, 0, 1, 0], [0, 0, 0, 7], [1, 1, 1, 1]], dtype=np.uint8)            # nonzero = observed
    eng = ShardEngine(N, D, 4, Q)
    dp, up, lp = _lib._dp, _lib._u8p, ctypes.POINTER(ctypes.c_int64)
    d2, idx, x = np.full(n, 7.0), np.full(n, 7, dtype=np.int64), np.full((n, Q), 7.0)

    def call(Y_train, o, want_x, n=n, Y=Ys):
        return lib.gp_nearest_rows_masked(eng.h, 0 if Y_train is None else Y_train.shape[0], None if Y_train is None else Y_train.ctypes.data_as(dp), n,
                                          Y.ctypes.data_as(dp), None if o is None else o.ctypes.data_as(up), d2.ctypes.data_as(dp), idx.ctypes.data_as(lp),
                                          x.ctypes.data_as(dp) if want_x else None)

    def run(rows):
        assert call(None, obs, True) == _lib.GP_ERR_STATE and b'gp_upload_shard' in lib.gp_last_error(eng.h)      # resident rows before an upload
        assert call(Yt, obs, True) == _lib.GP_ERR_BAD_ARG and b'x_near' in lib.gp_last_error(eng.h)                # x_near with host rows
        assert call(Yt, None, False) == _lib.GP_ERR_BAD_ARG and b'observed' in lib.gp_last_error(eng.h)            # a NULL mask
        none = obs.copy()
        none[1] = 0
        assert call(Yt, none, False) == _lib.GP_ERR_BAD_ARG and b'no observed column' in lib.gp_last_error(eng.h)
        bad = Ys.copy()
        bad[0, 2] = np.nan                                                                                       # observed by row 0
        assert call(Yt, obs, False, Y=bad) == _lib.GP_ERR_BAD_ARG and b'not finite' in lib.gp_last_error(eng.h)
        badt = Yt.copy()
        badt[7, 1] = np.inf
        assert call(badt, obs, False) == _lib.GP_ERR_BAD_ARG and b'Y_train' in lib.gp_last_error(eng.h)
        assert call(Yt, obs, False, n=-1) == _lib.GP_ERR_BAD_ARG
        assert np.all(d2 == 7.0) and np.all(idx == 7) and np.all(x == 7.0)              # a failed call writes nothing
        assert call(Yt, obs, False, n=0) == _lib.GP_OK and np.all(d2 == 7.0)            # n = 0 writes nothing
        assert call(Yt, None, False, n=0) == _lib.GP_OK
        assert call(Yt[:0], obs, False) == _lib.GP_OK                                   # no training rows
        assert np.all(np.isinf(d2)) and np.all(d2 > 0) and np.all(idx == -1)
        ok = Ys.copy()
        ok[0, 1] = np.nan                                                               # not observed by row 0: legal
        ok[1, :3] = np.inf
        assert call(Yt, obs, False, Y=ok) == _lib.GP_OK
        want = masked_nearest(Ys, Yt, obs)
        assert np.array_equal(idx, want[1]) and np.allclose(d2, want[0], rtol=1e-14)
        assert lib.gp_nearest_rows_masked(eng.h, N, Yt.ctypes.data_as(dp), n, ok.ctypes.data_as(dp), obs.ctypes.data_as(up), None, None, None) == _lib.GP_OK
        d2[:], idx[:] = 7.0, 7
    _chunkings(run)
    eng.upload_shard(Yt, Xt, np.zeros(Xt.shape))
    assert call(None, obs, True) == _lib.GP_OK
    assert np.array_equal(idx, masked_nearest(Ys, Yt, obs)[1]) and np.array_equal(x, Xt[idx])
    with pytest.raises(AssertionError):
        eng.nearest_rows(Ys, cols=[0], observed=obs)
    with pytest.raises(AssertionError):
        eng.nearest_rows(Ys, observed=obs[:, :3])
    eng.close()


def test_the_evaluation_is_untouched():
    """An evaluation, the statistics part again, masked searches, then gp_predict / gp_phase2 / gp_finish equal the same sequence without them."""
    from gparml_amd.engine import ShardEngine
    from oracle import factorised as Fz
    N, D, M, Ql = 600, 5, 12, 3
    d = Fz.synthetic_shard(N, D, M, Ql, regime='B', seed=4, zseed=5, alpha_value=0.3)
    obs = random_masks(np.random.RandomState(1), 37, D)
    eng = ShardEngine(N, D, M, Ql)
    eng.upload_shard(d['Y'], d['X_mu'], d['X_S'])

    def sequence(with_search):
        eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
        first = eng.evaluate(True)
        eng.phase1()
        eng.global_step(sync=True)
        if with_search:
            eng.nearest_rows(np.where(obs, d['Y'][:37] + 0.1, np.nan), observed=obs)                            # resident rows
            eng.nearest_rows(d['Y'][:17], observed=obs[:17], Y_train=d['Y'][100:500])                            # host rows
        pred = eng.predict(d['X_mu'][:20])
        eng.phase2(True)
        out = eng.finish()
        return [first['F'], first['grad_Z'], first['grad_X_mu'], out['F'], out['grad_Z'], out['grad_alpha'], out['grad_sf2'], out['grad_beta'],
                eng.download('GRAD_X_MU'), eng.download('GRAD_X_S'), pred[0], pred[1]]
    try:
        plain = sequence(False)
        for searched in _chunkings(lambda rows: sequence(True)):
            for a, b in zip(plain, searched):
                assert np.array_equal(np.asarray(a), np.asarray(b))
    finally:
        eng.close()


def _python_problem():
    """D 8, M 12, Q 2: a small trained model for the Predictor; 40 new rows with 2 to 4 hidden columns each; three host shards of 50 rows with
    integer-valued outputs, so that the device's search and the host's k-d trees are both exact and agree on ties and on the cut-off."""
    import predict_ref as R
    from gparml_amd.predict import Predictor
    rs = np.random.RandomState(11)
    M, Ql, D, N = 12, 2, 8, 200
    Xm, Xs = rs.randn(N, Ql), np.full((N, Ql), 0.02)
    A = rs.randn(Ql, D)
    Y = np.sin(Xm.dot(A)) + 0.5 * Xm.dot(A) + rs.randn(N, D) / np.sqrt(50.0)
    Z, sf2, alpha, beta = Xm[rs.choice(N, M, replace=False)].copy(), 1.0, np.ones(Ql), 50.0
    Psi2, C = R.statistics(Z, sf2, alpha, Y, Xm, Xs)
    gs = dict(Z=Z, sf2=sf2, alpha=alpha, beta=beta)
    acc = dict(sum_YYT=np.sum(Y ** 2), sum_exp_K_mi_K_im=Psi2, sum_exp_K_miY=C, sum_exp_K_ii=N * sf2, sum_KL=0.0)
    Ytr = rs.randint(-3, 4, size=(150, D)).astype(float)
    Xtr = rs.randn(150, Ql)
    Ytr[120] = Ytr[10]                                                               # the same outputs in the first and the third shard
    training = [(Ytr[:50], Xtr[:50]), (Ytr[50:100], Xtr[50:100]), (Ytr[100:], Xtr[100:])]
    n = 40
    Yn = Ytr[rs.randint(150, size=n)] + rs.randint(-1, 2, size=(n, D))
    Yn[0] = Ytr[10]
    Yn[1] = Ytr[3] + 30.0                                                           # beyond the cut-off
    Yn[2] = Ytr[5]
    hidden = [rs.choice(D, size=rs.randint(2, 5), replace=False) for _ in range(n)]
    hidden[2] = np.array([6, 7])
    for i, h in enumerate(hidden):
        Yn[i, h] = np.nan
    Yn[2, :6] = Ytr[5, :6] + np.array([6.0, 0, 0, 0, 0, 0])                         # candidates for exactly 6 away: the cut-off is strict
    return Predictor, gs, acc, N, D, Z, training, Yn


def test_through_python_on_the_device():
    from gparml_amd.engine import ShardEngine
    Predictor, gs, acc, N, D, Z, training, Yn = _python_problem()
    n = Yn.shape[0]
    S0 = np.full((n, Z.shape[1]), 0.5)
    rs = np.random.RandomState(12)
    Mz = rs.randint(-3, 4, size=(Z.shape[0], D)).astype(float)
    Mz[7] = Mz[2]

    class Spy(ShardEngine):
        starts, searches, stub_mz = [], 0, False

        def infer_latent_rows(self, Y, X_mu, X_S, **kw):
            Spy.starts.append(np.array(X_mu))
            return ShardEngine.infer_latent_rows(self, Y, X_mu, X_S, **kw)

        def nearest_rows(self, *a, **kw):
            Spy.searches += 1
            return ShardEngine.nearest_rows(self, *a, **kw)

        def predict(self, X, *a, **kw):
            return (Mz, None) if Spy.stub_mz else ShardEngine.predict(self, X, *a, **kw)

    pred = Predictor(gs, acc, N, D, engine_class=Spy)

    def run(rows):
        Spy.starts, Spy.searches, Spy.stub_mz = [], 0, False
        host = pred.infer(Yn, X_S0=S0, training=training, iterations=3, ragged=True)
        assert Spy.searches == 0
        dev = pred.infer(Yn, X_S0=S0, training=iter(training), iterations=3, ragged=True, nearest='device')
        assert Spy.searches == len(training), rows
        assert np.array_equal(Spy.starts[0], Spy.starts[1]), rows                    # row for row
        assert all(np.array_equal(a, b) for a, b in zip(host, dev))
        zero = np.all(Spy.starts[1] == 0.0, axis=1)
        assert zero[1] and not zero[0] and 1 <= zero.sum() <= n // 2, zero.sum()     # the cut-off is hit by some rows, not by most
        assert np.array_equal(Spy.starts[1][0], training[0][1][10])                  # the first shard keeps the tie with the third
        Spy.stub_mz = True
        pred.infer(Yn, X_S0=S0, start='inducing', iterations=3, ragged=True, nearest='device')
        assert Spy.searches == len(training) + 1
        assert np.array_equal(Spy.starts[2], Predictor.inducing_start(Yn, ~np.isnan(Yn), Z, Mz)), rows
    _chunkings(run)
    # ResidentModel.infer_start and init.nearest_start on real engines, resident rows: the per-row loop over column lists
    from gparml_amd import init
    engines = [_engine(y, x) for y, x in training]
    try:
        obs = ~np.isnan(Yn)
        got = init.nearest_start(engines, Yn, observed=obs)
        for i in range(n):
            one = init.nearest_start(engines, Yn[i:i + 1], cols=list(np.flatnonzero(obs[i])))
            assert all(np.array_equal(a[i:i + 1], b) for a, b in zip(got, one)), i
    finally:
        for e in engines:
            e.close()
