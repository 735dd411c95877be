"""gp_nearest_rows (csrc/nearest.hip): per new row the nearest training row -- the start of latent inference (predict.py:44-66) -- through the C ABI,
ShardEngine.nearest_rows, gparml_amd.init.nearest_start on real engines, ResidentModel.infer_start and Predictor.infer / test (nearest='device').

Every new row is checked against brute force, no exclusions: the numpy float64 squared distance (direct form, the same columns in the same order)
at the returned index is at most the row's minimum times 1 + 1e-12, and the returned dist2 agrees with it to 1e-12 relative.  Both sides add the
same non-negative terms, so each is within (D + 2) 2^-53 relative of the exact sum: under 1e-12 for any D below 4000.  Everything else here is
exact: indices, ties, x_near = X_mu[index], host rows against resident rows, chunked against unchunked, and the reference's recorded starting means."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from nearest_util import sqdist_cols

pytestmark = pytest.mark.gpu

TOL = 1e-12
SCATTERED = [0, 3, 17, 29, 41, 56, 63, 78, 90, 99]
# (N, D, n, cols)
SHAPES = [(5000, 7, 300, None), (3000, 100, 64, None), (3000, 100, 64, SCATTERED), (1000, 130, 33, None), (257, 3, 5, [2]), (1, 4, 3, None),
          (700, 1, 40, None), (5000, 7, 1, None)]
Q = 3


def _case(N, D, n, seed=0):
    rs = np.random.RandomState(seed + 7 * N + D)
    return rs.randn(N, D), rs.randn(N, Q), rs.randn(n, D)


def _engine(Yt, Xt, M=4):
    from gparml_amd.engine import ShardEngine
    eng = ShardEngine(Yt.shape[0], Yt.shape[1], M, Xt.shape[1])
    eng.upload_shard(Yt, Xt, np.zeros(Xt.shape))
    return eng


def _set_rows(k):
    from gparml_amd import _lib
    assert _lib.load().gp_debug_set_option(b'nearest_rows', k) == 0


def check(Yt, Xt, Ys, cols, out, where=''):
    """The module docstring's checks on one call's (dist2, index, x_near); returns the chosen distances."""
    d2, idx, x = out
    n, N = Ys.shape[0], Yt.shape[0]
    assert d2.shape == (n,) and idx.shape == (n,) and idx.dtype == np.int64, where
    assert idx.min() >= 0 and idx.max() < N, (where, idx.min(), idx.max())
    ref = sqdist_cols(Ys, Yt, cols)
    lo, chosen = ref.min(axis=1), ref[np.arange(n), idx]
    excess = float(np.max((chosen - lo) / np.where(lo > 0, lo, 1.0)))
    err = float(np.max(np.abs(d2 - chosen) / np.where(chosen > 0, chosen, 1.0)))
    print('%s N=%d D=%d n=%d: index excess %.2e, dist2 error %.2e' % (where, N, Yt.shape[1], n, excess, err))
    assert np.all(chosen <= lo * (1.0 + TOL)), (where, 'a new row is not at its nearest training row', excess)
    assert np.all(np.abs(d2 - chosen) <= TOL * chosen), (where, err)
    if x is not None:
        assert np.array_equal(x, Xt[idx]), where
    return chosen


def test_reference_pin():
    """The reference's own starting means (the first half of the first recorded flat vector of runs A and C) from two engines that hold the
    fixture's training shards and trained embeddings."""
    from gparml_amd import init
    z = np.load(os.path.join(GOLDEN_DIR, 'predict_gplvm_2shards.npz'))
    engines = [_engine(z['train_Y_%d' % i], z['train_X_%d' % i]) for i in range(2)]
    try:
        XA = init.nearest_start(engines, z['A_Y_test'])[0]
        assert np.array_equal(XA.ravel(), z['A_call0_x'][:6])
        XC = init.nearest_start(engines, z['C_Y_test'], cols=[int(v) for v in z['C_mask']])[0]
        assert np.array_equal(XC.ravel(), z['C_call0_x'][:8])
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize('N,D,n,cols', SHAPES, ids=['N5000_D7_n300', 'N3000_D100_n64', 'N3000_D100_n64_cols10', 'N1000_D130_n33', 'N257_D3_n5_col2',
                                                    'N1_D4_n3', 'N700_D1_n40', 'N5000_D7_n1'])
def test_every_new_row_against_brute_force(N, D, n, cols):
    Yt, Xt, Ys = _case(N, D, n)
    if cols is not None:
        Ys = Ys.copy()
        Ys[:, [c for c in range(D) if c not in cols]] = np.nan          # the unobserved columns are never read
    eng = _engine(Yt, Xt)
    try:
        out = eng.nearest_rows(Ys, cols=cols)
        check(Yt, Xt, np.nan_to_num(Ys), cols, out, 'resident')
        d2, idx, x = eng.nearest_rows(Ys, cols=cols, want_x=False)
        assert x is None and np.array_equal(d2, out[0]) and np.array_equal(idx, out[1])
    finally:
        eng.close()


def test_padding_never_wins():
    """N = 130 of Np = 256: the training rows lie around 50, so a padded row -- zeros, or whatever an evaluation or the poison mode leaves -- would
    be the nearest to a new row of zeros if it were looked at."""
    from gparml_amd import _lib
    from oracle import factorised as Fz
    lib = _lib.load()
    N, D, M = 130, 6, 9
    d = Fz.synthetic_shard(N, D, M, Q, regime='A', seed=3, zseed=4, alpha_value=0.5)
    Yt = 50.0 + d['Y']
    Ys = np.zeros((2, D))
    Ys[1] = 50.0

    def run(where):
        from gparml_amd.engine import ShardEngine
        eng = ShardEngine(N, D, M, Q)
        eng.upload_shard(Yt, d['X_mu'], d['X_S'])
        try:
            first = eng.nearest_rows(Ys)
            check(Yt, d['X_mu'], Ys, None, first, where)
            assert first[1].max() < N and first[0][0] > first[0][1] > 0.0
            eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
            eng.evaluate(False)                                    # Psi1 columns and padded rows now hold what an evaluation leaves
            after = eng.nearest_rows(Ys)
            check(Yt, d['X_mu'], Ys, None, after, where + ', after an evaluation')
            assert all(np.array_equal(a, b) for a, b in zip(first, after))
            for cols in ([0], [D - 1], [1, 4]):
                check(Yt, d['X_mu'], Ys, cols, eng.nearest_rows(Ys, cols=cols), where + ', cols %s' % cols)
        finally:
            eng.close()

    run('plain')
    assert lib.gp_debug_set_option(b'poison_alloc', 1) == 0
    try:
        run('poisoned')
    finally:
        lib.gp_debug_set_option(b'poison_alloc', 0)


def test_ties_go_to_the_lowest_index():
    N, D = 5000, 7
    Yt, Xt, Ys = _case(N, D, 4, seed=1)
    Yt[900] = Yt[7]
    Yt[4100] = Yt[7]                      # another thread, another workgroup slice, another tile -- and another chunk of host rows below
    Yt[3000, [2, 5]] = Yt[1234, [2, 5]]   # two different rows that agree on the columns 2 and 5
    Ys[0] = Yt[7]
    Ys[1, [2, 5]] = Yt[1234, [2, 5]]
    Ys[2] = Yt[4100]
    eng = _engine(Yt, Xt)
    try:
        for Y_train in (None, Yt):
            for rows in (0, 256):
                _set_rows(rows)
                try:
                    d2, idx, _ = eng.nearest_rows(Ys, Y_train=Y_train)
                    assert idx[0] == 7 and d2[0] == 0.0 and idx[2] == 7 and d2[2] == 0.0
                    d2, idx, _ = eng.nearest_rows(Ys, cols=[2, 5], Y_train=Y_train)
                    assert idx[1] == 1234 and d2[1] == 0.0
                    assert np.array_equal(idx, np.argmin(sqdist_cols(Ys, Yt, [2, 5]), axis=1))
                finally:
                    _set_rows(0)
    finally:
        eng.close()


def test_host_rows_equal_resident_rows_and_chunks_do_not_matter():
    N, D, n, _ = SHAPES[0]
    Yt, Xt, Ys = _case(N, D, n)
    eng = _engine(Yt, Xt)
    try:
        res = eng.nearest_rows(Ys)
        host = eng.nearest_rows(Ys, Y_train=Yt)
        check(Yt, Xt, Ys, None, host, 'host rows')
        assert host[2] is None and np.array_equal(res[0], host[0]) and np.array_equal(res[1], host[1])
        again = eng.nearest_rows(Ys)
        assert all(np.array_equal(a, b) for a, b in zip(res, again))
        assert all(np.array_equal(a, b) for a, b in zip(host[:2], eng.nearest_rows(Ys, Y_train=Yt)[:2]))
        for rows in (64, 300, 1000):      # 5 chunks of new rows and 20 of host rows; one and a ragged second; one and 5
            _set_rows(rows)
            try:
                chunked, chunked_host = eng.nearest_rows(Ys), eng.nearest_rows(Ys, Y_train=Yt)
                cols = eng.nearest_rows(Ys, cols=[1, 6], Y_train=Yt)
            finally:
                _set_rows(0)
            assert all(np.array_equal(a, b) for a, b in zip(res, chunked)), rows
            assert np.array_equal(res[0], chunked_host[0]) and np.array_equal(res[1], chunked_host[1]), rows
            assert all(np.array_equal(a, b) for a, b in zip(cols[:2], eng.nearest_rows(Ys, cols=[1, 6])[:2])), rows
    finally:
        eng.close()


def test_the_evaluation_is_untouched():
    """An evaluation, the statistics part again, gp_nearest_rows, then gp_predict / gp_phase2 / gp_finish equal the same sequence without the search."""
    from gparml_amd.engine import ShardEngine
    from oracle import factorised as Fz
    N, D, M, Ql = 3000, 5, 40, 10
    d = Fz.synthetic_shard(N, D, M, Ql, regime='B', seed=4, zseed=5, alpha_value=0.3)
    eng = ShardEngine(N, D, M, Ql)
    eng.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    runs = []
    for with_search in (False, True):
        eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
        first = eng.evaluate(True)
        eng.phase1()
        eng.global_step(sync=True)
        if with_search:
            eng.nearest_rows(d['Y'][:50] + 0.1)                                # resident rows
            eng.nearest_rows(d['Y'][:20], cols=[1, 3], Y_train=d['Y'][100:900])      # host rows
        pred = eng.predict(d['X_mu'][:20])
        eng.phase2(True)
        out = eng.finish()
        runs.append([first['F'], first['grad_Z'], first['grad_X_mu'], out['F'], out['grad_Z'], out['grad_alpha'], out['grad_sf2'], out['grad_beta'],
                     eng.download('GRAD_X_MU'), eng.download('GRAD_X_S'), pred[0], pred[1]])
    eng.close()
    for a, b in zip(*runs):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_shards_and_cut_off():
    from gparml_amd import init
    N, D, n = 2000, 7, 50
    Yt, Xt, Ys = _case(N, D, n, seed=2)
    cut = 777
    Yt[cut + 5] = Yt[40]                  # a duplicate in both shards: the first shard keeps it
    Ys[0] = Yt[40]
    Ys[1] = 100.0                         # farther than 6 from everything
    whole, parts = _engine(Yt, Xt), [_engine(Yt[:cut], Xt[:cut]), _engine(Yt[cut:], Xt[cut:])]
    try:
        X1, dist1, owner1, index1 = init.nearest_start([whole], Ys)
        X2, dist2, owner2, index2 = init.nearest_start(parts, Ys)
        found = owner1 >= 0
        assert found.sum() >= n - 5 and not found[1]
        assert np.array_equal(X1, X2) and np.array_equal(dist1, dist2)
        assert np.array_equal(np.where(owner2 > 0, cut, 0)[found] + index2[found], index1[found]) and np.array_equal(owner2 >= 0, found)
        assert owner2[0] == 0 and index2[0] == 40 and dist2[0] == 0.0
        assert np.all(X2[1] == 0.0) and owner2[1] == -1 and index2[1] == -1 and dist2[1] > 6.0
        assert np.array_equal(index1[found], np.argmin(sqdist_cols(Ys, Yt), axis=1)[found])
        # the same shards as host rows through one engine, and the host's k-d tree path
        from gparml_amd.predict import Predictor
        X3 = init.nearest_start([(whole, Yt[:cut], Xt[:cut]), (whole, Yt[cut:], Xt[cut:])], Ys)
        assert np.array_equal(X3[0], X2) and np.array_equal(X3[2], owner2) and np.array_equal(X3[3], index2)
        assert np.array_equal(X2, Predictor.nearest_training_embeddings(Ys, [(Yt[:cut], Xt[:cut]), (Yt[cut:], Xt[cut:])], Q))
    finally:
        for e in [whole] + parts:
            e.close()


def test_end_to_end_predictor_and_resident_model():
    from gparml_amd.driver import transform_back
    from gparml_amd.predict import Predictor
    from gparml_amd.resident import ResidentModel
    from oracle import factorised as Fz
    z = np.load(os.path.join(GOLDEN_DIR, 'predict_gplvm_2shards.npz'))
    gs = dict(Z=z['global_Z'], sf2=z['global_sf2'], alpha=z['global_alpha'], beta=z['global_beta'])
    acc = {k: z['acc_' + k] for k in ('sum_YYT', 'sum_exp_K_mi_K_im', 'sum_exp_K_miY', 'sum_exp_K_ii', 'sum_KL')}
    training = [(z['train_Y_%d' % i], z['train_X_%d' % i]) for i in range(2)]
    p = Predictor(gs, acc, int(z['N']), int(z['D']))
    for tag, mask in (('A', None), ('C', [int(v) for v in z['C_mask']])):
        Yt = z[tag + '_Y_test']
        S0 = np.full((Yt.shape[0], int(z['Q'])), 0.5)
        host = p.infer(Yt, mask=mask, X_S0=S0, training=training, iterations=20)
        dev = p.infer(Yt, mask=mask, X_S0=S0, training=iter(training), iterations=20, nearest='device')
        assert all(np.array_equal(a, b) for a, b in zip(host, dev)), tag
    # Predictor.test's start: the device search gives the optimiser the reference's first flat vector, as the host search does
    np.random.seed(32)
    best_h = p.test(z['C_Y_test'], iterations=1, training=training, mask=[int(v) for v in z['C_mask']])
    np.random.seed(32)
    best_d = p.test(z['C_Y_test'], iterations=1, training=iter(training), mask=[int(v) for v in z['C_mask']], nearest='device')
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(best_h, best_d))
    # ResidentModel.infer without a start is infer with infer_start's
    N, D, M = 600, 6, 24
    d = Fz.synthetic_shard(N, D, M, Q, regime='A', seed=0, zseed=1, alpha_value=0.5)
    model = ResidentModel([(d['Y'][:250], d['X_mu'][:250], d['X_S'][:250]), (d['Y'][250:], d['X_mu'][250:], d['X_S'][250:])], M, Q, D,
                          fixed_embeddings=True)
    try:
        x = np.concatenate([d['Z'].ravel(), [d['sf2']], d['alpha'], [d['beta']]])
        flat = np.array([transform_back(b, v) for b, v in zip(model.bounds, x)])
        Y = d['Y'][[3, 300, 599, 17]] + 0.01
        Y[3] = 30.0                                                 # no training row within the cut-off: a zero start
        S = np.full((4, Q), 0.5)
        start = model.infer_start(Y)
        assert np.array_equal(start[:3], d['X_mu'][np.argmin(sqdist_cols(Y[:3], d['Y']), axis=1)]) and np.all(start[3] == 0.0)
        a = model.infer(flat, Y, None, S, max_iters=10)
        b = model.infer(flat, Y, start, S, max_iters=10)
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    finally:
        model.close()


def test_errors_leave_the_context_usable():
    from gparml_amd import _lib
    from gparml_amd.engine import ShardEngine
    lib = _lib.load()
    N, D = 50, 4
    Yt, Xt, Ys = _case(N, D, 3)
    eng = ShardEngine(N, D, 4, Q)
    dp, ip, lp = _lib._dp, _lib._ip, ctypes.POINTER(ctypes.c_int64)
    d2, idx, x = np.full(3, 7.0), np.full(3, 7, dtype=np.int64), np.full((3, Q), 7.0)
    cols = np.array([0, 2], dtype=np.int32)

    def call(Y_train, c, nc, want_x, n=3):
        return lib.gp_nearest_rows(eng.h, 0 if Y_train is None else Y_train.shape[0], None if Y_train is None else Y_train.ctypes.data_as(dp), n,
                                   Ys.ctypes.data_as(dp), None if c is None else c.ctypes.data_as(ip), nc, d2.ctypes.data_as(dp), idx.ctypes.data_as(lp),
                                   x.ctypes.data_as(dp) if want_x else None)

    assert call(None, None, 0, True) == _lib.GP_ERR_STATE and b'gp_upload_shard' in lib.gp_last_error(eng.h)     # the resident form before any upload
    assert call(Yt, None, 0, True) == _lib.GP_ERR_BAD_ARG and b'x_near' in lib.gp_last_error(eng.h)               # x_near with host rows
    assert call(Yt, np.array([0, D], dtype=np.int32), 2, False) == _lib.GP_ERR_BAD_ARG and b'cols[1]' in lib.gp_last_error(eng.h)
    assert call(Yt, np.array([-1], dtype=np.int32), 1, False) == _lib.GP_ERR_BAD_ARG
    assert call(Yt, cols, 0, False) == _lib.GP_ERR_BAD_ARG and b'n_cols' in lib.gp_last_error(eng.h)
    assert call(Yt, None, 0, False, n=-1) == _lib.GP_ERR_BAD_ARG
    bad = Yt.copy()
    bad[7, 1] = np.inf
    assert call(bad, None, 0, False) == _lib.GP_ERR_BAD_ARG and b'not finite' in lib.gp_last_error(eng.h)
    assert np.all(d2 == 7.0) and np.all(idx == 7) and np.all(x == 7.0)              # a failed call writes nothing
    assert call(Yt, None, 0, False, n=0) == _lib.GP_OK and np.all(d2 == 7.0)        # n = 0: a no-op
    assert call(Yt[:0], None, 0, False) == _lib.GP_OK                               # no training rows
    assert np.all(np.isinf(d2)) and np.all(d2 > 0) and np.all(idx == -1)
    # the context is usable: host rows now, resident rows after an upload; a NaN in an observed column of Y_test is refused, elsewhere it is not read
    assert call(Yt, cols, 2, False) == _lib.GP_OK
    assert np.array_equal(idx, np.argmin(sqdist_cols(Ys, Yt, [0, 2]), axis=1))
    eng.upload_shard(Yt, Xt, np.zeros(Xt.shape))
    assert call(None, None, 0, True) == _lib.GP_OK
    check(Yt, Xt, Ys, None, (d2, idx, x), 'after the errors')
    Ys[1, 1] = np.nan
    assert call(None, None, 0, True) == _lib.GP_ERR_BAD_ARG and b'Y_test' in lib.gp_last_error(eng.h)
    assert call(None, cols, 2, True) == _lib.GP_OK
    assert lib.gp_nearest_rows(eng.h, 0, None, 3, Ys.ctypes.data_as(dp), cols.ctypes.data_as(ip), 2, None, None, None) == _lib.GP_OK     # every output may be NULL
    with pytest.raises(AssertionError):
        eng.nearest_rows(np.ones((2, D + 1)))
    eng.close()
