"""gp_knn_rows (csrc/knn.hip): the k nearest rows in latent space, through the C ABI, ShardEngine.knn_rows, gparml_amd.init.knn on real engines and
ResidentModel.knn_training.

The oracle is brute force (tests/knn_util.py): numpy d2 in the direct form, then lexsort on (row, d2).  On inputs with small integer coordinates
(|x| <= 8) and weights that are 0, 1 or powers of two every product and sum is exact in float64, so rows and dist2 must equal the oracle bit for
bit -- and such inputs are full of exact ties, so they hold the tie rule.  Every shape runs as it is and under the "knn_rows" test option (more
than one chunk of either side, more than one slice, short tiles).  Real-valued data: dist2 within (Q + 2) 2^-53 d2, relative, of a long-double
evaluation of the same sums, rows equal wherever the long-double distances decide them (knn_util.real_reference)."""
import ctypes

import numpy as np
import pytest

from knn_util import brute, integer_case, real_case, real_reference

pytestmark = pytest.mark.gpu

# (n_train, n, Q, k, what): what = '' | 'skip' | 'zero' (a zero weight) | 'self' (both sides resident, bit 0)
EXACT = [(1, 1, 1, 1, ''), (5, 3, 2, 8, ''), (257, 65, 10, 5, ''), (700, 300, 16, 16, ''), (600, 130, 17, 4, ''), (300, 40, 70, 3, ''),
         (513, 513, 10, 32, 'self'), (257, 65, 10, 5, 'skip'), (257, 65, 10, 5, 'zero'), (90, 20, 3, 32, 'skip')]
IDS = ['%dx%d_Q%d_k%d%s' % (c[0], c[1], c[2], c[3], '_' + c[4] if c[4] else '') for c in EXACT]


def _engine(Q, X_mu=None):
    from gparml_amd.engine import ShardEngine
    N = 1 if X_mu is None else X_mu.shape[0]
    eng = ShardEngine(N, 1, 2, Q)
    if X_mu is not None:
        eng.upload_shard(np.zeros((N, 1)), X_mu, np.zeros(X_mu.shape))
    return eng


def _set_rows(v):
    from gparml_amd import _lib
    assert _lib.load().gp_debug_set_option(b'knn_rows', int(v)) == 0


def _weights(Q, what, seed):
    if what == 'zero':
        w = np.ones(Q)
        w[[0, Q // 2]] = 0.0
        return w
    return None if seed % 2 else np.random.RandomState(seed).choice([0.25, 0.5, 1.0, 2.0, 4.0], size=Q)


@pytest.mark.parametrize('case', EXACT, ids=IDS)
def test_exact_cases_equal_brute_force_bit_for_bit(case):
    n_train, n, Q, k, what = case
    seed = EXACT.index(case)
    T, X = integer_case(n_train, n, Q, seed)
    skip = None
    if what == 'skip':
        skip = np.random.RandomState(seed).randint(-1, n_train, size=n).astype(np.int64)
        skip[0], skip[-1] = n_train - 1, -1
    if what == 'self':
        X, skip = T, np.arange(n_train)
    eng = _engine(Q, T if what == 'self' else None)
    try:
        for weight in ((None, np.full(Q, 2.0)) if what == 'self' else (None, _weights(Q, what, seed))):
            ref = brute(X, T, k, weight, skip)
            outs = []
            for opt in (0, max(2, min(n, n_train) // 2)):
                _set_rows(opt)
                if what == 'self':
                    outs.append(eng.knn_rows(None, k, weight=weight, skip_self=True))
                else:
                    outs.append(eng.knn_rows(X, k, X_train=T, weight=weight, skip=skip))
            _set_rows(0)
            for (d2, rows), where in zip(outs, ('as it is', 'chunked')):
                assert d2.shape == (n, k) and rows.shape == (n, k) and rows.dtype == np.int64
                print('%s, %s, weight %s: %d of %d lists differ' % (IDS[seed], where, weight is not None, int(np.any(rows != ref[1], axis=1).sum()), n))
                assert np.array_equal(rows, ref[1]), where
                assert np.array_equal(d2, ref[0]), where
            if what == '' and k > n_train:
                assert np.all(outs[0][1][:, n_train:] == -1) and np.all(np.isinf(outs[0][0][:, n_train:]))
    finally:
        _set_rows(0)
        eng.close()


def test_real_valued_case_against_long_double():
    T, X, k = real_case()
    d2_ld, bound, rows_ld, decided = real_reference(T, X, k)
    assert np.mean(~decided) <= 0.01
    eng = _engine(X.shape[1])
    try:
        for weight in (None, np.ones(X.shape[1])):               # a weight of one is an exact product: the same bits
            d2, rows = eng.knn_rows(X, k, X_train=T, weight=weight)
            ref = np.take_along_axis(d2_ld, rows, axis=1)
            err = float(np.max(np.abs(d2 - ref) / ref))
            print('real-valued case: dist2 error %.2e of the bound %.2e, %d of %d queries undecided' % (err, bound, int((~decided).sum()), len(X)))
            assert np.all(np.abs(d2 - ref) <= bound * ref)
            assert np.array_equal(rows[decided], rows_ld[decided])
            assert np.all(np.diff(d2, axis=1) >= 0)
    finally:
        eng.close()


def test_a_query_alone_in_a_batch_reversed_host_against_resident_and_twice():
    rs = np.random.RandomState(5)
    Q, k = 10, 7
    T, X = rs.randn(900, Q), rs.randn(70, Q)
    w = np.abs(rs.randn(Q))
    eng = _engine(Q, T)
    try:
        for weight in (None, w):
            base = eng.knn_rows(X, k, weight=weight)                       # host queries, resident training rows
            same = lambda out, sel=slice(None): np.array_equal(out[0], base[0][sel]) and np.array_equal(out[1], base[1][sel])
            assert same(eng.knn_rows(X, k, weight=weight))                 # two calls in a row
            assert same(eng.knn_rows(X[17:18], k, weight=weight), slice(17, 18))
            rev = eng.knn_rows(X[::-1], k, weight=weight)
            assert same((rev[0][::-1], rev[1][::-1]))
            assert same(eng.knn_rows(X, k, X_train=eng.download('X_MU'), weight=weight))        # host rows against the resident rows
            _set_rows(64)
            assert same(eng.knn_rows(X, k, weight=weight))
            _set_rows(0)
            # resident queries: the host copy of the same rows, and bit 0 against a skip list
            own = eng.knn_rows(None, k, weight=weight, skip_self=True)
            host = eng.knn_rows(T, k, X_train=T, weight=weight, skip=np.arange(len(T)))
            assert np.array_equal(own[0], host[0]) and np.array_equal(own[1], host[1])
            assert not np.any(own[1] == np.arange(len(T))[:, None])
    finally:
        _set_rows(0)
        eng.close()


def test_evaluation_after_a_search_is_bit_identical():
    """A full evaluation, gp_knn_rows, then gp_phase2 / gp_finish (and gp_predict) equal the same sequence without the search."""
    from gparml_amd.engine import ShardEngine
    from oracle import factorised as Fz
    N, D, M, Q = 3000, 5, 40, 10
    d = Fz.synthetic_shard(N, D, M, Q, regime='B', seed=4, zseed=5, alpha_value=0.3)
    eng = ShardEngine(N, D, M, Q)
    eng.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    runs = []
    for with_search in (False, True):
        eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
        first = eng.evaluate(True)
        eng.phase1()
        eng.global_step(sync=True)
        if with_search:
            eng.knn_rows(None, 10, weight=d['alpha'], skip_self=True)          # resident rows on both sides
            eng.knn_rows(d['X_mu'][:100] + 0.5, 3, X_train=d['Z'])             # host rows on both sides
        pred = eng.predict(d['X_mu'][:20])
        eng.phase2(True)
        out = eng.finish()
        runs.append([first['F'], first['grad_Z'], out['F'], out['grad_Z'], out['grad_alpha'], out['grad_sf2'], out['grad_beta'],
                     eng.download('GRAD_X_MU'), eng.download('GRAD_X_S'), pred[0], pred[1]])
    eng.close()
    for a, b in zip(*runs):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_error_codes_and_the_empty_sides():
    from gparml_amd import _lib
    lib = _lib.load()
    Q, k = 3, 2
    eng = _engine(Q)
    dp, lp = _lib._dp, ctypes.POINTER(ctypes.c_int64)
    X, T = np.arange(12.0).reshape(4, Q), np.arange(18.0).reshape(6, Q) / 2
    dist2, rows = np.full((6, k), 7.0), np.full((6, k), 7, dtype=np.int64)
    ptr = lambda a, t=dp: None if a is None else a.ctypes.data_as(t)

    def call(n_train, t, n, x, w=None, kk=k, skip=None, flags=0):
        return lib.gp_knn_rows(eng.h, n_train, ptr(t), n, ptr(x), ptr(w), kk, ptr(skip, lp), flags, ptr(dist2), ptr(rows, lp))
    BAD, STATE, UNSUP = _lib.GP_ERR_BAD_ARG, _lib.GP_ERR_STATE, _lib.GP_ERR_UNSUPPORTED
    assert call(6, T, -1, X) == BAD
    assert call(-1, T, 4, X) == BAD
    assert call(6, T, 4, X, kk=0) == BAD
    assert call(6, T, 4, X, kk=33) == UNSUP and b'32' in lib.gp_last_error(eng.h)
    assert call(6, T, 4, X, flags=2) == BAD
    assert call(6, T, 4, X, flags=1) == BAD                                   # bit 0 without both sides resident
    assert call(6, None, 4, X) == STATE and call(6, T, 1, None) == STATE     # a resident side before an upload
    for bad in (np.nan, np.inf):
        b = X.copy(); b[2, 1] = bad
        assert call(6, T, 4, b) == BAD and b'not finite' in lib.gp_last_error(eng.h)
        b = T.copy(); b[5, 2] = bad
        assert call(6, b, 4, X) == BAD
        assert call(6, T, 4, X, w=np.array([1.0, bad, 1.0])) == BAD
    assert call(6, T, 4, X, w=np.array([1.0, -0.5, 1.0])) == BAD
    assert call(6, T, 4, X, skip=np.array([0, 6, -1, 2], dtype=np.int64)) == BAD
    assert call(6, T, 4, X, skip=np.array([0, 5, -2, 2], dtype=np.int64)) == BAD
    eng.upload_shard(np.zeros((1, 1)), np.ones((1, Q)), np.zeros((1, Q)))
    assert call(0, None, 4, None) == BAD                                      # X NULL: n must be N_s
    assert call(0, None, 4, None, flags=1) == BAD
    assert call(0, None, 1, None, skip=np.array([0], dtype=np.int64), flags=1) == BAD
    assert np.all(dist2 == 7.0) and np.all(rows == 7)                         # a failed call writes nothing
    assert call(6, T, 0, X) == _lib.GP_OK and np.all(dist2 == 7.0) and np.all(rows == 7)      # n = 0 writes nothing
    assert call(0, T, 4, X) == _lib.GP_OK                                     # n_train = 0 writes the padding
    assert np.all(np.isinf(dist2[:4])) and np.all(rows[:4] == -1) and np.all(dist2[4:] == 7.0) and np.all(rows[4:] == 7)
    # the one resident row: itself, or nothing when it is left out
    assert call(0, None, 1, None) == _lib.GP_OK and rows[0, 0] == 0 and dist2[0, 0] == 0.0 and rows[0, 1] == -1
    assert call(0, None, 1, None, flags=1) == _lib.GP_OK and np.all(rows[0] == -1) and np.all(np.isinf(dist2[0]))
    # either output may be NULL
    assert lib.gp_knn_rows(eng.h, 6, ptr(T), 4, ptr(X), None, k, None, 0, None, ptr(rows, lp)) == _lib.GP_OK
    assert np.array_equal(rows[:4], brute(X, T, k)[1])
    with pytest.raises(AssertionError):
        eng.knn_rows(np.ones((2, Q + 1)), 1, X_train=T)
    eng.close()


def test_init_knn_on_engines_and_resident_model_leave_one_out():
    """Two shards of three well-separated labelled blobs: init.knn over the engines equals brute force over all rows, the leave-one-out error is 0,
    and with one label flipped it is the count by hand: the flipped row itself, and nobody else (k = 5: four right votes outnumber one wrong)."""
    from gparml_amd import init
    from gparml_amd.resident import ResidentModel
    rs = np.random.RandomState(2)
    Q, D, M, per = 3, 4, 6, 40
    centres = np.array([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [0.0, 10.0, 0.0]])
    labels = np.repeat(np.arange(3), per)
    X = centres[labels] + 0.3 * rs.randn(3 * per, Q)
    order = rs.permutation(3 * per)
    X, labels = X[order], labels[order]
    cut = 47
    shards = [(rs.randn(len(x), D), x, np.zeros(x.shape)) for x in (X[:cut], X[cut:])]
    model = ResidentModel(shards, M, Q, D, fixed_embeddings=True)
    try:
        k = 5
        ref = brute(X, X, k, skip=np.arange(len(X)))
        d2, shard, row = init.knn(model.engines, None, k, skip_self=True)
        assert np.array_equal(np.where(shard == 1, cut + row, row), ref[1])
        assert np.all(np.abs(d2 - ref[0]) <= 2 * (Q + 2) * 2.0 ** -53 * ref[0])      # both sides within the direct form's bound of the exact sum
        out = model.knn_training(k, weight=None)
        assert all(np.array_equal(a, b) for a, b in zip(out, (d2, shard, row)))
        assert model.knn_training(k, labels=labels, weight=None) == 0.0
        assert model.knn_training(k, labels=[labels[:cut], labels[cut:]], weight=np.array([1.0, 1.0, 0.0])) == 0.0
        flipped = labels.copy()
        flipped[60] = (flipped[60] + 1) % 3
        assert model.knn_training(k, labels=flipped, weight=None) == 1.0 / len(X)
        # the ARD metric of a parameter vector
        flat = np.concatenate([np.zeros(M * Q), [0.0], [0.3, -1.0, 2.0], [0.0]])
        from gparml_amd.driver import split_flat, transform_vec
        alpha = split_flat(transform_vec(model._pos, flat), M, Q)[2]
        got = model.knn_training(k, weight='alpha', flat_array=flat)
        want = init.knn(model.engines, None, k, weight=alpha, skip_self=True)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    finally:
        model.close()
