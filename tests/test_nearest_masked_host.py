"""The masked nearest start without a device: gparml_amd.init.nearest_start(observed=) over a numpy stand-in for
ShardEngine.nearest_rows(observed=), and what Predictor.infer(ragged=True) does with it.  The reference for a masked start is the per-row loop of
nearest_start(cols=...): a row with its own column list, one call per row, the rules unchanged."""
import itertools

import numpy as np

from gparml_amd import init
from nearest_masked_util import CountingPredictorEngine, NumpyMaskedNearestEngine, masked_sqdist, random_masks, stub_predictor
from nearest_util import FakeRanks

Q = 2


def _problem(seed=0, N=150, D=6, n=24):
    """Integer-valued rows: every distance is exact, ties are ties, and sqrt(36) = 6 exactly."""
    rs = np.random.RandomState(seed)
    Yt = rs.randint(-3, 4, size=(N, D)).astype(float)
    Xt = rs.randn(N, Q)
    Ys = rs.randint(-3, 4, size=(n, D)).astype(float)
    obs = random_masks(rs, n, D)
    shards = [(Yt[:50], Xt[:50]), (Yt[50:100], Xt[50:100]), (Yt[100:], Xt[100:])]
    return Yt, Xt, Ys, obs, shards


def _per_row(shards, Ys, obs, **kw):
    """nearest_start(cols=the row's columns) row by row: the four arrays stacked."""
    out = [init.nearest_start([NumpyMaskedNearestEngine(y, x) for y, x in shards], Ys[i:i + 1], cols=list(np.flatnonzero(obs[i])), **kw) for i in range(len(Ys))]
    return [np.concatenate([o[k] for o in out]) for k in range(4)]


def test_masked_start_equals_the_per_row_loop_over_parts_and_ranks():
    Yt, Xt, Ys, obs, shards = _problem()
    # a duplicate of a first-shard row in the third shard, at distance zero from a new row: the later part needs to be strictly nearer
    shards[2][0][7] = shards[0][0][11]
    Ys[5] = shards[0][0][11]
    obs[5] = True
    # a row at exactly the cut-off over its own columns: row 6 observes columns 0 and 1 only and lies at (10, 0); the training values are in
    # [-3, 3], so every row is at 7 or more from it, but for one at (4, 0): exactly 6
    obs[6] = False
    obs[6, :2] = True
    Ys[6, :2] = [10.0, 0.0]
    shards[1][0][3, :2] = [4.0, 0.0]
    Yn = np.where(obs, Ys, np.nan)
    want = _per_row(shards, Ys, obs)
    got = init.nearest_start([NumpyMaskedNearestEngine(y, x) for y, x in shards], Yn, observed=obs)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert got[2][5] == 0 and got[3][5] == 11 and got[1][5] == 0.0                 # the first shard keeps the tie
    assert got[1][6] == 6.0 and got[2][6] == -1 and np.all(got[0][6] == 0.0)       # strict cut-off: exactly 6 keeps a zero mean
    assert (got[2] >= 0).sum() >= len(Ys) // 2
    loose = init.nearest_start([NumpyMaskedNearestEngine(y, x) for y, x in shards], Yn, observed=obs, cutoff=np.nextafter(6.0, 7.0))
    assert loose[2][6] == 1 and loose[3][6] == 3
    # host rows through one engine, as Predictor passes its shards
    eng = NumpyMaskedNearestEngine()
    host = init.nearest_start(((eng, y, x) for y, x in shards), Yn, observed=obs)
    assert all(np.array_equal(a, b) for a, b in zip(host, want))
    # two emulated ranks: the first shard on rank 0, the others on rank 1
    ranks = FakeRanks(2)
    res = ranks.run(lambda r, red: init.nearest_start([NumpyMaskedNearestEngine(y, x) for y, x in (shards[:1] if r == 0 else shards[1:])], Yn,
                                                      observed=obs, allreduce=red, rank=r, world=2))
    for r in range(2):
        assert all(np.array_equal(a, b) for a, b in zip(res[r], want)), r
    # cols and observed are alternatives
    try:
        init.nearest_start([NumpyMaskedNearestEngine(Yt, Xt)], Yn, cols=[0], observed=obs)
    except AssertionError as e:
        assert 'alternatives' in str(e)
    else:
        raise AssertionError('cols together with observed must be refused')


def _ragged_problem():
    """D = 9, every pair of columns hidden once: 36 rows, 36 patterns; three shards of integer-valued rows."""
    rs = np.random.RandomState(3)
    D, M = 9, 5
    pairs = list(itertools.combinations(range(D), 2))
    Yt = rs.randint(-2, 3, size=(90, D)).astype(float)
    Xt = rs.randn(90, Q)
    Y = Yt[rs.randint(90, size=len(pairs))] + rs.randint(-1, 2, size=(len(pairs), D))
    Y[4] += 50.0                                                                    # beyond the cut-off: a zero start
    for i, pr in enumerate(pairs):
        Y[i, list(pr)] = np.nan
    training = [(Yt[:30], Xt[:30]), (Yt[30:60], Xt[30:60]), (Yt[60:], Xt[60:])]
    return D, rs.randn(M, Q), Y, training


def test_ragged_device_start_is_one_search_per_shard():
    D, Z, Y, training = _ragged_problem()
    assert len({r.tobytes() for r in np.isnan(Y)}) == 36

    class Eng(CountingPredictorEngine):
        pass
    Eng.searches, Eng.rows_calls = 0, []
    pred = stub_predictor(Z, D, Eng)
    res = pred.infer(Y, training=iter(training), X_S0=np.full((36, Q), 0.5), iterations=1, ragged=True, nearest='device')
    assert Eng.searches == len(training)                                             # not patterns x shards
    (call,) = Eng.rows_calls
    assert np.array_equal(call['observed'], ~np.isnan(Y))
    want = init.nearest_start([NumpyMaskedNearestEngine(y, x) for y, x in training], Y, observed=~np.isnan(Y))[0]
    assert np.array_equal(call['X_mu'], want) and np.array_equal(res[0], want)
    assert np.all(want[4] == 0.0) and np.abs(want).sum(axis=1).astype(bool).sum() >= 30
    # the k-d tree path per pattern picks the same rows on this exact data
    from gparml_amd.predict import Predictor
    for i in (0, 4, 17, 35):
        c = np.flatnonzero(~np.isnan(Y[i]))
        assert np.array_equal(want[i:i + 1], Predictor.nearest_training_embeddings(Y[i:i + 1], training, Q, c))


def test_ragged_host_start_is_unchanged():
    """nearest='host' (the default) with ragged=True: per pattern in order of first occurrence, the k-d trees over that pattern's columns -- the
    parent's loop restated -- and no search on the engine."""
    D, Z, Y, training = _ragged_problem()
    Y = np.concatenate([Y, Y[:6] + 1.0])                                            # six patterns with two rows each

    class Eng(CountingPredictorEngine):
        pass
    Eng.searches, Eng.rows_calls = 0, []
    pred = stub_predictor(Z, D, Eng)
    n = Y.shape[0]
    pred.infer(Y, training=training, X_S0=np.full((n, Q), 0.5), iterations=1, ragged=True)
    assert Eng.searches == 0
    from gparml_amd.predict import Predictor
    observed = ~np.isnan(Y)
    groups = {}
    for i in range(n):
        groups.setdefault(observed[i].tobytes(), []).append(i)
    want = np.empty((n, Q))
    for key in sorted(groups, key=lambda k: groups[k][0]):
        rows = np.asarray(groups[key])
        want[rows] = Predictor.nearest_training_embeddings(Y[rows], training, Q, np.flatnonzero(observed[rows[0]]))
    assert np.array_equal(Eng.rows_calls[0]['X_mu'], want)


def test_inducing_start_on_the_device_path_makes_inducing_starts_choice():
    D, Z, Y, _ = _ragged_problem()
    rs = np.random.RandomState(5)
    Mz = rs.randint(-2, 3, size=(Z.shape[0], D)).astype(float)
    Mz[3] = Mz[1]                                                                   # two inducing points predict the same outputs: the lower wins

    class Eng(CountingPredictorEngine):
        pass
    Eng.searches, Eng.rows_calls, Eng.Mz = 0, [], Mz
    pred = stub_predictor(Z, D, Eng)
    S0 = np.full((36, Q), 0.5)
    pred.infer(Y, start='inducing', X_S0=S0, iterations=1, ragged=True, nearest='device')
    assert Eng.searches == 1
    pred.infer(Y, start='inducing', X_S0=S0, iterations=1, ragged=True)
    assert Eng.searches == 1                                                        # the default stays host arithmetic
    from gparml_amd.predict import Predictor
    want = Predictor.inducing_start(Y, ~np.isnan(Y), Z, Mz)
    assert np.array_equal(Eng.rows_calls[0]['X_mu'], want) and np.array_equal(Eng.rows_calls[1]['X_mu'], want)
    assert np.array_equal(want, Z[np.argmin(masked_sqdist(Y, Mz, ~np.isnan(Y)), axis=1)])
