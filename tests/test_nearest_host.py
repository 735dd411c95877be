"""gparml_amd.init.nearest_start (the host rules around ShardEngine.nearest_rows) with a numpy stand-in for the device search: the strictly-nearer
rule across parts, the strict cut-off, and the combination over ranks.  The reference is Predictor.nearest_training_embeddings, the k-d tree path
that restates predict.py:44-66 and reproduces the reference's recorded starting means exactly.  No GPU."""
import numpy as np

from nearest_util import FakeRanks, NumpyNearestEngine, sqdist_cols


def _host(Y_test, shards, Q, cols=None):
    from gparml_amd.predict import Predictor
    return Predictor.nearest_training_embeddings(Y_test, shards, Q, cols)


def _data(seed=0, N=400, D=5, Q=3, n=60, scale=4.0):
    rs = np.random.RandomState(seed)
    return scale * rs.randn(N, D), rs.randn(N, Q), scale * rs.randn(n, D)


def test_resident_parts_and_host_parts_equal_the_kd_tree_path():
    """Random data with rows on both sides of the cut-off: the means are the k-d tree path's bit for bit, owner and index name the global row."""
    from gparml_amd import init
    Yt, Xt, Ys = _data()
    cuts = [0, 130, 131, 400]
    shards = [(Yt[a:b], Xt[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    for cols in (None, [0, 3], [4]):
        ref = _host(Ys, shards, 3, cols)
        X, dist, owner, index = init.nearest_start([NumpyNearestEngine(y, x) for y, x in shards], Ys, cols=cols)
        assert np.array_equal(X, ref)
        far = ~(dist < 6.0)
        assert far.any() or cols is not None
        assert np.all(owner[far] == -1) and np.all(index[far] == -1) and np.all(X[far] == 0.0)
        g = np.asarray(cuts)[owner[~far]] + index[~far]
        d2 = sqdist_cols(Ys, Yt, cols)
        assert np.array_equal(g, np.argmin(d2, axis=1)[~far]) and np.array_equal(dist, np.sqrt(d2.min(axis=1)))
        eng = NumpyNearestEngine()
        Xh = init.nearest_start(((eng, y, x) for y, x in shards), Ys, cols=cols)            # a generator: one shard at a time
        assert np.array_equal(Xh[0], ref) and np.array_equal(Xh[2], owner) and np.array_equal(Xh[3], index)
    assert (~(init.nearest_start([NumpyNearestEngine(Yt, Xt)], Ys)[1] < 6.0)).any()      # the all-column case has rows beyond the cut-off


def test_a_later_part_wins_only_when_strictly_nearer():
    from gparml_amd import init
    Yt, Xt, Ys = _data(1, N=50, n=4, scale=1.0)
    Ys[0] = Yt[7]                                           # row 7 sits in both parts: the first one keeps it
    Ys[1] = Yt[3] + 0.5
    first, second = NumpyNearestEngine(Yt[:20], Xt[:20]), NumpyNearestEngine(np.vstack([Yt[7:8], Yt[20:]]), np.vstack([Xt[7:8] + 9.0, Xt[20:]]))
    X, dist, owner, index = init.nearest_start([first, second], Ys)
    assert owner[0] == 0 and index[0] == 7 and dist[0] == 0.0 and np.array_equal(X[0], Xt[7])
    X2, _, owner2, index2 = init.nearest_start([second, first], Ys)
    assert owner2[0] == 0 and index2[0] == 0 and np.array_equal(X2[0], Xt[7] + 9.0)
    # a strictly nearer row of the later part does win
    near = NumpyNearestEngine(Ys[1:2] + 1e-9, np.full((1, 3), 5.0))
    X3, _, owner3, index3 = init.nearest_start([first, near], Ys)
    assert owner3[1] == 1 and index3[1] == 0 and np.array_equal(X3[1], np.full(3, 5.0))
    assert np.array_equal(X3[[0, 2, 3]], init.nearest_start([first], Ys)[0][[0, 2, 3]])
    for parts in ([first, second], [second, first], [first, near]):
        shards = [(p.Y, p.X_mu) for p in parts]
        assert np.array_equal(init.nearest_start(parts, Ys)[0], _host(Ys, shards, 3))


def test_the_cut_off_is_strict():
    """A row at exactly 6.0 keeps a zero mean, one at nextafter(6, 0) takes the embedding: cKDTree's distance_upper_bound, checked against it."""
    from gparml_amd import init
    Yt, Xt = np.zeros((1, 2)), np.array([[1.5, -2.5]])
    below = np.nextafter(6.0, 0.0)
    Ys = np.array([[6.0, 0.0], [below, 0.0], [0.0, -6.0], [0.0, -below], [3.0, 4.0]])
    X, dist, owner, index = init.nearest_start([NumpyNearestEngine(Yt, Xt)], Ys)
    assert np.array_equal(dist, [6.0, below, 6.0, below, 5.0])
    assert np.array_equal(X, [[0, 0], [1.5, -2.5], [0, 0], [1.5, -2.5], [1.5, -2.5]])
    assert np.array_equal(owner, [-1, 0, -1, 0, 0]) and np.array_equal(index, [-1, 0, -1, 0, 0])
    assert np.array_equal(X, _host(Ys, [(Yt, Xt)], 2))
    assert np.array_equal(init.nearest_start([NumpyNearestEngine(Yt, Xt)], Ys, cutoff=5.0)[2], [-1, -1, -1, -1, -1])
    # no training rows at all: zero means
    X0, d0, o0, i0 = init.nearest_start([(NumpyNearestEngine(), np.zeros((0, 2)), np.zeros((0, 2)))], Ys)
    assert np.all(X0 == 0.0) and X0.shape == (5, 2) and np.all(np.isinf(d0)) and np.all(o0 == -1) and np.all(i0 == -1)


def test_two_emulated_ranks_equal_one_process():
    from gparml_amd import init
    Yt, Xt, Ys = _data(2, N=300, n=40)
    Xt[11, 1] = -0.0                                        # a negative zero survives the sum over ranks
    Ys[5] = Yt[11]
    cuts = [0, 90, 200, 201, 300]
    shards = [(Yt[a:b], Xt[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    for cols in (None, [1, 4]):
        one = init.nearest_start([NumpyNearestEngine(y, x) for y, x in shards], Ys, cols=cols)
        for split in (1, 3, 4):                             # rank 0 holds the first `split` parts; 4: rank 1 holds none
            ranks = FakeRanks(2)
            res = ranks.run(lambda r, red: init.nearest_start([NumpyNearestEngine(y, x) for y, x in (shards[:split] if r == 0 else shards[split:])],
                                                              Ys, cols=cols, allreduce=red, rank=r, world=2))
            assert ranks.calls == 2                         # the distances, then the winners' rows
            for got in res:
                for a, b in zip(got, one):
                    assert np.array_equal(a, b) and a.dtype == b.dtype
                assert np.array_equal(got[0].view(np.int64), one[0].view(np.int64))          # bit for bit, the sign of the zero included


def test_the_lowest_rank_wins_ties():
    from gparml_amd import init
    Yt, Xt, Ys = _data(3, N=40, n=6, scale=1.0)
    Ys[2] = Yt[9]
    mine = lambda r: [NumpyNearestEngine(Yt, Xt + 100.0 * r)]          # every rank holds the same rows, with means that tell the ranks apart
    ranks = FakeRanks(3)
    res = ranks.run(lambda r, red: init.nearest_start(mine(r), Ys, allreduce=red, rank=r, world=3))
    one = init.nearest_start(mine(0), Ys)
    for got in res:
        assert np.array_equal(got[0], one[0]) and np.all(got[2] == 0) and np.array_equal(got[3], one[3])
    assert res[0][3][2] == 9 and res[0][1][2] == 0.0
    # strictly nearer on a higher rank wins
    extra = NumpyNearestEngine(Ys[4:5] + 1e-9, np.full((1, 3), 7.0))
    ranks = FakeRanks(3)
    res = ranks.run(lambda r, red: init.nearest_start(mine(r) + ([extra] if r == 2 else []), Ys, allreduce=red, rank=r, world=3))
    for got in res:
        assert got[2][4] == 3 and got[3][4] == 0 and np.array_equal(got[0][4], np.full(3, 7.0))          # parts 0, 1, 2 are the ranks' copies
        assert np.array_equal(np.delete(got[0], 4, axis=0), np.delete(one[0], 4, axis=0))
