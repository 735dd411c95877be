"""gparml_amd.init.knn / knn_merge / knn_vote without a device: the merge of the shards' neighbour lists by (distance, shard, row) on fake parts
whose ``knn_rows`` is numpy brute force (tests/knn_util.py), against the brute force over the concatenation; the vote's tie rule on hand-made
lists; and the seed of the real-valued device case (tests/test_gpu_knn.py): its gap rule leaves out at most 1 % of the queries."""
import numpy as np
import pytest

from knn_util import brute, integer_case, real_case, real_reference, sqdist


class FakePart(object):
    """A shard of training rows with ShardEngine's knn_rows / knn_queries, in numpy"""

    def __init__(self, T):
        self.T = np.asarray(T, dtype=np.float64)

    def knn_rows(self, X=None, k=1, weight=None, skip_self=False):
        assert X is None or not skip_self
        skip = np.arange(len(self.T)) if skip_self else None
        return brute(self.T if X is None else X, self.T, k, weight, skip)

    def knn_queries(self):
        return self.T


def split(T, cuts):
    return [FakePart(t) for t in np.split(T, cuts)]


def global_rows(shard, row, cuts):
    start = np.concatenate([[0], cuts]).astype(np.int64)
    return np.where(row >= 0, start[np.maximum(shard, 0)] + row, -1)


CUTS = [[], [13], [5, 31]]          # 1, 2 and 3 uneven shards of 40 rows


@pytest.mark.parametrize('cuts', CUTS, ids=['1shard', '2shards', '3shards'])
@pytest.mark.parametrize('k', [1, 4, 9])
def test_merged_lists_equal_brute_force_over_the_concatenation(cuts, k):
    """integer coordinates in two dimensions: equal distances within and across shards at every query.  The order (d2, shard, row) of the merge
    is the order (d2, global row) of the concatenation, so the lists are equal slot by slot."""
    from gparml_amd import init
    T, X = integer_case(40, 17, 2, seed=3)
    w = np.array([1.0, 0.5])
    for weight in (None, w):
        ref_d, ref_r = brute(X, T, k, weight)
        full = np.sort(sqdist(X, T, weight), axis=1)
        assert np.any(full[:, k - 1] == full[:, k]), 'no query has a tie where its list ends'
        d2, shard, row = init.knn(split(T, cuts), X, k, weight=weight)
        assert d2.shape == (17, k) and shard.dtype == np.int64 and row.dtype == np.int64
        assert np.array_equal(d2, ref_d) and np.array_equal(global_rows(shard, row, cuts), ref_r)


@pytest.mark.parametrize('cuts', CUTS, ids=['1shard', '2shards', '3shards'])
def test_own_rows_as_queries_leave_themselves_out_only_in_their_own_shard(cuts):
    """X None: every shard's rows are the queries, in shard order.  Duplicated rows across shards: the copy in ANOTHER shard is a neighbour at
    distance zero, the row itself is not."""
    from gparml_amd import init
    T, _ = integer_case(40, 1, 2, seed=5)
    T[35] = T[2]                    # the same point in the first and in the last shard
    k = 6
    ref_d, ref_r = brute(T, T, k, skip=np.arange(40))
    d2, shard, row = init.knn(split(T, cuts), None, k, skip_self=True)
    g = global_rows(shard, row, cuts)
    assert np.array_equal(d2, ref_d) and np.array_equal(g, ref_r)
    assert not np.any(g == np.arange(40)[:, None])
    assert d2[2, 0] == 0.0 and 35 in g[2, d2[2] == 0.0] and 2 in g[35, d2[35] == 0.0]
    # without skip_self every row finds itself first (distance zero, and of equal rows the lowest)
    d2, shard, row = init.knn(split(T, cuts), None, k)
    assert np.all(d2[:, 0] == 0.0) and global_rows(shard, row, cuts)[35, 0] == 2


def test_short_lists_are_padded():
    from gparml_amd import init
    T, X = integer_case(5, 3, 2, seed=1)
    d2, shard, row = init.knn(split(T, [2]), X, 8)
    ref_d, ref_r = brute(X, T, 8)
    assert np.array_equal(d2, ref_d) and np.array_equal(global_rows(shard, row, [2]), ref_r)
    assert np.all(np.isinf(d2[:, 5:])) and np.all(shard[:, 5:] == -1) and np.all(row[:, 5:] == -1)
    # a shard without rows, and a merge that asks for more than the lists hold
    d2, shard, row = init.knn_merge([(np.zeros((3, 0)), np.zeros((3, 0), dtype=np.int64)), brute(X, T, 2)], 4)
    assert np.array_equal(d2[:, :2], ref_d[:, :2]) and np.all(shard[:, :2] == 1) and np.all(row[:, 2:] == -1) and np.all(np.isinf(d2[:, 2:]))


class FakeEngine(object):
    """ShardEngine's constructor, knn_rows and close, in numpy (Predictor's engine_class hook)"""

    def __init__(self, N, D, M, Q, device=0):
        self.Q = Q

    def knn_rows(self, X=None, k=1, X_train=None, weight=None, skip=None, skip_self=False):
        assert X is not None and X_train is not None and not skip_self, 'no resident rows here'
        return brute(X, X_train, k, weight, skip)

    def close(self):
        pass


def test_predictor_knn_searches_the_training_embeddings_in_the_ard_metric():
    from gparml_amd.predict import Predictor
    T, X = integer_case(40, 9, 2, seed=7)
    alpha = np.array([2.0, 0.25])
    pred = Predictor(dict(Z=np.zeros((3, 2)), sf2=1.0, alpha=alpha[None, :], beta=1.0), {}, 40, 4, engine_class=FakeEngine)
    training = [(None, T[:13]), (None, T[13:])]
    for weight, w in (('alpha', alpha), (None, None)):
        d2, shard, row = pred.knn(X, 5, training, weight=weight)
        ref_d, ref_r = brute(X, T, 5, w)
        assert np.array_equal(d2, ref_d) and np.array_equal(global_rows(shard, row, [13]), ref_r)


def test_vote_majority_and_ties():
    from gparml_amd import init
    L = np.array([[2, 1, 1, 2, 3],       # 2 and 1 tie at two votes: 2's nearest member comes first
                  [1, 2, 2, 1, 3],       # the same tie the other way round
                  [3, 1, 1, 2, 2],       # 1 and 2 tie, 3 is nearest but has one vote: 1
                  [4, 4, 5, 5, 5],       # a clear majority that is not nearest
                  [7, 8, 9, 6, 5]])      # all different: the nearest
    assert list(init.knn_vote(L)) == [2, 1, 1, 5, 7]
    # empty slots (a non-finite distance) do not vote
    d2 = np.array([[0.0, 1.0, np.inf, np.inf, np.inf],
                   [0.0, 1.0, 2.0, np.inf, np.inf],
                   [np.inf] * 5])
    L = np.array([[1, 2, 2, 2, 2], [3, 4, 4, 3, 3], [1, 1, 1, 1, 1]])
    assert list(init.knn_vote(L, d2)) == [1, 4, -1]
    assert list(init.knn_vote(np.array([[6], [5]]))) == [6, 5]


def test_the_real_valued_case_is_decided_by_its_long_double_distances():
    """The seed of the device test's real-valued case: the gap rule (the k + 1 nearest long-double distances pairwise further apart than twice the
    direct form's rounding bound) leaves out at most 1 % of the queries, and float64 brute force agrees with the long-double rows on the others."""
    T, X, k = real_case()
    d2, bound, rows, decided = real_reference(T, X, k)
    assert np.mean(~decided) <= 0.01, np.mean(~decided)
    bd, br = brute(X, T, k)
    assert np.array_equal(br[decided], rows[decided])
    ref = np.take_along_axis(d2, br, axis=1)
    assert np.all(np.abs(bd - ref) <= bound * ref)
