"""gparml_amd.init.kmeans (the host loop around ShardEngine.kmeans_accumulate) against scipy.cluster.vq.kmeans, with a numpy stand-in for the device
pass: the loop is scipy's _kmeans restated on per-part sums, counts and summed distances, so given the same seeds it must return scipy's centres
and mean distance (parallel_GPLVM.py:179-186 is ``cl.kmeans(embeddings, M)``).  No GPU.

Bounds: 1e-10 on centres and mean distance (scipy's distances come from the expanded form |x|^2 - 2 x.z + |z|^2 for Q >= 5 and its sums run in
another order: ~1e-15 relative; measured here 0 on the centres and <= 4e-15 on the distance).  That only holds while no label can flip under
rounding, so every pass's smallest relative gap between the best and the second-best squared distance is recomputed and must exceed 1e-9
(measured 4.3e-6 / 3.7e-6 / 1.9e-4 over the three trajectories)."""
import os

import numpy as np
import pytest
import scipy.cluster.vq as cl

from kmeans_util import BLOBS, NumpyEngine, blob_case

TOL = 1e-10


def _parts(X, cuts=None):
    from gparml_amd import init
    cuts = [0, X.shape[0]] if cuts is None else cuts
    return [init.HostRows(NumpyEngine(1, 1, 1, X.shape[1]), X[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]


@pytest.fixture(autouse=True)
def _fresh_stand_in():
    NumpyEngine.gaps, NumpyEngine.made = [], []
    yield
    NumpyEngine.gaps = None


@pytest.mark.parametrize('case', BLOBS, ids=['N20000_Q10_K64', 'N5000_Q3_K33', 'N3000_Q2_K16'])
def test_same_seeds_give_what_scipy_returns(case):
    from gparml_amd import init
    N, Q, K, B, seed = case
    X, seeds = blob_case(*case)
    ref_c, ref_d = cl.kmeans(X, seeds, thresh=1e-5)
    c, d, passes = init.kmeans(_parts(X), K, seeds=seeds, thresh=1e-5)
    gap = min(NumpyEngine.gaps)
    print('centres %s (scipy %s), max |diff| %.3e, mean distance diff %.3e, %d passes, smallest relative gap %.3e'
          % (c.shape, ref_c.shape, np.max(np.abs(c - ref_c)) if c.shape == ref_c.shape else np.nan, abs(d - ref_d), passes, gap))
    assert gap > 1e-9, 'a label of this data set could flip under rounding: %.3e' % gap
    assert c.shape == ref_c.shape
    if seed == 0:
        assert c.shape[0] == K - 1                   # the case that loses one empty cluster
    assert np.max(np.abs(c - ref_c)) <= TOL
    assert abs(d - ref_d) <= TOL
    # rows split over three ragged parts: the same answer
    c3, d3, p3 = init.kmeans(_parts(X, [0, N // 7, N // 2 + 3, N]), K, seeds=seeds, thresh=1e-5)
    assert p3 == passes and c3.shape == c.shape
    assert np.max(np.abs(c3 - c)) <= TOL and abs(d3 - d) <= TOL


def test_max_iters_stops_the_loop():
    from gparml_amd import init
    X, seeds = blob_case(*BLOBS[2])
    c, d, passes = init.kmeans(_parts(X), 16, seeds=seeds, max_iters=3)
    assert passes == 3


def test_seed_draw_and_restarts_with_a_fixed_generator():
    """seeds None: K distinct rows over all parts (global row order) from ``rng``, once per restart; the run with the lowest mean distance wins."""
    from gparml_amd import init
    N, Q, K, B, seed = BLOBS[1]
    X, _ = blob_case(*BLOBS[1])
    runs = []
    rs = np.random.RandomState(5)
    for _ in range(3):
        idx = rs.choice(N, K, replace=False)
        assert len(set(idx.tolist())) == K
        runs.append(cl.kmeans(X, X[idx], thresh=1e-5))
    assert len({round(r[1], 12) for r in runs}) > 1, 'the restarts of this test must differ for the choice to mean anything'
    ref_c, ref_d = min(runs, key=lambda r: r[1])
    for cuts in (None, [0, 1234, 1300, N]):
        c, d, _ = init.kmeans(_parts(X, cuts), K, restarts=3, rng=np.random.RandomState(5))
        assert c.shape == ref_c.shape and np.max(np.abs(c - ref_c)) <= TOL and abs(d - ref_d) <= TOL
    # the default generator is numpy's global stream
    np.random.seed(5)
    c, d, _ = init.kmeans(_parts(X), K, restarts=3)
    assert np.max(np.abs(c - ref_c)) <= TOL and abs(d - ref_d) <= TOL
    assert min(NumpyEngine.gaps) > 1e-9


def _write_shards(tmp_path, shards):
    dirs = {k: str(tmp_path / k) for k in ('input', 'embeddings', 'statistics')}
    for d in dirs.values():
        os.makedirs(d)
    for i, X in enumerate(shards):
        open(os.path.join(dirs['input'], 'shard_%d' % i), 'w').write('0\n')
        np.save(os.path.join(dirs['embeddings'], 'shard_%d.embedding.npy' % i), X)
    return dirs


def test_init_statistics_without_the_option_is_the_parent_path_bit_for_bit(tmp_path):
    from gparml_amd import driver, gpu_MapReduce as mr
    rs = np.random.RandomState(11)
    shards = [rs.randn(30, 3), rs.randn(50, 3), rs.randn(40, 3)]
    M, Q = 40, 3
    opts = dict(_write_shards(tmp_path, shards), M=M, Q=Q, load=False)
    np.random.seed(7)
    _, gs = driver.init_statistics(mr, dict(opts))
    # the parent's lines, restated: the first shards that reach M rows, scipy's k-means from the global stream, top-up, noise
    np.random.seed(7)
    emb = np.concatenate(shards[:2])
    Z = cl.kmeans(emb, M)[0]
    if M - Z.shape[0] > 0:
        Z = np.concatenate((Z, emb[:M - Z.shape[0]]))
    Z = Z + np.random.randn(M, Q) * 0.05
    assert gs['Z'].shape == (M, Q) and np.array_equal(gs['Z'], Z)
    assert not NumpyEngine.made                       # no engine was asked for


def test_init_statistics_device_option_clusters_all_shards_and_tops_up(tmp_path):
    """init_Z='device': init.kmeans over the embeddings of every shard, one engine per device; 12 distinct points for M = 16 centres, so duplicate
    seeds tie, the higher index gets no members and is dropped: the reference's top-up with the first embeddings fills Z, then its noise."""
    from gparml_amd import driver, gpu_MapReduce as mr
    rs = np.random.RandomState(12)
    pts = 3.0 * rs.randn(12, 2)
    shards = [pts[rs.randint(12, size=n)] for n in (20, 25, 30)]
    M, Q = 16, 2
    opts = dict(_write_shards(tmp_path, shards), M=M, Q=Q, load=False, init_Z='device', devices=[0, 1])
    np.random.seed(9)
    _, gs = driver.init_statistics(mr, dict(opts), engine_class=NumpyEngine)
    assert len(NumpyEngine.made) == 2 and [e.device for e in NumpyEngine.made] == [0, 1] and all(e.closed for e in NumpyEngine.made)
    np.random.seed(9)
    X = np.concatenate(shards)
    Zk = cl.kmeans(X, X[np.random.choice(X.shape[0], M, replace=False)], thresh=1e-5)[0]
    missing = M - Zk.shape[0]
    assert missing > 0                                # the top-up is exercised
    Z = np.concatenate((Zk, shards[0][:missing])) + np.random.randn(M, Q) * 0.05
    assert gs['Z'].shape == (M, Q) and np.max(np.abs(gs['Z'] - Z)) <= TOL


def _rank_worker(rank, world, port, q):
    """One rank of a gloo group holding two ragged parts of blob case 2; rank 1's generator is out of step on purpose (rank 0's draw is used)."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, 'tests'))
    import torch.distributed as dist
    from gparml_amd import init
    from kmeans_util import BLOBS, NumpyEngine, blob_case
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    N, Q, K, B, seed = BLOBS[1]
    X, seeds = blob_case(*BLOBS[1])
    cuts = [[0, 700, 2100], [2100, 2101, N]][rank]
    parts = [init.HostRows(NumpyEngine(1, 1, 1, Q), X[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    given = init.kmeans(parts, K, seeds=seeds, dist_group=True)
    drawn = init.kmeans(parts, K, restarts=2, rng=np.random.RandomState(5 + rank), dist_group=dist.group.WORLD)
    q.put((rank, given, drawn))
    dist.destroy_process_group()


def test_two_ranks_equal_one_process():
    """dist_group: sums, counts and distances all-reduced per pass, seeds drawn over the rows of all ranks (rank-major global order)."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180), q.get(timeout=180)], key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    N, Q, K, B, seed = BLOBS[1]
    X, seeds = blob_case(*BLOBS[1])
    ref = cl.kmeans(X, seeds, thresh=1e-5)
    rs = np.random.RandomState(5)
    runs = [cl.kmeans(X, X[rs.choice(N, K, replace=False)], thresh=1e-5) for _ in range(2)]
    ref_drawn = min(runs, key=lambda r: r[1])
    for rank, given, drawn in res:
        assert given[0].shape == ref[0].shape and np.max(np.abs(given[0] - ref[0])) <= TOL and abs(given[1] - ref[1]) <= TOL
        assert drawn[0].shape == ref_drawn[0].shape and np.max(np.abs(drawn[0] - ref_drawn[0])) <= TOL and abs(drawn[1] - ref_drawn[1]) <= TOL
    assert np.array_equal(res[0][1][0], res[1][1][0]) and np.array_equal(res[0][2][0], res[1][2][0])      # every rank returns the same centres
