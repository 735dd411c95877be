"""gp_kmeans_accumulate (csrc/kmeans.hip): one Lloyd assignment pass of the k-means that places the inducing points (scipy.cluster.vq.kmeans in
parallel_GPLVM.init_statistics, parallel_GPLVM.py:179-186), through the C ABI, and gparml_amd.init.kmeans / driver.init_statistics(init_Z='device')
on real engines.

Labels are checked for EVERY row: the float64 numpy squared distance (direct form) to the device's centre is at most the row's minimum times
1 + 1e-12 (the device adds the same Q terms with one fma each: a few 1e-16 relative).  counts must equal bincount(labels) exactly.  sums and dist2
are recomputed from the device's own labels with 80-bit accumulators and must agree to 1e-12 relative -- for sums[k][q] relative to
sum |x_q| over the centre's rows (the scale of the terms: a fixed-order float64 sum of n terms is within about log2(n) 1.1e-16 of it), for dist2
relative to the value."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import scipy.cluster.vq as cl

from conftest import ROOT
from kmeans_util import BLOBS, blob_case, sqdist

pytestmark = pytest.mark.gpu

LABEL_TOL = 1e-12
SUM_TOL = 1e-12


def check_pass(X, C, out, where=''):
    """Checks (1) and (2) of the module docstring on one call's outputs; returns the figures."""
    sums, counts, dist2, lab = out
    n, Q = X.shape
    K = C.shape[0]
    assert lab.shape == (n,) and lab.dtype == np.int32 and lab.min() >= 0 and lab.max() < K, where
    chosen, worst = np.empty(n), 0.0
    for i in range(0, n, 8192):                                   # every row, no exclusions
        d2 = sqdist(X[i:i + 8192], C)
        lo = d2.min(axis=1)
        chosen[i:i + 8192] = d2[np.arange(d2.shape[0]), lab[i:i + 8192]]
        excess = chosen[i:i + 8192] - lo
        worst = max(worst, float(np.max(np.where(lo > 0, excess / np.where(lo > 0, lo, 1.0), excess))))
        assert np.all(chosen[i:i + 8192] <= lo * (1.0 + LABEL_TOL)), (where, 'a row is not at its nearest centre', worst)
    assert counts.dtype == np.int64 and np.array_equal(counts, np.bincount(lab, minlength=K)), where
    ref = np.zeros((K, Q), dtype=np.longdouble)
    scale = np.zeros((K, Q))
    np.add.at(ref, lab, X.astype(np.longdouble))
    np.add.at(scale, lab, np.abs(X))
    err_s = float(np.max(np.abs(sums - ref).astype(np.float64) / np.where(scale > 0, scale, 1.0)))
    rd = np.array([chosen.astype(np.longdouble).sum(), np.sqrt(chosen.astype(np.longdouble)).sum()], dtype=np.float64)
    err_d = float(np.max(np.abs(dist2 - rd) / np.where(rd > 0, rd, 1.0)))
    print('%s n=%d Q=%d K=%d: label excess %.2e, sums %.2e, dist2 %.2e' % (where, n, Q, K, worst, err_s, err_d))
    assert np.all(np.isfinite(sums)) and np.all(np.isfinite(dist2)), where
    assert np.all(np.abs(sums - ref).astype(np.float64) <= SUM_TOL * scale), (where, err_s)
    assert np.all(np.abs(dist2 - rd) <= SUM_TOL * rd), (where, err_d)


def shapes():
    """(name, X, centres): the blob cases at their seeds, N 1e5 / Q 10 / K 512 normal data, K = 1, K > n, Q = 1, the wide case that needs many
    centre tiles (Q 50, K 1024: 400 KB), Q > 64 (rows and centres from memory), duplicated centres."""
    for case in BLOBS:
        X, seeds = blob_case(*case)
        yield 'blob%d' % case[4], X, seeds
    rs = np.random.RandomState(3)
    X = rs.randn(100000, 10)
    yield 'N1e5_Q10_K512', X, X[rs.choice(100000, 512, replace=False)]
    yield 'K1', X[:30000], rs.randn(1, 10)
    X = rs.randn(50, 4)
    yield 'K_gt_n', X, rs.randn(200, 4)
    X = rs.randn(3000, 1)
    yield 'Q1', X, X[rs.choice(3000, 7, replace=False)]
    X = rs.randn(4096, 50)
    yield 'wide_Q50_K1024', X, X[rs.choice(4096, 1024, replace=False)]
    X = rs.randn(700, 70)
    yield 'Q70', X, X[rs.choice(700, 9, replace=False)]


def run_checks(engine_class):
    """(1)-(3): every shape, twice, bit-identical; ties; a call that spans two chunks."""
    from gparml_amd import _lib
    lib = _lib.load()
    for name, X, C in shapes():
        eng = engine_class(1, 1, 1, X.shape[1])
        out = eng.kmeans_accumulate(C, X=X, want_labels=True)
        check_pass(X, C, out, name)
        again = eng.kmeans_accumulate(C, X=X, want_labels=True)
        assert all(np.array_equal(a, b) for a, b in zip(out, again)), (name, 'two calls differ')
        eng.close()
    # ties go to the lowest index: centres 7, 11 and 30 repeat centres 2, 2 and 29
    X, C = blob_case(*BLOBS[1])
    C = C.copy()
    C[7] = C[2]; C[11] = C[2]; C[30] = C[29]
    eng = engine_class(1, 1, 1, X.shape[1])
    out = eng.kmeans_accumulate(C, X=X, want_labels=True)
    check_pass(X, C, out, 'ties')
    assert not np.isin(out[3], [7, 11, 30]).any() and (out[3] == 2).any() and (out[3] == 29).any()
    assert np.array_equal(out[3], np.argmin(sqdist(X, C), axis=1))            # gaps of this data set are >= 3.7e-6: numpy's first minimum is the label
    # n spans two chunks and is not a multiple of the chunk size: 4096 + 1500 rows; the labels do not depend on the chunking
    X, C = blob_case(*BLOBS[0])
    X = X[:5596]
    whole = eng_out = None
    eng2 = engine_class(1, 1, 1, X.shape[1])
    whole = eng2.kmeans_accumulate(C, X=X, want_labels=True)
    assert lib.gp_debug_set_option(b'kmeans_rows', 4096) == 0
    try:
        eng_out = eng2.kmeans_accumulate(C, X=X, want_labels=True)
        check_pass(X, C, eng_out, 'two_chunks')
        again = eng2.kmeans_accumulate(C, X=X, want_labels=True)
    finally:
        lib.gp_debug_set_option(b'kmeans_rows', 0)
    assert all(np.array_equal(a, b) for a, b in zip(eng_out, again))
    assert np.array_equal(eng_out[3], whole[3]) and np.array_equal(eng_out[1], whole[1])
    eng.close(); eng2.close()


def test_labels_sums_counts_distances_every_shape_and_twice():
    from gparml_amd.engine import ShardEngine
    run_checks(ShardEngine)


def test_resident_rows_equal_host_rows_bit_for_bit():
    from gparml_amd.engine import ShardEngine
    rs = np.random.RandomState(8)
    N, D, M, Q = 9000, 2, 8, 10
    X = rs.randn(N, Q)
    C = X[rs.choice(N, 100, replace=False)]
    eng = ShardEngine(N, D, M, Q)
    eng.upload_shard(rs.randn(N, D), X, np.zeros((N, Q)))
    res = eng.kmeans_accumulate(C, want_labels=True)
    host = eng.kmeans_accumulate(C, X=X, want_labels=True)
    check_pass(X, C, res, 'resident')
    assert all(np.array_equal(a, b) for a, b in zip(res, host))
    assert eng.n_rows == N and np.array_equal(eng.take_rows([5, 0, N - 1]), X[[5, 0, N - 1]])
    eng.close()


def test_evaluation_after_a_pass_is_bit_identical():
    """A full evaluation, gp_kmeans_accumulate, then gp_phase2 / gp_finish (and gp_predict) equal the same sequence without the k-means call."""
    from gparml_amd.engine import ShardEngine
    from oracle import factorised as Fz
    N, D, M, Q = 3000, 5, 40, 10
    d = Fz.synthetic_shard(N, D, M, Q, regime='B', seed=4, zseed=5, alpha_value=0.3)
    eng = ShardEngine(N, D, M, Q)
    eng.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    runs = []
    for with_kmeans in (False, True):
        eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
        first = eng.evaluate(True)
        eng.phase1()
        eng.global_step(sync=True)
        if with_kmeans:
            eng.kmeans_accumulate(d['Z'])                                  # resident rows
            eng.kmeans_accumulate(d['Z'][:7], X=d['X_mu'][:100] + 0.5)     # host rows
        pred = eng.predict(d['X_mu'][:20])
        eng.phase2(True)
        out = eng.finish()
        runs.append([first['F'], first['grad_Z'], out['F'], out['grad_Z'], out['grad_alpha'], out['grad_sf2'], out['grad_beta'],
                     eng.download('GRAD_X_MU'), eng.download('GRAD_X_S'), pred[0], pred[1]])
    eng.close()
    for a, b in zip(*runs):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_error_codes_and_the_empty_call():
    from gparml_amd import _lib
    from gparml_amd.engine import ShardEngine
    lib = _lib.load()
    Q = 3
    eng = ShardEngine(6, 1, 2, Q)
    dp, ip, lp = _lib._dp, _lib._ip, ctypes.POINTER(ctypes.c_int64)
    X, C = np.arange(12.0).reshape(4, Q), np.ones((2, Q))
    sums, counts, dist2, lab = np.full((2, Q), 7.0), np.full(2, 7, dtype=np.int64), np.full(2, 7.0), np.zeros(4, dtype=np.int32)
    call = lambda n, x, K, c: lib.gp_kmeans_accumulate(eng.h, n, None if x is None else x.ctypes.data_as(dp), K, None if c is None else c.ctypes.data_as(dp),
                                                       sums.ctypes.data_as(dp), counts.ctypes.data_as(lp), dist2.ctypes.data_as(dp), lab.ctypes.data_as(ip))
    assert call(-1, X, 2, C) == _lib.GP_ERR_BAD_ARG
    assert call(4, X, 0, C) == _lib.GP_ERR_BAD_ARG
    assert call(4, X, 2, None) == _lib.GP_ERR_BAD_ARG
    bad = X.copy(); bad[2, 1] = np.nan
    assert call(4, bad, 2, C) == _lib.GP_ERR_BAD_ARG and b'not finite' in lib.gp_last_error(eng.h)
    badc = C.copy(); badc[1, 0] = np.inf
    assert call(4, X, 2, badc) == _lib.GP_ERR_BAD_ARG
    assert call(6, None, 2, C) == _lib.GP_ERR_STATE                  # the resident X_mu before an upload
    assert np.all(sums == 7.0) and np.all(counts == 7) and np.all(dist2 == 7.0)      # a failed call writes nothing
    assert call(0, X, 2, C) == _lib.GP_OK
    assert np.all(sums == 0.0) and np.all(counts == 0) and np.all(dist2 == 0.0)      # n = 0: zeros
    eng.upload_shard(np.zeros((6, 1)), np.arange(18.0).reshape(6, Q), np.zeros((6, Q)))
    assert call(4, None, 2, C) == _lib.GP_ERR_BAD_ARG                # X NULL: n must be N_s
    assert call(6, None, 2, C) == _lib.GP_OK and counts.sum() == 6
    # every output may be NULL
    assert lib.gp_kmeans_accumulate(eng.h, 4, X.ctypes.data_as(dp), 2, C.ctypes.data_as(dp), None, None, None, None) == _lib.GP_OK
    assert lib.gp_kmeans_accumulate(eng.h, 4, X.ctypes.data_as(dp), 2, C.ctypes.data_as(dp), None, None, dist2.ctypes.data_as(dp), None) == _lib.GP_OK
    assert dist2[0] > 0 and abs(dist2[0] - sqdist(X, C).min(axis=1).sum()) <= 1e-12 * dist2[0]
    with pytest.raises(AssertionError):
        eng.kmeans_accumulate(np.ones((2, Q + 1)))
    eng.close()


@pytest.mark.parametrize('case', BLOBS, ids=['N20000_Q10_K64', 'N5000_Q3_K33', 'N3000_Q2_K16'])
def test_init_kmeans_on_engines_equals_scipy(case):
    """init.kmeans over host rows through one engine, and over the resident X_mu of two shards, against scipy.cluster.vq.kmeans(X, seeds): 1e-10
    (tests/test_kmeans_host.py has the bound's reasoning and asserts the label gaps of these data sets)."""
    from gparml_amd import init
    from gparml_amd.engine import ShardEngine
    N, Q, K, B, seed = case
    X, seeds = blob_case(*case)
    ref_c, ref_d = cl.kmeans(X, seeds, thresh=1e-5)
    eng = ShardEngine(1, 1, 1, Q)
    c, d, passes = init.kmeans([init.HostRows(eng, X[:N // 3]), init.HostRows(eng, X[N // 3:])], K, seeds=seeds, thresh=1e-5)
    eng.close()
    print('host rows: %d passes, centres %s, max |diff| %.3e, distance diff %.3e' % (passes, c.shape, np.max(np.abs(c - ref_c)) if c.shape == ref_c.shape else np.nan, abs(d - ref_d)))
    assert c.shape == ref_c.shape and np.max(np.abs(c - ref_c)) <= 1e-10 and abs(d - ref_d) <= 1e-10
    cut = N // 2 + 17
    shards = []
    for Xs in (X[:cut], X[cut:]):
        e = ShardEngine(Xs.shape[0], 1, 4, Q)
        e.upload_shard(np.zeros((Xs.shape[0], 1)), Xs, np.zeros(Xs.shape))
        shards.append(e)
    c2, d2, p2 = init.kmeans(shards, K, seeds=seeds, thresh=1e-5)
    assert p2 == passes and c2.shape == ref_c.shape and np.max(np.abs(c2 - ref_c)) <= 1e-10 and abs(d2 - ref_d) <= 1e-10
    # seeds drawn over the resident rows of both shards: K distinct rows of X in the global order
    c3, d3, _ = init.kmeans(shards, K, rng=np.random.RandomState(3))
    idx = np.random.RandomState(3).choice(N, K, replace=False)
    r3 = cl.kmeans(X, X[idx], thresh=1e-5)
    assert c3.shape == r3[0].shape and np.max(np.abs(c3 - r3[0])) <= 1e-10 and abs(d3 - r3[1]) <= 1e-10
    for e in shards:
        e.close()


def test_resident_model_init_Z():
    from gparml_amd.resident import ResidentModel
    N, Q, K, B, seed = BLOBS[1]
    X, seeds = blob_case(*BLOBS[1])
    rs = np.random.RandomState(1)
    shards = [(rs.randn(b - a, 2), X[a:b], np.zeros((b - a, Q))) for a, b in ((0, 2000), (2000, N))]
    model = ResidentModel(shards, K, Q, 2, fixed_embeddings=True)
    c, d, passes = model.init_Z(seeds=seeds)
    model.close()
    ref_c, ref_d = cl.kmeans(X, seeds, thresh=1e-5)
    assert c.shape == ref_c.shape and np.max(np.abs(c - ref_c)) <= 1e-10 and abs(d - ref_d) <= 1e-10


def test_init_statistics_on_the_device_gives_a_Z_an_evaluation_accepts():
    """driver.init_statistics with init_Z='device': an (M, Q) Z from the embeddings of all shards, from which one evaluation through Driver succeeds
    without the jitter retry (conftest's _no_silent_jitter fails this test if one is taken)."""
    from gparml_amd import driver, gpu_MapReduce
    from oracle import factorised as Fz
    N, D, M, Q = 1500, 3, 20, 4
    d = Fz.synthetic_shard(N, D, M, Q, regime='A', seed=5, zseed=6, alpha_value=0.5)
    gpu_MapReduce._reset()
    with tempfile.TemporaryDirectory() as work:
        dirs = {k: os.path.join(work, k) for k in ('input', 'embeddings', 'statistics', 'tmp')}
        for v in dirs.values():
            os.makedirs(v)
        for i, (a, b) in enumerate(((0, 15), (15, 800), (800, N))):      # the first shard alone has fewer than M rows
            np.savetxt(os.path.join(dirs['input'], 'shard_%d' % i), d['Y'][a:b], delimiter=',', fmt='%.17g')
            np.save(os.path.join(dirs['embeddings'], 'shard_%d.embedding.npy' % i), d['X_mu'][a:b])
            np.save(os.path.join(dirs['embeddings'], 'shard_%d.variance.npy' % i), np.zeros((b - a, Q)))
        options = dict(input=dirs['input'], embeddings=dirs['embeddings'], statistics=dirs['statistics'], tmp=dirs['tmp'], parallel='local', keep=True,
                       load=False, M=M, Q=Q, D=D, N=N, fixed_embeddings=True, fixed_beta=False, drop_out_fraction=0, init_Z='device')
        np.random.seed(2)
        options, gs = driver.init_statistics(gpu_MapReduce, options)
        assert gs['Z'].shape == (M, Q) and np.all(np.isfinite(gs['Z']))
        # the centres come from ALL shards: every centre (before the 0.05 noise) is near rows of the data, and the last shard is represented
        near = np.argmin(sqdist(gs['Z'], d['X_mu']), axis=1)
        assert (near >= 800).any()
        drv = driver.Driver(options, gpu_MapReduce, fast=True)
        f, g = drv.likelihood_and_gradient(driver.initial_flat_vector(options, gs), 0)
        assert np.isfinite(f) and np.all(np.isfinite(g))
        assert all(s['engine']._jitter_used == 0 for s in gpu_MapReduce._shards.values())
    gpu_MapReduce._reset()


CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from gparml_amd import _lib
from gparml_amd.engine import ShardEngine
lib = _lib.load()
assert lib.gp_debug_set_option(b'poison_alloc', 1) == 0
import test_gpu_kmeans as t
t.run_checks(ShardEngine)
print('KMEANS_POISON_OK', flush=True)
'''


def test_every_check_with_poisoned_allocations(tmp_path):
    """(1)-(3) once more in a fresh process under the poison mode (GPARML_POISON=1 / poison_alloc: every buffer of the plan is NaN-filled when it is
    allocated): a kernel that reads what the call did not write returns NaN."""
    script = tmp_path / 'kmeans_poison_child.py'
    script.write_text(CHILD % {'root': ROOT, 'tests': os.path.join(ROOT, 'tests')})
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=900, cwd=ROOT, env=dict(os.environ, GPARML_POISON='1'))
    assert r.returncode == 0 and 'KMEANS_POISON_OK' in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
