"""gp_scatter_accumulate / gp_project_rows (csrc/pca.hip): the device passes of the PCA that initialises the embeddings, through the C ABI, and
gparml_amd.init.pca / ResidentModel.init_X / gpu_MapReduce.init(init_X='device') on real engines.

The bounds are derived, not measured.  With u = 2^-53 and Yc = Y - centre, a float64 sum of n products of rounded differences, in ANY order and with
or without fused multiply-adds, satisfies |gram_ij - truth_ij| <= gamma_(n+2) (|Yc|^T |Yc|)_ij, gamma_k = k u / (1 - k u) (the standard dot-product
bound with two more roundings for the two subtractions); the column sums the same with |Yc|'s column sums; a projected row
|x_q - truth_q| <= gamma_(D+2) sum_d |y_d - mean_d| |P_dq|.  The truths are 80-bit (pca_util).  Everything else is bit for bit."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from pca_util import assert_columns_close, gamma, project_truth, rows, scatter_truth, svd_pca
from pipeline_util import load_pipeline

pytestmark = pytest.mark.gpu

DS = [1, 5, 16, 17, 100, 129, 260]      # below an MFMA tile, one tile, one tile + 1, a padded 128 tile, the first off-diagonal tile pair, three tiles
NS = [1, 63, 64, 65, 4097]              # 4097 rows: nine row slices of 512
Q_OUT = {1: 1, 5: 3, 16: 8, 17: 9, 100: 10, 129: 50, 260: 70}     # every width of the projection kernel (8, 16, 32, 64 and two q tiles)


def check_scatter(Y, centre, out, key, where):
    ssum, gram = out
    n, D = Y.shape
    t_sum, t_gram, a_sum, a_gram = scatter_truth(Y, centre, key)
    assert ssum.shape == (D,) and gram.shape == (D, D) and np.all(np.isfinite(ssum)) and np.all(np.isfinite(gram)), where
    assert np.array_equal(gram, gram.T), (where, 'gram is not symmetric bit for bit')
    g = gamma(n + 2)
    e_gram, e_sum = np.abs(gram - t_gram).astype(np.float64), np.abs(ssum - t_sum).astype(np.float64)
    print('%s: gram at %.3g of its bound, sum at %.3g' % (where, np.max(e_gram / (g * a_gram)), np.max(e_sum / (g * a_sum))))
    assert np.all(e_gram <= g * a_gram), (where, float(np.max(e_gram / (g * a_gram))))
    assert np.all(e_sum <= g * a_sum), (where, float(np.max(e_sum / (g * a_sum))))


def check_project(Y, mean, P, X, where):
    truth, scale = project_truth(Y, mean, P)
    assert X.shape == truth.shape and np.all(np.isfinite(X)), where
    err = np.abs(X - truth).astype(np.float64)
    g = gamma(Y.shape[1] + 2)
    print('%s: projection at %.3g of its bound' % (where, np.max(err / (g * scale))))
    assert np.all(err <= g * scale), (where, float(np.max(err / (g * scale))))


def check_shape(engine_class, D, n):
    """One (D, n): resident and host rows, twice, sum-only, projection, a row alone."""
    where = 'D=%d n=%d' % (D, n)
    Y, centre = rows(n, D)
    eng = engine_class(n, D, 1, 1)
    eng.upload_shard(Y, np.zeros((n, 1)), np.zeros((n, 1)))
    res = eng.scatter_accumulate(centre)
    check_scatter(Y, centre, res, (D, n), where)
    again, host, only = eng.scatter_accumulate(centre), eng.scatter_accumulate(centre, Y=Y), eng.scatter_accumulate(centre, want_gram=False)
    assert np.array_equal(res[0], again[0]) and np.array_equal(res[1], again[1]), (where, 'two calls differ')
    assert np.array_equal(res[0], host[0]) and np.array_equal(res[1], host[1]), (where, 'host rows and resident rows differ')
    assert only[1] is None and np.array_equal(res[0], only[0]), (where, 'the sum-only pass gives another sum')
    rs = np.random.RandomState(D + n)
    P = rs.randn(D, Q_OUT[D])
    mean = centre + 0.1
    X = eng.project_rows(mean, P)
    check_project(Y, mean, P, X, where)
    assert np.array_equal(X, eng.project_rows(mean, P)) and np.array_equal(X, eng.project_rows(mean, P, Y=Y)), where
    for r in sorted({0, n // 2, n - 1}):
        assert np.array_equal(eng.project_rows(mean, P, Y=Y[r:r + 1])[0], X[r]), (where, 'row %d alone differs' % r)
    eng.close()


def check_chunks(engine_class):
    """Host rows that cross chunk boundaries (the chunk length set to 1024 rows through the test hook): the bits of the unchunked call and of the
    resident rows; rows on either side of a boundary project as they do alone."""
    from gparml_amd import _lib
    lib = _lib.load()
    n, D = 2500, 17
    Y, centre = rows(n, D, seed=1)
    P, mean = np.random.RandomState(4).randn(D, 3), centre - 0.2
    eng = engine_class(n, D, 1, 1)
    eng.upload_shard(Y, np.zeros((n, 1)), np.zeros((n, 1)))
    whole, Xw = eng.scatter_accumulate(centre, Y=Y), eng.project_rows(mean, P, Y=Y)
    assert lib.gp_debug_set_option(b'kmeans_rows', 1024) == 0
    try:
        parts, res = eng.scatter_accumulate(centre, Y=Y), eng.scatter_accumulate(centre)
        only = eng.scatter_accumulate(centre, Y=Y, want_gram=False)
        Xc, Xr = eng.project_rows(mean, P, Y=Y), eng.project_rows(mean, P)
    finally:
        lib.gp_debug_set_option(b'kmeans_rows', 0)
    check_scatter(Y, centre, parts, ('chunks', n), 'three chunks')
    for a in (whole, res):
        assert np.array_equal(parts[0], a[0]) and np.array_equal(parts[1], a[1])
    assert np.array_equal(parts[0], only[0])
    check_project(Y, mean, P, Xc, 'three chunks')
    assert np.array_equal(Xc, Xw) and np.array_equal(Xc, Xr)
    for r in (1023, 1024, 2047, 2048):
        assert np.array_equal(eng.project_rows(mean, P, Y=Y[r:r + 1])[0], Xc[r]), r
    eng.close()


def check_slice_plans(engine_class):
    """The two branches of the slice length L = max(512, ceil(n / S) rounded up to 64), S = min(512, 64 MB / (T x 128 KB)), that the shapes above
    (all L = 512) never take: n / 512 > 512 at one tile pair (n = 300000, D = 5: L = 640, 469 slices), and a D-dependent S (D = 260: T = 6,
    S = 85; n = 45000: L = 576, 79 slices).  Resident rows (one launch) against host rows in chunks of two slices: the same bits.  The first
    case is held to the 80-bit truth; the second, whose truth would take numpy half a minute, to numpy's float64 Gram matrix at twice the bound
    (both sides are float64 sums of the same n rounded products: each within gamma_(n+2) |Yc|^T |Yc| of the truth)."""
    from gparml_amd import _lib
    lib = _lib.load()
    for n, D, L in ((300000, 5, 640), (45000, 260, 576)):
        Y, centre = rows(n, D, seed=2)
        eng = engine_class(n, D, 1, 1)
        eng.upload_shard(Y, np.zeros((n, 1)), np.zeros((n, 1)))
        res = eng.scatter_accumulate(centre)
        assert lib.gp_debug_set_option(b'kmeans_rows', 2 * L) == 0
        try:
            host = eng.scatter_accumulate(centre, Y=Y)
            short = eng.scatter_accumulate(centre, Y=Y[:3 * L + 5])          # another n: its own plan (L = 512), not a prefix of this one
        finally:
            lib.gp_debug_set_option(b'kmeans_rows', 0)
        assert np.array_equal(res[0], host[0]) and np.array_equal(res[1], host[1]), (n, D, 'host chunks of two slices differ from the resident rows')
        assert np.array_equal(res[1], res[1].T) and np.array_equal(short[1], short[1].T)
        if D == 5:
            check_scatter(Y, centre, res, ('plan', n), 'n=%d D=%d' % (n, D))
        else:
            Yc = Y - centre
            A = np.abs(Yc)
            g = 2.0 * gamma(n + 2)
            assert np.all(np.abs(res[1] - Yc.T.dot(Yc)) <= g * A.T.dot(A)) and np.all(np.abs(res[0] - Yc.sum(axis=0)) <= g * A.sum(axis=0)), (n, D)
        eng.close()


def run_checks(engine_class, Ds=DS):
    for D in Ds:
        for n in NS:
            check_shape(engine_class, D, n)
    check_chunks(engine_class)
    check_slice_plans(engine_class)


@pytest.mark.parametrize('D', DS)
def test_scatter_and_projection_every_shape(D):
    from gparml_amd.engine import ShardEngine
    for n in NS:
        check_shape(ShardEngine, D, n)


def test_rows_across_chunk_boundaries():
    from gparml_amd.engine import ShardEngine
    check_chunks(ShardEngine)


def test_slice_lengths_beyond_the_shortest():
    from gparml_amd.engine import ShardEngine
    check_slice_plans(ShardEngine)


def test_evaluation_after_the_passes_is_bit_identical():
    """A full evaluation, a scatter and a projection pass, then gp_phase2 / gp_finish (and gp_predict) equal the same sequence without them."""
    from gparml_amd.engine import ShardEngine
    from oracle import factorised as Fz
    N, D, M, Q = 3000, 5, 40, 10
    d = Fz.synthetic_shard(N, D, M, Q, regime='B', seed=4, zseed=5, alpha_value=0.3)
    eng = ShardEngine(N, D, M, Q)
    eng.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    P = np.random.RandomState(0).randn(D, 4)
    runs = []
    for with_pca in (False, True):
        eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
        first = eng.evaluate(True)
        eng.phase1()
        eng.global_step(sync=True)
        if with_pca:
            eng.scatter_accumulate(np.ones(D))                               # resident rows
            eng.project_rows(np.ones(D), P)
            eng.scatter_accumulate(np.zeros(D), Y=d['Y'][:100] + 0.5)        # host rows
            eng.project_rows(np.zeros(D), P, Y=d['Y'][:100] + 0.5)
        pred = eng.predict(d['X_mu'][:20])
        eng.phase2(True)
        out = eng.finish()
        runs.append([first['F'], first['grad_Z'], out['F'], out['grad_Z'], out['grad_alpha'], out['grad_sf2'], out['grad_beta'],
                     eng.download('GRAD_X_MU'), eng.download('GRAD_X_S'), eng.download('X_MU'), pred[0], pred[1]])
    eng.close()
    for a, b in zip(*runs):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_error_codes_and_the_empty_call():
    from gparml_amd import _lib
    from gparml_amd.engine import ShardEngine
    lib = _lib.load()
    D = 3
    eng = ShardEngine(6, D, 2, 2)
    dp = _lib._dp
    ptr = lambda a: None if a is None else a.ctypes.data_as(dp)
    Y, c, P = np.arange(12.0).reshape(4, D), np.ones(D), np.ones((D, 2))
    ssum, gram, X = np.full(D, 7.0), np.full((D, D), 7.0), np.full((4, 2), 7.0)
    scat = lambda n, y, cen: lib.gp_scatter_accumulate(eng.h, n, ptr(y), ptr(cen), ptr(ssum), ptr(gram))
    proj = lambda n, y, m, p, q=2: lib.gp_project_rows(eng.h, n, ptr(y), ptr(m), ptr(p), q, ptr(X))
    bad = Y.copy(); bad[2, 1] = np.nan
    badc = c.copy(); badc[1] = np.nan
    assert scat(-1, Y, c) == _lib.GP_ERR_BAD_ARG and proj(-1, Y, c, P) == _lib.GP_ERR_BAD_ARG
    assert scat(4, Y, None) == _lib.GP_ERR_BAD_ARG and proj(4, Y, None, P) == _lib.GP_ERR_BAD_ARG and proj(4, Y, c, None) == _lib.GP_ERR_BAD_ARG
    assert scat(4, bad, c) == _lib.GP_ERR_BAD_ARG and b'not finite' in lib.gp_last_error(eng.h)
    assert proj(4, bad, c, P) == _lib.GP_ERR_BAD_ARG
    assert scat(4, Y, badc) == _lib.GP_ERR_BAD_ARG and proj(4, Y, badc, P) == _lib.GP_ERR_BAD_ARG
    assert proj(4, Y, c, P, 0) == _lib.GP_ERR_BAD_ARG
    assert scat(6, None, c) == _lib.GP_ERR_STATE and proj(6, None, c, P) == _lib.GP_ERR_STATE      # the resident Y before an upload
    assert np.all(ssum == 7.0) and np.all(gram == 7.0) and np.all(X == 7.0)                          # a failed call writes nothing
    assert scat(0, Y, c) == _lib.GP_OK and proj(0, Y, c, P) == _lib.GP_OK
    assert np.all(ssum == 0.0) and np.all(gram == 0.0) and np.all(X == 7.0)                          # n = 0: zeros
    eng.upload_shard(np.arange(18.0).reshape(6, D), np.zeros((6, 2)), np.zeros((6, 2)))
    assert scat(4, None, c) == _lib.GP_ERR_BAD_ARG and proj(4, None, c, P) == _lib.GP_ERR_BAD_ARG    # Y NULL: n must be N_s
    assert scat(6, None, c) == _lib.GP_OK and ssum[0] == np.sum(np.arange(0.0, 18.0, 3.0) - 1.0)
    # either output may be NULL
    assert lib.gp_scatter_accumulate(eng.h, 4, ptr(Y), ptr(c), None, None) == _lib.GP_OK
    assert lib.gp_scatter_accumulate(eng.h, 4, ptr(Y), ptr(c), None, ptr(gram)) == _lib.GP_OK
    assert gram[0, 0] == np.sum((Y[:, 0] - 1.0) ** 2) and np.array_equal(gram, gram.T)
    assert proj(4, Y, c, P) == _lib.GP_OK and np.array_equal(X, (Y - c).dot(P))                      # small integers: exact
    with pytest.raises(AssertionError):
        eng.scatter_accumulate(np.ones(D + 1))
    eng.close()


def _two_shards(seed=3, D=7, sizes=(211, 150)):
    rs = np.random.RandomState(seed)
    W = rs.randn(4, D) * np.array([4.0, 2.5, 1.5, 0.4])[:, None]
    return [rs.randn(n, 4).dot(W) + 0.1 * rs.randn(n, D) + 50.0 for n in sizes]


def test_resident_model_init_X():
    from gparml_amd.resident import ResidentModel
    D, Q, M = 7, 3, 12
    Ys = _two_shards()
    rs = np.random.RandomState(1)
    S = [rs.uniform(-1.0, 0.0, (Y.shape[0], Q)) for Y in Ys]              # raw variances
    model = ResidentModel([(Y, np.zeros((Y.shape[0], Q)), s) for Y, s in zip(Ys, S)], M, Q, D)
    mean, V, std = model.init_X()
    Yall = np.concatenate(Ys)
    ref = svd_pca(Yall, Q)
    X = np.concatenate([e.download('X_MU') for e in model.engines])
    assert_columns_close(X, ref, what='init_X')
    assert_columns_close((Yall - mean).dot(V) / std, ref, what='init_X axes')
    flat = np.concatenate([(X[:M] + 0.05 * rs.randn(M, Q)).ravel(), [0.5], 0.5 * np.ones(Q), [0.5]])
    f, g = model.likelihood_and_gradient(flat, 0)
    model.close()
    assert np.isfinite(f) and np.all(np.isfinite(g))


def _init_dirs(work, shards, **extra):
    dirs = {d: os.path.join(str(work), d) for d in ('input', 'embeddings', 'statistics', 'tmp')}
    for d in dirs.values():
        os.makedirs(d)
    for i, Y in enumerate(shards):
        np.savetxt(os.path.join(dirs['input'], 'shard_%d' % i), Y, delimiter=',', fmt='%.17g')
    opts = dict(input=dirs['input'], embeddings=dirs['embeddings'], statistics=dirs['statistics'], tmp=dirs['tmp'], parallel='local', iterations=2,
                keep=True, load=False, init='PCA', optimiser='SCG_adapted', drop_out_fraction=0, local_no_pool=False, fixed_embeddings=False,
                fixed_beta=False)
    opts.update(extra)
    return opts


def _count_device_passes(monkeypatch):
    """Wraps ShardEngine's two PCA methods: the list of (pass, rows passed from the host or None) of every call from here on."""
    from gparml_amd.engine import ShardEngine
    calls = []
    scat, proj = ShardEngine.scatter_accumulate, ShardEngine.project_rows

    def scatter_accumulate(self, centre, Y=None, want_gram=True):
        calls.append(('gram' if want_gram else 'sum', None if Y is None else np.asarray(Y).shape[0]))
        return scat(self, centre, Y=Y, want_gram=want_gram)

    def project_rows(self, mean, P, Y=None):
        calls.append(('project', None if Y is None else np.asarray(Y).shape[0]))
        return proj(self, mean, P, Y=Y)
    monkeypatch.setattr(ShardEngine, 'scatter_accumulate', scatter_accumulate)
    monkeypatch.setattr(ShardEngine, 'project_rows', project_rows)
    return calls


def _embeddings(opts, ns):
    return [np.load(os.path.join(opts['embeddings'], 'shard_%d.embedding.npy' % i)) for i in range(ns)]


def test_init_with_init_X_device_equals_the_host_default(tmp_path, monkeypatch):
    """The device path must have run: per shard a sum-only, a Gram and a projection call with the shard's rows passed from the host, in pass
    order; the host default makes no device call at all."""
    from gparml_amd import gpu_MapReduce as mr
    Ys = _two_shards()
    calls = _count_device_passes(monkeypatch)
    out = {}
    for mode in ('host', 'device'):
        opts = _init_dirs(tmp_path / mode, Ys, M=12, Q=3, D=7)
        if mode == 'device':
            opts['init_X'] = 'device'
        np.random.seed(5)
        opts = mr.init(opts)
        assert opts['N'] == 361
        assert calls == ([] if mode == 'host' else [(k, n) for k in ('sum', 'gram', 'project') for n in (211, 150)]), (mode, calls)
        out[mode] = _embeddings(opts, 2) + [np.load(os.path.join(opts['embeddings'], 'shard_%d.variance.npy' % i)) for i in range(2)]
    for i in range(2):
        assert_columns_close(out['device'][i], out['host'][i], what='shard %d' % i)      # the same sign rule: no sign freedom
        assert np.array_equal(out['device'][2 + i], out['host'][2 + i])                  # the variances: the same draws
    assert_columns_close(np.concatenate(out['device'][:2]), svd_pca(np.concatenate(Ys), 3), what='svd form')


@pytest.mark.parametrize('name', ['gplvm_2shards', 'config1_1shard'])
def test_init_X_device_reproduces_the_reference_embeddings(name, tmp_path, monkeypatch):
    """The reference's own PCA embedding files (recorded in the pipeline goldens, tests/test_init_against_reference.py) from init_X = 'device':
    1e-9 up to the sign of a component."""
    from gparml_amd import gpu_MapReduce as mr
    g = load_pipeline(name)
    ns, D, M, Q = int(g['n_shards']), int(g['D']), int(g['M']), int(g['Q'])
    opts = _init_dirs(tmp_path, [g['Y_%d' % i] for i in range(ns)], M=M, Q=Q, D=D, init_X='device')
    calls = _count_device_passes(monkeypatch)
    opts = mr.init(opts)
    assert opts['N'] == int(g['N'])
    sizes = [g['Y_%d' % i].shape[0] for i in range(ns)]
    assert calls == [(k, n) for k in ('sum', 'gram', 'project') for n in sizes], calls      # the embeddings below come from the device passes
    for i, emb in enumerate(_embeddings(opts, ns)):
        assert_columns_close(emb, g['call0_in_shard%d_embedding' % i], signed=False, what='%s shard %d' % (name, i))


CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from gparml_amd import _lib
from gparml_amd.engine import ShardEngine
lib = _lib.load()
assert lib.gp_debug_set_option(b'poison_alloc', 1) == 0
import test_gpu_pca as t
t.run_checks(ShardEngine)
print('PCA_POISON_OK', flush=True)
'''


def test_every_check_with_poisoned_allocations(tmp_path):
    """Every shape and the chunked calls once more in a fresh process under the poison mode (GPARML_POISON=1 / poison_alloc: every buffer of the
    plan is NaN-filled when it is allocated): a kernel that reads what the call did not write returns NaN and misses its bound."""
    script = tmp_path / 'pca_poison_child.py'
    script.write_text(CHILD % {'root': ROOT, 'tests': os.path.join(ROOT, 'tests')})
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=900, cwd=ROOT, env=dict(os.environ, GPARML_POISON='1'))
    assert r.returncode == 0 and 'PCA_POISON_OK' in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
