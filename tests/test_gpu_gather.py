"""gp_gather_shard / gp_scatter_embeddings (csrc/gather.hip) and gparml_amd.svi.ResidentSVI on the device.

A gathered batch context and one uploaded with the same rows hold the same bytes and run the same kernels, so everything is compared with
np.array_equal: there is no tolerance to set.  Shapes: the source has N = 300 rows (Np = 384); batches of 1, 64 and 129 rows (129 crosses a 128-row
padding tile); D = 3 and 130 (Dp = 256: a second column tile); Q = 2, M = 8; fixed embeddings, free ones with plain variances and free ones stored raw.

The one comparison with a tolerance is the local step of the free-embedding driver, x' = x + lr_x g on the device against the same expression in
numpy: one rounding of the fused multiply-add, |x' - (x + lr_x g)| <= eps (|x| + |lr_x g|).  There g is GRAD_X_MU for the means; the variances
are stored raw and move along the raw gradient GRAD_X_S dS/draw, which the device forms once (gp_phase2's grad_latest) -- the test takes that
vector, and holds it to numpy's GRAD_X_S / (1 + e^-raw) within 6 eps: on either side the exp is good to one ulp and the sum, the quotient and the
product round once each, 2.5 eps a side to first order and 5 eps between the two."""
import ctypes

import numpy as np
import pytest

from gparml_amd import _lib
from oracle import factorised as Fz

pytestmark = pytest.mark.gpu
N_SRC, M, Q = 300, 8, 2
REGIMES = ('A', 'B', 'Braw')
EPS = 2.0 ** -52


def _data(D, regime, N=N_SRC, seed=0):
    d = Fz.synthetic_shard(N, D, M, Q, regime='A' if regime == 'A' else 'B', seed=seed, zseed=seed + 1, alpha_value=0.5)
    if regime == 'Braw':
        d['X_S'] = np.log(np.expm1(d['X_S']))
    d['raw'] = regime == 'Braw'
    return d


def _engine(n, D, m=M, q=Q):
    from gparml_amd.engine import ShardEngine
    return ShardEngine(n, D, m, q, device=0)


def _uploaded(d, rows=slice(None)):
    Y, X_mu, X_S = d['Y'][rows], d['X_mu'][rows], d['X_S'][rows]
    e = _engine(len(Y), Y.shape[1])
    e.upload_shard(Y, X_mu, X_S, xs_is_raw=d['raw'])
    return e


def _evaluate(e, d, emb):
    """Everything an evaluation leaves, as a list of arrays."""
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    o = e.evaluate(want_embedding_grads=emb)
    res = [e.scalars()['sum_YYT'], o['F'], o['grad_Z'], o['grad_alpha'], o['grad_sf2'], o['grad_beta'], e.download('PSI1TY'), e.download('X_MU'),
           e.cg_peek('Xs')]
    if emb:
        res += [e.download('GRAD_X_MU'), e.download('GRAD_X_S')]
    return [np.asarray(r) for r in res]


def _same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), 'item %d differs: max |difference| %.3e' % (k, float(np.max(np.abs(x - y))))


def _indices(n, seed=3):
    """Unsorted, with a repeat, rows 0 and N - 1 among them (a single row: the last one)."""
    if n == 1:
        return np.array([N_SRC - 1])
    rng = np.random.RandomState(seed)
    base = 1 + rng.permutation(N_SRC - 2)[:n - 3]
    idx = np.concatenate([base, [0, N_SRC - 1, base[0]]])
    rng.shuffle(idx)
    assert len(idx) == n and np.any(np.diff(idx) < 0) and len(set(idx)) == n - 1
    return idx


_SRC = {}


def _source(D, regime):
    """One resident source per (D, regime), shared and never written by the tests that use it."""
    if (D, regime) not in _SRC:
        d = _data(D, regime)
        _SRC[D, regime] = (_uploaded(d), d)
    return _SRC[D, regime]


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('D', [3, 130])
@pytest.mark.parametrize('n', [1, 64, 129])
def test_a_gathered_batch_is_the_uploaded_batch_bit_for_bit(n, D, regime):
    src, d = _source(D, regime)
    idx = _indices(n)
    emb = regime != 'A'
    got = _engine(n, D)
    got.gather_from(src, idx)
    want = _uploaded(d, idx)
    _same(_evaluate(got, d, emb), _evaluate(want, d, emb))
    got.close()
    want.close()


def test_padding_is_written_not_inherited():
    n, D = 129, 3
    d = _data(D, 'A')
    ones = dict(d, Y=np.ones_like(d['Y']))
    src = _uploaded(ones)
    idx = _indices(n)
    used = _uploaded(_data(D, 'A', seed=5), slice(0, n))            # held another upload before
    _evaluate(used, d, False)
    used.gather_from(src, idx)
    fresh = _engine(n, D)                                           # never held anything: its rows n.. and columns D.. are as allocated
    fresh.gather_from(src, idx)
    want = _evaluate(_uploaded(ones, idx), d, False)
    _same(_evaluate(used, d, False), want)
    _same(_evaluate(fresh, d, False), want)
    for e in (src, used, fresh):
        e.close()


def test_scatter_writes_exactly_the_batch_rows_back():
    from gparml_amd.engine import ShardEngine
    n, D = 64, 3
    d = _data(D, 'Braw')
    full = _uploaded(d)
    idx = np.sort(np.random.RandomState(8).permutation(N_SRC)[:n])
    b = _engine(n, D)
    b.gather_from(full, idx)
    _evaluate(b, d, True)
    b.cg_set_grads()
    b.cg_update(ShardEngine.CG_UPDATE_X, 0.01)
    b.scatter_embeddings_to(full, idx)
    mu, s = d['X_mu'].copy(), d['X_S'].copy()
    mu[idx], s[idx] = b.download('X_MU'), b.cg_peek('Xs')
    assert not np.array_equal(mu[idx], d['X_mu'][idx]) and not np.array_equal(s[idx], d['X_S'][idx])        # the step moved them
    assert np.array_equal(full.download('X_MU'), mu) and np.array_equal(full.cg_peek('Xs'), s)            # those rows, and no other
    edited = _uploaded(dict(d, X_mu=mu, X_S=s))
    _same(_evaluate(full, d, True), _evaluate(edited, d, True))
    for e in (full, b, edited):
        e.close()


def test_a_gather_returns_the_rows_the_source_has_moved_to():
    from gparml_amd.engine import ShardEngine
    n, D = 64, 3
    d = _data(D, 'Braw')
    src = _uploaded(d)
    _evaluate(src, d, True)
    src.cg_set_grads()
    src.cg_update(ShardEngine.CG_UPDATE_X, 0.02)
    mu, s = src.download('X_MU'), src.cg_peek('Xs')
    assert not np.array_equal(mu, d['X_mu'])
    idx = _indices(n)
    b = _engine(n, D)
    b.gather_from(src, idx)
    assert np.array_equal(b.download('X_MU'), mu[idx]) and np.array_equal(b.cg_peek('Xs'), s[idx])
    want = _uploaded(dict(d, X_mu=mu, X_S=s), idx)
    _same(_evaluate(b, d, True), _evaluate(want, d, True))
    for e in (src, b, want):
        e.close()


def _rows(a):
    a = np.ascontiguousarray(a, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def test_status_codes_leave_both_contexts_as_they_were():
    n, D = 64, 3
    d = _data(D, 'Braw')
    full = _uploaded(d)
    good = np.sort(np.random.RandomState(9).permutation(N_SRC)[:n])
    b = _engine(n, D)
    b.gather_from(full, good)
    base_full, base_b = _evaluate(full, d, True), _evaluate(b, d, True)
    lib = full.lib
    other_D, other_Q, empty = _engine(n, D + 1), _engine(n, D, q=Q + 1), _engine(n, D)
    empty_full = _engine(N_SRC, D)
    plain = _uploaded(_data(D, 'B'), slice(0, n))                    # variances stored plainly: not what `full` holds
    G, S = lib.gp_gather_shard, lib.gp_scatter_embeddings
    bad_hi, bad_neg, desc, rep = good.copy(), good.copy(), good.copy(), good.copy()
    bad_hi[5], bad_neg[7] = N_SRC, -1
    desc[[10, 11]] = desc[[11, 10]]
    rep[20] = rep[19]
    BAD, STATE = _lib.GP_ERR_BAD_ARG, _lib.GP_ERR_STATE
    cases = [
        ('gather: n is not the batch context\'s', lambda: G(b.h, full.h, n - 1, _rows(good)[1]), BAD),
        ('scatter: n is not the batch context\'s', lambda: S(full.h, b.h, n - 1, _rows(good)[1]), BAD),
        ('gather: an index equal to N_s', lambda: G(b.h, full.h, n, _rows(bad_hi)[1]), BAD),
        ('scatter: an index equal to N_s', lambda: S(full.h, b.h, n, _rows(bad_hi)[1]), BAD),
        ('gather: a negative index', lambda: G(b.h, full.h, n, _rows(bad_neg)[1]), BAD),
        ('scatter: a negative index', lambda: S(full.h, b.h, n, _rows(bad_neg)[1]), BAD),
        ('scatter: a descending pair', lambda: S(full.h, b.h, n, _rows(desc)[1]), BAD),
        ('scatter: a repeated row', lambda: S(full.h, b.h, n, _rows(rep)[1]), BAD),
        ('gather: D differs', lambda: G(other_D.h, full.h, n, _rows(good)[1]), BAD),
        ('gather: Q differs', lambda: G(other_Q.h, full.h, n, _rows(good)[1]), BAD),
        ('scatter: D differs', lambda: S(full.h, other_D.h, n, _rows(good)[1]), BAD),
        ('scatter: Q differs', lambda: S(full.h, other_Q.h, n, _rows(good)[1]), BAD),
        ('scatter: variances stored differently', lambda: S(full.h, plain.h, n, _rows(good)[1]), BAD),
        ('gather: the source holds no data', lambda: G(b.h, empty_full.h, n, _rows(good)[1]), STATE),
        ('scatter: the source holds no data', lambda: S(full.h, empty.h, n, _rows(good)[1]), STATE),
        ('scatter: the destination holds no data', lambda: S(empty_full.h, b.h, n, _rows(good)[1]), STATE),
        ('gather: rows is NULL', lambda: G(b.h, full.h, n, None), BAD),
        ('scatter: rows is NULL', lambda: S(full.h, b.h, n, None), BAD),
        ('gather: src is NULL', lambda: G(b.h, None, n, _rows(good)[1]), BAD),
        ('gather: dst is NULL', lambda: G(None, full.h, n, _rows(good)[1]), BAD),
        ('scatter: src is NULL', lambda: S(full.h, None, n, _rows(good)[1]), BAD),
        ('scatter: dst is NULL', lambda: S(None, b.h, n, _rows(good)[1]), BAD),
        ('gather: one context on both sides', lambda: G(full.h, full.h, N_SRC, _rows(np.arange(N_SRC))[1]), BAD),
    ]
    for what, call, code in cases:
        assert call() == code, what
        _same(_evaluate(full, d, True), base_full)
        _same(_evaluate(b, d, True), base_b)
    for e in (full, b, other_D, other_Q, empty, empty_full, plain):
        e.close()


def _second_device():
    import torch
    return torch.cuda.device_count() >= 2


@pytest.mark.skipif(not _second_device(), reason='one device visible: the refusal across devices needs two')
def test_two_devices_are_refused():
    from gparml_amd.engine import ShardEngine
    n, D = 64, 3
    d = _data(D, 'A')
    full = _uploaded(d)
    far = ShardEngine(n, D, M, Q, device=1)
    idx = np.arange(n)
    assert full.lib.gp_gather_shard(far.h, full.h, n, _rows(idx)[1]) == _lib.GP_ERR_UNSUPPORTED
    far.upload_shard(d['Y'][:n], d['X_mu'][:n], d['X_S'][:n])
    assert full.lib.gp_scatter_embeddings(full.h, far.h, n, _rows(idx)[1]) == _lib.GP_ERR_UNSUPPORTED
    full.close()
    far.close()


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
N_DRV, B_DRV, D_DRV = 256, 64, 3


def _options(d, **more):
    return dict(dict(Z=d['Z'], sf2=d['sf2'], alpha=d['alpha'], beta=d['beta'], batch=B_DRV, seed=1), **more)


def test_driver_with_fixed_embeddings_is_the_host_driver_bit_for_bit():
    """One iteration each from the same seed, options and data: the two differ only in how the rows arrive."""
    from gparml_amd.svi import SVI, ResidentSVI
    d = _data(D_DRV, 'A', N=N_DRV)
    full = _uploaded(d)
    host = SVI((D_DRV, M, Q), d['Y'], d['X_mu'], _options(d))
    res = ResidentSVI(full, _options(d))
    assert not res.free
    Fh, Fr = host.step(0.5, learn=True), res.step(0.5, learn=True)
    assert np.array_equal(host.last_batch, res.last_batch)
    assert Fh == Fr
    assert np.array_equal(host.flat, res.flat)
    sh, sr = host.eng.svi_get(), res.eng.svi_get()
    for k in ('Lam', 'H', 'Mv', 'Sv'):
        assert np.array_equal(sh[k], sr[k]), k
    host.close()
    res.close()
    assert full.h is not None            # close() leaves the caller's shard open
    full.close()


def test_driver_with_free_embeddings_steps_the_batch_rows_and_no_other():
    from gparml_amd.svi import ResidentSVI
    d = _data(D_DRV, 'Braw', N=N_DRV)
    full = _uploaded(d)
    lr_x = 0.05
    res = ResidentSVI(full, _options(d, lr_x=lr_x))
    assert res.free
    seen = {}
    local_step = res._local_step

    def watched():           # what the batch context holds when the local step starts
        seen['g_mu'], seen['g_s'], seen['latest'] = res.eng.download('GRAD_X_MU'), res.eng.download('GRAD_X_S'), res.eng.download('GRAD_LATEST')
        local_step()
    res._local_step = watched
    res.step(0.5, learn=True)
    idx = res.last_batch
    assert np.array_equal(seen['g_mu'], -seen['latest'][0])
    slope = 1.0 / (1.0 + np.exp(-d['X_S'][idx]))
    g_raw = -seen['latest'][1]
    assert np.all(np.abs(g_raw - seen['g_s'] * slope) <= 6 * EPS * np.abs(seen['g_s'] * slope))
    mu, s = full.download('X_MU'), full.cg_peek('Xs')
    for got, x, g in ((mu, d['X_mu'], seen['g_mu']), (s, d['X_S'], g_raw)):
        want = x[idx] + lr_x * g
        err, tol = np.abs(got[idx] - want), EPS * (np.abs(x[idx]) + np.abs(lr_x * g))
        print('local step: worst error %.2e of its bound' % float(np.max(err / tol)))
        assert np.all(err <= tol)
        assert np.any(got[idx] != x[idx])
        rest = np.setdiff1d(np.arange(N_DRV), idx)
        assert np.array_equal(got[rest], x[rest])
    res.close()
    full.close()


def _toy_gplvm_run():
    """tests/test_gpu_svi.py::test_svi_driver_on_a_toy_regression's budget and criterion on a toy GPLVM: 50 iterations at rho = 1 / t with everything
    but q(u) fixed, the full-data bound, 30 learning iterations at rho = 0.2, the bound again."""
    from gparml_amd.svi import ResidentSVI
    rng = np.random.RandomState(0)
    N, D, Qg, Mg = 256, 4, 2, 16
    X = rng.randn(N, Qg)
    Y = np.sin(X.dot(rng.randn(Qg, D))) + 0.1 * rng.randn(N, D)
    Yc = Y - Y.mean(0)
    U, sv, _ = np.linalg.svd(Yc, full_matrices=False)                # the PCA start: the first two principal scores, unit variance
    X0 = U[:, :Qg] * np.sqrt(N)
    full = _engine(N, D, m=Mg, q=Qg)
    full.upload_shard(Yc, X0, np.full((N, Qg), np.log(np.expm1(0.5))), xs_is_raw=True)
    Z = X0[np.random.RandomState(1).permutation(N)[:Mg]]
    res = ResidentSVI(full, dict(Z=Z, sf2=1.0, alpha=np.ones(Qg), beta=10.0, batch=64, seed=1, lr_x=1e-3))
    for t in range(1, 51):
        res.step(1.0 / t)
    before = res.bound()
    for _ in range(30):
        res.step(0.2, learn=True)
    after = res.bound()
    moved = not np.array_equal(full.download('X_MU'), X0)
    res.close()
    full.close()
    return before, after, moved


def test_driver_trains_a_toy_gplvm_and_repeats_itself():
    before, after, moved = _toy_gplvm_run()
    print('toy GPLVM: full-data bound %.6f before, %.6f after 30 learning iterations' % (before, after))
    assert moved
    assert after > before
    assert (before, after, moved) == _toy_gplvm_run()               # a fresh pair of contexts returns the same bits
