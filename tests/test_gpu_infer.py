"""gp_infer_objective / gp_infer_latent on the GPU: the per-row bound of new, partially observed rows and its per-row optimiser against
tests/infer_ref.py (numpy) and scipy's L-BFGS-B.  Every test fails without the two entry points."""
import os
import subprocess
import sys

import numpy as np
import pytest

import infer_ref as I
from conftest import ROOT
from test_gpu_predictive import _bench_model, _engine, _model, _tol

pytestmark = pytest.mark.gpu


def _mdl(e, d):
    return I.Model(d['Z'], d['sf2'], d['alpha'], d['beta'], e.download('PSI2_SUM'), e.download('PSI1TY'))


def _bounds(mdl, d, tol, Y, cols, mu, S):
    """The value is beta/2 times a sum over the D_o observed outputs of (y - mean)^2 + var, whose mean and variance tests/test_gpu_predictive.py
    bounds by tol relative to max(1, |mean|) and sf2: |dL| <= beta D_o / 2 (2 max|y - mean| tol max(1, |mean|) + tol sf2), plus a few roundings of L
    itself.  A gradient component multiplies the same sums by factors u (mu - z), w (mu - zb) <= max(1, alpha) max(1, |mu - z|)."""
    import predict_ref as R
    c = mdl.cols(cols)
    mean, _ = R.predict(mdl.Z, mdl.sf2, mdl.alpha, mdl.beta, mdl.Psi2, mdl.C, mu, S)
    ms, rmax = max(1.0, np.max(np.abs(mean[:, c]))), np.max(np.abs(Y[:, c] - mean[:, c]))
    tl = 0.5 * d['beta'] * len(c) * tol * (2 * rmax * ms + d['sf2'])
    span = max(1.0, np.max(np.abs(mu[:, None, :] - mdl.Z[None, :, :]))) * max(1.0, np.max(mdl.alpha))
    return tl, 4 * tl * span


def _check_objective(e, d, mdl, tol, Y, cols, mu, S, what):
    Yn = Y.copy()
    if cols is not None:
        Yn[:, np.setdiff1d(np.arange(Y.shape[1]), cols)] = np.nan             # never read
    tl, tg = _bounds(mdl, d, tol, Y, cols, mu, S)
    for raw in (False, True):
        xs = I.softplus_inv(S) if raw else S
        Lr, gmr, gsr = I.objective(mdl, Y, cols, mu, xs, xs_is_raw=raw)
        Ld, gmd, gsd = e.infer_objective(Yn, mu, xs, cols=cols, xs_is_raw=raw)
        eL = np.max(np.abs(Ld - Lr) - 1e-13 * np.abs(Lr))
        gscale = max(1.0, np.max(np.abs(gmr)), np.max(np.abs(gsr)))
        eg = max(np.max(np.abs(gmd - gmr)), np.max(np.abs(gsd - gsr))) - 1e-12 * gscale
        print('[infer objective] %s raw=%d: L err %.3g (bound %.3g), grad err %.3g (bound %.3g, scale %.3g)' % (what, raw, eL, tl, eg, tg, gscale))
        assert eL <= tl, '%s: L %.3g > %.3g' % (what, eL, tl)
        assert eg <= tg, '%s: gradient %.3g > %.3g' % (what, eg, tg)
    return tl, tg


@pytest.mark.parametrize('M,Q,D,regime', [(5, 1, 1, 'A'), (1, 2, 3, 'B'), (64, 2, 3, 'B'), (130, 10, 7, 'A'), (130, 16, 5, 'B'), (130, 17, 3, 'B'), (64, 50, 3, 'B'),
                                          (64, 70, 3, 'B'), (200, 10, 100, 'B')])
def test_objective_against_numpy_reference(M, Q, D, regime):
    """All columns and a strict subset (NaN in the rest), plain and raw variances, both regimes, M off the tile, M = 1, D = 1, every latent width family."""
    N = max(300, M + 100)
    d = _model(N, D, M, Q, regime, seed=M + Q + D)
    e = _engine(d, N, D, M, Q)
    mdl = _mdl(e, d)
    tol = _tol(d, M, mdl.Psi2)
    rs = np.random.RandomState(11)
    n = 21
    mu, S, Y = rs.randn(n, Q), rs.uniform(0.05, 0.5, size=(n, Q)), rs.randn(n, D)
    tl, tg = _check_objective(e, d, mdl, tol, Y, None, mu, S, 'all columns')
    if D > 1:
        cols = np.sort(rs.choice(D, max(1, D // 2), replace=False))
        _check_objective(e, d, mdl, tol, Y, cols, mu, S, 'subset')
    # the bound catches a dropped term: without the KL part of the gradients (-mu, -(1 - 1/S)/2) the reference is off by O(1) >> bound,
    # and without the psi2 term of the value by beta/2 sum(G o psi2)
    gm_drop = I.objective(mdl, Y, None, mu, S, drop='kl_grad')[1]
    L_drop = I.objective(mdl, Y, None, mu, S, drop='psi2')[0]
    Ld, gmd, _ = e.infer_objective(Y, mu, S)
    assert np.max(np.abs(gmd - gm_drop)) > 100 * tg and np.max(np.abs(Ld - L_drop)) > 100 * tl
    e.close()


def test_objective_on_set_local_statistics_and_two_chunks():
    from gparml_amd import _lib
    from gparml_amd.engine import ShardEngine
    M, Q, D, N = 40, 3, 6, 400
    d = _model(N, D, M, Q, 'B', seed=17)
    one = _engine(d, N, D, M, Q)
    sc = one.scalars()
    e = ShardEngine(1, D, M, Q)
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'], N_global=N)
    e.set_local_statistics(sc['sum_YYT'], one.download('PSI2_SUM'), one.download('PSI1TY'), sc['sum_exp_K_ii'], sc['KL'])
    e.global_step(sync=True)
    mdl = _mdl(one, d)
    rs = np.random.RandomState(5)
    n = 300
    mu, S, Y = rs.randn(n, Q), rs.uniform(0.05, 0.5, size=(n, Q)), rs.randn(n, D)
    lib = _lib.load()
    lib.gp_debug_set_option(b'infer_rows', 128)                 # 300 rows: chunks of 128, 128, 44
    try:
        _check_objective(e, d, mdl, _tol(d, M, mdl.Psi2), Y, [0, 2, 3, 5], mu, S, 'set_local_statistics, three chunks')
    finally:
        lib.gp_debug_set_option(b'infer_rows', 0)
    one.close()
    e.close()


def _opt_setup(seed=3, M=30, Q=3, D=6, N=400, n=200):
    d = _model(N, D, M, Q, 'B', seed=seed)
    e = _engine(d, N, D, M, Q)
    rs = np.random.RandomState(seed)
    return d, e, rs.randn(n, D), 0.5 * rs.randn(n, Q), rs.uniform(0.2, 0.6, size=(n, Q))


def test_rows_are_independent_bit_for_bit():
    """A row alone, in a batch, and across a chunk boundary: identical bits from both entry points."""
    from gparml_amd import _lib
    d, e, Y, mu, S = _opt_setup()
    cols = [0, 1, 4]
    whole_o = e.infer_objective(Y, mu, S, cols=cols)
    whole_l = e.infer_latent(Y, mu, S, cols=cols, max_iters=12, gtol=1e-6)
    for i in (0, 77, 199):
        o = e.infer_objective(Y[i:i + 1], mu[i:i + 1], S[i:i + 1], cols=cols)
        l = e.infer_latent(Y[i:i + 1], mu[i:i + 1], S[i:i + 1], cols=cols, max_iters=12, gtol=1e-6)
        assert all(np.array_equal(a[0], b[i]) for a, b in zip(o, whole_o))
        assert all(np.array_equal(a[0], b[i]) for a, b in zip(l, whole_l))
    lib = _lib.load()
    lib.gp_debug_set_option(b'infer_rows', 128)
    try:
        part_o = e.infer_objective(Y, mu, S, cols=cols)
        part_l = e.infer_latent(Y, mu, S, cols=cols, max_iters=12, gtol=1e-6)
    finally:
        lib.gp_debug_set_option(b'infer_rows', 0)
    assert all(np.array_equal(a, b) for a, b in zip(part_o, whole_o))
    assert all(np.array_equal(a, b) for a, b in zip(part_l, whole_l))
    assert np.any(whole_l[3] > 0)
    e.close()


def test_optimiser_exact_properties():
    """L returned = gp_infer_objective at the returned point (same bits); L >= L(start); rows that stopped early have max |gradient| <= gtol."""
    d, e, Y, mu, S = _opt_setup(seed=4)
    mdl = _mdl(e, d)
    gtol, iters = 1e-5, 60
    for raw in (False, True):
        xs = I.softplus_inv(S) if raw else S
        L0 = e.infer_objective(Y, mu, xs, xs_is_raw=raw, want_grads=False)[0]
        m1, s1, L1, it = e.infer_latent(Y, mu, xs, xs_is_raw=raw, max_iters=iters, gtol=gtol)
        La, gma, gsa = e.infer_objective(Y, m1, s1, xs_is_raw=raw)
        assert np.array_equal(La, L1)
        assert np.all(L1 >= L0)
        assert np.all((it >= 0) & (it <= iters))
        done = it < iters
        print('[infer optimiser] raw=%d: %d of %d rows met gtol, mean iterations %.1f, mean gain %.3g' % (raw, done.sum(), len(it), it.mean(), (L1 - L0).mean()))
        assert done.sum() >= len(it) // 2
        S1 = I.softplus(s1) if raw else s1
        _, gm, gs = I.objective(mdl, Y[done], None, m1[done], I.softplus_inv(S1[done]), xs_is_raw=True)      # the optimised variables: (mu, raw S)
        _, tg = _bounds(mdl, d, _tol(d, 30, mdl.Psi2), Y[done], None, m1[done], S1[done])
        assert max(np.max(np.abs(gm)), np.max(np.abs(gs))) <= gtol + tg
    m0, s0, Lz, itz = e.infer_latent(Y[:5], mu[:5], S[:5], max_iters=0)
    assert np.array_equal(m0, mu[:5]) and np.array_equal(s0, S[:5]) and np.all(itz == 0)
    assert np.array_equal(Lz, e.infer_objective(Y[:5], mu[:5], S[:5], want_grads=False)[0])
    e.close()


def _issue_predictor(p):
    from gparml_amd.predict import Predictor
    import predict_ref as R
    Psi2, C = R.statistics(p['Z'], p['sf2'], p['alpha'], p['Y'], p['X_mu'], p['X_S'])
    gs = dict(Z=p['Z'], sf2=p['sf2'], alpha=p['alpha'], beta=p['beta'])
    acc = dict(sum_YYT=np.sum(p['Y'] ** 2), sum_exp_K_mi_K_im=Psi2, sum_exp_K_miY=C, sum_exp_K_ii=p['N'] * p['sf2'], sum_KL=0.0)
    return Predictor(gs, acc, p['N'], p['D']), I.Model(p['Z'], p['sf2'], p['alpha'], p['beta'], Psi2, C)


def test_optimiser_against_lbfgs_and_imputation():
    """The optimiser problem of tests/infer_ref.py (issue_problem): scipy's L-BFGS-B and CG on the numpy objective agree on the final L for at least 38 of
    the 40 rows (re-checked here: 1e-6 relative), and the device's per-row SCG matches L-BFGS-B's L to 1e-6 relative or exceeds it on at least 36.
    Then columns 5-7 are imputed: mean absolute error below the predict-zero baseline."""
    p = I.issue_problem()
    pred, mdl = _issue_predictor(p)
    n = p['Yt'].shape[0]
    ref = np.array([I.optimise_row(mdl, p['Yt'][i], p['cols'], p['X0'][i], p['S0'][i])[2] for i in range(n)])
    cg = np.array([I.optimise_row(mdl, p['Yt'][i], p['cols'], p['X0'][i], p['S0'][i], method='CG')[2] for i in range(n)])
    assert np.sum(np.abs(ref - cg) <= 1e-6 * np.maximum(1.0, np.abs(ref))) >= 38
    res = pred.infer(p['Yt'], mask=p['cols'], X_mu0=p['X0'], X_S0=p['S0'], iterations=300, gtol=1e-7)
    good = res[2] >= ref - 1e-6 * np.abs(ref)
    print('[infer optimiser vs L-BFGS-B] %d of %d rows match or exceed; worst shortfall %.3g' % (good.sum(), n, np.max(ref - res[2])))
    assert good.sum() >= 36, (good.sum(), np.sort(ref - res[2])[-6:])
    Ynan = p['Yt'].copy()
    Ynan[:, p['hidden']] = np.nan
    mean, var, res2 = pred.impute(Ynan, p['cols'], training=[(p['Y'], p['X_mu'])], X_S0=p['S0'], iterations=300, gtol=1e-7)
    assert np.array_equal(res2[2], res[2])                     # the nearest-training-output start is that problem's start
    hid = p['hidden']
    mae, base = np.abs(mean[:, hid] - p['Yt'][:, hid]).mean(), np.abs(p['Yt'][:, hid]).mean()
    print('[infer imputation] MAE %.3f against predict-zero %.3f' % (mae, base))
    assert mae < base


def test_restarts_are_rows():
    p = I.issue_problem()
    pred, mdl = _issue_predictor(p)
    n, R = 6, 5
    np.random.seed(3)
    res = pred.infer(p['Yt'][:n], mask=p['cols'], is_random_init=True, random_restarts=R, iterations=150, gtol=1e-7)
    np.random.seed(3)
    starts = p['Z'][np.random.randint(p['M'], size=(n, R + 1))]
    S0 = np.clip(np.ones((n, 2)) * 0.5 + 0.01 * np.random.randn(n, 2), 0.001, 1)
    e = pred._trained_engine()
    for i in range(n):
        Ls = [e.infer_latent(p['Yt'][i:i + 1], starts[i, k:k + 1], S0[i:i + 1], cols=p['cols'], max_iters=150, gtol=1e-7)[2][0] for k in range(R + 1)]
        assert res[2][i] == max(Ls)
    e.close()


@pytest.mark.jitter_expected
def test_state_and_argument_errors():
    from gparml_amd import _lib
    from gparml_amd.engine import ShardEngine
    M, Q, D, N = 16, 2, 3, 100
    d = _model(N, D, M, Q, 'A', seed=25)
    e = ShardEngine(N, D, M, Q)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    Y, mu, S = np.zeros((2, D)), np.zeros((2, Q)), np.full((2, Q), 0.3)
    calls = (lambda: e.infer_objective(Y, mu, S), lambda: e.infer_latent(Y, mu, S, max_iters=2))

    def stale():
        for f in calls:
            with pytest.raises(_lib.GparmlHipError):
                f()
    stale()                                                     # no global step yet
    e.phase1()
    stale()
    e.global_step(sync=True)
    for f in calls:
        f()
    for bad in (dict(X_S=-S), dict(X_S=0 * S), dict(X_S=np.full((2, Q), np.nan)), dict(X_mu=np.full((2, Q), np.inf)), dict(Y=np.full((2, D), np.nan)),
                dict(cols=[1, 1]), dict(cols=[2, 1]), dict(cols=[0, D]), dict(cols=[-1]), dict(cols=[])):
        a = dict(Y=Y, X_mu=mu, X_S=S, cols=None)
        a.update(bad)
        with pytest.raises(AssertionError):
            e.infer_objective(a['Y'], a['X_mu'], a['X_S'], cols=a['cols'])
        with pytest.raises(AssertionError):
            e.infer_latent(a['Y'], a['X_mu'], a['X_S'], cols=a['cols'], max_iters=2)
    Yn = np.full((2, D), np.nan)
    Yn[:, 1] = 0.5
    e.infer_objective(Yn, mu, S, cols=[1])                      # NaN outside cols is fine
    lib = _lib.load()
    assert lib.gp_infer_objective(e.h, -1, None, None, 0, None, None, 0, None, None, None) == _lib.GP_ERR_BAD_ARG
    assert lib.gp_infer_objective(e.h, 0, None, None, 0, None, None, 0, None, None, None) == _lib.GP_OK
    assert lib.gp_infer_latent(e.h, 0, None, None, 0, None, None, 0, 5, 1e-5, None, None) == _lib.GP_OK
    assert lib.gp_infer_latent(e.h, 1, None, None, 0, None, None, 0, -1, 1e-5, None, None) == _lib.GP_ERR_BAD_ARG
    out = e.infer_latent(np.zeros((0, D)), np.zeros((0, Q)), np.zeros((0, Q)))
    assert out[0].shape == (0, Q) and out[2].shape == (0,)
    # every call of gp_predict's list that invalidates the posterior
    Psi2, C, sc = e.download('PSI2_SUM'), e.download('PSI1TY'), e.scalars()
    other = _engine(d, N, D, M, Q)

    def fresh():
        e.set_local_statistics(sc['sum_YYT'], Psi2, C, sc['sum_exp_K_ii'], sc['KL'])
        e.global_step(sync=True)
        for f in calls:
            f()
    for invalidate in (lambda: e.set_local_statistics(sc['sum_YYT'], Psi2, C, sc['sum_exp_K_ii'], sc['KL']), lambda: e.combine(other, 'stats', 'add'),
                       lambda: e.scale_buffer('stats', 0.5), lambda: e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta']),
                       lambda: (e.stats_pack(), e.stats_unpack()), lambda: e.phase1()):
        fresh()
        invalidate()
        stale()
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    e.set_local_statistics(sc['sum_YYT'], -10.0 * np.eye(M), C, sc['sum_exp_K_ii'], sc['KL'])     # K + beta Psi2 indefinite
    e.global_step(sync=False)
    stale()                                                     # the step asks for the jitter retry
    e.global_step(sync=False, jitter=2)
    stale()                                                     # the retry failed as well
    other.close()
    e.close()


def test_no_side_effects_on_the_evaluation():
    from test_gpu_predictive import _run_sequence
    from gparml_amd.engine import ShardEngine
    M, Q, D, N = 64, 3, 5, 500
    d = _model(N, D, M, Q, 'B', seed=13)
    a = _run_sequence(d, N, D, M, Q, False)
    e = ShardEngine(N, D, M, Q)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    e.phase1()
    e.global_step(sync=True)
    rs = np.random.RandomState(1)
    Y, mu, S = rs.randn(50, D), rs.randn(50, Q), rs.uniform(0.1, 0.4, size=(50, Q))
    e.infer_objective(Y, mu, S, cols=[0, 3])
    e.infer_latent(Y, mu, S, max_iters=5)
    e.phase2(True)
    b = e.finish()
    b['grad_X_mu'], b['grad_X_S'] = e.download('GRAD_X_MU'), e.download('GRAD_X_S')
    e.close()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_poison_mode():
    """The value, optimiser and state tests again with every buffer NaN-filled on allocation."""
    from gparml_amd import _lib
    lib = _lib.load()
    lib.gp_debug_set_option(b'poison_alloc', 1)
    try:
        for args in (1, 2, 3, 'B'), (130, 10, 7, 'A'), (130, 17, 3, 'B'), (64, 70, 3, 'B'):
            test_objective_against_numpy_reference(*args)
        test_objective_on_set_local_statistics_and_two_chunks()
        test_rows_are_independent_bit_for_bit()
        test_optimiser_exact_properties()
        test_no_side_effects_on_the_evaluation()
    finally:
        lib.gp_debug_set_option(b'poison_alloc', 0)


LEAK = r'''
import sys, time
import numpy as np
sys.path.insert(0, %(root)r)
from gparml_amd import _lib
from gparml_amd.engine import ShardEngine
from oracle import factorised as Fz
lib = _lib.load()
SLACK = 64 << 20
probe = ShardEngine(128, 1, 1, 1)
def free_now(base=None):
    if base is None:
        time.sleep(0.5)
    t0 = time.time()
    while True:
        free = probe.memory_info()[0]
        if base is None or abs(free - base) <= SLACK or time.time() - t0 > 5.0:
            return free
        time.sleep(0.05)
N, D, M, Q = 20000, 10, 512, 5
d = Fz.synthetic_shard(N, D, M, Q, regime='A', seed=1, zseed=2, alpha_value=0.3)
def make():
    e = ShardEngine(N, D, M, Q)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    e.evaluate(False)
    return e
rs = np.random.RandomState(3)
Y, X, S = rs.randn(40, D), rs.randn(40, Q), np.full((40, Q), 0.2)
assert lib.gp_debug_set_option(b'infer_rows', 16384) == 0        # V and LEA are 67 MB each: a leak cannot hide in the slack
base = free_now()
for rnd in range(3):                                              # a context that inferred leaks nothing
    e = make()
    e.infer_objective(Y, X, S)
    e.infer_latent(Y, X, S, cols=[0, 3, 4], max_iters=3)
    e.close()
    assert abs(free_now(base) - base) <= SLACK, ('device memory drifts', rnd)
k = 1
while True:                                                       # the k-th allocation of the first inference made to fail
    e = make()
    assert lib.gp_debug_set_option(b'alloc_fail_after', k) == 0
    try:
        e.infer_latent(Y, X, S, max_iters=2)
        ok = True
    except _lib.GparmlHipError as err:
        ok = False
        assert 'injected' in str(err), (k, str(err))
    finally:
        lib.gp_debug_set_option(b'alloc_fail_after', 0)
    e.close()
    free = free_now(base)
    assert abs(free - base) <= SLACK, ('leaks after the failed allocation', k, (free - base) / 2**20)
    if ok:
        break
    k += 1
assert k - 1 >= 20, k
print('INFER_LEAK_OK', k - 1, 'failures', flush=True)
'''


def test_no_leak_and_failed_allocations_leave_nothing_behind(tmp_path):
    path = tmp_path / 'infer_leak.py'
    path.write_text(LEAK.replace('%(root)r', repr(ROOT)))
    r = subprocess.run([sys.executable, str(path)], capture_output=True, text=True, timeout=900, cwd=ROOT, env=dict(os.environ))
    assert r.returncode == 0 and 'INFER_LEAK_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_benchmark_conditioning():
    """configs[2]'s model at its conditioning (cond(Kmm + beta Psi2) ~ 1.9e10, tests/test_gpu_predictive.py _bench_model): L of 2000 rows over all
    100 columns and over 60 of them, a row sample against the 80-bit long-double evaluation from the same float64 statistics.  The bound is about
    20x the error DESIGN.md section 12 records."""
    e, d = _bench_model()
    mdl = I.Model(d['Z'], d['sf2'], d['alpha'], d['beta'], d['Psi2'], d['C'])
    rs = np.random.RandomState(12)
    n, Q, D = 2000, 10, 100
    mu, S = rs.randn(n, Q), rs.uniform(0.05, 0.5, size=(n, Q))
    Y = np.sin(mu.dot(np.random.RandomState(1234).randn(Q, D))) + 0.1 * rs.randn(n, D)
    idx = rs.choice(n, 6, replace=False)
    errs = {}
    for name, cols in (('all', None), ('subset', np.sort(rs.choice(D, 60, replace=False)))):
        Ld = e.infer_objective(Y, mu, S, cols=cols, want_grads=False)[0]
        Lt = I.objective_ld(mdl, Y[idx], cols, mu[idx], S[idx])
        errs[name] = float(np.max(np.abs(np.asarray(Ld[idx], dtype=np.longdouble) - Lt)))
        errs[name + '_scale'] = float(np.max(np.abs(Lt)))
    print('[infer benchmark-conditioning errors]', errs)
    out = os.environ.get('GPARML_INFER_ERR_OUT')
    if out:
        import json
        with open(out, 'w') as fh:
            json.dump(errs, fh)
    assert errs['all'] <= TOL_BENCH_L and errs['subset'] <= TOL_BENCH_L
    e.close()


# measured on MI355X at cond(Kmm + beta Psi2) = 1.9e10: 1.4e-7 over all 100 columns (|L| <= 446), 1.1e-7 over 60; the bound is
# about 20x that.  (A priori, from section 11's per-output errors 3.8e-9 and 1.7e-9: 5 * 100 * (2 * 3.8e-9 + 1.7e-9) = 4.7e-6 if every output erred alike.)
TOL_BENCH_L = 3e-6
