"""gp_select_begin / run / candidate / apply / end (csrc/select.hip): greedy conditional-variance selection of the inducing points, through the C
ABI, gparml_amd.init.greedy_select, driver.init_statistics(init_Z='greedy') and ResidentModel.init_Z(method='greedy') on real engines.

Every case of tests/select_ref.py: the pivots and K' equal the long-double reference's exactly (tests/test_select_cpu.py asserts, on the CPU, that
every choice is clear of rounding); L, d (gp_debug_peek) and the trace are within EIGHT TIMES the float64 mirror's own worst error against that
reference, one figure per case measured here on the CPU (select_ref.reference: max |dL| / sqrt(sf2), max |dd| / sf2, max |dtrace| / (n sf2));
the device's fexp and fused multiply-adds differ from numpy's roundings, hence the factor.  The factorisation's two identities hold on the
device's own L and d within the same figure.  Measured on MI355X (mirror error -> device error): see DESIGN.md section 9.2."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT
import select_ref as R

pytestmark = pytest.mark.gpu

LD = np.longdouble


def device_run(eng, X, sf2, alpha, K, stepwise=False):
    """The selection of host rows X (None: the engine's resident rows) on the device: (pivots, trace, L (n, K'), d).  stepwise: the candidate /
    apply loop in place of gp_select_run."""
    eng.select_begin(K, sf2, alpha, tol=R.TOL, X=X)
    try:
        if not stepwise:
            rows, trace = eng.select_run(K)
            again = eng.select_run(K)                    # nothing is left to do: K reached, or the stopping rule holds again
            assert again[0].size == 0 or rows.size + again[0].size <= K
            assert again[0].size == 0, 'a second gp_select_run found more pivots'
        else:
            rows, trace = [], []
            for j in range(K):
                d, row, x, l = eng.select_candidate(j)
                if row < 0 or not d > R.TOL * sf2:
                    break
                trace.append(eng.select_apply(x, l, d, own_row=row))
                rows.append(row)
            rows, trace = np.array(rows, dtype=np.int64), np.array(trace)
        L, d = eng.select_peek(len(rows))
    finally:
        eng.select_end()
    return rows, trace, L.T.copy(), d


def check_case(name, out):
    """Pivots, K', L, d, trace and the identities of one device result against the reference; returns (mirror error, device error)."""
    X, sf2, alpha, K = R.make_case(name)
    ref, mir, err = R.reference(name)
    rows, trace, L, d = out
    assert np.array_equal(rows, ref['pivots']), (name, 'pivots', rows, ref['pivots'])
    assert trace.shape == ref['trace'].shape and L.shape == ref['L'].shape
    assert np.all(np.isfinite(L)) and np.all(np.isfinite(d)) and np.all(np.isfinite(trace)), name
    dev = R.deviation(ref, L, d, trace, sf2)
    e1, e2 = R.identities(X, sf2, alpha, rows, L, d)
    print('%s: K\' = %d, mirror error %.3e, device error %.3e (bound %.3e), identities %.3e %.3e' % (name, len(rows), err, dev, 8 * err, e1, e2))
    assert dev <= 8 * err, (name, dev, err)
    assert e1 <= 8 * err and e2 <= 8 * err, (name, e1, e2, err)
    return err, dev


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def run_checks(engine_class, names=None):
    """Every case: against the reference, a second run and the candidate / apply loop bit for bit; host rows in one chunk and in three."""
    from gparml_amd import _lib
    lib = _lib.load()
    for name in (names or sorted(R.CASES)):
        X, sf2, alpha, K = R.make_case(name)
        eng = engine_class(1, 1, 1, X.shape[1])
        out = device_run(eng, X, sf2, alpha, K)
        check_case(name, out)
        assert same_bits(out, device_run(eng, X, sf2, alpha, K)), (name, 'two runs differ')
        if X.shape[0] <= 300:
            assert same_bits(out, device_run(eng, X, sf2, alpha, K, stepwise=True)), (name, 'gp_select_run and the candidate / apply loop differ')
        if name == 'n129_Q10_K65':
            assert lib.gp_debug_set_option(b'select_rows', 50) == 0          # 129 rows: chunks of 50, 50 and 29
            try:
                chunked = device_run(eng, X, sf2, alpha, K)
            finally:
                lib.gp_debug_set_option(b'select_rows', 0)
            assert same_bits(out, chunked), (name, 'one chunk and three differ')
        eng.close()


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_case_against_the_reference_twice_and_stepwise(name):
    from gparml_amd.engine import ShardEngine
    run_checks(ShardEngine, [name])


def test_duplicates_stop_early_and_are_never_selected():
    from gparml_amd.engine import ShardEngine
    name = 'dup_n40_Q3_K20'
    X, sf2, alpha, K = R.make_case(name)
    eng = ShardEngine(1, 1, 1, X.shape[1])
    rows, trace, L, d = device_run(eng, X, sf2, alpha, K)
    eng.close()
    assert len(rows) == R.DUP_DISTINCT < K
    assert len(np.unique(X[rows], axis=0)) == R.DUP_DISTINCT          # no row twice, no duplicate of a selected row
    assert abs(trace[-1]) <= 1e-10 * X.shape[0] * sf2


class Peeking(object):
    """A HostRows part that keeps (L, d) as they lie on the device when the selection ends."""

    def __init__(self, engine, X):
        from gparml_amd import init
        self.part, self.engine, self.steps, self.kept = init.HostRows(engine, X), engine, 0, None
        self.n_rows, self.Q, self.device = self.part.n_rows, self.part.Q, self.part.device

    def take_rows(self, idx):
        return self.part.take_rows(idx)

    def select_begin(self, *a, **kw):
        self.steps = 0
        return self.part.select_begin(*a, **kw)

    def select_run(self, steps):
        out = self.part.select_run(steps)
        self.steps += len(out[0])
        return out

    def select_candidate(self, j):
        return self.part.select_candidate(j)

    def select_apply(self, *a, **kw):
        self.steps += 1
        return self.part.select_apply(*a, **kw)

    def select_end(self):
        self.kept = self.engine.select_peek(self.steps)
        return self.part.select_end()


@pytest.mark.parametrize('name,cut', [('n129_Q10_K65', 70), ('n20000_Q10_K40', 7777), ('dup_n40_Q3_K20', 13)])
def test_one_context_and_two_give_the_same_pivots_and_bits(name, cut):
    from gparml_amd import init
    from gparml_amd.engine import ShardEngine
    X, sf2, alpha, K = R.make_case(name)
    ref = R.reference(name)[0]
    engs = [ShardEngine(1, 1, 1, X.shape[1]) for _ in range(3)]
    one = Peeking(engs[0], X)
    Z1, piv1, tr1 = init.greedy_select([one], K, sf2, alpha, tol=R.TOL)
    two = [Peeking(engs[1], X[:cut]), Peeking(engs[2], X[cut:])]
    Z2, piv2, tr2 = init.greedy_select(two, K, sf2, alpha, tol=R.TOL)
    for e in engs:
        e.close()
    assert np.array_equal(piv1[:, 1], ref['pivots']) and np.all(piv1[:, 0] == 0)
    assert np.array_equal(piv2[:, 1] + cut * piv2[:, 0], ref['pivots']) and set(piv2[:, 0].tolist()) <= {0, 1}
    assert np.array_equal(Z1, X[ref['pivots']]) and np.array_equal(Z2, Z1)
    assert np.array_equal(np.concatenate([two[0].kept[0], two[1].kept[0]], axis=1), one.kept[0]), 'L differs between one context and two'
    assert np.array_equal(np.concatenate([two[0].kept[1], two[1].kept[1]]), one.kept[1]), 'd differs between one context and two'
    n = X.shape[0]
    assert np.max(np.abs(tr2 - tr1)) <= 1e-13 * n * sf2                 # the one quantity with a summation order


def test_resident_rows_equal_host_rows_and_the_evaluation_is_untouched():
    """The selection over the resident X_mu carries the bits of the one over the same host rows; and a full evaluation, a selection, then gp_predict /
    gp_phase2 / gp_finish equal the same sequence without the selection."""
    from gparml_amd.engine import ShardEngine
    from oracle import factorised as Fz
    N, D, M, Q = 3000, 5, 40, 10
    dd = Fz.synthetic_shard(N, D, M, Q, regime='B', seed=4, zseed=5, alpha_value=0.3)
    alpha = np.full(Q, 0.1)
    eng = ShardEngine(N, D, M, Q)
    eng.upload_shard(dd['Y'], dd['X_mu'], dd['X_S'])
    runs, sel = [], []
    for with_select in (False, True):
        eng.set_globals(dd['Z'], dd['sf2'], dd['alpha'], dd['beta'])
        first = eng.evaluate(True)
        eng.phase1()
        eng.global_step(sync=True)
        if with_select:
            sel.append(device_run(eng, None, 1.3, alpha, 20))                       # resident rows
            sel.append(device_run(eng, dd['X_mu'], 1.3, alpha, 20))                 # the same rows from the host
            sel.append(device_run(eng, dd['X_mu'][:100] + 0.5, 1.3, alpha, 7, stepwise=True))
        pred = eng.predict(dd['X_mu'][:20])
        eng.phase2(True)
        out = eng.finish()
        runs.append([first['F'], first['grad_Z'], out['F'], out['grad_Z'], out['grad_alpha'], out['grad_sf2'], out['grad_beta'],
                     eng.download('GRAD_X_MU'), eng.download('GRAD_X_S'), pred[0], pred[1]])
    eng.close()
    for a, b in zip(*runs):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert len(sel[0][0]) == 20 and same_bits(sel[0], sel[1])
    ref = R.select(dd['X_mu'], 1.3, alpha, 20, R.TOL)
    assert ref['gap'][1:].min() >= R.MIN_GAP and np.array_equal(sel[0][0], ref['pivots'])


def _chol_solve_trace(Kmm, Psi2):
    """tr(Kmm^-1 Psi2) in long double (a plain Cholesky: numpy.linalg has no long double)."""
    A, B = Kmm.astype(LD), Psi2.astype(LD)
    m = A.shape[0]
    Lc = np.zeros((m, m), dtype=LD)
    for i in range(m):
        for j in range(i + 1):
            s = A[i, j] - (Lc[i, :j] * Lc[j, :j]).sum()
            Lc[i, j] = np.sqrt(s) if i == j else s / Lc[j, j]
    W = B.copy()
    for i in range(m):                       # Lc W = B
        W[i] = (W[i] - Lc[i, :i] @ W[:i]) / Lc[i, i]
    for i in range(m - 1, -1, -1):           # Lc^T V = W
        W[i] = (W[i] - Lc[i + 1:, i] @ W[i + 1:]) / Lc[i, i]
    return np.trace(W)


def test_final_trace_equals_the_bound_s_residual_through_the_library():
    """Fixed embeddings, Z on the selected rows: Psi0 - tr(K_mm^-1 Psi2) from the library's own K_mm and Psi2 equals the selection's last trace to
    1e-8 N sf2 (cond(K_mm) < 1e8 times the unit roundoff, with two orders of room)."""
    from gparml_amd.engine import ShardEngine
    name = 'xcheck_n300_Q2_K12'
    X, sf2, alpha, K = R.make_case(name)
    N, Q = X.shape
    eng = ShardEngine(N, 3, K, Q)
    eng.upload_shard(np.random.RandomState(0).randn(N, 3), X, np.zeros((N, Q)))
    rows, trace, L, d = device_run(eng, None, sf2, alpha, K)
    assert len(rows) == K
    eng.set_globals(X[rows], sf2, alpha, 2.0)
    eng.phase1()
    eng.global_step(sync=True)
    Kmm, Psi2, psi0 = eng.download('KMM'), eng.download('PSI2_SUM'), eng.scalars()['sum_exp_K_ii']
    eng.close()
    assert np.linalg.cond(Kmm) < 1e8
    resid = float(LD(psi0) - _chol_solve_trace(Kmm, Psi2))
    print('trace %.12e, Psi0 - tr(Kmm^-1 Psi2) %.12e, difference %.3e (bound %.3e)' % (trace[-1], resid, abs(resid - trace[-1]), 1e-8 * N * sf2))
    assert abs(resid - trace[-1]) <= 1e-8 * N * sf2


def test_init_statistics_greedy_places_Z_on_data_rows_and_refuses_rank_deficiency():
    from gparml_amd import driver, gpu_MapReduce
    from oracle import factorised as Fz
    N, D, M, Q = 1500, 3, 20, 4
    dd = Fz.synthetic_shard(N, D, M, Q, regime='A', seed=5, zseed=6, alpha_value=0.5)
    gpu_MapReduce._reset()
    with tempfile.TemporaryDirectory() as work:
        dirs = {k: os.path.join(work, k) for k in ('input', 'embeddings', 'statistics', 'tmp')}
        for v in dirs.values():
            os.makedirs(v)
        for i, (a, b) in enumerate(((0, 15), (15, 800), (800, N))):
            np.savetxt(os.path.join(dirs['input'], 'shard_%d' % i), dd['Y'][a:b], delimiter=',', fmt='%.17g')
            np.save(os.path.join(dirs['embeddings'], 'shard_%d.embedding.npy' % i), dd['X_mu'][a:b])
            np.save(os.path.join(dirs['embeddings'], 'shard_%d.variance.npy' % i), np.zeros((b - a, Q)))
        options = dict(input=dirs['input'], embeddings=dirs['embeddings'], statistics=dirs['statistics'], tmp=dirs['tmp'], parallel='local', keep=True,
                       load=False, M=M, Q=Q, D=D, N=N, fixed_embeddings=True, fixed_beta=False, drop_out_fraction=0, init_Z='greedy')
        options, gs = driver.init_statistics(gpu_MapReduce, options)
        Z = gs['Z']
        assert Z.shape == (M, Q)
        rows = [int(np.nonzero((dd['X_mu'] == z).all(axis=1))[0][0]) for z in Z]          # every point IS a data row
        # (the initial alpha = 1 leaves far rows with d = sf2 to the last bits: the choice among them is within rounding, so the pivots are not
        # compared with the long-double reference here -- the cases of select_ref are)
        assert rows[0] == 0 and len(set(rows)) == M and max(rows) >= 800
        drv = driver.Driver(options, gpu_MapReduce, fast=True)
        f, g = drv.likelihood_and_gradient(driver.initial_flat_vector(options, gs), 0)
        assert np.isfinite(f) and np.all(np.isfinite(g))
        # the same files with every embedding one of five rows: five points at most
        for i, (a, b) in enumerate(((0, 15), (15, 800), (800, N))):
            np.save(os.path.join(dirs['embeddings'], 'shard_%d.embedding.npy' % i), dd['X_mu'][np.arange(a, b) % 5])
        with pytest.raises(np.linalg.LinAlgError) as ei:
            driver.init_statistics(gpu_MapReduce, options)
        assert "K' = 5" in str(ei.value) and 'M = %d' % M in str(ei.value)
    gpu_MapReduce._reset()


def test_resident_model_init_Z_greedy_equals_greedy_select():
    from gparml_amd import init
    from gparml_amd.engine import ShardEngine
    from gparml_amd.resident import ResidentModel
    name = 'n129_Q10_K65'
    X, sf2, alpha, K = R.make_case(name)
    ref = R.reference(name)[0]
    rs = np.random.RandomState(1)
    shards = [(rs.randn(b - a, 2), X[a:b], np.zeros((b - a, X.shape[1]))) for a, b in ((0, 50), (50, 129))]
    model = ResidentModel(shards, 30, X.shape[1], 2, fixed_embeddings=True)
    Z, piv, tr = model.init_Z(method='greedy', sf2=sf2, alpha=alpha)
    c, dist, passes = model.init_Z(seeds=X[:30])                  # the default method is k-means still
    model.close()
    engs = [ShardEngine(1, 1, 1, X.shape[1]) for _ in range(2)]
    Z2, piv2, tr2 = init.greedy_select([init.HostRows(engs[0], X[:50]), init.HostRows(engs[1], X[50:])], 30, sf2, alpha)
    for e in engs:
        e.close()
    assert Z.shape == (30, X.shape[1]) and np.array_equal(Z, Z2) and np.array_equal(piv, piv2) and np.array_equal(tr, tr2)
    assert np.array_equal(piv[:, 1] + 50 * piv[:, 0], ref['pivots'][:30]) and c.shape[1] == X.shape[1] and passes >= 1


def test_status_codes_and_the_empty_selection():
    from gparml_amd import _lib
    from gparml_amd.engine import ShardEngine
    lib = _lib.load()
    Q = 3
    eng = ShardEngine(6, 1, 2, Q)
    dp, lp = _lib._dp, ctypes.POINTER(ctypes.c_int64)
    X, alpha = np.arange(12.0).reshape(4, Q) / 7, np.full(Q, 0.5)
    done, rows, trace = ctypes.c_int32(7), np.full(4, 7, dtype=np.int64), np.full(4, 7.0)
    d, row, x, l = ctypes.c_double(7.0), ctypes.c_int64(7), np.zeros(Q), np.zeros(4)
    begin = lambda n, xx, K, sf2, al, tol: lib.gp_select_begin(eng.h, n, None if xx is None else xx.ctypes.data_as(dp), K, sf2,
                                                               None if al is None else al.ctypes.data_as(dp), tol)
    run = lambda steps: lib.gp_select_run(eng.h, steps, ctypes.byref(done), rows.ctypes.data_as(lp), trace.ctypes.data_as(dp))
    cand = lambda: lib.gp_select_candidate(eng.h, ctypes.byref(d), ctypes.byref(row), x.ctypes.data_as(dp), l.ctypes.data_as(dp))
    apply_ = lambda dpv, own: lib.gp_select_apply(eng.h, x.ctypes.data_as(dp), l.ctypes.data_as(dp), dpv, own, None)
    # calls out of order
    assert run(1) == _lib.GP_ERR_STATE and cand() == _lib.GP_ERR_STATE and apply_(1.0, -1) == _lib.GP_ERR_STATE
    assert lib.gp_select_end(eng.h) == _lib.GP_ERR_STATE
    # arguments
    assert begin(-1, X, 2, 1.0, alpha, 1e-10) == _lib.GP_ERR_BAD_ARG
    assert begin(4, X, 0, 1.0, alpha, 1e-10) == _lib.GP_ERR_BAD_ARG
    for tol in (-1e-3, np.nan, np.inf):
        assert begin(4, X, 2, 1.0, alpha, tol) == _lib.GP_ERR_BAD_ARG
    for sf2 in (0.0, -1.0, np.nan):
        assert begin(4, X, 2, sf2, alpha, 1e-10) == _lib.GP_ERR_BAD_ARG
    for bad in (-0.1, np.nan, np.inf):
        a = alpha.copy(); a[1] = bad
        assert begin(4, X, 2, 1.0, a, 1e-10) == _lib.GP_ERR_BAD_ARG
    badx = X.copy(); badx[2, 1] = np.nan
    assert begin(4, badx, 2, 1.0, alpha, 1e-10) == _lib.GP_ERR_BAD_ARG and b'not finite' in lib.gp_last_error(eng.h)
    assert begin(6, None, 2, 1.0, alpha, 1e-10) == _lib.GP_ERR_STATE                 # the resident X_mu before an upload
    assert run(1) == _lib.GP_ERR_STATE                                               # a refused begin leaves no plan
    # a factor that cannot fit: decided from the free bytes, nothing allocated
    free0 = eng.memory_info()[0]
    big = np.zeros((1 << 21, Q))
    assert begin(1 << 21, big, 1 << 17, 1.0, alpha, 1e-10) == _lib.GP_ERR_UNSUPPORTED and b'2097152' in lib.gp_last_error(eng.h)
    assert eng.memory_info()[0] >= free0 - (64 << 20)
    # n = 0 is legal and finds nothing
    assert begin(0, X, 2, 1.0, alpha, 1e-10) == _lib.GP_OK
    assert run(2) == _lib.GP_OK and done.value == 0
    assert cand() == _lib.GP_OK and row.value == -1 and d.value == -np.inf
    assert lib.gp_select_end(eng.h) == _lib.GP_OK and lib.gp_select_end(eng.h) == _lib.GP_ERR_STATE
    # resident rows: n must be N_s
    eng.upload_shard(np.zeros((6, 1)), np.arange(18.0).reshape(6, Q) / 5, np.zeros((6, Q)))
    assert begin(4, None, 2, 1.0, alpha, 1e-10) == _lib.GP_ERR_BAD_ARG
    assert begin(6, None, 2, 1.0, alpha, 1e-10) == _lib.GP_OK
    assert run(-1) == _lib.GP_ERR_BAD_ARG
    assert cand() == _lib.GP_OK and row.value == 0 and d.value == 1.0                 # step 0 is row 0 of the shard
    assert apply_(0.0, -1) == _lib.GP_ERR_BAD_ARG and apply_(np.nan, -1) == _lib.GP_ERR_BAD_ARG
    assert apply_(1.0, 6) == _lib.GP_ERR_BAD_ARG and apply_(1.0, -2) == _lib.GP_ERR_BAD_ARG
    assert apply_(d.value, 0) == _lib.GP_OK
    assert cand() == _lib.GP_OK and row.value > 0
    assert apply_(d.value, row.value) == _lib.GP_OK
    assert apply_(1.0, -1) == _lib.GP_ERR_STATE                                       # K = 2 steps are done
    assert run(1) == _lib.GP_OK and done.value == 0
    # a new begin replaces the plan; K above the number of rows finds them all
    assert begin(4, X, 9, 1.0, alpha, 1e-10) == _lib.GP_OK
    rows9, trace9 = np.full(9, 7, dtype=np.int64), np.full(9, 7.0)
    assert lib.gp_select_run(eng.h, 9, ctypes.byref(done), rows9.ctypes.data_as(lp), trace9.ctypes.data_as(dp)) == _lib.GP_OK
    assert done.value == 4 and sorted(rows9[:4].tolist()) == [0, 1, 2, 3] and rows9[0] == 0 and np.all(rows9[4:] == 7)
    assert lib.gp_select_end(eng.h) == _lib.GP_OK
    with pytest.raises(AssertionError):
        eng.select_begin(2, 1.0, np.ones(Q + 1))
    eng.close()


CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from gparml_amd import _lib
from gparml_amd.engine import ShardEngine
lib = _lib.load()
assert lib.gp_debug_set_option(b'poison_alloc', 1) == 0
import test_gpu_select as t
t.run_checks(ShardEngine)
t.test_duplicates_stop_early_and_are_never_selected()
for args in (('n129_Q10_K65', 70), ('dup_n40_Q3_K20', 13)):
    t.test_one_context_and_two_give_the_same_pivots_and_bits(*args)
t.test_resident_rows_equal_host_rows_and_the_evaluation_is_untouched()
t.test_final_trace_equals_the_bound_s_residual_through_the_library()
t.test_resident_model_init_Z_greedy_equals_greedy_select()
t.test_status_codes_and_the_empty_selection()
print('SELECT_POISON_OK', flush=True)
'''


def test_every_check_with_poisoned_allocations(tmp_path):
    """The file's checks once more in one fresh process under the poison mode (GPARML_POISON=1 / poison_alloc: every buffer of the plan is NaN-filled
    when it is allocated): a kernel that reads what the selection did not write returns NaN and misses its bound."""
    script = tmp_path / 'select_poison_child.py'
    script.write_text(CHILD % {'root': ROOT, 'tests': os.path.join(ROOT, 'tests')})
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=900, cwd=ROOT, env=dict(os.environ, GPARML_POISON='1'))
    assert r.returncode == 0 and 'SELECT_POISON_OK' in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
