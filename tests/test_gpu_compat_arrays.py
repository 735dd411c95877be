"""Psi1 and the reference-shaped arrays of csrc/compat.hip (GP_ARR_PSI1, GP_ARR_PSI2_POINTS, GP_ARR_KMM, the six derivative tensors,
gp_grad_from_parts) against tests/compat_ref.py: the long-double value of every element and the bound derived in that module's docstring,
|dev - ref| <= 2 (T + n_terms u A) + 2^-1022, elementwise.  None of these arrays passes through a matrix inverse, so a layout, stride or tail
mistake is an O(1) error in some elements -- 1e13 bounds -- and cannot hide in a block norm.  One case per dispatch (compat_ref.CASES: the LE table
interleaved and point-major, the generic psi2 tables, more than one column slab, Mp / Np / Dp > 128, every Psi1 kernel), the far field of exp, Psi1
alone at four column waves in every compiled width, a common offset of (X, Z), the tensor-size guard, the consumers of the arrays (the driver's
compat mode) and the whole case list once more under the poison mode.  Each case prints its worst error / bound per array (pytest -s); DESIGN.md
section 4.2 holds them."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import compat_ref as R
from conftest import ROOT, assert_close
from test_gpu_parity import F_RTOL, G_RTOL

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.available(), reason='numpy long double has no 64-bit significand here')]

_REFS = {}


def reference(d, names=R.ARRAYS, origin=None, tag=''):
    """{array: (value, A, T)} of the inputs ``d`` in long double, computed once per case and process; with COMPAT_REF_DIR set (the poison test's
    child) read from the file the parent left there."""
    key = d['name'] + tag
    if key not in _REFS:
        cache = os.environ.get('COMPAT_REF_DIR')
        if cache:
            z = np.load(os.path.join(cache, key + '.npz'))
            _REFS[key] = {k: (z[k + '_v'], z[k + '_A'], z[k + '_T']) for k in names}
        else:
            _REFS[key] = R.all_arrays(*R.inputs_ld(d), origin=origin, names=names)
    return _REFS[key]


def engine_for(d, step=True):
    from gparml_amd.engine import ShardEngine
    eng = ShardEngine(d['N'], d['D'], d['M'], d['Q'])
    eng.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    eng.phase1()
    if step:
        eng.global_step()
    return eng


def hold(what, got, ref, N, names=None):
    """Every array of ``got`` against the bound; prints the worst ratio per array and fails with the worst element of each array beyond it."""
    bad = []
    for k in (names or got.keys()):
        ratio, idx = R.worst(got[k], *ref[k], R.n_terms(k, N))
        print('[compat arrays] %-26s %-15s worst error / bound %.3g at %s' % (what, k, ratio, idx))
        if not ratio <= 1.0:
            bad.append('%s: %.3g times the bound at %s (device %r, reference %r)' % (k, ratio, idx, float(np.asarray(got[k])[idx]),
                                                                                  float(ref[k][0][idx])))
    assert not bad, '%s: %s' % (what, '; '.join(bad))


def check_case(case):
    d = R.case_inputs(case)
    ref = reference(d)
    eng = engine_for(d)
    got = {k: eng.download(R.DEVICE_NAME[k]) for k in R.ARRAYS}
    eng.close()
    hold(d['name'], got, ref, d['N'])
    p2 = got['psi2_points']
    assert np.array_equal(p2, np.transpose(p2, (0, 2, 1))), '%s: the per-point psi2 is not symmetric bit for bit' % d['name']
    if d['regime'] == 'A':
        p1 = got['psi1']
        assert np.array_equal(p2, p1[:, :, None] * p1[:, None, :]), '%s: psi2_n is not the outer product of the downloaded Psi1 row' % d['name']


def run_case_list():
    for case in R.CASES:
        check_case(case)


@pytest.mark.parametrize('case', R.CASES, ids=R.CASE_NAMES)
def test_every_array_elementwise(case):
    check_case(case)


@pytest.mark.parametrize('regime', ['A', 'B'])
@pytest.mark.parametrize('q', R.PSI1_WIDTHS)
def test_psi1_alone_at_four_column_waves(q, regime):
    """M = 513 (Mp >= 512: four waves across the columns, two columns per lane up to QP = 32) in every width psi1_qp rounds to, and Q = 65 on the
    generic kernel.  Fixed embeddings run without and with embedding gradients: the trial point is prepared in its two forms (fixa)."""
    d = R.psi1_case_inputs(q, regime)
    ref = reference(d, names=('psi1',))
    eng = engine_for(d, step=False)
    hold(d['name'], {'psi1': eng.download('PSI1')}, ref, d['N'])
    if regime == 'A':
        eng.global_step()
        eng.phase2(True)                                   # rebuilds the trial point and Psi1 in the embedding-gradient form
        hold(d['name'] + ' emb', {'psi1': eng.download('PSI1')}, ref, d['N'])
        eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
        eng.phase1()                                       # ... and a whole phase 1 in that mode
        hold(d['name'] + ' emb 2', {'psi1': eng.download('PSI1')}, ref, d['N'])
    eng.close()


SHIFT = 2.0 ** 10


@pytest.mark.parametrize('name', ['B_q17_first_point_major', 'A_q2_Mp384'])
def test_arrays_at_a_shifted_origin(name):
    """2^10 added to every coordinate of Z and X_mu, held against the reference of the UN-shifted inputs: the shifted inputs are rounded to
    float64 at magnitude 2^10, and the bound with |mu + c| and |z + c| in place of the centred magnitudes says how much that may cost.  The
    compat kernels read the centred Z and mu, so nothing beyond that rounding may appear."""
    d = R.case_inputs(R.CASES[R.CASE_NAMES.index(name)])
    ref = reference(d, origin=np.full(d['Q'], -SHIFT), tag='_shifted')
    s = dict(d, Z=d['Z'] + SHIFT, X_mu=d['X_mu'] + SHIFT)
    eng = engine_for(s)
    got = {k: eng.download(R.DEVICE_NAME[k]) for k in R.ARRAYS}
    eng.close()
    hold(name + ' + 2^10', got, ref, d['N'])


@pytest.mark.parametrize('M,Q,D', [(130, 17, 129), (1, 1, 1)])
def test_grad_from_parts(M, Q, D):
    """gp_grad_from_parts on seeded random parts: several workgroups of gradz_parts_kernel (M Q > 256), M and D above 128, and the smallest
    context.  The diagonal of the Kmm term is counted once, as partial_terms.py:226-231 does."""
    from gparml_amd.partial_terms import partial_terms
    rs = np.random.RandomState(1000 + M)
    pt = partial_terms(rs.randn(M, Q), 1.0, np.ones(Q), 1.0, M, Q, 2, D, update_global_statistics=False)
    A, B, C = rs.randn(M, M), rs.randn(M, D), rs.randn(M, M)
    zp = [A, rs.randn(M, Q, M), B, rs.randn(M, Q, D), C, rs.randn(M, Q, M)]
    ap = [A, rs.randn(Q, M, M), B, rs.randn(Q, M, D), C, rs.randn(Q, M, M)]
    got = {'grad_z': pt.grad_Z(*zp), 'grad_alpha': pt.grad_alpha(*ap)}
    ref = {'grad_z': R.grad_z_from_parts(*R.to_ld(*zp), err=True), 'grad_alpha': R.grad_alpha_from_parts(*R.to_ld(*ap), err=True)}
    bad = []
    for k, nt in (('grad_z', 2 * M + D), ('grad_alpha', 2 * M * M + M * D)):
        ratio, idx = R.worst(got[k], *ref[k], nt)
        print('[compat arrays] parts (%d, %d, %d) %-10s worst error / bound %.3g at %s' % (M, Q, D, k, ratio, idx))
        if not ratio <= 1.0:
            bad.append('%s %.3g at %s' % (k, ratio, idx))
    assert not bad, '; '.join(bad)
    # a NULL argument and which = 2: GP_ERR_BAD_ARG, the wrapper's AssertionError
    from gparml_amd import _lib
    eng = pt._engine()
    p = [np.ascontiguousarray(x).ctypes.data_as(_lib._dp) for x in zp]
    out = np.empty((M, Q))
    po = out.ctypes.data_as(_lib._dp)
    assert eng.lib.gp_grad_from_parts(eng.h, 2, p[0], p[1], p[2], p[3], p[4], p[5], po) == _lib.GP_ERR_BAD_ARG
    for i in range(7):
        args = p + [po]
        args[i] = None
        assert eng.lib.gp_grad_from_parts(eng.h, 0, *args) == _lib.GP_ERR_BAD_ARG, 'NULL argument %d' % i
    with pytest.raises(AssertionError):
        pt._from_parts(2, *zp, out)
    eng.close()


def _limit_inputs():
    """N M M = 4097 * 256 * 256 = 2^28 + 2^16: just above the guard; the shard itself is 4097 x 1.  The 256 inducing points sit on a jittered
    16 x 16 grid of spacing h with alpha = 4 / h^2, so that Kmm factorises."""
    N, D, M, Q = 4097, 1, 256, 2
    rs = np.random.RandomState(4097)
    h = 0.25
    g = (np.arange(16) - 7.5) * h
    Z = np.stack(np.meshgrid(g, g, indexing='ij'), axis=-1).reshape(M, Q) + rs.uniform(-0.1, 0.1, size=(M, Q)) * h
    X = rs.uniform(-8 * h, 8 * h, size=(N, Q))
    Y = np.sin(X.sum(axis=1, keepdims=True)) + 0.1 * rs.randn(N, D)
    return dict(N=N, D=D, M=M, Q=Q, regime='A', Z=Z, sf2=1.0, alpha=np.full(Q, 4.0 / (h * h)), beta=10.0, X_mu=X, X_S=np.zeros((N, Q)), Y=Y,
                name='A_limit_4097_256')


def test_tensor_size_guard():
    from gparml_amd import _lib
    d = _limit_inputs()
    assert d['N'] * d['M'] * d['M'] > 2 ** 28 >= (d['N'] - 1) * d['M'] * d['M']
    names = ('psi1', 'dpsi1ty_dz', 'dkmm_dz')
    ref = reference(d, names=names)
    eng = engine_for(d)

    def fast():
        eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
        eng.phase1()
        eng.global_step()
        eng.phase2(False)
        return eng.finish()
    before = fast()
    for name in ('PSI2_POINTS', 'DPSI2_DZ', 'DPSI2_DALPHA'):
        with pytest.raises(_lib.GparmlHipError, match='too large'):
            eng.download(name)
    hold(d['name'], {k: eng.download(R.DEVICE_NAME[k]) for k in names}, ref, d['N'])
    after = fast()
    eng.close()
    for k in ('F', 'grad_Z', 'grad_alpha', 'grad_sf2', 'grad_beta'):
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k])), 'the fast path moved in %s after the refused downloads' % k


@pytest.mark.parametrize('name', ['B_q17_first_point_major', 'B_q10_Mp256'])
def test_the_consumers_of_the_arrays(name):
    """The driver in compat mode (statistics_MR's derivative tensors, partial_terms.grad_Z / grad_alpha from explicit parts) and the fast path
    on the same inputs, both against the oracle at the suite's tolerances: this goes through the global step."""
    from gparml_amd import gpu_MapReduce
    from gparml_amd.driver import Driver, transform_back, transform_grad_vec
    from oracle import factorised as Fz
    d = R.case_inputs(R.CASES[R.CASE_NAMES.index(name)])
    M, Q = d['M'], d['Q']
    ref = Fz.evaluate(d['Z'], d['sf2'], d['alpha'], d['beta'], d['Y'], d['X_mu'], d['X_S'])
    want = np.concatenate([ref['grad_Z'].reshape(-1), [ref['grad_sf2']], np.asarray(ref['grad_alpha']).reshape(-1), [ref['grad_beta']]])
    for fast in (False, True):
        gpu_MapReduce._reset()
        with tempfile.TemporaryDirectory() as work:
            dirs = {k: os.path.join(work, k) for k in ('input', 'embeddings', 'statistics', 'tmp')}
            for v in dirs.values():
                os.makedirs(v)
            np.savetxt(os.path.join(dirs['input'], 'shard_0'), d['Y'], delimiter=',', fmt='%.17g')
            np.save(os.path.join(dirs['embeddings'], 'shard_0.embedding.npy'), d['X_mu'])
            np.save(os.path.join(dirs['embeddings'], 'shard_0.variance.npy'), np.log(np.expm1(d['X_S'])))      # stored raw (softplus inverse)
            options = dict(input=dirs['input'], embeddings=dirs['embeddings'], statistics=dirs['statistics'], tmp=dirs['tmp'], parallel='local',
                           keep=True, load=False, M=M, Q=Q, D=d['D'], N=d['N'], fixed_embeddings=False, fixed_beta=False, drop_out_fraction=0)
            drv = Driver(options, gpu_MapReduce, fast=fast)
            gs = {'Z': d['Z'], 'sf2': np.array([[d['sf2']]]), 'alpha': np.asarray(d['alpha']).reshape(1, -1), 'beta': np.array([[d['beta']]])}
            x = np.array([transform_back(b, v) for b, v in zip(options['flat_global_statistics_bounds'], drv.flatten_global_statistics(gs))])
            f, g = drv.likelihood_and_gradient(x, 0)
        gpu_MapReduce._reset()
        grad = -g / transform_grad_vec(drv._pos, x)
        mode = 'fast' if fast else 'compat'
        assert_close(-f, ref['F'], F_RTOL, what='%s F (%s)' % (name, mode))
        n = M * Q
        for what, sl in (('grad_Z', slice(0, n)), ('grad_sf2', slice(n, n + 1)), ('grad_alpha', slice(n + 1, n + 1 + Q)), ('grad_beta', slice(n + 1 + Q, None))):
            assert_close(grad[sl], want[sl], G_RTOL, what='%s %s (%s)' % (name, what, mode))


CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from gparml_amd import _lib
assert _lib.load().gp_debug_set_option(b'poison_alloc', 1) == 0
import test_gpu_compat_arrays as t
t.run_case_list()
print('COMPAT_POISON_OK', flush=True)
'''


def test_case_list_with_poisoned_allocations(tmp_path):
    """The case list once more in a fresh process under the poison mode (GPARML_POISON=1 / poison_alloc): the compat buffers are DA_RAW allocations,
    filled with NaN bytes there, so an element a kernel leaves unwritten shows up as NaN (ratio inf), not as a stale value.  The references come from
    this process, as files (COMPAT_REF_DIR)."""
    refs = tmp_path / 'refs'
    refs.mkdir()
    for case in R.CASES:
        d = R.case_inputs(case)
        ref = reference(d)
        np.savez(str(refs / (d['name'] + '.npz')), **{k + s: ref[k][i] for k in R.ARRAYS for i, s in enumerate(('_v', '_A', '_T'))})
    script = tmp_path / 'compat_poison_child.py'
    script.write_text(CHILD % {'root': ROOT, 'tests': os.path.join(ROOT, 'tests')})
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env=dict(os.environ, GPARML_POISON='1', COMPAT_REF_DIR=str(refs)))
    assert r.returncode == 0 and 'COMPAT_POISON_OK' in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
