"""p2_fast8_kernel's chunk staging with a held lane offset and scalar base advance (mma_f64.h, stage8_kf_s), at the shapes where its addressing can
go wrong: N not a multiple of the row tile, M = 128 / 384 / 512 (MT = 1, 3, 4), D = 4 / 100 / 128 / 132 (Dp rolls over to 256, the row stride ld to
384 / 512 / 640 / 768 doubles), Q = 3 / 7 / 10 / 11 (p2_fast8_kernel<1, 2, 3>), one tile per slice, empty trailing slices, a ragged last round
(p2_rem_kernel, which keeps stage8_kf, beside it), and one shard whose Kaug exceeds 4 GiB.  The small cases are held element by element to the dense
reference and bound of tests/fixed_ref.py through test_gpu_fixed_elementwise's helpers (psi1_kernel's output, the device's Bbar and Abar as exact
inputs); the same cases once more under the NaN-poison mode must give the same bits.

The large case: M = 128, D = 4, so a row of Kaug is 256 doubles = 2 KiB and byte offset 2^32 is row 2 097 152; N = 2 097 152 + 2048 + 37, so the last
4096 rows straddle that offset.  Every earlier row lies in the far field with Y = 0 (Psi1 = 0 exactly, fixed_ref's '_far' construction): it adds
exact zeros to every sum, and Psi2, C and the phase-2 sums of the whole shard are held to the reference of the last 4096 rows at THEIR bound (4096
terms).  An offset wrapped at 2^32 reads rows of zeros where the tail's belong, or the tail's rows a second time."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import compat_ref as R
import fixed_ref as F
import test_gpu_fixed_elementwise as E
from conftest import ROOT

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.available(), reason='numpy long double has no 64-bit significand here')]

# (N, D, M, Q), what family() must say about the case
SMALL = (
    ((129, 4, 128, 3), dict(p2='fast8', NRB=1, MT=1, S=2, tps=1, rem=None)),                  # one tile per slice, NRB 1, ld = 256
    ((1000, 100, 512, 10), dict(p2='fast8', NRB=3, MT=4, S=8, tps=1, rem=None, wait=True)),   # the headline's M, D, Q; ld = 640
    ((4099, 132, 128, 11), dict(p2='fast8', NRB=3, MT=1, S=33, tps=1, rem=None)),             # Dp = 256; 33 slices: seven empty trailing ones
    ((200, 128, 384, 7), dict(p2='fast8', NRB=2, MT=3, S=2, tps=1, rem=None, wait=True)),     # NRB 2, MT 3, Dp = 128: ld = 512
    ((33074, 4, 129, 10), dict(p2='fast8', NRB=3, MT=2, S=256, tps=1, rem=(1, 3), wait=True)),  # ragged last round: 259 row tiles on 256 slices
)
IDS = ['n%d_d%d_m%d_q%d' % s for s, _ in SMALL]
_BITS = {}


def _inputs(shape):
    return F.case_inputs(F._case(*shape, tag='_stage8'))


def _bits(dev):
    h = hashlib.sha256()
    for k in ('psi1', 'psi2_sum', 'psi1ty', 'stats', 'Bm', 'grads'):
        h.update(np.ascontiguousarray(dev[k], dtype=np.float64).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize('shape,listed', SMALL, ids=IDS)
def test_small_shapes_elementwise(shape, listed):
    N, D, M, Q = shape
    fam = F.family(N, D, M, Q, False)
    if shape == SMALL[2][0]:
        assert fam['S'] % 8 != 0, 'the case is there for its empty trailing slices'
    wrong = {k: (v, fam.get(k)) for k, v in listed.items() if fam.get(k) != v}
    assert not wrong, '%s: (listed, planned) %s' % (shape, wrong)
    d = _inputs(shape)
    first, second = E.run_device(d)
    assert np.all(np.isfinite(first['Bbar'])) and np.all(np.isfinite(first['Abar'])), 'the global step failed'
    ref = E.reference(d, first)
    got = dict(psi1=first['psi1'], psi2_sum=first['psi2_sum'], psi1ty=first['psi1ty'], grad_z_data=first['grads'][:M * Q].reshape(M, Q),
               grad_alpha_data=first['grads'][M * Q:])
    bad = E._hold(d['name'], got, ref, shape)
    for k in first:
        if not np.array_equal(first[k], second[k], equal_nan=True):
            bad.append('%s of a second evaluation on the same context differs' % k)
    assert not bad, '%s: %s' % (d['name'], '; '.join(bad))
    _BITS[shape] = _bits(first)


CHILD = r'''
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from gparml_amd import _lib
assert _lib.load().gp_debug_set_option(b'poison_alloc', 1) == 0
import test_gpu_fixed_elementwise as E
import test_gpu_stage8_buffer as T
print('STAGE8_BITS ' + json.dumps([T._bits(E.run_device(T._inputs(s), evaluations=1)[0]) for s, _ in T.SMALL]), flush=True)
'''


def test_small_shapes_under_poison_give_the_same_bits(tmp_path):
    """GPARML_POISON=1 (read once per process: a child): every allocation starts as NaN, so a read outside the staged windows, or an element left
    unwritten, changes bits."""
    for shape, _ in SMALL:
        if shape not in _BITS:
            _BITS[shape] = _bits(E.run_device(_inputs(shape), evaluations=1)[0])
    script = tmp_path / 'stage8_child.py'
    script.write_text(CHILD % {'root': ROOT, 'tests': os.path.join(ROOT, 'tests')})
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, GPARML_POISON='1'))
    lines = [l for l in r.stdout.splitlines() if l.startswith('STAGE8_BITS ')]
    assert r.returncode == 0 and lines, r.stdout[-3000:] + r.stderr[-3000:]
    poisoned = json.loads(lines[-1][len('STAGE8_BITS '):])
    differ = [IDS[i] for i, (s, _) in enumerate(SMALL) if _BITS[s] != poisoned[i]]
    assert not differ, 'the poisoned run differs in bits at %s' % differ


def test_kaug_beyond_4_gib():
    from gparml_amd.engine import ShardEngine
    D, M, Q, NT = 4, 128, 3, 4096
    N = (1 << 32) // (256 * 8) + 2048 + 37
    assert N % 128 != 0 and N * 256 * 8 > (1 << 32) > (N - NT) * 256 * 8
    d = F.case_inputs(F._case(NT, D, M, Q, tag='_stage8_tail'))
    far = F.case_inputs(F._case(1, D, M, Q, tag='_far'))['X_mu'][0]          # a far-field point for THIS M (the shift depends on M only)
    assert far[0] > 1e3 / np.sqrt(d['alpha'][0])
    X_mu = np.empty((N, Q))
    X_mu[:] = far
    X_mu[N - NT:] = d['X_mu']
    Y = np.zeros((N, D))
    Y[N - NT:] = d['Y']
    # Psi1 of the tail rows from a shard that holds only them (psi1_kernel works row by row from the same centred Z)
    small = ShardEngine(NT, D, M, Q)
    small.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    small.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    small.phase1()
    K = small.download('PSI1')
    small.close()
    eng = ShardEngine(N, D, M, Q)
    eng.upload_shard(Y, X_mu, np.zeros((N, Q)))
    runs = []
    for _ in range(2):
        eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
        eng.phase1()
        out = dict(psi2_sum=eng.download('PSI2_SUM'), psi1ty=eng.download('PSI1TY'))
        eng.global_step()
        Bbar = np.ascontiguousarray(eng.peek('Bbar', M * M).reshape(M, M))
        Abar = np.ascontiguousarray(eng.peek('Abar', M * 128).reshape(M, 128)[:, :D])
        eng.phase2(False)
        g = eng.peek('grads', M * Q + Q)
        out.update(grad_z_data=g[:M * Q].reshape(M, Q), grad_alpha_data=g[M * Q:])
        runs.append(out)
    eng.close()
    assert np.all(np.isfinite(Bbar)) and np.all(np.isfinite(Abar)), 'the global step failed'
    zc, mc, o = F.centred(d['Z'], d['X_mu'])
    ref = F.phase1(K, d['Y'], d['sf2'])
    ref.update(F.phase2(K, d['Y'], Bbar, Abar, zc, mc, o, d['alpha'], points=False))
    bad = F.hold('kaug_beyond_4_gib', dict(runs[0]), ref, (NT, D, M, Q), tag='stage8')
    for k in runs[0]:
        if not np.array_equal(runs[0][k], runs[1][k]):
            bad.append('%s of a second evaluation differs' % k)
    assert not bad, '; '.join(bad)
