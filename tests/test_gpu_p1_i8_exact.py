"""The int8 phase 1 (gparml_amd/csrc/p1i8.hip and the digit writer of psi1_kernel, psi1.hip:110-122) against tests/i8_ref.py, element by element.  The
path's arithmetic is exact by construction -- integer sums of digit products -- so the reference is not another float64 kernel but the digits
themselves: the device's own Psi1 (the float64 values psi1_kernel digitised; Psi1 itself is held by test_gpu_compat_arrays.py), Y as uploaded and sf2
are digitised on the host as the kernels do it, the per-order integer sums are formed exactly, and every element of Psi2 and C must lie within
|dev - exact| <= gamma_n A of the exact value, n counted from the shape's own slice plan (18 roundings at 72 slices, 14 at 40; 194 / 195 on the
diagonal, which comes from float64 sums of squares) -- and must equal, bit for bit, the same conversion carried out in the device's order.  An exact
probe on integer data asks for the statistics bit for bit with nothing emulated at all.  The guard's three numbers are recomputed in long double, and
the every-64th-evaluation re-check is walked through.  Nothing here compares the int8 statistics with p1v2_kernel's.

Shapes: the smallest the path applies to (N >= 65536, M >= 385 -> Mp >= 512), each for a branch: 14 tiles in 72 slices of 28 or 29 k-steps; ragged rows,
40 padded columns of Psi1, two column blocks of Y and 25 tiles in 40 slices; Q = 1 and Q = 16 (both ends of psi1_qp <= 16) with 127 padded columns.
The "shared slices" placement of p1i8_prepare is taken at no shape (test_i8_ref_cpu.py enumerates the restated rule), so no case can run it.
Each case prints its worst error / bound per array (pytest -s); DESIGN.md section 6 holds them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import compat_ref as R
import i8_ref as I8
from conftest import ROOT

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.available(), reason='numpy long double has no 64-bit significand here')]

SC_COUNT = 8                         # csrc/gp_common.h: the scalars behind Psi2 and C in the statistics buffer
U = I8.U
CASES = {
    'slices72_n65536_d100_m512_q10': dict(N=65536, D=100, M=512, Q=10, sf2=0.7, alpha=0.4, seed=31, plan=(14, 72, 0)),
    'ragged_n66003_d130_m600_q7': dict(N=66003, D=130, M=600, Q=7, sf2=2.5, alpha=0.4, seed=32, plan=(25, 40, 0)),
    'q1_n65536_d3_m385': dict(N=65536, D=3, M=385, Q=1, sf2=1.3, alpha=2e4, seed=33, plan=(14, 72, 0)),
    'q16_n65536_d3_m385': dict(N=65536, D=3, M=385, Q=16, sf2=0.9, alpha=1.0 / 16, seed=34, plan=(14, 72, 0)),
    'probe_n65536_d8_m512_q2': dict(N=65536, D=8, M=512, Q=2, plan=(14, 72, 0)),
}
_REFS = {}


def _lib():
    from gparml_amd import _lib
    return _lib.load()


def inputs(name):
    c = CASES[name]
    if name.startswith('probe'):
        return I8.probe_inputs(c['N'], c['M'])
    from oracle import factorised as Fz
    N, D, M, Q = c['N'], c['D'], c['M'], c['Q']
    d = Fz.synthetic_shard(N, D, M, Q, regime='A', seed=c['seed'], zseed=c['seed'] + 100, alpha_value=c['alpha'])
    d['sf2'] = c['sf2']
    d['Y'] = d['Y'] * np.linspace(0.01, 30.0, D)[None, :]                # columns of very different scale: per-column digit scales
    if Q == 1:
        d['Z'] = np.linspace(-2.5, 2.5, M)[:, None]                      # 385 inducing points on a line: evenly spaced, so that K_mm stays well conditioned
    if D >= 100:
        d['Y'][:, 3] = 0.0                                               # a zero column
        d['Y'][:, 4] = np.clip(d['Y'][:, 4], -0.9, 0.9); d['Y'][17, 4] = 1.0       # maximum exactly a power of two
        d['Y'][:, 5] = -np.abs(d['Y'][:, 5]); d['Y'][19, 5] = -4.0                  # ... and the extreme negative
    d.update(N=N, D=D, M=M, Q=Q)
    return d


def run_device(d):
    """The path on, the guard's first evaluation accepted, then one phase 1 on the int8 statistics: Psi1, Psi2, C and the statistics image."""
    from gparml_amd.engine import ShardEngine
    lib = _lib()
    N, D, M, Q = d['N'], d['D'], d['M'], d['Q']
    Mp, Dp = I8.pad(M), I8.pad(D)
    assert lib.gp_debug_set_option(b'p1_i8', 1) == 0
    eng = ShardEngine(N, D, M, Q)
    try:
        eng.upload_shard(d['Y'], d['X_mu'], d['X_S'])
        eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
        eng.evaluate(False)                                              # the guard's check: both phase-1 paths, float64 statistics used
        st = eng.i8_status()
        assert st['state'] == 1 and st['checks'] == 1, st
        eng.phase1()
        out = dict(psi1=eng.download('PSI1'), psi2=eng.download('PSI2_SUM'), c=eng.download('PSI1TY'), stats=eng.peek('stats', Mp * Mp + Mp * Dp + SC_COUNT), status=st)
        assert eng.i8_status()['checks'] == 1                            # that phase 1 ran on the int8 kernels alone
    finally:
        eng.close()
        lib.gp_debug_set_option(b'p1_i8', 0)
    return out


def reference(name, d, psi1):
    """i8_ref.reference for the device's Psi1, once per case and process (the device's Psi1 is the same from run to run: checked by its checksum); with
    I8_REF_DIR set (a child process) from the file the parent left there"""
    crc = I8.checksum(psi1)
    if name in _REFS and _REFS[name][0] == crc:
        return _REFS[name][1]
    ref = None
    cache = os.environ.get('I8_REF_DIR')
    if cache and os.path.exists(os.path.join(cache, name + '.npz')):
        ref = I8.load(os.path.join(cache, name + '.npz'), crc)
    if ref is None:
        ref = I8.reference(psi1, d['Y'], d['sf2'])
        assert (ref['plan']['T'], ref['plan']['S'], ref['plan']['n_shared']) == CASES[name]['plan']
    _REFS[name] = (crc, ref)
    return ref


def check_case(name):
    d = inputs(name)
    N, D, M = d['N'], d['D'], d['M']
    Mp, Dp = I8.pad(M), I8.pad(D)
    pl = I8.plan(N, D, M)
    assert (pl['T'], pl['S'], pl['n_shared']) == CASES[name]['plan'], 'the restated plan of %s: %r' % (name, (pl['T'], pl['S'], pl['n_shared']))
    dev = run_device(d)
    st = dev['stats']
    P2, C = st[:Mp * Mp].reshape(Mp, Mp), st[Mp * Mp:Mp * Mp + Mp * Dp].reshape(Mp, Dp)
    bad = []
    if not np.array_equal(dev['psi2'], dev['psi2'].T):
        bad.append('Psi2 is not symmetric bit for bit')
    if not (np.array_equal(P2[:M, :M], dev['psi2']) and np.array_equal(C[:M, :D], dev['c'])):
        bad.append('the downloads are not the windows of the statistics image')
    for what, img, r, c in (('Psi2', P2, M, M), ('C', C, M, D)):
        if np.any(img[r:, :] != 0.0) or np.any(img[:, c:] != 0.0) or not np.all(np.isfinite(img)):
            bad.append('the padding of %s in the statistics image is not exact zero' % what)
    if name.startswith('probe'):
        psi1 = dev['psi1']
        on = psi1[np.arange(N), d['cls']]
        off = psi1.copy(); off[np.arange(N), d['cls']] = 0.0
        assert np.all(on == d['sf2']), 'Psi1 of a row that coincides with its inducing point is not sf2 bit for bit'
        assert off.max() * (0.5 / d['sf2']) < 2.0 ** -43 and off.min() >= 0.0, 'an off-class entry of Psi1 has a non-zero digit: %g' % off.max()
        e2, eC = I8.probe_expected(d)
        if not np.array_equal(dev['psi2'], e2):
            wrong = np.argwhere(dev['psi2'] != e2)
            bad.append('Psi2 differs from sf2^2 diag(class counts) at %d elements, first %s: %r for %r' % (len(wrong), wrong[0], dev['psi2'][tuple(wrong[0])], e2[tuple(wrong[0])]))
        if not np.array_equal(dev['c'], eC):
            wrong = np.argwhere(dev['c'] != eC)
            bad.append('C differs from sf2 times the per-class sums of Y at %d elements, columns %s, first %s: %r for %r' % (
                len(wrong), sorted(set(wrong[:, 1])), wrong[0], dev['c'][tuple(wrong[0])], eC[tuple(wrong[0])]))
        print('%s: Psi2 and C bit for bit the integer sums: %s' % (name, not bad))
    else:
        bad += I8.hold(name, dev['psi2'], dev['c'], reference(name, d, dev['psi1']))
    assert not bad, '%s: %s' % (name, '; '.join(bad))
    return dev


def run_case_list(names):
    for name in names:
        check_case(name)


@pytest.mark.parametrize('name', sorted(CASES))
def test_int8_statistics_elementwise(name):
    check_case(name)


CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from gparml_amd import _lib
assert _lib.load().gp_debug_set_option(b'poison_alloc', 1) == 0
import test_gpu_p1_i8_exact as t
t.run_case_list(%(names)r)
print('I8_CHILD_OK', flush=True)
'''
POISONED = ('ragged_n66003_d130_m600_q7', 'probe_n65536_d8_m512_q2')


def test_ragged_case_and_probe_with_poisoned_allocations(tmp_path):
    """The two cases with padded rows and columns once more in a fresh process under the poison mode: the digit buffer is allocated raw (DA_RAW,
    p1i8.hip:306), so a padded row or column whose digits were never written is NaN bytes there and shows as a wrong integer sum.  The reference comes
    from this process as a file (made for the Psi1 a run here gives; the child computes its own if its Psi1 differs in a bit)."""
    refs = tmp_path / 'refs'
    refs.mkdir()
    for name in POISONED:
        if name.startswith('probe'):
            continue
        d = inputs(name)
        if name not in _REFS:
            reference(name, d, run_device(d)['psi1'])
        I8.save(str(refs / (name + '.npz')), _REFS[name][1], _REFS[name][0])
    script = tmp_path / 'i8_child.py'
    script.write_text(CHILD % {'root': ROOT, 'tests': os.path.join(ROOT, 'tests'), 'names': list(POISONED)})
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env=dict(os.environ, I8_REF_DIR=str(refs), GPARML_POISON='1'))
    print(r.stdout[-20000:])
    assert r.returncode == 0 and 'I8_CHILD_OK' in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _rel(a, b):
    a, b = np.asarray(a, dtype=I8.LD), np.asarray(b, dtype=I8.LD)
    return float(np.sqrt(np.sum((a - b) ** 2) / np.sum(b * b)))


def test_the_guards_numbers():
    """gp_i8_status against its definition (p1i8.hip:412-414): rel_psi2 and rel_c are the Frobenius distances of the padded int8 images from the float64
    ones, cond_lower_bound = (sf2 + beta max_i Psi2_ii) max_i P_ii with the float64 Psi2 and P = (K_mm + beta Psi2)^-1 of the checked evaluation.
    The device adds n / 16384 squares per thread with one fma each (one more rounding in x - y, counted twice for the square), folds 256 threads in
    8 levels and adds 64 block sums in order (p1i8.hip:421-441): n_s = n / 16384 + 2 + 8 + 64 roundings on each of the two sums of positive terms; the
    quotient and the root add two more and the root halves what came before: |rel_dev - rel| <= (n_s + 2) u rel, taken with a factor 1.01 for the second
    order.  The lower bound is two products and a sum: 3 roundings, held to 4 u."""
    from gparml_amd.engine import ShardEngine
    name = 'slices72_n65536_d100_m512_q10'
    d = inputs(name)
    N, D, M, Q = d['N'], d['D'], d['M'], d['Q']
    Mp, Dp = I8.pad(M), I8.pad(D)
    n2, nc = Mp * Mp, Mp * Dp
    lib = _lib()
    eng = ShardEngine(N, D, M, Q)
    try:
        eng.upload_shard(d['Y'], d['X_mu'], d['X_S'])
        eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
        eng.phase1()                                                     # the float64 statistics
        s64 = eng.peek('stats', n2 + nc + SC_COUNT)
        assert eng.i8_status()['checks'] == 0
        assert lib.gp_debug_set_option(b'p1_i8', 1) == 0
        eng.evaluate(False)
        st = eng.i8_status()
        assert st['state'] == 1 and st['checks'] == 1, st
        P = eng.download('KMM_PLUS_OP_INV')
        eng.phase1()                                                     # the int8 statistics
        s8 = eng.peek('stats', n2 + nc + SC_COUNT)
    finally:
        lib.gp_debug_set_option(b'p1_i8', 0)
        eng.close()
    assert not np.array_equal(s8[:n2 + nc], s64[:n2 + nc])
    for key, lo, n in (('rel_psi2', 0, n2), ('rel_c', n2, nc)):
        want = _rel(s8[lo:lo + n], s64[lo:lo + n])
        ns = -(-n // 16384) + 2 + 8 + 64
        tol = 1.01 * (ns + 2) * U * want
        print('%s: device %.17g, long double %.17g, difference %.3g of the bound (%d roundings)' % (key, st[key], want, abs(st[key] - want) / tol, ns + 2))
        assert want > 0 and abs(st[key] - want) <= tol, (key, st[key], want)
    psi2_diag = np.diag(s64[:n2].reshape(Mp, Mp))[:M]
    want = (I8.LD(d['sf2']) + I8.LD(d['beta']) * I8.LD(psi2_diag.max())) * I8.LD(np.diag(P).max())
    print('cond_lower_bound: device %.17g, long double %.17g' % (st['cond_lower_bound'], float(want)))
    assert abs(I8.LD(st['cond_lower_bound']) - want) <= 4 * U * want and st['cond_lower_bound'] > 1


def test_every_64th_evaluation_is_checked_again():
    """psi.hip:260: after acceptance evaluations 2 .. 64 run on the int8 statistics (checks stays 1); the 65th runs both paths again and uses the float64
    statistics -- its outputs are the float64 library's bit for bit -- and the 66th is the 2nd again."""
    from gparml_amd.engine import ShardEngine
    d = inputs('slices72_n65536_d100_m512_q10')
    keys = ('F', 'grad_Z', 'grad_alpha', 'grad_sf2', 'grad_beta')
    same = lambda a, b: all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in keys)
    lib = _lib()
    eng = ShardEngine(d['N'], d['D'], d['M'], d['Q'])
    try:
        eng.upload_shard(d['Y'], d['X_mu'], d['X_S'])
        eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
        f64 = eng.evaluate(False)                                        # the float64 library
        assert lib.gp_debug_set_option(b'p1_i8', 1) == 0
        first = eng.evaluate(False)
        assert same(first, f64) and eng.i8_status()['checks'] == 1 and eng.i8_status()['state'] == 1
        second = eng.evaluate(False)
        assert not same(second, f64)
        for i in range(3, 65):
            out = eng.evaluate(False)
            assert eng.i8_status()['checks'] == 1, i
        assert same(out, second)                                         # the 64th: int8 statistics, bit-identical repeats
        out65 = eng.evaluate(False)
        st = eng.i8_status()
        assert st['checks'] == 2 and st['state'] == 1, st
        assert same(out65, f64)
        out66 = eng.evaluate(False)
        assert eng.i8_status()['checks'] == 2 and same(out66, second)
    finally:
        lib.gp_debug_set_option(b'p1_i8', 0)
        eng.close()
