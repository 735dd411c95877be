"""The fixed-embedding (regime A) kernels of both phases against tests/fixed_ref.py, element by element: psi1_kernel's output as the exact input,
p1v2_kernel<8, 26> / p1v2_reduce_kernel (p1_kernel8 / p1_reduce_kernel / p1_scalars_kernel where p1v2 does not apply) in phase 1;
p2_fast8_kernel<1, 2, 3>, p2_rem_kernel / p2_rem_fix_kernel, p2_gen8_kernel<false> and <true> + point_kernel, p2_reduce_kernel and colsum2_kernel in
phase 2.  The global step is taken out of the comparison: the device's own Bbar and Abar are the exact inputs of the phase-2 reference.  Every element
is held to |dev - ref| <= 2 (T + n_terms u A) + 2^-1022 with the derived A, T of fixed_ref's docstring.  One case per launch shape
(fixed_ref.CASES), each asserted to land on the plan it is listed for; the free-running form (GPARML_P2_SYNC=0) in a child process, every value of
the remainder option on one context each, the whole default list once more under the poison mode.  Each case prints its worst error / bound per
array (pytest -s); DESIGN.md section 4.2 holds them."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import compat_ref as R
import fixed_ref as F
from conftest import ROOT

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.available(), reason='numpy long double has no 64-bit significand here')]

_REFS = {}


def _pad(n):
    return (n + 127) // 128 * 128


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def reference(d, dev):
    """{array: (value, A, T)} for the device's own K, Bbar and Abar: once per (case, bits of those inputs) and process -- they are bit-identical from
    run to run, so the runs of a case share it.  With FIXED_REF_DIR set (a child process) it comes from the file the parent left there, if the
    inputs are the parent's bit for bit."""
    key = _digest(dev['psi1'], dev['Bbar'], dev['Abar'])
    name = d['name']
    if name in _REFS and _REFS[name][0] == key:
        return _REFS[name][1]
    cache = os.environ.get('FIXED_REF_DIR')
    path = os.path.join(cache, name + '.npz') if cache else None
    if path and os.path.exists(path):
        z = np.load(path)
        if str(z['key']) == key:
            ref = {k: (z[k + '_v'], z[k + '_A'], z[k + '_T']) for k in ('psi1',) + F.PHASE1 + F.PHASE2 + (F.POINTS if 'grad_x_mu_v' in z.files else ())}
            _REFS[name] = (key, ref)
            return ref
    if 'Z0' in d:
        ref = shifted_reference(d, dev)
    else:
        zc, mc, o = F.centred(d['Z'], d['X_mu'])
        ref = F.phase1(dev['psi1'], d['Y'], d['sf2'])
        ref.update(F.phase2(dev['psi1'], d['Y'], dev['Bbar'], dev['Abar'], zc, mc, o, d['alpha'], points=d['emb']))
        ref['psi1'] = R.psi1(*R.to_ld(d['Z'], d['sf2'], d['alpha'], d['X_mu'], d['X_S']), err=True)
    _REFS[name] = (key, ref)
    return ref


def shifted_reference(d, dev):
    """The case at a shifted origin against the reference of the UN-shifted inputs (tests/test_gpu_compat_arrays.py::test_arrays_at_a_shifted_origin):
    Psi1 from compat_ref with origin = -2^10, i.e. with |mu + c| and |z + c| where the centred magnitudes stand; everything behind it from that Psi1
    rounded to float64 and the un-shifted centred coordinates, with fixed_ref.input_error_terms added to T: what the rounding of the shifted inputs
    at magnitude 2^10 may cost, propagated to first order.  Bbar and Abar stay the device's own (the global step is not under test).  grad_x_mu's KL
    part is in the caller's coordinates: the shifted run returns the un-shifted value minus 2^10."""
    ld = R.to_ld(d['Z0'], d['sf2'], d['alpha'], d['X0'], d['X_S'])
    v, A, T = R.psi1(*ld, origin=np.full(d['Q'], -F.SHIFT), err=True)
    K = np.asarray(v, dtype=np.float64)
    eK = np.asarray(T, dtype=np.float64) + 2 * F.U * np.asarray(A, dtype=np.float64)
    zc, mc, o = F.centred(d['Z0'], d['X0'])
    ref = F.phase1(K, d['Y'], d['sf2'])
    ref.update(F.phase2(K, d['Y'], dev['Bbar'], dev['Abar'], zc, mc, o, d['alpha'], points=d['emb']))
    extra = F.input_error_terms(K, eK, d['Y'], dev['Bbar'], dev['Abar'], zc, mc, F.U * np.abs(d['Z']), F.U * np.abs(d['X_mu']), d['alpha'], points=d['emb'])
    for k, e in extra.items():
        val, A_, T_ = ref[k]
        ref[k] = (val, A_, T_ + e)
    if d['emb']:
        val, A_, T_ = ref['grad_x_mu']
        ref['grad_x_mu'] = (val - R.LD(F.SHIFT), A_ + F.SHIFT, T_ + (F.M_D_FIN(d) * F.U) * F.SHIFT)
    ref['psi1'] = (v, A, T)
    return ref


def save_reference(path, name):
    key, ref = _REFS[name]
    np.savez(path, key=key, **{k + s: np.asarray(ref[k][i]) for k in ref for i, s in enumerate(('_v', '_A', '_T'))})


def run_device(d, evaluations=2):
    """``evaluations`` evaluations on one context, stage by stage; everything the checks need, as host arrays, per evaluation."""
    from gparml_amd.engine import ShardEngine
    N, D, M, Q = d['N'], d['D'], d['M'], d['Q']
    Mp, Dp = _pad(M), _pad(D)
    eng = ShardEngine(N, D, M, Q)
    eng.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    outs = []
    for _ in range(evaluations):
        eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
        eng.phase1()
        out = dict(psi1=eng.download('PSI1'), psi2_sum=eng.download('PSI2_SUM'), psi1ty=eng.download('PSI1TY'),
                   stats=eng.peek('stats', Mp * Mp + Mp * Dp + F.SC_COUNT))
        out['zc'] = eng.peek('Z', Mp * Q).reshape(Mp, Q)[:M]
        out['mc'] = eng.peek('mu', _pad(N) * Q).reshape(_pad(N), Q)[:N]
        eng.global_step()
        out['Bbar_image'] = eng.peek('Bbar', Mp * Mp).reshape(Mp, Mp)
        out['Abar_image'] = eng.peek('Abar', Mp * Dp).reshape(Mp, Dp)
        out['Bm'] = eng.peek('Bm', (Mp + Dp) * Mp).reshape(Mp + Dp, Mp)
        out['Bbar'], out['Abar'] = np.ascontiguousarray(out['Bbar_image'][:M, :M]), np.ascontiguousarray(out['Abar_image'][:M, :D])
        eng.phase2(False)
        out['grads'] = eng.peek('grads', M * Q + Q)
        if d['emb']:
            eng.phase2(True)
            out['grads_emb'] = eng.peek('grads', M * Q + Q)
            out['grad_x_mu'], out['grad_x_s'] = eng.download('GRAD_X_MU'), eng.download('GRAD_X_S')
            out['psi1_emb'] = eng.download('PSI1')
            eng.phase2(False)                                            # back to the fixed-embedding features for the next evaluation
        outs.append(out)
    eng.close()
    return outs


def check_case(case, p2_rem=1, p2_sync=True):
    d = F.case_inputs(case)
    N, D, M, Q = shape = (d['N'], d['D'], d['M'], d['Q'])
    fam = F.family(N, D, M, Q, False, p2_rem=p2_rem, p2_sync=p2_sync)
    if d['emb']:
        fam.update({k: v for k, v in F.family(N, D, M, Q, True).items() if k in ('p2',)})
    wrong = {k: (v, fam.get(k)) for k, v in d['family'].items() if fam.get(k) != (v if (k != 'wait' or p2_sync) else False)}
    assert not wrong, '%s is listed for %s: (listed, planned) %s' % (d['name'], d['family'], wrong)
    if p2_sync and p2_rem == (2 if case is F.REM_LONG else 1):
        planned = F.identity(F.family(N, D, M, Q, d['emb'], p2_rem=p2_rem))
        assert planned == F.LISTED[d['name']], '%s is listed for "%s" and runs on "%s"' % (d['name'], F.LISTED[d['name']], planned)
    first, second = run_device(d)
    dev = first
    Mp, Dp = _pad(M), _pad(D)
    st = dev['stats']
    P2, C = st[:Mp * Mp].reshape(Mp, Mp), st[Mp * Mp:Mp * Mp + Mp * Dp].reshape(Mp, Dp)
    sc = st[Mp * Mp + Mp * Dp:]
    bad = []
    zc, mc, _ = F.centred(d['Z'], d['X_mu'])
    if not (np.array_equal(zc, dev['zc']) and np.array_equal(mc, dev['mc'])):
        bad.append('the centred coordinates are not the host\'s bit for bit')
    if not np.array_equal(dev['psi2_sum'], dev['psi2_sum'].T):
        bad.append('Psi2 is not symmetric bit for bit')
    if not (np.array_equal(P2[:M, :M], dev['psi2_sum']) and np.array_equal(C[:M, :D], dev['psi1ty'])):
        bad.append('the downloads are not the windows of the statistics image')
    for what, img, r, c in (('Psi2', P2, M, M), ('C', C, M, D)):
        if np.any(img[r:, :] != 0.0) or np.any(img[:, c:] != 0.0) or not np.all(np.isfinite(img)):
            bad.append('the padding of %s in the statistics image is not exact zero' % what)
    if sc[F.SC_NLOCAL] != float(N) or np.any(sc[4:] != 0.0):
        bad.append('the scalar slots: n = %r, spare %r' % (sc[F.SC_NLOCAL], sc[4:]))
    assert np.all(np.isfinite(dev['Bbar'])) and np.all(np.isfinite(dev['Abar'])), 'the global step failed: its accuracy is not under test, its success is'
    Bm = dev['Bm']
    if not (np.array_equal(Bm[:Mp], 2.0 * dev['Bbar_image']) and np.array_equal(Bm[Mp:], dev['Abar_image'].T)):
        bad.append('the Bm image is not [2 Bbar ; Abar^T] bit for bit')
    if np.any(dev['Bbar_image'][M:, :] != 0.0) or np.any(dev['Bbar_image'][:, M:] != 0.0) or np.any(dev['Abar_image'][M:, :] != 0.0) or np.any(dev['Abar_image'][:, D:] != 0.0):
        bad.append('the padding of the Bbar / Abar images is not exact zero')
    if d['emb'] and not np.array_equal(dev['psi1'], dev['psi1_emb']):
        bad.append('Psi1 of phase2(True) differs from phase 1\'s')
    ref = reference(d, dev)
    got = dict(psi1=dev['psi1'], psi2_sum=dev['psi2_sum'], psi1ty=dev['psi1ty'], psi0=sc[F.SC_PSI0], sum_yyt=sc[F.SC_SUM_YYT], kl=sc[F.SC_KL],
               grad_z_data=dev['grads'][:M * Q].reshape(M, Q), grad_alpha_data=dev['grads'][M * Q:])
    bad += [b for b in _hold(d['name'], got, ref, shape)]
    if d['emb']:
        got = dict(grad_z_data=dev['grads_emb'][:M * Q].reshape(M, Q), grad_alpha_data=dev['grads_emb'][M * Q:], grad_x_mu=dev['grad_x_mu'],
                   grad_x_s=dev['grad_x_s'])
        bad += _hold(d['name'] + ' phase2(True)', got, ref, shape)
        if np.any(dev['grad_x_s'] != 0.0):
            bad.append('grad_x_s of a fixed-embedding shard is not exact zero')
    if d['name'].endswith('_far'):
        for k in ('psi1', 'psi2_sum', 'psi1ty', 'grads') + (('grads_emb',) if d['emb'] else ()):
            if np.any(dev[k] != 0.0):
                bad.append('far field: %s is not exact zero' % k)
    for k in first:
        if not np.array_equal(first[k], second[k], equal_nan=True):
            bad.append('%s of a second evaluation on the same context differs' % k)
    assert not bad, '%s: %s' % (d['name'], '; '.join(bad))


def _hold(what, got, ref, shape):
    psi1 = {k: got.pop(k) for k in ('psi1',) if k in got}
    bad = F.hold(what, got, ref, shape)
    if psi1:                                                            # compat_ref's own bound for the same inputs: one term, n_terms 1
        v, A, T = ref['psi1']
        ratio, idx = R.worst(psi1['psi1'], v, A, T, 1)
        print('[fixed elementwise] %-30s %-16s worst error / bound %.3g at %s' % (what, 'psi1', ratio, idx))
        if not ratio <= 1.0:
            bad.append('psi1: %.3g times compat_ref\'s bound at %s' % (ratio, idx))
    return bad


def run_case_list(cases, **kw):
    for case in cases:
        check_case(case, **kw)


def _lib():
    from gparml_amd import _lib as L
    return L.load()


@pytest.mark.parametrize('case', F.CASES, ids=F.CASE_NAMES)
def test_both_phases_elementwise(case):
    check_case(case)


@pytest.mark.parametrize('mode', [0, 2])
def test_remainder_option(mode):
    """The MT = 2 remainder case at the other values of gp_debug_set_option('p2_rem', .): 0 the whole-tile plan (family: no remainder, tps = 2),
    2 the hard limits only (the same plan as 1 here); value 1 is the default list's run."""
    assert _lib().gp_debug_set_option(b'p2_rem', mode) == 0
    try:
        name, N, D, M, Q, emb, fam = F.REM_CASE
        listed = dict(fam, rem=None, tps=2, S=130) if mode == 0 else fam
        check_case((name, N, D, M, Q, emb, listed), p2_rem=mode)
    finally:
        _lib().gp_debug_set_option(b'p2_rem', 1)


def test_remainder_of_all_but_one_slice():
    """r = S - 1 at MT = 1: 511 remainder row tiles, one split each; the default ratio limit refuses it, value 2 of the option runs it."""
    assert _lib().gp_debug_set_option(b'p2_rem', 2) == 0
    try:
        check_case(F.REM_LONG, p2_rem=2)
    finally:
        _lib().gp_debug_set_option(b'p2_rem', 1)


CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from gparml_amd import _lib
assert _lib.load().gp_debug_set_option(b'poison_alloc', %(poison)d) == 0
import fixed_ref as F
import test_gpu_fixed_elementwise as t
t.run_case_list(%(cases)s, p2_sync=%(sync)r)
print('FIXED_CHILD_OK', flush=True)
'''


def _child(tmp_path, tag, cases_expr, cases, env, poison=0, sync=True, timeout=600):
    """The cases in a fresh process (GPARML_P2_SYNC and the poison mode are read once per process).  The references come from this process, as files,
    for the K, Bbar and Abar a default-mode evaluation gives here (neither switch reaches Psi1 or the global step; the child computes its own where
    its inputs differ in a bit)."""
    refs = tmp_path / ('refs_' + tag)
    refs.mkdir()
    for case in cases:
        d = F.case_inputs(case)
        if d['name'] not in _REFS:
            reference(d, run_device(d, evaluations=1)[0])
        save_reference(str(refs / (d['name'] + '.npz')), d['name'])
    script = tmp_path / ('fixed_child_%s.py' % tag)
    script.write_text(CHILD % {'root': ROOT, 'tests': os.path.join(ROOT, 'tests'), 'poison': poison, 'cases': cases_expr, 'sync': sync})
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=timeout, cwd=ROOT,
                       env=dict(os.environ, FIXED_REF_DIR=str(refs), **env))
    print(r.stdout[-30000:])
    assert r.returncode == 0 and 'FIXED_CHILD_OK' in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_free_running_form(tmp_path):
    """p2_fast8_kernel without the in-step wait where the default has it on: the MT >= 2 cases again under GPARML_P2_SYNC=0."""
    _child(tmp_path, 'nosync', 'F.WAIT_CASES', F.WAIT_CASES, {'GPARML_P2_SYNC': '0'}, sync=False, timeout=300)


def test_case_list_with_poisoned_allocations(tmp_path):
    """The default-mode case list once more in a fresh process under the poison mode: an element a kernel leaves unwritten, or a padding entry it reads
    and should not, shows up as NaN (ratio inf), not as a stale value."""
    _child(tmp_path, 'poison', 'F.CASES', F.CASES, {'GPARML_POISON': '1'}, poison=1, timeout=600)
