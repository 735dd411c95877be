"""The free-embedding (regime B) kernels of both phases against tests/psi2_ref.py, element by element: psi2_pairs_kernel, psi2_pairs_mfma_kernel, the
generic path and their reduces in phase 1; psi2_cols_kernel, psi2_sym_kernel, psi2_tile_kernel, the generic path, bbar_interleave_kernel,
pt2_points_finish_kernel and the pb2 reduces in phase 2.  The global step is taken out of the comparison: the device's own Bbar and Abar
(gp_debug_peek) are the exact float64 inputs of the phase-2 reference, so every output is a plain sum of products of exponentials and is held to
|dev - ref| <= 2 (T + n_terms u A) + 2^-1022 with the long-double value and the derived A, T of psi2_ref's docstring -- about eight orders of magnitude
below the 1e-5 of a block's largest entry that the parity tests can ask for behind the global step.  One case per launch shape (psi2_ref.CASES), the
forced modes in one child process per setting, the whole default list once more under the poison mode.  Each case prints its worst error / bound per
array (pytest -s); DESIGN.md section 4.2 holds them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import compat_ref as R
import psi2_ref as P
from conftest import ROOT

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.available(), reason='numpy long double has no 64-bit significand here')]

_REFS = {}
SC_COUNT, SC_PSI0, SC_KL = 8, 1, 2           # csrc/gp_common.h: the scalars behind Psi2 and C in the statistics buffer


def _pad(n):
    return (n + 127) // 128 * 128


def _load(path):
    z = np.load(path)
    out = {k: (z[k + '_v'], z[k + '_A'], z[k + '_T']) for k in P.PHASE1 + (P.PHASE2 if 'Bbar' in z.files else ())}
    return out, (z['Bbar'], z['Abar']) if 'Bbar' in z.files else None


def save_reference(path, ref, partials):
    arrays = {k + s: np.asarray(ref[k][i]) for k in ref for i, s in enumerate(('_v', '_A', '_T'))}
    if partials is not None:
        arrays.update(Bbar=partials[0], Abar=partials[1])
    np.savez(path, **arrays)


def reference(d, Bbar=None, Abar=None):
    """{array: (value, A, T)} of the case ``d`` in long double: phase 1 once per case and process, phase 2 once per (case, Bbar, Abar) -- the device's
    partials are bit-identical from run to run, so the tests of a case share it.  With PSI2_REF_DIR set (a child process) both come from the files
    the parent left there, phase 2 only if the partials are the parent's bit for bit."""
    name = d['name']
    cache = os.environ.get('PSI2_REF_DIR')
    if name not in _REFS:
        path = os.path.join(cache, name + '.npz') if cache else None
        if path and os.path.exists(path):
            ref, partials = _load(path)
            _REFS[name] = [{k: ref[k] for k in P.PHASE1}, partials, {k: ref[k] for k in P.PHASE2} if partials else None]
        else:
            _REFS[name] = [P.phase1(*R.inputs_ld(d)), None, None]
    slot = _REFS[name]
    if Bbar is None:
        return slot[0]
    if slot[1] is None or not (np.array_equal(slot[1][0], Bbar) and np.array_equal(slot[1][1], Abar)):
        slot[1] = (Bbar.copy(), Abar.copy())
        slot[2] = P.phase2(*R.inputs_ld(d), *R.to_ld(Bbar, Abar))
    return slot[2]


def run_device(d):
    """One evaluation stage by stage; everything the checks need, as host arrays."""
    from gparml_amd.engine import ShardEngine
    N, D, M, Q = d['N'], d['D'], d['M'], d['Q']
    Mp, Dp = _pad(M), _pad(D)
    eng = ShardEngine(N, D, M, Q)
    eng.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    eng.phase1()
    out = dict(psi2_sum=eng.download('PSI2_SUM'), psi1ty=eng.download('PSI1TY'), stats=eng.peek('stats', Mp * Mp + Mp * Dp + SC_COUNT))
    eng.global_step()
    out['Bbar_image'] = eng.peek('Bbar', Mp * Mp).reshape(Mp, Mp)
    out['Abar_image'] = eng.peek('Abar', Mp * Dp).reshape(Mp, Dp)
    out['Bbar'], out['Abar'] = np.ascontiguousarray(out['Bbar_image'][:M, :M]), np.ascontiguousarray(out['Abar_image'][:M, :D])
    assert np.array_equal(out['Bbar'], eng.download('DF_DPSI2')) and np.array_equal(out['Abar'], eng.download('DF_DPSI1TY')), 'the windows of the padded images'
    eng.phase2(True)
    out['grads'] = eng.peek('grads', M * Q + Q)
    out['grad_x_mu'], out['grad_x_s'] = eng.download('GRAD_X_MU'), eng.download('GRAD_X_S')
    eng.phase2(False)
    out['grads_no_emb'] = eng.peek('grads', M * Q + Q)
    eng.close()
    return out


def check_case(case, forced_tiles=False, maxq=12):
    d = P.case_inputs(case)
    N, D, M, Q = shape = (d['N'], d['D'], d['M'], d['Q'])
    # the family the case is listed for, by choose_b_path's rule (psi2_ref.family restates csrc/psi2.hip:733-754: no query reports the plan)
    assert P.family(M, Q, forced_tiles, maxq) == d['family'], '%s runs on %s' % (d['name'], P.family(M, Q, forced_tiles, maxq))
    dev = run_device(d)
    Mp, Dp = _pad(M), _pad(D)
    st = dev['stats']
    P2, C = st[:Mp * Mp].reshape(Mp, Mp), st[Mp * Mp:Mp * Mp + Mp * Dp].reshape(Mp, Dp)
    sc = st[Mp * Mp + Mp * Dp:]
    bad = []
    if not np.array_equal(dev['psi2_sum'], dev['psi2_sum'].T):
        bad.append('Psi2 is not symmetric bit for bit')
    if not (np.array_equal(P2[:M, :M], dev['psi2_sum']) and np.array_equal(C[:M, :D], dev['psi1ty'])):
        bad.append('the downloads are not the windows of the statistics image')
    for what, img, r, c in (('Psi2', P2, M, M), ('C', C, M, D)):
        if np.any(img[r:, :] != 0.0) or np.any(img[:, c:] != 0.0) or not np.all(np.isfinite(img)):
            bad.append('the padding of %s in the statistics image is not exact zero' % what)
    ref = dict(reference(d))
    ref.update(reference(d, dev['Bbar'], dev['Abar']))
    got = dict(psi2_sum=dev['psi2_sum'], psi1ty=dev['psi1ty'], psi0=sc[SC_PSI0], kl=sc[SC_KL], grad_z_data=dev['grads'][:M * Q].reshape(M, Q),
               grad_alpha_data=dev['grads'][M * Q:], grad_x_mu=dev['grad_x_mu'], grad_x_s=dev['grad_x_s'])
    bad += P.hold(d['name'], got, ref, shape)
    no_emb = dict(grad_z_data=dev['grads_no_emb'][:M * Q].reshape(M, Q), grad_alpha_data=dev['grads_no_emb'][M * Q:])
    bad += P.hold(d['name'] + ' phase2(False)', no_emb, ref, shape)
    assert not bad, '%s: %s' % (d['name'], '; '.join(bad))


def run_case_list(cases, **kw):
    for case in cases:
        check_case(case, **kw)


@pytest.mark.parametrize('case', P.CASES, ids=P.CASE_NAMES)
def test_both_phases_elementwise(case):
    check_case(case)


def test_zero_variances_among_free_rows_are_refused():
    """Rows with S = 0 among free ones: the KL term and grad_X_S of such a row are infinite (log 0 and 1 / S, partial_terms.py:85, 421-427).  The library
    does not compute on them: the upload fails with the reference's floating-point error, and the context still takes a proper shard afterwards."""
    from gparml_amd.engine import ShardEngine
    d = P.case_inputs(P.CASES[P.CASE_NAMES.index('cols_n62_d2_m33_q5')])
    S0 = d['X_S'].copy()
    S0[[3, 17, 44]] = 0.0
    eng = ShardEngine(d['N'], d['D'], d['M'], d['Q'])
    with pytest.raises(FloatingPointError):
        eng.upload_shard(d['Y'], d['X_mu'], S0)
    eng.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    eng.phase1()
    ref = reference(d)
    bad = P.hold(d['name'] + ' after the refusal', dict(psi2_sum=eng.download('PSI2_SUM'), psi1ty=eng.download('PSI1TY')), ref, (d['N'], d['D'], d['M'], d['Q']))
    eng.close()
    assert not bad, '; '.join(bad)


CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from gparml_amd import _lib
assert _lib.load().gp_debug_set_option(b'poison_alloc', %(poison)d) == 0
import psi2_ref as P
import test_gpu_psi2_elementwise as t
t.run_case_list(%(cases)s, forced_tiles=%(tiles)r, maxq=%(maxq)d)
print('PSI2_CHILD_OK', flush=True)
'''


def _child(tmp_path, tag, cases_expr, cases, env, poison=0, tiles=False, maxq=12, timeout=600):
    """The cases in a fresh process (the forced modes and the poison mode are read once per process).  The references come from this process, as
    files: phase 1 from the inputs, phase 2 for the partials a default-mode evaluation of the same inputs gives here (neither switch reaches phase 1
    or the global step; the child computes its own where its partials differ in a bit)."""
    refs = tmp_path / ('refs_' + tag)
    refs.mkdir()
    for case in cases:
        d = P.case_inputs(case)
        if _REFS.get(d['name'], [None, None, None])[2] is None:
            dev = run_device(d)
            reference(d, dev['Bbar'], dev['Abar'])
        ref = dict(reference(d))
        slot = _REFS[d['name']]
        ref.update(slot[2])
        save_reference(str(refs / (d['name'] + '.npz')), ref, slot[1])
    script = tmp_path / ('psi2_child_%s.py' % tag)
    script.write_text(CHILD % {'root': ROOT, 'tests': os.path.join(ROOT, 'tests'), 'poison': poison, 'cases': cases_expr, 'tiles': tiles, 'maxq': maxq})
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=timeout, cwd=ROOT,
                       env=dict(os.environ, PSI2_REF_DIR=str(refs), **env))
    print(r.stdout[-20000:])
    assert r.returncode == 0 and 'PSI2_CHILD_OK' in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_tile_kernel_forced_below_q17(tmp_path):
    key = 'GPARML_B_PHASE2=tiles'
    _child(tmp_path, 'tiles', 'P.FORCED[%r]' % key, P.FORCED[key], {'GPARML_B_PHASE2': 'tiles'}, tiles=True)


def test_column_kernel_where_the_symmetric_one_would_run(tmp_path):
    key = 'GPARML_B_SYM_MAXQ=10'
    _child(tmp_path, 'maxq', 'P.FORCED[%r]' % key, P.FORCED[key], {'GPARML_B_SYM_MAXQ': '10'}, maxq=10)


def test_case_list_with_poisoned_allocations(tmp_path):
    """The default-mode case list once more in a fresh process under the poison mode: an element a kernel leaves unwritten, or a padding entry it reads
    and should not, shows up as NaN (ratio inf), not as a stale value."""
    _child(tmp_path, 'poison', 'P.CASES', P.CASES, {'GPARML_POISON': '1'}, poison=1, timeout=900)
