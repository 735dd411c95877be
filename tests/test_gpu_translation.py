"""Translation invariance of every evaluation path on the GPU: X_mu and Z shifted together by c in {0, 2^6, 2^12, 2^16} describe the same problem
(the shift is exact in float64 on the inputs' 2^-24 grid), so every kernel family must meet the suite's usual bounds at every shift -- against
tests/shift_ref.py, the long-double reference that forms each difference first (the float64 oracle expands the squares and degrades with c^2:
tests/test_shift_ref_cpu.py).  One shape per kernel family a width or size switch selects (shift_ref.CASES), well conditioned on purpose
(cond <= 1e4, asserted): what is measured is the rounding of the forms, not the solve.  Each case prints its measured errors (pytest -s);
profiles/translation_invariance.txt holds them."""
import numpy as np
import pytest

import shift_ref as R

pytestmark = pytest.mark.gpu

LD = np.longdouble
TOL = dict(Psi1=1e-12, Psi2=1e-11, C=1e-11, Psi0=1e-12, KL=1e-12, F=1e-6, grad_Z=1e-5, grad_alpha=1e-5, grad_sf2=1e-5, grad_beta=1e-5, grad_X_mu=1e-5,
           grad_X_S=1e-5)
_ids = lambda cases: [c[0] for c in cases]
_shift_id = lambda c: 'c=%g' % c


def _engine(d, emb, phase2=True):
    from gparml_amd.engine import ShardEngine
    eng = ShardEngine(d['N'], d['D'], d['M'], d['Q'])
    eng.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    eng.phase1()
    eng.global_step()
    if phase2:
        eng.phase2(emb)
    return eng


def _report(name, shift, errs):
    """Print every (block, error, bound) of a case, then fail on those beyond their bound."""
    bad = []
    for block, err, tol in errs:
        print('[translation] %-16s shift %-6g %-12s %.3e (bound %.0e)%s' % (name, shift, block, err, tol, '' if err <= tol else '  <-- FAILS'))
        if not err <= tol:
            bad.append('%s %.3e > %.0e' % (block, err, tol))
    assert not bad, '%s at shift %g: %s' % (name, shift, '; '.join(bad))


@pytest.mark.parametrize('shift', R.SHIFTS, ids=_shift_id)
@pytest.mark.parametrize('case', R.CASES, ids=_ids(R.CASES))
def test_evaluation_at_a_shifted_origin(case, shift):
    name, emb = case[0], case[6]
    d = R.shifted(R.case_inputs(case), shift)
    ref = R.evaluate(d)
    assert ref['cond_Kmm'] <= 1e4 and ref['cond_A'] <= 1e4, 'the case is not well conditioned: cond(Kmm) %.2e, cond(Kmm + beta Psi2) %.2e' % (
        ref['cond_Kmm'], ref['cond_A'])
    eng = _engine(d, emb)
    out = eng.finish()
    sc = eng.scalars()
    got = dict(out, Psi1=eng.download('PSI1'), Psi2=eng.download('PSI2_SUM'), C=eng.download('PSI1TY'), Psi0=sc['sum_exp_K_ii'], KL=sc['KL'])
    want = dict(ref, **{k: ref['stats'][k] for k in ('Psi1', 'Psi2', 'C', 'Psi0', 'KL')})
    blocks = ['Psi1', 'Psi2', 'C', 'Psi0', 'KL', 'F', 'grad_Z', 'grad_alpha', 'grad_sf2', 'grad_beta']
    if emb:
        got['grad_X_mu'] = eng.download('GRAD_X_MU')
        blocks.append('grad_X_mu')
        if case[5] == 'B':
            got['grad_X_S'] = eng.download('GRAD_X_S')
            blocks.append('grad_X_S')
    eng.close()
    errs = []
    for k in blocks:
        if k == 'KL' and case[5] == 'A':
            errs.append((k, abs(float(got[k])), 0.0))          # fixed embeddings: exactly zero
        else:
            errs.append((k, R.rel_err(got[k], want[k]), TOL[k]))
    _report(name, shift, errs)


@pytest.mark.parametrize('shift', R.SHIFTS, ids=_shift_id)
@pytest.mark.parametrize('case', R.PREDICT_CASES, ids=_ids(R.PREDICT_CASES))
def test_predict_and_infer_at_a_shifted_origin(case, shift):
    """gp_predict and gp_infer_objective on the shifted model, at the bounds of tests/test_gpu_predictive.py (max(1e-10, 1e-16 cond): 1e-10 here, the
    mean relative to max(1, |mean|), the variance to sf2) and of tests/test_gpu_infer.py (_bounds, from the same tolerance)."""
    name = case[0]
    d = R.shifted(R.case_inputs(case), shift)
    st = R.statistics(d)
    mdl = R.model(d, st)
    eng = _engine(d, False, phase2=False)
    tol = 1e-10
    errs = []
    for X_S, what in ((None, 'det'), (d['St'], 'unc')):
        for noise in (False, True):
            m, v = eng.predict(d['Xt'], X_S, include_noise=noise)
            mr, vr = R.predict(mdl, d['Xt'], X_S, include_noise=noise)
            tag = '%s%s' % (what, '+noise' if noise else '')
            errs.append(('mean ' + tag, float(np.max(np.abs(m - mr))) / max(1.0, float(np.max(np.abs(mr)))), tol))
            errs.append(('var ' + tag, float(np.max(np.abs(v - vr))) / d['sf2'], tol))
    mean = R.predict(mdl, d['Xt'], d['St'])[0]
    span = max(1.0, float(np.max(np.abs(d['Xt'][:, None, :] - d['Z'][None, :, :])))) * max(1.0, float(np.max(d['alpha'])))
    for cols in (None, [0, 2]):
        c = np.arange(d['D']) if cols is None else np.asarray(cols)
        ms, rmax = max(1.0, float(np.max(np.abs(mean[:, c])))), float(np.max(np.abs(d['Yt'][:, c] - mean[:, c])))
        tl = 0.5 * d['beta'] * len(c) * tol * (2 * rmax * ms + d['sf2'])
        tg = 4 * tl * span
        Lr, gmr, gsr = R.infer_objective(mdl, d['Yt'], cols, d['Xt'], d['St'])
        for raw in (False, True):
            xs = np.log(np.expm1(d['St'])) if raw else d['St']
            gsr_ = gsr / (1 + np.exp(-np.asarray(xs, dtype=LD))) if raw else gsr
            Ld, gmd, gsd = eng.infer_objective(d['Yt'], d['Xt'], xs, cols=cols, xs_is_raw=raw)
            gscale = max(1.0, float(np.max(np.abs(gmr))), float(np.max(np.abs(gsr_))))
            tag = '%s%s' % ('all' if cols is None else 'subset', ' raw' if raw else '')
            errs.append(('infer L ' + tag, float(np.max(np.abs(Ld - Lr) - 1e-13 * np.abs(Lr))), tl))
            errs.append(('infer grad ' + tag, float(max(np.max(np.abs(gmd - gmr)), np.max(np.abs(gsd - gsr_)))) - 1e-12 * gscale, tg))
    eng.close()
    _report(name, shift, errs)
