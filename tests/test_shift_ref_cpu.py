"""The shift-exact long-double reference (tests/shift_ref.py) checked on the CPU: it agrees with the float64 oracle where the oracle is good (no shift),
it does not move when X_mu and Z are translated together, a plain float64 evaluation through differences stays with it -- and the oracle, which
expands (mu - z)^2 and the coupling term into products of un-differenced coordinates, does not.  The last test restates the device kernels' expanded
pair exponent (csrc/psi2.hip: LEA_nm + LEA_nm' - 2 sum_q V_nq z_mq z_m'q) in float64 and shows its error growing with the square of the shift: the
motive of tests/test_gpu_translation.py, checkable without a GPU."""
import numpy as np
import pytest

import infer_ref
import predict_ref
import shift_ref as R
from oracle import factorised as Fz

LD = np.longdouble
STAT_TOL, GRAD_TOL = 1e-10, 1e-6     # oracle against reference at no shift
STILL = 1e-15                        # the reference against itself across the shifts
F64_DIRECT = 1e-14                   # float64 through differences against the reference

_cache = {}


def _eval(case, c):
    """The reference's evaluation of a case at shift c (computed once per session and left unchanged)."""
    key = (case[0], c)
    if key not in _cache:
        _cache[key] = R.evaluate(R.shifted(R.case_inputs(case), c))
    return _cache[key]


def test_long_double_is_extended():
    assert np.finfo(LD).eps < 2e-19, 'numpy long double is not the 80-bit format here: the reference would be no better than float64'


@pytest.mark.parametrize('case', R.CASES, ids=[c[0] for c in R.CASES])
def test_agrees_with_the_oracle_without_shift(case):
    d = R.case_inputs(case)
    ev = _eval(case, 0.0)
    o = Fz.evaluate(d['Z'], d['sf2'], d['alpha'], d['beta'], d['Y'], d['X_mu'], d['X_S'], pairs='direct')
    st = ev['stats']
    assert R.rel_err(Fz._psi1_chunk(d['Z'], d['sf2'], d['alpha'], d['X_mu'], d['X_S'])[0], st['Psi1']) <= STAT_TOL
    assert R.rel_err(o['stats']['sum_exp_K_mi_K_im'], st['Psi2']) <= STAT_TOL
    assert R.rel_err(o['stats']['exp_K_miY'], st['C']) <= STAT_TOL
    assert R.rel_err(o['stats']['sum_exp_K_ii'], st['Psi0']) <= STAT_TOL
    assert abs(o['stats']['KL'] - st['KL']) <= STAT_TOL * abs(st['KL'])
    assert R.rel_err(o['F'], ev['F']) <= GRAD_TOL
    for k in ('grad_Z', 'grad_alpha', 'grad_sf2', 'grad_beta', 'grad_X_mu') + (('grad_X_S',) if case[5] == 'B' else ()):
        assert R.rel_err(o[k], ev[k]) <= GRAD_TOL, k
    # the conditioning the GPU tests rely on
    assert ev['cond_Kmm'] <= 1e4 and ev['cond_A'] <= 1e4


@pytest.mark.parametrize('case', R.CASES, ids=[c[0] for c in R.CASES])
def test_reference_does_not_move_under_translation(case):
    d0 = R.case_inputs(case)
    e0 = _eval(case, 0.0)
    for c in R.SHIFTS[1:]:
        ec = _eval(case, c)
        for k in ('Psi1', 'Psi2', 'C'):
            assert R.rel_err(ec['stats'][k], e0['stats'][k]) <= STILL, (k, c)
        for k in ('grad_Z', 'grad_alpha', 'grad_sf2', 'grad_beta') + (('grad_X_S',) if case[5] == 'B' else ()):
            assert R.rel_err(ec[k], e0[k]) <= STILL, (k, c)
        # F moves by exactly the mu^2 term of the KL (nothing for fixed embeddings) ...
        dkl = R.kl_shift(d0, c)
        assert abs(ec['stats']['KL'] - (e0['stats']['KL'] + dkl)) <= STILL * abs(ec['stats']['KL'])
        assert abs(ec['F'] + dkl - e0['F']) <= STILL * max(abs(ec['F']), abs(e0['F'])), c
        # ... and grad_X_mu by its derivative -c.  The library (like the reference implementation) keeps that -mu in grad_X_mu with every variance zero as
        # well, so the closed form is the same in both regimes (the block's largest entry is then of the size of c)
        assert R.rel_err(ec['grad_X_mu'] + LD(c), e0['grad_X_mu']) <= STILL * max(1.0, c / float(np.max(np.abs(e0['grad_X_mu'])))), c


@pytest.mark.parametrize('case', R.PREDICT_CASES, ids=[c[0] for c in R.PREDICT_CASES])
def test_predict_and_infer(case):
    """predict / infer_objective agree with tests/predict_ref.py and tests/infer_ref.py at no shift, and move under translation by the KL term only."""
    d0 = R.case_inputs(case)
    base = None
    for c in R.SHIFTS:
        d = R.shifted(d0, c)
        mdl = R.model(d, R.statistics(d))
        outs = [R.predict(mdl, d['Xt']), R.predict(mdl, d['Xt'], d['St'], include_noise=True), R.infer_objective(mdl, d['Yt'], [0, 2], d['Xt'], d['St'])]
        if base is None:
            base = outs
            st = R.statistics(d, np.float64)
            for got, (X_S, noise) in zip(outs[:2], ((None, False), (d['St'], True))):
                m, v = predict_ref.predict(d['Z'], d['sf2'], d['alpha'], d['beta'], st['Psi2'], st['C'], d['Xt'], X_S, noise)
                assert R.rel_err(m, got[0]) <= STAT_TOL and np.max(np.abs(v - got[1])) <= STAT_TOL * d['sf2']
            im = infer_ref.Model(d['Z'], d['sf2'], d['alpha'], d['beta'], st['Psi2'], st['C'])
            for a, b in zip(infer_ref.objective(im, d['Yt'], [0, 2], d['Xt'], d['St']), outs[2]):
                assert R.rel_err(a, b) <= STAT_TOL
            continue
        for k in range(2):
            assert R.rel_err(outs[k][0], base[k][0]) <= STILL and R.rel_err(outs[k][1], base[k][1]) <= STILL, c
        mu0 = np.asarray(d0['Xt'], dtype=LD)
        dkl = LD(c) * mu0.sum(1) + mu0.shape[1] * LD(c) * LD(c) / 2
        assert np.max(np.abs(outs[2][0] + dkl - base[2][0])) <= STILL * float(np.max(np.abs(outs[2][0])))
        assert R.rel_err(outs[2][1] + LD(c), base[2][1]) <= STILL * max(1.0, c / float(np.max(np.abs(base[2][1]))))
        assert R.rel_err(outs[2][2], base[2][2]) <= STILL


F64_CASES = [c for c in R.CASES if c[0] in ('fixed_q3', 'fixed_q64', 'free_q10', 'free_q17', 'free_q64')]


@pytest.mark.parametrize('case', F64_CASES, ids=[c[0] for c in F64_CASES])
def test_float64_through_differences_stays_and_the_oracle_does_not(case):
    d0 = R.case_inputs(case)
    worst = 0.0
    for c in R.SHIFTS:
        d = R.shifted(d0, c)
        ref, f64 = _eval(case, c)['stats'], R.statistics(d, np.float64)
        for k in ('Psi1', 'Psi2', 'C'):
            e = R.rel_err(f64[k], ref[k])
            worst = max(worst, e)
            assert e <= F64_DIRECT, (k, c, e)
    # the float64 oracle at the largest shift: it expands the squares, so it must NOT be taken as the reference of the translation tests
    d = R.shifted(d0, R.SHIFTS[-1])
    o = Fz.phase1(d['Z'], d['sf2'], d['alpha'], d['Y'], d['X_mu'], d['X_S'], pairs='direct')
    e_oracle = R.rel_err(o['sum_exp_K_mi_K_im'], _eval(case, R.SHIFTS[-1])['stats']['Psi2'])
    print('[shift ref] %s: float64 through differences %.2e at worst; oracle Psi2 at shift 2^16: %.2e' % (case[0], worst, e_oracle))
    assert e_oracle > 1e-11


def psi2_expanded_f64(d, offset=None):
    """Psi2 in float64 in the form the free-embedding device kernels use (csrc/psi2.hip): LE from differences, then
    LEA_nm = LE_nm + sum_q V_nq z_mq^2 and the pair exponent LEA_nm + LEA_nm' - 2 sum_q V_nq z_mq z_m'q, V = -(alpha - w) / 4 -- three products of
    un-differenced inducing coordinates.  ``offset`` (Q,) is subtracted from Z and X_mu first: the centring of gp_set_globals."""
    Z, mu, S, a, s2 = d['Z'], d['X_mu'], d['X_S'], d['alpha'], d['sf2']
    if offset is not None:
        Z, mu = Z - offset, mu - offset
    d2 = 2.0 * a * S + 1.0
    w = a / d2
    V = -0.25 * (a - w)
    dd = mu[:, None, :] - Z[None, :, :]
    LE = 0.5 * np.log(s2 * s2 / np.sqrt(np.prod(d2, axis=1)))[:, None] - 0.5 * np.einsum('nq,nmq->nm', w, dd * dd)
    LEA = LE + V.dot((Z * Z).T)
    G = np.matmul(Z[None, :, :] * V[:, None, :], Z.T)
    return np.exp(LEA[:, :, None] + LEA[:, None, :] - 2.0 * G).sum(0)


def test_expanded_pair_exponent_grows_with_the_square_of_the_shift():
    """The CPU model of the finding: the expanded form loses accuracy as c^2, centred coordinates give it back."""
    case = [c for c in R.CASES if c[0] == 'free_q10'][0]
    d0 = R.case_inputs(case)
    errs, centred = [], []
    for c in R.SHIFTS:
        d = R.shifted(d0, c)
        ref = _eval(case, c)['stats']['Psi2']
        errs.append(R.rel_err(psi2_expanded_f64(d), ref))
        centred.append(R.rel_err(psi2_expanded_f64(d, offset=d['Z'].mean(0)), ref))
    print('[shift ref] expanded pair exponent, Psi2 error at shifts 0, 2^6, 2^12, 2^16: %s; centred: %s' % (
        ' '.join('%.1e' % e for e in errs), ' '.join('%.1e' % e for e in centred)))
    assert errs[0] <= 1e-13 and max(centred) <= 1e-13
    assert errs[2] > 1e-11 and errs[3] > 1e-11                      # beyond the suite's Psi2 bound from 2^12 on
    assert 0.1 * 2.0 ** 8 <= errs[3] / errs[2] <= 10 * 2.0 ** 8     # (2^16 / 2^12)^2 = 2^8, within a factor of ten
