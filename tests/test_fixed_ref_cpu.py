"""tests/fixed_ref.py on the CPU: the reference reproduces oracle/factorised.py and the regime-A goldens from host-computed Psi1 and the oracle's
Bbar, Abar; the float64 mirror stays inside the bound WITHOUT its factor 2 at every case of the GPU test (the three longest at fewer points:
fixed_ref.REDUCED_N); the mirror with ONE (n, m, m') term left out, and separately one (n, d) term, exceeds the full bound in every array the term
enters; family() agrees with hand-checked plans; the two exact-value routes agree."""
import numpy as np
import pytest

import compat_ref as R
import fixed_ref as F
from conftest import assert_close, load_golden

pytestmark = pytest.mark.skipif(not R.available(), reason='numpy long double has no 64-bit significand here')


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _host(d):
    return dict(d, N=d['X_mu'].shape[0], M=d['Z'].shape[0], Q=d['Z'].shape[1])


def _against_oracle(Z, sf2, alpha, beta, Y, X_mu, st=None, Bbar=None, Abar=None):
    from oracle import factorised as Fz
    N, D = Y.shape
    X_S = np.zeros_like(X_mu)
    alpha = np.asarray(alpha, dtype=np.float64).reshape(-1)
    o1 = Fz.phase1(Z, sf2, alpha, Y, X_mu, X_S)
    if Bbar is None:
        gs = Fz.global_step(Z, sf2, alpha, beta, o1, N, D)
        Bbar, Abar = gs['Bbar'], gs['Abar']
    o2 = Fz.phase2(Z, sf2, alpha, Y, X_mu, X_S, Abar, Bbar)
    K = F.host_psi1(dict(Z=Z, X_mu=X_mu, alpha=alpha, sf2=sf2, N=N, M=Z.shape[0], Q=Z.shape[1]))
    zc, mc, o = F.centred(Z, X_mu)
    p1 = F.phase1(K, Y, sf2)
    p2 = F.phase2(K, Y, Bbar, Abar, zc, mc, o, alpha)
    for k, want in (('psi2_sum', o1['sum_exp_K_mi_K_im']), ('psi1ty', o1['exp_K_miY']), ('psi0', o1['sum_exp_K_ii']), ('sum_yyt', o1['sum_YYT'])):
        assert_close(_f64(p1[k][0]), want, 1e-12, what=k)
    assert float(p1['kl'][0]) == 0.0 == o1['KL']
    for k, want in (('grad_z_data', o2['grad_Z_data']), ('grad_alpha_data', o2['grad_alpha_data']), ('grad_x_mu', o2['grad_X_mu'])):
        assert_close(_f64(p2[k][0]), want, 1e-12, what=k)
    assert not np.any(_f64(p2['grad_x_s'][0]))
    return o1


@pytest.mark.parametrize('N,D,M,Q,alpha', [(23, 3, 11, 3, 0.5), (40, 130, 7, 12, 0.3), (19, 2, 5, 70, 0.05)])
def test_reference_agrees_with_the_factorised_oracle(N, D, M, Q, alpha):
    from oracle import factorised as Fz
    d = Fz.synthetic_shard(N, D, M, Q, regime='A', seed=31, zseed=32, alpha_value=alpha)
    _against_oracle(d['Z'], d['sf2'], d['alpha'], d['beta'], d['Y'], d['X_mu'])


@pytest.mark.parametrize('name', ['regimeA_small', 'regimeA_q10'])
def test_reference_reproduces_the_goldens(name):
    """The regime-A goldens (pt_q1_m1 carries positive variances: it is a free-embedding fixture, tests/test_psi2_ref_cpu.py holds it)."""
    inp, ref = load_golden(name)
    N, M = inp['X_mu'].shape[0], inp['M']
    assert not np.any(inp['X_S'])
    Y = inp['Y'].reshape(N, -1)
    Bbar, Abar = ref['dF_dexp_K_mi_K_im'], ref['dF_dexp_K_miY'].reshape(M, -1)
    Bbar = (Bbar + Bbar.T) / 2
    o1 = _against_oracle(inp['Z'], inp['sf2'], inp['alpha'], inp['beta'], Y, inp['X_mu'], Bbar=Bbar, Abar=Abar)
    assert_close(o1['sum_exp_K_mi_K_im'], ref['sum_exp_K_mi_K_im'], 1e-12, what='psi2_sum')
    assert_close(o1['exp_K_miY'], ref['exp_K_miY'].reshape(M, -1), 1e-12, what='psi1ty')


# (N, D, M, Q, emb, p2_rem) -> the entries checked by hand against p1v2.hip, psi.hip and p2_rem.hip (the first five: tests/test_gpu_p2_remainder.py's
# shapes and their r; M = 512, D = 100 is the plan p1v2.hip's header states: 44 F-slices, 60 G-slices)
HAND = [((257 * 128, 100, 512, 10, False, 1), dict(p1='p1v2', NBY=26, cap=512, SF=44, SG=60, p2='fast8', NRB=3, S=128, tps=2, rem=(2, 1), wait=True)),
        ((260 * 128 + 77, 100, 512, 10, False, 1), dict(SF=44, SG=60, S=128, tps=2, rem=(2, 5), wait=True)),
        ((515 * 128, 10, 128, 3, False, 1), dict(NBY=8, cap=256, SF=0, SG=256, NRB=1, S=512, tps=1, rem=(1, 3), wait=False, klast=3)),
        ((258 * 128, 100, 256, 1, False, 1), dict(S=256, tps=1, rem=(1, 2), NRB=1, wait=True)),
        ((258 * 128 + 50, 100, 256, 7, False, 1), dict(S=256, tps=1, rem=(1, 3), NRB=2, wait=True)),
        ((258 * 128 + 50, 100, 256, 7, False, 0), dict(S=130, tps=2, rem=None, wait=True)),
        ((2000, 2, 129, 3, False, 1), dict(cap=256, SF=97, SG=79, S=16, tps=1, rem=None)),
        ((200, 2, 1281, 2, False, 1), dict(cap=256, SF=4, SG=3, MT=11)),
        ((196609, 2, 5, 3, False, 1), dict(cap=512, SG=512, S=512, tps=3, rem=(3, 1), wait=False)),
        ((1023 * 128, 2, 5, 3, False, 1), dict(S=512, tps=2, rem=None)),
        ((1023 * 128, 2, 5, 3, False, 2), dict(S=512, tps=1, rem=(1, 511))),
        ((129, 105, 5, 3, False, 1), dict(p1='tiles', klast=3)),
        ((150, 2, 1409, 2, False, 1), dict(p1='tiles', MT=12, S=2, wait=True)),
        ((150, 2, 5, 12, False, 1), dict(p2='gen8_fixed', wait=False)),
        ((150, 2, 129, 3, True, 1), dict(p2='gen8_points', wait=False, rem=None))]


def test_family_agrees_with_the_hand_checked_plans():
    for (N, D, M, Q, emb, mode), want in HAND:
        f = F.family(N, D, M, Q, emb, p2_rem=mode)
        assert {k: f.get(k) for k in want} == want, (N, D, M, Q, emb, mode, f)
    for c in F.CASES:
        f = F.family(*c[1:6])
        if c[5]:
            f.update(wait=F.family(c[1], c[2], c[3], c[4], False)['wait'] if 'wait' in c[6] else f['wait'])
        assert {k: f.get(k) for k in c[6]} == c[6], (c[0], f)
    assert len(set(F.CASE_NAMES)) == len(F.CASES)


def test_the_two_exact_routes_agree():
    from oracle import factorised as Fz
    # twelve points: the long-double sum is then itself good to 12 * 2^-64 A < 2^-60 A; chunks of five rows, so that the integer sums are added
    d = _host(Fz.synthetic_shard(12, 3, 9, 3, regime='A', seed=5, zseed=6, alpha_value=0.5))
    K = F.host_psi1(d)
    KY = np.concatenate([K, d['Y']], axis=1)
    a, b = F.atb_ld(K, KY), F.atb_exact(K, KY, rows=5)
    assert np.all(np.abs(a - b) <= R.LD(2.0 ** -60) * (np.abs(K).T @ np.abs(KY)))
    p = F.phase1(K, d['Y'], d['sf2'], exact='dd')
    assert np.array_equal(np.concatenate([p['psi2_sum'][0], p['psi1ty'][0]], axis=1), F.atb_exact(K, KY))


_WORST = {}
_EXCESS = {}


@pytest.mark.parametrize('case', list(F.CASES) + [F.REM_LONG], ids=F.CASE_NAMES + [F.REM_LONG[0]])
def test_float64_mirror(case):
    """Inside the bound without its factor 2; with one near-field (n, m, m') term left out, and separately one (n, d) term, outside the full bound
    wherever that term enters."""
    d = F.case_inputs(case, N=F.REDUCED_N.get(case[0]))
    shape = (d['N'], d['D'], d['M'], d['Q'])
    K = F.host_psi1(d)
    Bbar, Abar = F.synthetic_partials(d)
    zc, mc, o = F.centred(d['Z'], d['X_mu'])
    ref = F.phase1(K, d['Y'], d['sf2'])
    ref.update(F.phase2(K, d['Y'], Bbar, Abar, zc, mc, o, d['alpha']))

    def mirror(**kw):
        out = F.phase1(K, d['Y'], d['sf2'], mirror=True, **kw)
        out.update(F.phase2(K, d['Y'], Bbar, Abar, zc, mc, o, d['alpha'], mirror=True, **kw))
        return {k: v[0] for k, v in out.items()}
    got = mirror()
    assert all(np.asarray(v).dtype == np.float64 for v in got.values())
    bad = F.hold(d['name'], got, ref, shape, factor=1.0, tag='fixed mirror')
    assert not bad, '%s: %s' % (d['name'], '; '.join(bad))
    if d['name'].split('_at_')[0].endswith('_far'):
        return          # the far field: every term is exact zero; the case is there for the exact zeros and the floor
    # the terms to leave out: the point and inducing point with the largest Psi1 entry, and of that element of G the largest (n, m') and (n, d)
    # terms -- terms the inputs do not hide
    n, m = (int(i) for i in np.unravel_index(np.argmax(K), K.shape))
    m2 = int(np.argmax(K[n] * np.abs(Bbar[:, m])))
    dd = int(np.argmax(np.abs(d['Y'][n] * Abar[m])))
    seen = {}
    for tag, kw, arrays in (('(n, m, m\')', dict(drop=(n, m, m2)), (('psi2_sum', (m, m2)), ('grad_z_data', m), ('grad_alpha_data', Ellipsis), ('grad_x_mu', n))),
                            ('(n, d)', dict(drop_y=(n, m, dd)), (('psi1ty', (m, dd)), ('grad_z_data', m), ('grad_alpha_data', Ellipsis), ('grad_x_mu', n)))):
        mut = mirror(**kw)
        for k, idx in arrays:
            v, A, T = ref[k]
            r = np.abs(np.asarray(mut[k], dtype=R.LD)[idx] - v[idx]) / R.bound(A[idx], T[idx], F.n_terms(k, *shape))
            seen['%s %s' % (k, tag)] = float(np.max(r))
    _EXCESS[d['name']] = min(seen.values())
    print('[fixed mirror] %-30s one term left out at n = %d, m = %d, m\' = %d, d = %d: smallest error / bound %.3g (%s); smallest so far %.3g'
          % (d['name'], n, m, m2, dd, min(seen.values()), min(seen, key=seen.get), min(_EXCESS.values())))
    # what the largest term does not show: a MEDIAN-size (n, m') term of the same element of G, reported only -- a typical term is far below the largest,
    # and the bound, whose n_terms counts every pair behind an element, does not see all of them (DESIGN.md section 4.2 gives the figures)
    size = K[n] * np.abs(Bbar[:, m])
    mm = int(np.argsort(size)[d['M'] // 2])
    mut = mirror(drop=(n, m, mm))
    med = {}
    for k, idx in (('grad_z_data', m), ('grad_alpha_data', Ellipsis), ('grad_x_mu', n)):
        v, A, T = ref[k]
        med[k] = float(np.max(np.abs(np.asarray(mut[k], dtype=R.LD)[idx] - v[idx]) / R.bound(A[idx], T[idx], F.n_terms(k, *shape))))
    print('[fixed mirror] %-30s a median-size term (m\' = %d, %.3g of the largest) left out: error / bound %s'
          % (d['name'], mm, size[mm] / size[m2] if size[m2] else 0.0, ', '.join('%s %.3g' % kv for kv in sorted(med.items()))))
    assert all(r > 10.0 for r in seen.values()), '%s: leaving out one term stays inside ten bounds: %s' % (d['name'], seen)
