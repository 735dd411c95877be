"""tests/psi2_ref.py on the CPU: the long-double reference of the two free-embedding phases reproduces the goldens captured from the imported
reference (statistics, grad_X_mu, grad_X_S, and the data parts as the contractions of the golden derivative tensors with the golden dF terms) and
oracle/factorised.py at fresh shapes; the float64 mirror of the same formulas stays inside the bound WITHOUT its factor 2 at every case of the GPU
test; and the mirror with ONE (n, m, m') term left out exceeds the full bound in every array that term enters, so the bound is not vacuous at the
sizes chosen."""
import numpy as np
import pytest

import compat_ref as R
import psi2_ref as P
from conftest import assert_close, golden_names, load_golden

pytestmark = pytest.mark.skipif(not R.available(), reason='numpy long double has no 64-bit significand here')


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _free_goldens():
    return [n for n in golden_names() if np.all(load_golden(n)[0]['X_S'] > 0)]


@pytest.mark.parametrize('name', _free_goldens())
def test_reference_reproduces_the_goldens(name):
    inp, ref = load_golden(name)
    N, M, Q = inp['X_mu'].shape[0], inp['M'], inp['Q']
    Y = inp['Y'].reshape(N, -1)
    Bbar, Abar = ref['dF_dexp_K_mi_K_im'], ref['dF_dexp_K_miY'].reshape(M, -1)
    assert np.allclose(Bbar, Bbar.T, rtol=1e-9, atol=1e-12 * np.max(np.abs(Bbar)))
    Bbar = (Bbar + Bbar.T) / 2
    ld = R.to_ld(inp['Z'], inp['sf2'], inp['alpha'], inp['X_mu'], inp['X_S'], Y)
    p1 = P.phase1(*ld)
    assert_close(_f64(p1['psi2_sum'][0]), ref['sum_exp_K_mi_K_im'], 1e-12, what='psi2_sum')
    assert_close(_f64(p1['psi1ty'][0]), ref['exp_K_miY'].reshape(M, -1), 1e-12, what='psi1ty')
    assert_close(float(p1['psi0'][0]), ref['sum_exp_K_ii'], 1e-12, what='psi0')
    assert_close(float(p1['kl'][0]), ref['KL'], 1e-12, what='kl')
    p2 = P.phase2(*ld, *R.to_ld(Bbar, Abar))
    assert_close(_f64(p2['grad_x_mu'][0]), ref['grad_X_mu'], 1e-12, what='grad_x_mu')
    assert_close(_f64(p2['grad_x_s'][0]), ref['grad_X_S'], 1e-12, what='grad_x_s')
    # the data parts: the golden derivative tensors contracted with the golden dF terms (oracle.literal's grad_Z / grad_alpha without the Kmm term)
    gz = np.sum(Abar[:, None, :] * ref['dexp_K_miY_dZ'], axis=2) + 2 * np.sum(Bbar[:, None, :] * ref['dexp_K_mi_K_im_dZ'], axis=2)
    ga = np.sum(Abar[None] * ref['dexp_K_miY_dalpha'], axis=(1, 2)) + np.sum(Bbar[None] * ref['dexp_K_mi_K_im_dalpha'], axis=(1, 2))
    # (the reference's psi2 tensor carries -1/4 sum (Bbar o Psi2)(z - z')^2, which the library leaves to the global step: psi2_ref's docstring)
    dz = inp['Z'][:, None, :] - inp['Z'][None, :, :]
    ga_step = -0.25 * np.einsum('ab,abq->q', Bbar * ref['sum_exp_K_mi_K_im'], dz * dz)
    assert_close(_f64(p2['grad_z_data'][0]), gz, 1e-12, what='grad_z_data')
    assert_close(_f64(p2['grad_alpha_data'][0]) + ga_step, ga, 1e-12, what='grad_alpha_data')


@pytest.mark.parametrize('N,D,M,Q,alpha', [(23, 3, 11, 17, 0.1), (19, 2, 7, 70, 0.05), (30, 130, 5, 4, 0.5)])
def test_reference_agrees_with_the_factorised_oracle(N, D, M, Q, alpha):
    from oracle import factorised as Fz
    d = Fz.synthetic_shard(N, D, M, Q, regime='B', seed=31, zseed=32, alpha_value=alpha)
    st = Fz.phase1(d['Z'], d['sf2'], d['alpha'], d['Y'], d['X_mu'], d['X_S'])
    gs = Fz.global_step(d['Z'], d['sf2'], d['alpha'], d['beta'], st, N, D)
    o2 = Fz.phase2(d['Z'], d['sf2'], d['alpha'], d['Y'], d['X_mu'], d['X_S'], gs['Abar'], gs['Bbar'])
    ld = R.inputs_ld(d)
    p1 = P.phase1(*ld)
    p2 = P.phase2(*ld, *R.to_ld(gs['Bbar'], gs['Abar']))
    for k, want in (('psi2_sum', st['sum_exp_K_mi_K_im']), ('psi1ty', st['exp_K_miY']), ('psi0', st['sum_exp_K_ii']), ('kl', st['KL'])):
        assert_close(_f64(p1[k][0]), want, 1e-12, what=k)
    for k, want in (('grad_z_data', o2['grad_Z_data']), ('grad_alpha_data', o2['grad_alpha_data']), ('grad_x_mu', o2['grad_X_mu']),
                    ('grad_x_s', o2['grad_X_S'])):
        assert_close(_f64(p2[k][0]), want, 1e-12, what=k)


def test_every_case_lands_on_the_family_it_is_listed_for():
    for c in P.CASES:
        assert P.family(c[3], c[4]) == c[6], c[0]
    for c in P.FORCED['GPARML_B_PHASE2=tiles']:
        assert P.family(c[3], c[4], forced_tiles=True) == c[6] and P.family(c[3], c[4]) != 'TILES', c[0]
    for c in P.FORCED['GPARML_B_SYM_MAXQ=10']:
        assert P.family(c[3], c[4], maxq=10) == c[6] == 'COLS' and P.family(c[3], c[4]) == 'SYM', c[0]
    assert len(set(P.CASE_NAMES)) == len(P.CASES)


def _inputs(case):
    d = P.case_inputs(case, N=P.REDUCED_N.get(case[0]))
    Bbar, Abar = P.synthetic_partials(d)
    return d, Bbar, Abar


_CACHE = {}


def _reference(case):
    if case[0] not in _CACHE:
        d, Bbar, Abar = _inputs(case)
        ld = R.inputs_ld(d)
        ref = P.phase1(*ld)
        ref.update(P.phase2(*ld, *R.to_ld(Bbar, Abar)))
        _CACHE.clear()                                       # one case at a time: the two tests of a case run next to each other
        _CACHE[case[0]] = ref
    return _CACHE[case[0]]


def _mirror(d, Bbar, Abar, drop=None):
    args = (d['Z'], d['sf2'], d['alpha'], d['X_mu'], d['X_S'], d['Y'])
    out = P.phase1(*args, drop=drop)
    out.update(P.phase2(*args, Bbar, Abar, drop=drop))
    return {k: v[0] for k, v in out.items()}


@pytest.mark.parametrize('case', P.CASES, ids=P.CASE_NAMES)
def test_float64_mirror(case):
    """Inside the bound without its factor 2; and with one near-field term left out, outside the full bound wherever that term enters."""
    d, Bbar, Abar = _inputs(case)
    ref = _reference(case)
    shape = (d['N'], d['D'], d['M'], d['Q'])
    got = _mirror(d, Bbar, Abar)
    assert all(np.asarray(v).dtype == np.float64 for v in got.values())
    bad = P.hold(d['name'], got, ref, shape, factor=1.0, tag='psi2 mirror')
    assert not bad, '%s: %s' % (d['name'], '; '.join(bad))
    # the term to leave out: a point with positive variances and the two inducing points nearest to it (the same one twice when M = 1)
    n = next(i for i in range(d['N'] // 2, d['N'] // 2 + d['N']) if np.all(d['X_S'][i % d['N']] > 0)) % d['N']
    near = np.argsort(np.sum((d['X_mu'][n] - d['Z']) ** 2, axis=1))
    m, m2 = int(near[0]), int(near[min(1, d['M'] - 1)])
    mut = _mirror(d, Bbar, Abar, drop=(n, m, m2))
    seen = {}
    for k, idx in (('psi2_sum', (m, m2)), ('grad_z_data', m2), ('grad_alpha_data', Ellipsis), ('grad_x_mu', n), ('grad_x_s', n)):
        v, A, T = ref[k]
        r = np.abs(np.asarray(mut[k], dtype=R.LD)[idx] - v[idx]) / R.bound(A[idx], T[idx], P.n_terms(k, *shape))
        seen[k] = float(np.max(r))
    print('[psi2 mirror] %-28s one term (%d, %d, %d) left out: error / bound %s' % (d['name'], n, m, m2, ', '.join('%s %.3g' % kv for kv in seen.items())))
    if d['name'].endswith('_far'):
        return          # the far field: the near pair of the middle point is itself below the floor; the case is there for the floor term
    assert all(r > 1.0 for r in seen.values()), '%s: leaving out one term stays inside the bound: %s' % (d['name'], seen)
