"""tests/compat_ref.py on the CPU: the long-double reference reproduces the goldens captured from the imported reference (so it is pinned to that,
not to this library) and oracle/literal.py at two fresh shapes; a float64 mirror of the same formulas, summed over the points in ascending order
as the kernels do, stays inside the bound of compat_ref's docstring WITHOUT its factor 2 at every case of the GPU test (the bound is neither
vacuous nor too tight for an honest float64 implementation); the far-field case really reaches the tail of exp."""
import numpy as np
import pytest

import compat_ref as R
from conftest import assert_close, golden_names, load_golden

pytestmark = pytest.mark.skipif(not R.available(), reason='numpy long double has no 64-bit significand here')

GOLDEN_KEY = dict(psi1='exp_K_mi', kmm='Kmm', psi2_points='exp_K_mi_K_im', dkmm_dz='dKmm_dZ', dkmm_dalpha='dKmm_dalpha', dpsi1ty_dz='dexp_K_miY_dZ',
                  dpsi1ty_dalpha='dexp_K_miY_dalpha', dpsi2_dz='dexp_K_mi_K_im_dZ', dpsi2_dalpha='dexp_K_mi_K_im_dalpha')


def _f64(x):
    return np.asarray(x, dtype=np.float64)


@pytest.mark.parametrize('name', golden_names())
def test_reference_reproduces_the_goldens(name):
    inp, ref = load_golden(name)
    args = R.to_ld(inp['Z'], inp['sf2'], inp['alpha'], inp['X_mu'], inp['X_S'], inp['Y'].reshape(inp['X_mu'].shape[0], -1))
    got = R.all_arrays(*args)
    for k in R.ARRAYS:
        assert_close(_f64(got[k][0]), ref[GOLDEN_KEY[k]], 1e-12, what=k)
        single = getattr(R, k)(*args)                    # the public function of the array: the same value and A as the shared pass
        assert len(single) == 2 and np.array_equal(single[0], got[k][0]) and np.array_equal(single[1], got[k][1])
    parts = R.to_ld(ref['dF_dKmm'], ref['dKmm_dZ'], ref['dF_dexp_K_miY'], ref['dexp_K_miY_dZ'], ref['dF_dexp_K_mi_K_im'], ref['dexp_K_mi_K_im_dZ'])
    assert_close(_f64(R.grad_z_from_parts(*parts)[0]), ref['grad_Z'], 1e-12, what='grad_Z(parts)')
    parts = R.to_ld(ref['dF_dKmm'], ref['dKmm_dalpha'], ref['dF_dexp_K_miY'], ref['dexp_K_miY_dalpha'], ref['dF_dexp_K_mi_K_im'],
                    ref['dexp_K_mi_K_im_dalpha'])
    assert_close(_f64(R.grad_alpha_from_parts(*parts)[0]), ref['grad_alpha'], 1e-12, what='grad_alpha(parts)')


def test_grad_z_from_parts_counts_the_diagonal_once():
    """partial_terms.py:226-231 writes row j and column j of one (M, M) mask: entry (j, j) is written twice and summed once.  For the true
    dKmm_dZ that entry is zero; for arbitrary parts it is not."""
    rs = np.random.RandomState(3)
    M, Q, D = 5, 2, 3
    A, a3, B, b3, C, c3 = rs.randn(M, M), rs.randn(M, Q, M), rs.randn(M, D), rs.randn(M, Q, D), rs.randn(M, M), rs.randn(M, Q, M)
    want = np.zeros((M, Q))
    for j in range(M):
        for k in range(Q):
            mask = np.zeros((M, M))
            mask[j, :] = a3[j, k, :]
            mask[:, j] = a3[j, k, :]
            want[j, k] = np.sum(A * mask) + np.sum(B[j] * b3[j, k]) + 2 * np.sum(C[j] * c3[j, k])
    got, absum = R.grad_z_from_parts(*R.to_ld(A, a3, B, b3, C, c3))
    assert np.max(np.abs(_f64(got) - want)) <= 1e-14 * np.max(_f64(absum))


@pytest.mark.parametrize('N,D,M,Q,regime,alpha', [(23, 3, 11, 17, 'B', 0.1), (19, 2, 7, 70, 'B', 0.05)])
def test_reference_agrees_with_the_literal_oracle(N, D, M, Q, regime, alpha):
    from oracle import factorised as Fz
    from oracle.literal import PartialTermsOracle
    d = Fz.synthetic_shard(N, D, M, Q, regime=regime, seed=31, zseed=32, alpha_value=alpha)
    pt = PartialTermsOracle(d['Z'], d['sf2'], d['alpha'], d['beta'], M, Q, N, D)
    pt.set_data(d['Y'], d['X_mu'], d['X_S'], True)
    got = R.all_arrays(*R.to_ld(d['Z'], d['sf2'], d['alpha'], d['X_mu'], d['X_S'], d['Y']))
    want = dict(psi1=pt.exp_K_mi, kmm=pt.Kmm, psi2_points=pt.exp_K_mi_K_im, dkmm_dz=pt.dKmm_dZ(), dkmm_dalpha=pt.dKmm_dalpha(),
                dpsi1ty_dz=pt.dexp_K_miY_dZ(), dpsi1ty_dalpha=pt.dexp_K_miY_dalpha(), dpsi2_dz=pt.dexp_K_mi_K_im_dZ(),
                dpsi2_dalpha=pt.dexp_K_mi_K_im_dalpha())
    for k in R.ARRAYS:
        assert_close(_f64(got[k][0]), want[k], 1e-12, what=k)
    gZ = R.grad_z_from_parts(*R.to_ld(pt.dF_dKmm(), want['dkmm_dz'], pt.dF_dexp_K_miY(), want['dpsi1ty_dz'], pt.dF_dexp_K_mi_K_im(), want['dpsi2_dz']))[0]
    # (the oracle's einsum counts the diagonal of the Kmm term twice; dKmm_dZ[j, k, j] is zero, so the two agree here)
    assert_close(_f64(gZ), pt.grad_Z(pt.dF_dKmm(), want['dkmm_dz'], pt.dF_dexp_K_miY(), want['dpsi1ty_dz'], pt.dF_dexp_K_mi_K_im(), want['dpsi2_dz']),
                 1e-12, what='grad_Z(parts)')
    ga = R.grad_alpha_from_parts(*R.to_ld(pt.dF_dKmm(), want['dkmm_dalpha'], pt.dF_dexp_K_miY(), want['dpsi1ty_dalpha'], pt.dF_dexp_K_mi_K_im(),
                                          want['dpsi2_dalpha']))[0]
    assert_close(_f64(ga), pt.grad_alpha(pt.dF_dKmm(), want['dkmm_dalpha'], pt.dF_dexp_K_miY(), want['dpsi1ty_dalpha'], pt.dF_dexp_K_mi_K_im(),
                                         want['dpsi2_dalpha']), 1e-12, what='grad_alpha(parts)')


@pytest.mark.parametrize('case', R.CASES, ids=R.CASE_NAMES)
def test_float64_mirror_is_inside_the_bound_without_its_factor(case):
    d = R.case_inputs(case)
    ref = R.all_arrays(*R.inputs_ld(d))
    mirror = R.all_arrays(d['Z'], d['sf2'], d['alpha'], d['X_mu'], d['X_S'], d['Y'])
    bad = []
    for k in R.ARRAYS:
        assert mirror[k][0].dtype == np.float64
        ratio, idx = R.worst(mirror[k][0], *ref[k], R.n_terms(k, d['N']), factor=1.0)
        print('[compat mirror] %-24s %-15s worst error / bound (no factor 2) %.3f at %s' % (d['name'], k, ratio, idx))
        if not ratio <= 1.0:
            bad.append('%s %.3f at %s' % (k, ratio, idx))
    assert not bad, '%s: %s' % (d['name'], '; '.join(bad))


def test_float64_mirror_of_the_parts_contractions():
    rs = np.random.RandomState(17)
    M, Q, D = 130, 17, 129
    zp = [rs.randn(M, M), rs.randn(M, Q, M), rs.randn(M, D), rs.randn(M, Q, D), rs.randn(M, M), rs.randn(M, Q, M)]
    ap = [zp[0], rs.randn(Q, M, M), zp[2], rs.randn(Q, M, D), zp[4], rs.randn(Q, M, M)]
    for fn, parts, nt in ((R.grad_z_from_parts, zp, 2 * M + D), (R.grad_alpha_from_parts, ap, 2 * M * M + M * D)):
        ref = fn(*R.to_ld(*parts), err=True)
        ratio, idx = R.worst(fn(*parts)[0], *ref, nt, factor=1.0)
        print('[compat mirror] %s worst error / bound (no factor 2) %.3f' % (fn.__name__, ratio))
        assert ratio <= 1.0


def test_far_field_case_reaches_the_tail_of_exp():
    d = R.case_inputs(R.CASES[R.CASE_NAMES.index(R.FAR_FIELD)])
    p1 = R.psi1(*R.inputs_ld(d))[0]
    tiny = np.mean((p1 >= 2.0 ** -1022) & (p1 < 1e-280))                 # the last normal decades
    gone = np.mean(np.abs(_f64(p1)) < 2.0 ** -1022)                      # rounds to zero or a subnormal float64
    print('[compat far field] %.1f %% of Psi1 in [2^-1022, 1e-280), %.1f %% zero or subnormal in float64, smallest exponent %.1f'
          % (100 * tiny, 100 * gone, float(np.min(np.log(p1)))))
    assert tiny >= 0.05 and gone >= 0.05
    assert float(np.max(p1)) > 0.1 and float(np.min(np.log(p1))) < -760.0
