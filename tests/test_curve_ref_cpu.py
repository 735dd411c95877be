"""The curve energy without a device: the ABI surface, and the numpy reference (tests/curve_ref.py) tied to code that already exists -- joint_ref.joint's
covariance, grad_ref.grad_ld's metric tensor, differences of its own energy -- rather than to the new algebra; and the geodesic routine on that reference."""
import numpy as np
import pytest

import curve_ref as CR
import grad_ref as G
import joint_ref as J
import predict_ref as R
from test_joint_cpu import _model

SHAPES = [(5, 1, 1), (16, 2, 3), (33, 5, 4)]
N_CURVES, T_POINTS = 2, 5
EPS = np.finfo(float).eps

# Central differences of the long-double energy (unit roundoff u = 5.4e-20), as tests/test_grad_ref_cpu.py takes them for jac: with the step h the
# truncation is h^2 / 6 times a third derivative (O(alpha^(3/2)) <= 1 times the function's scale here) and the rounding u / h times the scale, 1.7e-11
# and 5.4e-15 at h = 1e-5 (achieved, relative to the largest gradient component: 3.5e-11 .. 1.2e-10).
H_LD = 1e-5
TOL_LD = 1e-8


def _setup(M, Q, D):
    N = max(300, M + 100)
    d = _model(N, D, M, Q, 'B' if Q > 1 else 'A', seed=M + Q + D)
    Psi2, C = R.statistics(d['Z'], d['sf2'], d['alpha'], d['Y'], d['X_mu'], d['X_S'])
    X = np.random.RandomState(11).randn(N_CURVES, T_POINTS, Q)
    return d, (d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2, C), X


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), np.finfo(float).tiny))


def test_lib_binds_gp_curve_energy_and_the_library_exports_it():
    import ctypes
    import os
    import __graft_entry__ as ge
    from conftest import ROOT
    from gparml_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'gparml_hip.h')).read()
    assert 'int gp_curve_energy(gp_ctx* ctx, int64_t n_curves, int T, const double* X' in src
    assert 'gp_curve_energy' in _lib.SIGNATURES and len(_lib.SIGNATURES['gp_curve_energy'][1]) == 8
    ge.build()
    lib = ctypes.CDLL(os.path.join(ROOT, 'gparml_amd', 'libgparml_hip.so'))
    assert hasattr(lib, 'gp_curve_energy'), 'the library does not export gp_curve_energy'


@pytest.mark.parametrize('M,Q,D', SHAPES)
def test_seg_is_the_twice_differenced_joint_posterior(M, Q, D):
    """seg_s = |mean_{s+1} - mean_s|^2 + D (c_ss + c_{s+1,s+1} - 2 c_{s,s+1}) from joint_ref.joint (float64) at the curve's points.  That form
    cancels: joint's covariance carries the project's float64 error rule, tol = max(1e-10, 1e-16 cond) of sf2 per element (four elements per
    segment, D outputs), its mean the same of max(1, |mean|) per element (two elements per output, each times 2 |dmean_d|).  Allowed:
    4 D tol sf2 + 4 tol max(1, |mean|) sum_d |dmean_d|.  Printed: the largest deviation as a multiple of eps D (c_ss + c_{s+1,s+1}), the rounding unit
    of the cancelling form (its relative size is that multiple times eps D (c_ss + c_{s+1,s+1}) / e_s).  Achieved: 750 .. 5.9e5 units, 1e-4 .. 7e-3 of
    what is allowed."""
    d, args, X = _setup(M, Q, D)
    tol = J.cond_tol(d['Z'], d['sf2'], d['alpha'], d['beta'], args[4])
    seg = np.asarray(CR.curve_ld(*args, X)['seg'], dtype=float)
    worst_units, worst_share = 0.0, 0.0
    for c in range(N_CURVES):
        mean, cov = J.joint(*args, X[c])
        dm = mean[1:] - mean[:-1]
        cd = np.diag(cov)
        form = np.sum(dm * dm, axis=1) + D * (cd[:-1] + cd[1:] - 2 * np.diag(cov, 1))
        allowed = 4 * D * tol * d['sf2'] + 4 * tol * max(1.0, np.max(np.abs(mean))) * np.sum(np.abs(dm), axis=1)
        dev = np.abs(seg[c] - form)
        units = dev / (EPS * D * (cd[:-1] + cd[1:]))
        worst_units, worst_share = max(worst_units, float(np.max(units))), max(worst_share, float(np.max(dev / allowed)))
        assert np.all(dev <= allowed), (c, dev, allowed)
        assert np.all(seg[c] > 0)
    print('seg against the joint covariance: %.3g units of eps D (c_ss + c_tt); %.3g of the allowed deviation (tol %.3g)' % (worst_units, worst_share, tol))


@pytest.mark.parametrize('M,Q,D', SHAPES)
def test_grad_is_the_central_difference_of_the_energy(M, Q, D):
    """h = 1e-5 in long double; all 2 T Q displaced curves of a curve go through curve_ld as one batch.  Achieved (curve_ld; the float64 curve against the
    same differences in brackets): (5,1,1) 1.2e-10 (1.4e-10); (16,2,3) 6.5e-11 (6.5e-11); (33,5,4) 3.5e-11 (3.5e-11), against 1e-8."""
    d, args, X = _setup(M, Q, D)
    g, g64 = CR.curve_ld(*args, X)['grad'], CR.curve(*args, X)['grad']
    fd = np.zeros((N_CURVES, T_POINTS, Q), dtype=R.LD)
    h = R.LD(H_LD)
    for c in range(N_CURVES):
        batch = np.repeat(X[c].astype(R.LD)[None], 2 * T_POINTS * Q, axis=0).reshape(2, T_POINTS, Q, T_POINTS, Q)
        for t in range(T_POINTS):
            for q in range(Q):
                batch[0, t, q, t, q] += h
                batch[1, t, q, t, q] -= h
        e = CR.curve_ld(*args, batch.reshape(-1, T_POINTS, Q))['energy'].reshape(2, T_POINTS, Q)
        fd[c] = (e[0] - e[1]) / (2 * h)
    errs = [_rel(g, fd), _rel(g64, fd)]
    print('grad %.3g (float64 form: %.3g), tol %.3g' % (errs[0], errs[1], TOL_LD))
    assert max(errs) <= TOL_LD, errs


@pytest.mark.parametrize('M,Q,D', SHAPES)
def test_a_fine_segment_is_the_metric_at_its_midpoint_to_second_order(M, Q, D):
    """e / (dx^T metric(x_mid) dx) -> 1 with a defect of second order in |dx|: halving the step divides the defect by 4 (long double: no rounding in
    the way).  Steps of 2^-5 and 2^-6 length scales.  Achieved defects 3.4e-5 .. 3.3e-4 at the larger step and ratios 3.997 .. 3.999."""
    d, args, X = _setup(M, Q, D)
    mid = X[:, 0, :]
    u = np.random.RandomState(5).randn(N_CURVES, Q)
    u /= np.sqrt(np.sum(d['alpha'] * u * u, axis=1))[:, None]            # one length scale long
    metric = G.grad_ld(*args, mid)['metric']
    defect = []
    for step in (2.0 ** -5, 2.0 ** -6):
        dx = (step * u).astype(R.LD)
        seg = CR.curve_ld(*args, np.stack([mid - dx / 2, mid + dx / 2], axis=1))['seg'][:, 0]
        defect.append(np.abs(seg / np.einsum('iq,iqr,ir->i', dx, metric, dx) - 1))
    ratio = defect[0] / defect[1]
    print('defect %s -> %s, ratio %s' % (np.asarray(defect[0], dtype=float), np.asarray(defect[1], dtype=float), np.asarray(ratio, dtype=float)))
    assert np.all(defect[0] < 1e-2) and np.all(ratio > 3.5) and np.all(ratio < 4.5)


@pytest.mark.parametrize('form', [CR.curve, CR.curve_B, CR.curve_ld], ids=['curve', 'curve_B', 'curve_ld'])
def test_a_repeated_point_gives_a_zero_segment_exactly(form):
    d, args, X = _setup(16, 2, 3)
    X[:, 2] = X[:, 1]
    out = form(*args, X)
    assert np.all(out['seg'][:, 1] == 0) and np.all(out['seg'][:, [0, 2, 3]] > 0)
    assert np.all(np.isfinite(np.asarray(out['grad'], dtype=float))) and np.all(np.isfinite(np.asarray(out['energy'], dtype=float)))


def _far(d, Q, T, rs):
    """A curve 1e3 length scales beyond every inducing point, its points within a length scale of each other."""
    far = np.max(d['Z'], axis=0) + 1e3 / np.sqrt(d['alpha'])
    return far + 0.3 * rs.rand(T, Q) / np.sqrt(d['alpha'])


@pytest.mark.parametrize('M,Q,D', SHAPES)
def test_far_field_is_the_prior(M, Q, D):
    """Far from every inducing point k = 0 exactly and e_s = 2 D (sf2 - kappa_s) within 2 ulp."""
    d, args, _ = _setup(M, Q, D)
    X = _far(d, Q, 6, np.random.RandomState(2))
    out = CR.curve(*args, X)
    dx = X[1:] - X[:-1]
    want = 2 * D * (-(d['sf2'] * np.expm1(-0.5 * np.sum(d['alpha'] * dx * dx, axis=1))))
    assert np.all(np.abs(out['seg'][0] - want) <= 2 * np.spacing(want)), np.max(np.abs(out['seg'][0] - want) / np.spacing(want))
    assert np.all(want > 0)


def test_geodesic_routine_finds_the_straight_line_in_the_far_field():
    """There the energy is D sf2 (T - 1) sum_s (1 - exp(-1/2 |dx_s|^2_alpha)), convex in the interior points while the end points are less than
    a length scale apart, with the equally spaced straight line as its minimiser.  From a perturbed start L-BFGS-B on curve_ref.curve came back to it
    within 1.6e-9 of the end points' distance (largest coordinate deviation; gtol 1e-10, 32 function evaluations); allowed: 10 x that, 1.6e-8."""
    from gparml_amd.predict import minimise_curves, straight_curves
    M, Q, D = 16, 2, 3
    d, args, _ = _setup(M, Q, D)
    rs = np.random.RandomState(4)
    far = np.max(d['Z'], axis=0) + 1e3 / np.sqrt(d['alpha'])
    x0 = far + np.zeros((2, Q))
    x1 = x0 + np.array([[0.6, 0.3], [-0.2, 0.5]]) / np.sqrt(d['alpha'])
    T = 8
    line = straight_curves(x0, x1, T)
    assert np.array_equal(line[:, 0], x0) and np.array_equal(line[:, -1], x1)
    start = line.copy()
    start[:, 1:-1] += 0.1 * rs.randn(2, T - 2, Q) / np.sqrt(d['alpha'])

    def f(X):
        out = CR.curve(*args, X)
        return out['energy'], out['grad']
    got, info = minimise_curves(f, start, iterations=200, gtol=1e-10)
    dist = np.sqrt(np.sum((x1 - x0) ** 2, axis=1))
    err = float(np.max(np.max(np.abs(got - line), axis=(1, 2)) / dist))
    print('geodesic in the far field: %.3g of the distance after %d evaluations (%s), allowed 1.6e-8' % (err, info['evaluations'], info['message']))
    assert np.array_equal(got[:, 0], x0) and np.array_equal(got[:, -1], x1)
    assert np.all(f(got)[0] <= info['energy0']) and np.all(f(got)[0] <= f(line)[0] * (1 + 1e-12))
    assert err <= 1.6e-8, err
