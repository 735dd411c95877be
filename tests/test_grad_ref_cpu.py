"""The predictive derivatives without a device: the ABI surface, and the numpy reference (tests/grad_ref.py) tied to code that already exists --
finite differences of predict_ref.predict_ld and of joint_ref.joint's covariance -- rather than to the new algebra."""
import ctypes
import os
import re

import numpy as np
import pytest

import grad_ref as G
import joint_ref as J
import predict_ref as R
from conftest import ROOT
from test_joint_cpu import _model

SHAPES = [(5, 1, 1), (16, 2, 3), (33, 5, 4)]
N_POINTS = 3

# Central differences of the long-double predictive (unit roundoff u = 5.4e-20): with the step h the truncation is h^2 / 6 times a third derivative
# (O(alpha^(3/2)) <= 1 times the function's scale here) and the rounding u / h times the scale, 1.7e-11 and 5.4e-15 at h = 1e-5 (achieved: 8e-12 .. 2.5e-10).
H_LD = 1e-5
TOL_LD = 1e-8
# Mixed central difference of the float64 covariance, [c(+,+) - c(+,-) - c(-,+) + c(-,-)] / (4 h^2): the rounding is 4 x 2.2e-16 sf2 x (a few units
# for the cancelling Gram products) / (4 h^2), the truncation h^2 / 6 times the fourth derivatives.  h = 2^-11 balances them near 1e-8 .. 1e-7.
H_COV = 2.0 ** -11
TOL_COV = 1e-6


def _setup(M, Q, D):
    N = max(300, M + 100)
    d = _model(N, D, M, Q, 'B' if Q > 1 else 'A', seed=M + Q + D)
    Psi2, C = R.statistics(d['Z'], d['sf2'], d['alpha'], d['Y'], d['X_mu'], d['X_S'])
    X = np.random.RandomState(11).randn(N_POINTS, Q)
    return d, (d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2, C), X


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), np.finfo(float).tiny))


def test_header_declares_gp_predict_grad_and_the_library_exports_it():
    import __graft_entry__ as ge
    from gparml_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'gparml_hip.h')).read()
    m = re.search(r'int\s+gp_predict_grad\s*\(([^)]*)\)\s*;', src)
    assert m, 'gp_predict_grad is not declared in include/gparml_hip.h'
    assert len(m.group(1).split(',')) == 8
    assert 'gp_predict_grad' in _lib.SIGNATURES and len(_lib.SIGNATURES['gp_predict_grad'][1]) == 8
    ge.build()
    lib = ctypes.CDLL(os.path.join(ROOT, 'gparml_amd', 'libgparml_hip.so'))
    assert hasattr(lib, 'gp_predict_grad'), 'the library does not export gp_predict_grad'


@pytest.mark.parametrize('M,Q,D', SHAPES)
def test_jac_and_dvar_are_the_central_differences_of_predict_ld(M, Q, D):
    """h = 1e-5 in long double.  Achieved (jac, dvar; float64 grad against the same differences in brackets): (5,1,1) 5.1e-11, 2.5e-10 (6.3e-11, 2.5e-10);
    (16,2,3) 2.8e-11, 2.2e-11 (3.3e-11, 2.3e-11); (33,5,4) 1.1e-11, 8.4e-12 (1.1e-11, 8.4e-12), against 1e-8."""
    d, args, X = _setup(M, Q, D)
    g, g64 = G.grad_ld(*args, X), G.grad(*args, X)
    jac, dvar = np.zeros((N_POINTS, D, Q), dtype=R.LD), np.zeros((N_POINTS, Q), dtype=R.LD)
    for q in range(Q):
        e = np.zeros(Q, dtype=R.LD)
        e[q] = R.LD(H_LD)
        mp, vp = R.predict_ld(*args, X.astype(R.LD) + e)
        mm, vm = R.predict_ld(*args, X.astype(R.LD) - e)
        jac[:, :, q] = (mp - mm) / (2 * R.LD(H_LD))
        dvar[:, q] = (vp - vm)[:, 0] / (2 * R.LD(H_LD))
    errs = [_rel(g['jac'], jac), _rel(g['dvar'], dvar), _rel(g64['jac'], jac), _rel(g64['dvar'], dvar)]
    print('jac %.3g dvar %.3g (float64 form: %.3g %.3g), tol %.3g' % (tuple(errs) + (TOL_LD,)))
    assert max(errs) <= TOL_LD, errs


@pytest.mark.parametrize('M,Q,D', SHAPES)
def test_metric_minus_jtj_is_d_times_the_mixed_difference_of_the_joint_covariance(M, Q, D):
    """h = 2^-11 in float64, relative to D sf2 max(alpha).  Achieved: (5,1,1) 3.5e-8; (16,2,3) 6.9e-8; (33,5,4) 3.2e-8, against 1e-6."""
    d, args, X = _setup(M, Q, D)
    g = G.grad(*args, X)
    cov_j = g['metric'] - np.einsum('idq,idr->iqr', g['jac'], g['jac'])
    pts = np.concatenate([X[:, None, None, :] + s * H_COV * np.eye(Q)[None, :, None, :] for s in (1.0, -1.0)], axis=2)   # (n, Q, 2, Q): x +- h e_q
    _, c = J.joint(*args, pts.reshape(-1, Q))
    c = c.reshape(N_POINTS, Q, 2, N_POINTS, Q, 2)
    fd = np.empty((N_POINTS, Q, Q))
    for i in range(N_POINTS):
        ci = c[i, :, :, i, :, :]                                           # [q][sign][r][sign]
        fd[i] = (ci[:, 0, :, 0] - ci[:, 0, :, 1] - ci[:, 1, :, 0] + ci[:, 1, :, 1]) / (4 * H_COV ** 2)
    err = float(np.max(np.abs(cov_j - D * fd)) / (D * d['sf2'] * np.max(d['alpha'])))
    print('Cov(J): %.3g (tol %.3g)' % (err, TOL_COV))
    assert err <= TOL_COV, err


@pytest.mark.parametrize('M,Q,D', SHAPES)
def test_the_three_forms_agree(M, Q, D):
    d, args, X = _setup(M, Q, D)
    tol = J.cond_tol(d['Z'], d['sf2'], d['alpha'], d['beta'], args[4])
    ref = G.grad_ld(*args, X)
    for form in (G.grad, G.grad_B):
        got = form(*args, X)
        for key in ('jac', 'dvar', 'metric', 'logdet'):
            err = float(np.max(np.abs(got[key] - ref[key])) / max(1.0, float(np.max(np.abs(ref[key])))))
            assert err <= tol, (form.__name__, key, err, tol)
        assert np.max(np.abs(got['metric'] - np.transpose(got['metric'], (0, 2, 1)))) <= 1e-12 * np.max(np.abs(got['metric']))


def test_exact_gp_limit():
    """Z = X, M = N = 40, fixed inputs: the sparse posterior's derivatives are the exact GP's."""
    rs = np.random.RandomState(3)
    X = np.stack(np.meshgrid(np.linspace(-3, 3, 8), np.linspace(-2, 2, 5)), -1).reshape(-1, 2)
    Y = np.sin(X.dot(rs.randn(2, 3))) + 0.1 * rs.randn(40, 3)
    sf2, alpha, beta = 1.3, np.array([0.8, 1.1]), 25.0
    Psi2, C = R.statistics(X, sf2, alpha, Y, X, np.zeros_like(X))
    Xs = rs.uniform(-3, 3, size=(13, 2))
    g = G.grad(X, sf2, alpha, beta, Psi2, C, Xs)
    je, ve = G.exact_gp_grad(X, Y, sf2, alpha, beta, Xs)
    assert np.max(np.abs(g['jac'] - je)) <= 1e-7 * max(1.0, np.max(np.abs(je)))
    assert np.max(np.abs(g['dvar'] - ve)) <= 1e-7 * sf2
