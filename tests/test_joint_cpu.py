"""The joint posterior predictive without a device: the ABI surface and the numpy reference (tests/joint_ref.py) the GPU tests compare against."""
import os
import re

import numpy as np
import pytest

import joint_ref as J
import predict_ref as R
from conftest import ROOT

SHAPES = [(5, 1, 1, 'A', 37), (64, 2, 3, 'B', 129), (130, 17, 3, 'B', 300), (130, 10, 100, 'A', 300), (64, 70, 3, 'B', 129)]


def _model(N, D, M, Q, regime, seed=0, spread=1.5):
    """tests/test_gpu_predictive.py's model: inducing points drawn apart from the data and a lengthscale short enough for cond(Kmm) < 1e6."""
    from oracle import factorised as Fz
    from oracle import literal as L
    d = Fz.synthetic_shard(N, D, M, Q, regime=regime, seed=seed, zseed=seed + 1, alpha_value=min(1.0, 1.0 / Q))
    rs = np.random.RandomState(seed + 7)
    d['Z'] = spread * rs.randn(M, Q)
    a = min(1.0, 1.0 / Q)
    while np.linalg.cond(L.rbf_gram(d['Z'], 1.0, np.full(Q, a))) > 1e6:
        a *= 1.5
    d['alpha'] = np.full(Q, a)
    return d


def test_header_declares_the_joint_entry_points_and_lib_binds_them():
    from gparml_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'gparml_hip.h')).read()
    for name, nargs in (('gp_predict_joint', 6), ('gp_predict_sample', 9)):
        m = re.search(r'int\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m, '%s is not declared in include/gparml_hip.h' % name
        assert len(m.group(1).split(',')) == nargs
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs


@pytest.mark.parametrize('M,Q,D,regime,n', SHAPES)
def test_the_two_forms_agree_and_the_diagonal_is_the_variance(M, Q, D, regime, n):
    N = max(300, M + 100)
    d = _model(N, D, M, Q, regime, seed=M + Q + D)
    Psi2, C = R.statistics(d['Z'], d['sf2'], d['alpha'], d['Y'], d['X_mu'], d['X_S'])
    X = np.random.RandomState(11).randn(n, Q)
    tol = J.cond_tol(d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2)
    args = (d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2, C, X)
    for noise in (False, True):
        m1, c1 = J.joint(*args, include_noise=noise)
        m2, c2 = J.joint_B(*args, include_noise=noise)
        err = np.max(np.abs(c1 - c2)) / d['sf2']
        print('forms differ by %.3g (tol %.3g)' % (err, tol))
        assert err <= tol, (err, tol)
        assert np.array_equal(m1, m2)
        mr, vr = R.predict(d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2, C, X, None, noise)
        assert np.max(np.abs(np.diag(c1) - vr[:, 0])) <= 1e-12 * d['sf2']
        assert np.max(np.abs(m1 - mr)) <= 1e-12 * max(1.0, np.max(np.abs(mr)))
        assert np.max(np.abs(c1 - c1.T)) <= 1e-14 * d['sf2']


def test_exact_gp_limit():
    """Z = X, M = N = 40, fixed inputs: the sparse posterior is the exact GP's, for the whole matrix."""
    rs = np.random.RandomState(3)
    X = np.stack(np.meshgrid(np.linspace(-3, 3, 8), np.linspace(-2, 2, 5)), -1).reshape(-1, 2)
    Y = np.sin(X.dot(rs.randn(2, 3))) + 0.1 * rs.randn(40, 3)
    sf2, alpha, beta = 1.3, np.array([0.8, 1.1]), 25.0
    Psi2, C = R.statistics(X, sf2, alpha, Y, X, np.zeros_like(X))
    Xs = rs.uniform(-3, 3, size=(13, 2))
    m, c = J.joint(X, sf2, alpha, beta, Psi2, C, Xs, include_noise=True)
    me, ce = J.exact_gp_joint(X, Y, sf2, alpha, beta, Xs)
    assert np.max(np.abs(m - me)) <= 1e-7 * max(1.0, np.max(np.abs(me)))
    assert np.max(np.abs(c - ce)) <= 1e-7 * sf2
    _, ve = R.exact_gp(X, Y, sf2, alpha, beta, Xs)
    assert np.max(np.abs(np.diag(ce) - ve[:, 0])) <= 1e-12
