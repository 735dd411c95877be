"""Pathwise posterior draws without a device: the ABI surface and the numpy mirror (tests/paths_ref.py) the GPU tests compare against."""
import os
import re

import numpy as np
import pytest

import joint_ref as J
import paths_ref as P
import predict_ref as R
from conftest import ROOT
from test_joint_cpu import _model

SHAPES = [(5, 1, 1, 'A', 37), (64, 2, 3, 'B', 129), (130, 17, 3, 'B', 300)]
# The seed of the frequencies in test_feature_gram_is_within_six_sigma, recorded: with RandomState(RFF_SEED) the mirror's largest deviation over the
# 10^4 elements is 3.25 times the bound sf2 / sqrt(2F) on an element's standard deviation (printed by the test).
RFF_SEED = 4


def _case(M, Q, D, regime, n, F):
    N = max(300, M + 100)
    d = _model(N, D, M, Q, regime, seed=M + Q + D)
    Psi2, C = R.statistics(d['Z'], d['sf2'], d['alpha'], d['Y'], d['X_mu'], d['X_S'])
    X = np.random.RandomState(11).randn(n, Q)
    omega = np.random.RandomState(12).randn(F, Q) * np.sqrt(d['alpha'])
    return d, Psi2, C, X, omega


def test_header_declares_the_paths_entry_points_and_lib_binds_them():
    from gparml_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'gparml_hip.h')).read(), flags=re.S)
    for name, nargs in (('gp_paths_set', 7), ('gp_paths_eval', 6), ('gp_paths_clear', 1)):
        m = re.search(r'int\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m, '%s is not declared in include/gparml_hip.h' % name
        assert len(m.group(1).split(',')) == nargs
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs


@pytest.mark.parametrize('M,Q,D,regime,n', SHAPES)
@pytest.mark.parametrize('F', [1, 24])
def test_implied_covariance_is_the_joint_one_plus_the_feature_defect(M, Q, D, regime, n, F):
    d, Psi2, C, X, omega = _case(M, Q, D, regime, n, F)
    centre = d['Z'].mean(axis=0)
    args = (d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2, C, X)
    tol = J.cond_tol(d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2)
    _, cov_f = J.joint(*args)
    defect, _, _ = P.rff_defect(d['Z'], d['sf2'], d['alpha'], X, omega, centre)
    err = np.max(np.abs(P.implied_cov(*args, omega, centre) - cov_f - defect)) / d['sf2']
    print('T T^T - cov_f - P (K_F - K) P^T: %.3g (tol %.3g)' % (err, tol))
    assert err <= tol, (err, tol)


def test_feature_gram_is_within_six_sigma():
    """Var cos <= 1/2: an element of K_F, a mean of F terms sf2 cos(theta_f - theta'_f), has a standard deviation <= sf2 / sqrt(2F)."""
    F, Q, sf2 = 4096, 3, 1.7
    alpha = np.array([0.5, 1.0, 2.0])
    X = np.random.RandomState(1).randn(100, Q)
    omega = np.random.RandomState(RFF_SEED).randn(F, Q) * np.sqrt(alpha)
    Phi = P.features(X, omega, X.mean(axis=0), sf2)
    from oracle import literal as L
    dev = np.max(np.abs(Phi.dot(Phi.T) - L.rbf_gram(X, sf2, alpha)))
    bound = 6.0 * sf2 / np.sqrt(2.0 * F)
    print('max |K_F - K| = %.3g = %.2f sigma (bound: 6 sigma = %.3g)' % (dev, 6.0 * dev / bound, bound))
    assert dev <= bound


def test_zero_normals_give_the_mean():
    M, Q, D, regime, n = SHAPES[1]
    d, Psi2, C, X, omega = _case(M, Q, D, regime, n, 24)
    args = (d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2, C, X)
    out, mean = P.draws(*args, omega, np.zeros((2, 48, D)), np.zeros((2, M, D)))
    mj, _ = J.joint(*args)
    assert np.array_equal(out[0], mean) and np.array_equal(out[1], mean) and np.array_equal(mean, mj)


@pytest.mark.parametrize('F', [1, 24, 100])
def test_feature_diagonal_is_sf2(F):
    sf2 = 1.3
    X = 3.0 * np.random.RandomState(2).randn(50, 4)
    Phi = P.features(X, np.random.RandomState(3).randn(F, 4), None, sf2)
    err = np.max(np.abs(np.sum(Phi * Phi, axis=1) - sf2)) / sf2
    print('diag(K_F) / sf2 - 1: %.3g' % err)
    # a few ulp: cos^2 + sin^2 of one phase is 1 to about two units of 2^-53 (two correctly rounded squares and a sum), the errors of the F phases
    # average rather than add in (sf2 / F) sum_f (...), and the scale sqrt(sf2 / F), squared, adds two more roundings
    assert err <= 4 * 2.0 ** -52
