"""numpy reference of the joint posterior predictive (gp_predict_joint / gp_predict_sample), built on predict_ref.posterior_parts.
Shared by tests/test_joint_cpu.py, tests/test_gpu_joint.py and tools/bench_joint.py."""
import numpy as np

from oracle import literal as L

import predict_ref as R


def joint(Z, sf2, alpha, beta, Psi2, C, X, include_noise=False):
    """(mean (n, D), cov (n, n)) in the signed inverse-factor form: cov = K** - a^T a + b^T b with a = Lk^-1 K*^T, b = La^-1 K*^T."""
    p = R.posterior_parts(Z, sf2, alpha, beta, Psi2, C)
    X = np.atleast_2d(X)
    k = L.psi1(Z, sf2, alpha, X, np.zeros_like(X))
    a = np.linalg.solve(p['Lk'], k.T)
    b = np.linalg.solve(p['La'], k.T)
    cov = L.rbf_gram(X, sf2, alpha) - a.T.dot(a) + b.T.dot(b)
    if include_noise:
        cov = cov + np.eye(X.shape[0]) / beta
    return k.dot(p['W']), cov


def joint_B(Z, sf2, alpha, beta, Psi2, C, X, include_noise=False):
    """The same as K** - K* B K*^T with B = Kmm^-1 - (Kmm + beta Psi2)^-1."""
    p = R.posterior_parts(Z, sf2, alpha, beta, Psi2, C)
    X = np.atleast_2d(X)
    k = L.psi1(Z, sf2, alpha, X, np.zeros_like(X))
    cov = L.rbf_gram(X, sf2, alpha) - k.dot(p['B']).dot(k.T)
    if include_noise:
        cov = cov + np.eye(X.shape[0]) / beta
    return k.dot(p['W']), cov


def exact_gp_joint(X, Y, sf2, alpha, beta, Xs, include_noise=True):
    """predict_ref.exact_gp's algebra for the full matrix: mean k*^T (K + I/beta)^-1 Y, cov = K** - K* (K + I/beta)^-1 K*^T (+ I/beta)."""
    K = L.rbf_gram(X, sf2, alpha) + np.eye(X.shape[0]) / beta
    ks = L.rbf_gram(Xs, sf2, alpha, X)
    cov = L.rbf_gram(Xs, sf2, alpha) - ks.dot(np.linalg.solve(K, ks.T))
    if include_noise:
        cov = cov + np.eye(Xs.shape[0]) / beta
    return ks.dot(np.linalg.solve(K, Y)), cov


def cond_tol(Z, sf2, alpha, beta, Psi2):
    """max(1e-10, 1e-16 cond), cond the larger of cond(Kmm) and cond(Kmm + beta Psi2): the rule of tests/test_gpu_predictive.py."""
    K = L.rbf_gram(Z, sf2, alpha)
    return max(1e-10, 1e-16 * max(np.linalg.cond(K), np.linalg.cond(K + beta * Psi2)))
