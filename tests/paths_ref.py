"""numpy mirror of the pathwise posterior draws (gp_paths_set / gp_paths_eval, include/gparml_hip.h), built from (Z, sf2, alpha, beta, Psi2, C) like
tests/joint_ref.py.  Shared by tests/test_paths_cpu.py, tests/test_gpu_paths.py and tools/bench_paths.py.

  theta_f(x) = sum_q omega[f][q] (x_q - c_q)            (difference first, q ascending)
  phi(x)     = sqrt(sf2 / F) [cos theta_0 .. cos theta_{F-1}, sin theta_0 .. sin theta_{F-1}]
  out[s]     = mean + Phi_X w_s - a^T Lk^-1 Phi_Z w_s + b^T eps_s,   a = Lk^-1 k(X, Z)^T,  b = La^-1 k(X, Z)^T
so out - mean = T [w ; eps_u] with T = [Phi_X - k Kmm^-1 Phi_Z | b^T] (n, 2F + M), and the covariance the draws imply is T T^T."""
import numpy as np

from oracle import literal as L

import predict_ref as R


def features(X, omega, centre, sf2):
    """Phi (n, 2F)."""
    X, omega = np.atleast_2d(X), np.atleast_2d(omega)
    F, Q = omega.shape
    d = X - (np.zeros(Q) if centre is None else np.asarray(centre, dtype=float))
    theta = np.zeros((X.shape[0], F))
    for q in range(Q):
        theta = theta + d[:, q:q + 1] * omega[None, :, q]
    return np.sqrt(sf2 / F) * np.concatenate([np.cos(theta), np.sin(theta)], axis=1)


def parts(Z, sf2, alpha, beta, Psi2, C, X, omega, centre):
    p = R.posterior_parts(Z, sf2, alpha, beta, Psi2, C)
    X = np.atleast_2d(X)
    k = L.psi1(Z, sf2, alpha, X, np.zeros_like(X))
    p.update(k=k, a=np.linalg.solve(p['Lk'], k.T), b=np.linalg.solve(p['La'], k.T), mean=k.dot(p['W']),
             PhiX=features(X, omega, centre, sf2), PhiZ=features(Z, omega, centre, sf2))
    return p


def linear_map(Z, sf2, alpha, beta, Psi2, C, X, omega, centre=None):
    """(mean (n, D), T (n, 2F + M)): out[s][:, d] - mean[:, d] = T [w[s][:, d] ; eps_u[s][:, d]]."""
    p = parts(Z, sf2, alpha, beta, Psi2, C, X, omega, centre)
    prior = p['PhiX'] - p['a'].T.dot(np.linalg.solve(p['Lk'], p['PhiZ']))
    return p['mean'], np.concatenate([prior, p['b'].T], axis=1)


def draws(Z, sf2, alpha, beta, Psi2, C, X, omega, w, eps_u, centre=None):
    """(out (S, n, D), mean (n, D)) for w (S, 2F, D), eps_u (S, M, D)."""
    mean, T = linear_map(Z, sf2, alpha, beta, Psi2, C, X, omega, centre)
    return mean[None] + np.einsum('nk,skd->snd', T, np.concatenate([w, eps_u], axis=1)), mean


def implied_cov(Z, sf2, alpha, beta, Psi2, C, X, omega, centre=None):
    """T T^T (n, n): the covariance of the draws over (w, eps_u), shared by all D outputs."""
    _, T = linear_map(Z, sf2, alpha, beta, Psi2, C, X, omega, centre)
    return T.dot(T.T)


def rff_defect(Z, sf2, alpha, X, omega, centre=None):
    """P (K_F - K) P^T (n, n), K_F = phi phi^T on (X, Z) jointly, P = [I, -k(X, Z) Kmm^-1]: what implied_cov differs from joint_ref.joint's cov by."""
    X = np.atleast_2d(X)
    XZ = np.concatenate([X, Z], axis=0)
    Phi = features(XZ, omega, centre, sf2)
    K = L.rbf_gram(XZ, sf2, alpha)
    n = X.shape[0]
    P = np.concatenate([np.eye(n), -np.linalg.solve(K[n:, n:], K[n:, :n]).T], axis=1)
    return P.dot(Phi.dot(Phi.T) - K).dot(P.T), Phi.dot(Phi.T), K
