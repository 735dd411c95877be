"""numpy mirror of the derivatives of the pathwise posterior draws (gp_paths_grad, include/gparml_hip.h), built on tests/paths_ref.py (the draws),
tests/grad_ref.py (dk, the mean's Jacobian) and tests/joint_ref.py's statistics.  Shared by tests/test_paths_grad_ref_cpu.py,
tests/test_gpu_paths_grad.py and tools/bench_paths_grad.py.

With theta_f(x) = sum_q omega[f][q] (x_q - c_q), scale = sqrt(sf2 / F), dk_q = -alpha_q (x_q - z_q) o k, a'_q = Lk^-1 dk_q, b'_q = La^-1 dk_q:
    dphi_q(x)                 = [ -(scale sin theta_f) omega[f][q]  (f < F) ;  (scale cos theta_f) omega[f][q] ]
    d out[s][i][d] / d x_q    = jac_mean[i][d][q] + dphi_q(x_i) . w_s[:, d] - a'_q(x_i) . G_s[:, d] + b'_q(x_i) . eps_s[:, d],   G_s = Lk^-1 Phi_Z w_s
so d out / d x_q - jac_mean = A_q [w ; eps_u] with A_q = [dphi_q - a'_q^T Lk^-1 Phi_Z | b'_q^T] (2F + M), the same for every output column."""
import numpy as np

from oracle import literal as L

import grad_ref as G
import joint_ref as J          # noqa: F401  (the statistics and cond_tol of the callers)
import paths_ref as P
import predict_ref as R


def _theta(X, omega, centre, dtype):
    X, omega = np.atleast_2d(np.asarray(X, dtype=dtype)), np.atleast_2d(np.asarray(omega, dtype=dtype))
    F, Q = omega.shape
    d = X - (np.zeros(Q, dtype=dtype) if centre is None else np.asarray(centre, dtype=dtype))
    theta = np.zeros((X.shape[0], F), dtype=dtype)
    for q in range(Q):
        theta = theta + d[:, q:q + 1] * omega[None, :, q]
    return theta, omega


def features(X, omega, centre, sf2, dtype=float):
    """paths_ref.features in the given precision: Phi (n, 2F)."""
    theta, omega = _theta(X, omega, centre, dtype)
    return np.sqrt(dtype(sf2) / dtype(omega.shape[0])) * np.concatenate([np.cos(theta), np.sin(theta)], axis=1)


def dfeatures(X, omega, centre, sf2, dtype=float):
    """dPhi (n, Q, 2F): d phi(x_i) / d x_q."""
    theta, omega = _theta(X, omega, centre, dtype)
    scale = np.sqrt(dtype(sf2) / dtype(omega.shape[0]))
    sn, cs = scale * np.sin(theta), scale * np.cos(theta)                     # (n, F)
    return np.concatenate([-sn[:, None, :] * omega.T[None], cs[:, None, :] * omega.T[None]], axis=2)


def _parts(Z, sf2, alpha, beta, Psi2, C, X, omega, centre):
    """float64: jac_rows (n, Q, D), dPhi (n, Q, 2F), Ap / Bp (n, Q, M), Lk^-1 Phi_Z (M, 2F)."""
    p = P.parts(Z, sf2, alpha, beta, Psi2, C, X, omega, centre)
    X, alpha = np.atleast_2d(X), np.asarray(alpha, dtype=float)
    n, Q = X.shape
    dk = G._dk(Z, alpha, X, p['k'])                                           # (n, Q, M)
    flat = dk.reshape(n * Q, -1).T
    Ap = np.linalg.solve(p['Lk'], flat).T.reshape(n, Q, -1)
    Bp = np.linalg.solve(p['La'], flat).T.reshape(n, Q, -1)
    return dk.dot(p['W']), dfeatures(X, omega, centre, sf2), Ap, Bp, np.linalg.solve(p['Lk'], p['PhiZ'])


def linear_map_jac(Z, sf2, alpha, beta, Psi2, C, X, omega, centre=None):
    """(jac_mean (n, D, Q), A (n, Q, 2F + M)): d out[s][i][d] / d x_q - jac_mean[i][d][q] = A[i, q] . [w[s][:, d] ; eps_u[s][:, d]]."""
    jm, dPhi, Ap, Bp, LiPhiZ = _parts(Z, sf2, alpha, beta, Psi2, C, X, omega, centre)
    return np.transpose(jm, (0, 2, 1)), np.concatenate([dPhi - Ap.dot(LiPhiZ), Bp], axis=2)


def draw_jac(Z, sf2, alpha, beta, Psi2, C, X, omega, w, eps_u, centre=None):
    """(jac (S, n, D, Q), jac_mean (n, D, Q)) in float64, term by term as the header states it (G_s formed first, as gp_paths_set does)."""
    jm, dPhi, Ap, Bp, LiPhiZ = _parts(Z, sf2, alpha, beta, Psi2, C, X, omega, centre)
    Gs = np.einsum('mk,skd->smd', LiPhiZ, w)                                  # (S, M, D)
    rows = jm[None] + np.einsum('nqk,skd->snqd', dPhi, w) - np.einsum('nqm,smd->snqd', Ap, Gs) + np.einsum('nqm,smd->snqd', Bp, eps_u)
    return np.transpose(rows, (0, 1, 3, 2)), np.transpose(jm, (0, 2, 1))


def _model_ld(Z, sf2, alpha, beta, Psi2, C):
    LD = R.LD
    Zl, al = np.asarray(Z, dtype=LD), np.asarray(alpha, dtype=LD)
    K = L.rbf_gram(Zl, LD(sf2), al)
    Lk, La = R._chol_ld(K), R._chol_ld(K + LD(beta) * np.asarray(Psi2, dtype=LD))
    W = LD(beta) * R._fwd_ld(La.T[::-1, ::-1], R._fwd_ld(La, C)[::-1])[::-1]
    return Zl, al, Lk, La, W


def draws_ld(Z, sf2, alpha, beta, Psi2, C, X, omega, w, eps_u, centre=None):
    """paths_ref.draws in 80-bit long double (the phases, the features and every product): out (S, n, D)."""
    LD = R.LD
    Zl, al, Lk, La, W = _model_ld(Z, sf2, alpha, beta, Psi2, C)
    Xl = np.atleast_2d(np.asarray(X, dtype=LD))
    k = L.psi1(Zl, LD(sf2), alpha, Xl, np.zeros_like(Xl))
    a, b = R._fwd_ld(Lk, k.T), R._fwd_ld(La, k.T)                             # (M, n)
    LiPhiZ = R._fwd_ld(Lk, features(Zl, omega, centre, sf2, LD))
    T = np.concatenate([features(Xl, omega, centre, sf2, LD) - a.T.dot(LiPhiZ), b.T], axis=1)
    z = np.concatenate([np.asarray(w, dtype=LD), np.asarray(eps_u, dtype=LD)], axis=1)
    return k.dot(W)[None] + np.einsum('nk,skd->snd', T, z)


def draw_jac_ld(Z, sf2, alpha, beta, Psi2, C, X, omega, w, eps_u, centre=None):
    """(jac (S, n, D, Q), jac_mean (n, D, Q)) in 80-bit long double from the same float64 statistics: the phase, the features, the triangular
    solves (predict_ref's _chol_ld / _fwd_ld) and every product in long double, every difference formed first.  Long-double arrays."""
    LD = R.LD
    Zl, al, Lk, La, W = _model_ld(Z, sf2, alpha, beta, Psi2, C)
    Xl = np.atleast_2d(np.asarray(X, dtype=LD))
    n, Q = Xl.shape
    k = L.psi1(Zl, LD(sf2), alpha, Xl, np.zeros_like(Xl))
    dk = G._dk(Zl, al, Xl, k)
    flat = dk.reshape(n * Q, -1).T
    Ap, Bp = R._fwd_ld(Lk, flat).T.reshape(n, Q, -1), R._fwd_ld(La, flat).T.reshape(n, Q, -1)
    LiPhiZ = R._fwd_ld(Lk, features(Zl, omega, centre, sf2, LD))
    A = np.concatenate([dfeatures(Xl, omega, centre, sf2, LD) - Ap.dot(LiPhiZ), Bp], axis=2)
    z = np.concatenate([np.asarray(w, dtype=LD), np.asarray(eps_u, dtype=LD)], axis=1)          # (S, 2F + M, D)
    jm = dk.dot(W)                                                            # (n, Q, D)
    rows = jm[None] + np.einsum('nqk,skd->snqd', A, z)
    return np.transpose(rows, (0, 1, 3, 2)), np.transpose(jm, (0, 2, 1))
