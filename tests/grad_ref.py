"""numpy reference of the predictive derivatives (gp_predict_grad), built on predict_ref.posterior_parts: the inverse-factor form, the form in
B = Ki - P, and an 80-bit long-double evaluation.  Shared by tests/test_grad_ref_cpu.py, tests/test_gpu_grad.py and tools/bench_grad.py.

With k = psi1(x), dk_q = -alpha_q (x_q - z_q) o k (difference first), a = Lk^-1 k, b = La^-1 k, a'_q = Lk^-1 dk_q, b'_q = La^-1 dk_q, W = beta E:
    jac[i, d, q]    = dk_q^T W_d
    dvar[i, q]      = -2 (a . a'_q - b . b'_q)
    metric[i, q, r] = sum_d jac_dq jac_dr + D (sf2 alpha_q [q == r] - a'_q . a'_r + b'_q . b'_r)
    logdet[i]       = ln det metric[i]"""
import numpy as np

from oracle import literal as L

import predict_ref as R


def _dk(Z, alpha, X, k):
    """dk[i, q, m] = -alpha_q (x_iq - z_mq) k_im"""
    diff = X[:, None, :] - Z[None, :, :]                                   # (n, M, Q)
    return np.transpose(-(alpha[None, None, :] * diff) * k[:, :, None], (0, 2, 1))


def _assemble(jac_rows, Ap, Bp, a, b, sf2, alpha, D, logdet):
    """jac_rows (n, Q, D), Ap / Bp (n, Q, M) rows a'_q / b'_q, a / b (n, M)."""
    dvar = -2.0 * (np.einsum('im,iqm->iq', a, Ap) - np.einsum('im,iqm->iq', b, Bp))
    cov = sf2 * np.diag(alpha)[None] - np.einsum('iqm,irm->iqr', Ap, Ap) + np.einsum('iqm,irm->iqr', Bp, Bp)
    metric = np.einsum('iqd,ird->iqr', jac_rows, jac_rows) + D * cov
    return dict(jac=np.transpose(jac_rows, (0, 2, 1)), dvar=dvar, metric=metric, logdet=logdet(metric))


def _slogdet(metric):
    return np.linalg.slogdet(metric)[1] if metric.shape[0] else np.zeros(0)


def grad(Z, sf2, alpha, beta, Psi2, C, X):
    """The inverse-factor form (float64): dict jac (n, D, Q), dvar (n, Q), metric (n, Q, Q), logdet (n,)."""
    p = R.posterior_parts(Z, sf2, alpha, beta, Psi2, C)
    X, alpha = np.atleast_2d(X), np.asarray(alpha, dtype=float)
    n, Q = X.shape
    k = L.psi1(Z, sf2, alpha, X, np.zeros_like(X))
    dk = _dk(Z, alpha, X, k)                                                # (n, Q, M)
    flat = dk.reshape(n * Q, -1).T                                          # (M, n Q)
    Ap = np.linalg.solve(p['Lk'], flat).T.reshape(n, Q, -1)
    Bp = np.linalg.solve(p['La'], flat).T.reshape(n, Q, -1)
    a, b = np.linalg.solve(p['Lk'], k.T).T, np.linalg.solve(p['La'], k.T).T
    return _assemble(dk.dot(p['W']), Ap, Bp, a, b, sf2, alpha, C.shape[1], _slogdet)


def grad_B(Z, sf2, alpha, beta, Psi2, C, X):
    """The same with the quadratic forms in B = Kmm^-1 - (Kmm + beta Psi2)^-1."""
    p = R.posterior_parts(Z, sf2, alpha, beta, Psi2, C)
    X, alpha = np.atleast_2d(X), np.asarray(alpha, dtype=float)
    k = L.psi1(Z, sf2, alpha, X, np.zeros_like(X))
    dk = _dk(Z, alpha, X, k)
    jac_rows = dk.dot(p['W'])
    dB = dk.dot(p['B'])                                                     # (n, Q, M)
    dvar = -2.0 * np.einsum('iqm,im->iq', dB, k)
    cov = sf2 * np.diag(alpha)[None] - np.einsum('iqm,irm->iqr', dB, dk)
    metric = np.einsum('iqd,ird->iqr', jac_rows, jac_rows) + C.shape[1] * cov
    return dict(jac=np.transpose(jac_rows, (0, 2, 1)), dvar=dvar, metric=metric, logdet=_slogdet(metric))


def grad_ld(Z, sf2, alpha, beta, Psi2, C, X):
    """The inverse-factor form in 80-bit long double from the same float64 statistics (predict_ref's _chol_ld / _fwd_ld), every difference formed
    first; logdet from a long-double Cholesky of the metric.  Long-double arrays."""
    LD = R.LD
    Z, X = np.asarray(Z, dtype=LD), np.atleast_2d(np.asarray(X, dtype=LD))
    alpha_ld, sf2, beta = np.asarray(alpha, dtype=LD), LD(sf2), LD(beta)
    n, Q = X.shape
    K = L.rbf_gram(Z, sf2, alpha_ld)
    Lk, La = R._chol_ld(K), R._chol_ld(K + beta * np.asarray(Psi2, dtype=LD))
    W = beta * R._fwd_ld(La.T[::-1, ::-1], R._fwd_ld(La, C)[::-1])[::-1]
    k = L.psi1(Z, sf2, alpha, X, np.zeros_like(X))
    dk = _dk(Z, alpha_ld, X, k)
    flat = dk.reshape(n * Q, -1).T
    Ap, Bp = R._fwd_ld(Lk, flat).T.reshape(n, Q, -1), R._fwd_ld(La, flat).T.reshape(n, Q, -1)
    a, b = R._fwd_ld(Lk, k.T).T, R._fwd_ld(La, k.T).T
    logdet = lambda m: np.array([2 * np.sum(np.log(np.diag(R._chol_ld(mi)))) for mi in m], dtype=LD)
    return _assemble(dk.dot(W), Ap, Bp, a, b, sf2, alpha_ld, C.shape[1], logdet)


def exact_gp_grad(X, Y, sf2, alpha, beta, Xs):
    """Derivatives of predict_ref.exact_gp's mean and variance with respect to the test input, by the same closed form: (jac (n, D, Q), dvar (n, Q))."""
    alpha = np.asarray(alpha, dtype=float)
    K = L.rbf_gram(X, sf2, alpha) + np.eye(X.shape[0]) / beta
    ks = L.rbf_gram(Xs, sf2, alpha, X)
    dks = _dk(X, alpha, Xs, ks)                                             # (n, Q, N)
    jac = np.transpose(dks.dot(np.linalg.solve(K, Y)), (0, 2, 1))
    dvar = -2.0 * np.einsum('iqn,in->iq', dks, np.linalg.solve(K, ks.T).T)
    return jac, dvar
