"""numpy reference of the posterior predictive (gp_predict): Titsias' optimal q(u) in the reference's statistics, built from
oracle.literal.rbf_gram / psi1 / psi2_point and numpy factorisations.  Shared by tests/test_predict_cpu.py and tests/test_gpu_predictive.py."""
import numpy as np

from oracle import literal as L


def posterior_parts(Z, sf2, alpha, beta, Psi2, C):
    """W = beta (Kmm + beta Psi2)^-1 C and B = Kmm^-1 - (Kmm + beta Psi2)^-1, both from Cholesky solves."""
    K = L.rbf_gram(Z, sf2, alpha)
    A = K + beta * Psi2
    Lk, La = np.linalg.cholesky(K), np.linalg.cholesky(A)
    eye = np.eye(K.shape[0])
    Ki = np.linalg.solve(Lk.T, np.linalg.solve(Lk, eye))
    P = np.linalg.solve(La.T, np.linalg.solve(La, eye))
    W = beta * np.linalg.solve(La.T, np.linalg.solve(La, C))
    return dict(K=K, Lk=Lk, La=La, Ki=Ki, P=P, W=W, B=Ki - P)


def predict(Z, sf2, alpha, beta, Psi2, C, X_mu, X_S=None, include_noise=False):
    """(mean (n, D), var): var (n, 1) for X_S None (sf2 - k^T B k formed as |Lk^-1 k|^2 - |La^-1 k|^2), (n, D) for uncertain inputs."""
    p = posterior_parts(Z, sf2, alpha, beta, Psi2, C)
    X_mu = np.atleast_2d(X_mu)
    noise = 1.0 / beta if include_noise else 0.0
    if X_S is None:
        k = L.psi1(Z, sf2, alpha, X_mu, np.zeros_like(X_mu))
        mean = k.dot(p['W'])
        a = np.linalg.solve(p['Lk'], k.T)
        b = np.linalg.solve(p['La'], k.T)
        var = sf2 - np.sum(a * a, axis=0) + np.sum(b * b, axis=0) + noise
        return mean, var[:, None]
    X_S = np.atleast_2d(X_S)
    k = L.psi1(Z, sf2, alpha, X_mu, X_S)
    mean = k.dot(p['W'])
    var = np.empty_like(mean)
    for i in range(X_mu.shape[0]):
        P2 = L.psi2_point(Z, sf2, alpha, X_mu[i], X_S[i])
        var[i] = sf2 - np.sum(p['B'] * P2) + np.sum(p['W'] * P2.dot(p['W']), axis=0) - mean[i] ** 2 + noise
    return mean, var


def statistics(Z, sf2, alpha, Y, X_mu, X_S):
    """Psi2 = sum_n psi2_n and C = Psi1^T Y of a training set (partial_terms.py:79-80)."""
    if np.all(X_S == 0):
        k = L.psi1(Z, sf2, alpha, X_mu, X_S)
        return k.T.dot(k), k.T.dot(Y)
    Psi2 = sum(L.psi2_point(Z, sf2, alpha, X_mu[i], X_S[i]) for i in range(X_mu.shape[0]))
    return Psi2, L.psi1_T_Y(Z, sf2, alpha, X_mu, X_S, Y)


def exact_gp(X, Y, sf2, alpha, beta, Xs):
    """Full GP posterior with noise precision beta: mean k*^T (K + I/beta)^-1 Y, var_y = k** - k*^T (K + I/beta)^-1 k* + 1/beta."""
    K = L.rbf_gram(X, sf2, alpha) + np.eye(X.shape[0]) / beta
    ks = L.rbf_gram(Xs, sf2, alpha, X)
    mean = ks.dot(np.linalg.solve(K, Y))
    var = sf2 - np.sum(ks * np.linalg.solve(K, ks.T).T, axis=1) + 1.0 / beta
    return mean, var[:, None]


# ---- extended precision (80-bit long double): the truth for the benchmark-conditioned checks ------------------------------------------------
LD = np.longdouble


def _chol_ld(A):
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    Lm = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - np.dot(Lm[j, :j], Lm[j, :j])
        if not d > 0:
            raise np.linalg.LinAlgError('long-double Cholesky: pivot %d is %r' % (j, d))
        Lm[j, j] = np.sqrt(d)
        Lm[j + 1:, j] = (A[j + 1:, j] - Lm[j + 1:, :j].dot(Lm[j, :j])) / Lm[j, j]
    return Lm


def _fwd_ld(Lm, B):
    """Lm^-1 B for lower-triangular Lm (long double)."""
    B = np.array(B, dtype=LD)
    X = np.zeros_like(B)
    for i in range(Lm.shape[0]):
        X[i] = (B[i] - Lm[i, :i].dot(X[:i])) / Lm[i, i]
    return X


def predict_ld(Z, sf2, alpha, beta, Psi2, C, X_mu, X_S=None):
    """predict() in long double from the same float64 statistics: (mean, var) as long-double arrays.  The deterministic variance uses the inverse
    factors, the uncertain one B = Ki - P formed in long double (no cancellation left at cond ~1e10: 19 significant digits)."""
    Z, alpha, X_mu = np.asarray(Z, dtype=LD), np.asarray(alpha, dtype=LD), np.atleast_2d(np.asarray(X_mu, dtype=LD))
    sf2, beta = LD(sf2), LD(beta)
    K = L.rbf_gram(Z, sf2, alpha)
    Lk, La = _chol_ld(K), _chol_ld(K + beta * np.asarray(Psi2, dtype=LD))
    W = beta * _fwd_ld(La.T[::-1, ::-1], _fwd_ld(La, C)[::-1])[::-1]        # La^-T (La^-1 C): the upper solve as a reversed lower one
    if X_S is None:
        k = L.psi1(Z, sf2, alpha, X_mu, np.zeros_like(X_mu))
        a, b = _fwd_ld(Lk, k.T), _fwd_ld(La, k.T)
        return k.dot(W), (sf2 - np.sum(a * a, axis=0) + np.sum(b * b, axis=0))[:, None]
    X_S = np.atleast_2d(np.asarray(X_S, dtype=LD))
    eye = np.eye(K.shape[0], dtype=LD)
    Lki, Lai = _fwd_ld(Lk, eye), _fwd_ld(La, eye)
    B = Lki.T.dot(Lki) - Lai.T.dot(Lai)
    k = L.psi1(Z, sf2, alpha, X_mu, X_S)
    mean = k.dot(W)
    var = np.empty_like(mean)
    for i in range(X_mu.shape[0]):
        P2 = L.psi2_point(Z, sf2, alpha, X_mu[i], X_S[i])
        var[i] = sf2 - np.sum(B * P2) + np.sum(W * P2.dot(W), axis=0) - mean[i] ** 2
    return mean, var
