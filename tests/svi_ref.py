"""Reference of the whitened uncollapsed bound (gp_svi_*, gparml_amd/csrc/svi.hip): bound, natural step, partials, scalars, publish and the
predictive of q(u), from given statistics.  Every function takes ``ld``: False computes in numpy float64 (LAPACK Cholesky), True in long double
with the Cholesky factorisation and the triangular solves written out (numpy's linalg has no long-double path), as loo_ref.py / predict_ref.py do.

Notation: L_k L_k^T = K_mm, a = L_k^-1, Psi2w = a Psi2 a^T, Cw = a C, q(v_d) = N(Mv[:, d], Sv), Lam = Sv^-1, H = Lam Mv."""
import numpy as np

LD = np.longdouble


def _t(ld):
    return LD if ld else np.float64


def kmm(Z, sf2, alpha, ld=False):
    T = _t(ld)
    Z, alpha = np.asarray(Z, T), np.asarray(alpha, T)
    dz = Z[:, None, :] - Z[None, :, :]
    return T(sf2) * np.exp(-0.5 * np.sum(alpha[None, None, :] * dz * dz, axis=2))


def stats_fixed(Z, sf2, alpha, X, Y, scale=1.0, ld=False):
    """dict(Psi2, C) of rows with fixed embeddings X, times ``scale`` (a batch's N / |B|): Psi1 = k(X, Z), Psi2 = Psi1^T Psi1, C = Psi1^T Y."""
    T = _t(ld)
    Z, alpha, X, Y = np.asarray(Z, T), np.asarray(alpha, T), np.asarray(X, T), np.asarray(Y, T)
    d = X[:, None, :] - Z[None, :, :]
    P1 = T(sf2) * np.exp(-0.5 * np.sum(alpha[None, None, :] * d * d, axis=2))
    return dict(Psi2=T(scale) * P1.T.dot(P1), C=T(scale) * P1.T.dot(Y))


def chol(A, ld=False):
    """Lower Cholesky factor; LinAlgError when a pivot is not positive."""
    if not ld:
        return np.linalg.cholesky(np.asarray(A, np.float64))
    A = np.array(A, LD)
    n = A.shape[0]
    Lm = np.zeros((n, n), LD)
    for j in range(n):
        d = A[j, j] - np.dot(Lm[j, :j], Lm[j, :j])
        if not d > 0:
            raise np.linalg.LinAlgError('not positive definite at pivot %d' % j)
        Lm[j, j] = np.sqrt(d)
        if j + 1 < n:
            Lm[j + 1:, j] = (A[j + 1:, j] - Lm[j + 1:, :j].dot(Lm[j, :j])) / Lm[j, j]
    return Lm


def fwd(Lm, B, ld=False):
    """L^-1 B by forward substitution."""
    if not ld:
        import scipy.linalg as sla
        return sla.solve_triangular(Lm, B, lower=True)
    B = np.array(B, LD)
    X = np.zeros_like(B)
    for i in range(Lm.shape[0]):
        X[i] = (B[i] - Lm[i, :i].dot(X[:i])) / Lm[i, i]
    return X


def tri_inv(Lm, ld=False):
    return fwd(Lm, np.eye(Lm.shape[0], dtype=_t(ld)), ld)


def logdet(Lm):
    return 2 * np.sum(np.log(np.diag(Lm)))


def whiten(K, Psi2, C, ld=False):
    """dict(Lk, a, P2w, Cw)."""
    T = _t(ld)
    Lk = chol(np.asarray(K, T), ld)
    a = tri_inv(Lk, ld)
    return dict(Lk=Lk, a=a, P2w=a.dot(np.asarray(Psi2, T)).dot(a.T), Cw=a.dot(np.asarray(C, T)))


def natural_step(Lam, H, w, beta, rho, ld=False):
    """(Lam, H) after one step of rate rho on the whitened statistics w; Psi2w symmetrised as the device does."""
    T = _t(ld)
    Lam, H, beta, rho = np.asarray(Lam, T), np.asarray(H, T), T(beta), T(rho)
    P = T(0.5) * (w['P2w'] + w['P2w'].T)
    M = Lam.shape[0]
    return (1 - rho) * Lam + rho * (np.eye(M, dtype=T) + beta * P), (1 - rho) * H + rho * (beta * w['Cw'])


def moments(Lam, H, ld=False):
    """dict(Ll, Lli, Sv, Mv, logdet_Lam)."""
    T = _t(ld)
    Ll = chol(np.asarray(Lam, T), ld)
    Lli = tri_inv(Ll, ld)
    Sv = Lli.T.dot(Lli)
    return dict(Ll=Ll, Lli=Lli, Sv=Sv, Mv=Sv.dot(np.asarray(H, T)), logdet_Lam=logdet(Ll))


def bound(K, st, Lam, H, beta, N, D, ld=False):
    """L of the issue's formula.  st: dict(Psi2, C, sum_YYT, Psi0, KL), as the statistics buffer holds them."""
    T = _t(ld)
    beta = T(beta)
    w = whiten(K, st['Psi2'], st['C'], ld)
    m = moments(Lam, H, ld)
    M = np.asarray(K).shape[0]
    W = D * m['Sv'] + m['Mv'].dot(m['Mv'].T)
    KLu = T(0.5) * D * (np.trace(m['Sv']) - M + m['logdet_Lam']) + T(0.5) * np.sum(m['Mv'] * m['Mv'])
    return (-T(0.5) * N * D * np.log(2 * T(np.pi) if not ld else 2 * LD(4) * np.arctan(LD(1))) + T(0.5) * N * D * np.log(beta)
            - T(0.5) * beta * T(st['sum_YYT']) + beta * np.sum(m['Mv'] * w['Cw']) - T(0.5) * beta * np.sum(w['P2w'] * W.T)
            - T(0.5) * beta * D * (T(st['Psi0']) - np.trace(w['P2w'])) - T(st['KL']) - KLu)


def step(Z, sf2, alpha, beta, st, Lam, H, N, D, regime_A=True, ld=False):
    """What gp_svi_step leaves, shaped like oracle.factorised.global_step's dict so that oracle.factorised.phase2 / finish complete the gradients:
    F, Abar, Bbar, dF_dKmm, grad_beta, grad_sf2, grad_Z_K, grad_alpha_K, BbarPsi2, Kmm, logdet_K, logdet_Lam."""
    T = _t(ld)
    Z, alpha, beta, s2 = np.asarray(Z, T), np.asarray(alpha, T), T(beta), T(sf2)
    Psi2, C = np.asarray(st['Psi2'], T), np.asarray(st['C'], T)
    K = kmm(Z, sf2, alpha, ld)
    M = K.shape[0]
    w = whiten(K, Psi2, C, ld)
    m = moments(Lam, H, ld)
    a, P2w, Cw, Sv, Mv = w['a'], w['P2w'], w['Cw'], m['Sv'], m['Mv']
    W = D * Sv + Mv.dot(Mv.T)
    G2 = T(0.5) * beta * D * np.eye(M, dtype=T) - T(0.5) * beta * W
    Gc = beta * Mv
    Bbar = a.T.dot(G2).dot(a)
    Abar = a.T.dot(Gc)
    R = 2 * G2.dot(P2w) + Gc.dot(Cw.T)
    Phi = np.tril(R, -1) + T(0.5) * np.diag(np.diag(R))
    dK = -a.T.dot(T(0.5) * (Phi + Phi.T)).dot(a)
    tMC, tPW, tP = np.sum(Mv * Cw), np.sum(P2w * W.T), np.trace(P2w)
    grad_beta = T(0.5) * N * D / beta - T(0.5) * T(st['sum_YYT']) + tMC - T(0.5) * tPW - T(0.5) * D * (T(st['Psi0']) - tP)
    dz = Z[:, None, :] - Z[None, :, :]
    S = (dK + dK.T) * K
    gZ_K = -alpha[None, :] * (Z * S.sum(1)[:, None] - S.dot(Z))
    V = dK * K
    ga_K = -T(0.5) * np.einsum('ab,abq->q', V, dz * dz)
    gs = (np.sum(V) + np.sum(Abar * C) + 2 * np.sum(Bbar * Psi2) - T(0.5) * beta * D * T(st['Psi0'])) / s2
    return dict(F=bound(K, st, Lam, H, beta, N, D, ld), Abar=Abar, Bbar=Bbar, dF_dKmm=dK, grad_beta=grad_beta, grad_sf2=gs, grad_Z_K=gZ_K,
                grad_alpha_K=ga_K, BbarPsi2=Bbar * Psi2, Kmm=K, logdet_K=logdet(w['Lk']), logdet_Lam=m['logdet_Lam'], Sv=Sv, Mv=Mv)


def optimum(K, st, beta, ld=False):
    """(Lam, H) of Titsias' optimum: one natural step of rate 1 from anywhere."""
    T = _t(ld)
    w = whiten(K, st['Psi2'], st['C'], ld)
    M = np.asarray(K).shape[0]
    return natural_step(np.eye(M, dtype=T), np.zeros_like(w['Cw']), w, beta, 1.0, ld)


def publish(K, Lam, H, beta, ld=False):
    """(Psi2_eff, C_eff): K + beta Psi2_eff = L_k Lam L_k^T."""
    T = _t(ld)
    Lk = chol(np.asarray(K, T), ld)
    Lam, H = np.asarray(Lam, T), np.asarray(H, T)
    return Lk.dot(Lam - np.eye(Lam.shape[0], dtype=T)).dot(Lk.T) / T(beta), Lk.dot(H) / T(beta)


def predict(Z, sf2, alpha, Lam, H, Xs, ld=False):
    """Mean (n, D) and latent variance (n,) of q(u)'s predictive at deterministic inputs Xs: k*^T a^T Mv and sf2 - |a k*|^2 + |L_l^-1 a k*|^2."""
    T = _t(ld)
    Z, alpha, Xs = np.asarray(Z, T), np.asarray(alpha, T), np.asarray(Xs, T)
    K = kmm(Z, sf2, alpha, ld)
    a = tri_inv(chol(K, ld), ld)
    m = moments(Lam, H, ld)
    d = Z[:, None, :] - Xs[None, :, :]
    ks = T(sf2) * np.exp(-0.5 * np.sum(alpha[None, None, :] * d * d, axis=2))          # (M, n)
    ak = a.dot(ks)
    lak = m['Lli'].dot(ak)
    return ak.T.dot(m['Mv']), T(sf2) - np.sum(ak * ak, axis=0) + np.sum(lak * lak, axis=0)
