"""numpy reference of the curve energy (gp_curve_energy), built on predict_ref.posterior_parts like grad_ref.py: the inverse-factor form, the form in
B = Ki - P, and an 80-bit long-double evaluation.  Shared by tests/test_curve_ref_cpu.py, tests/test_gpu_curve.py and tools/bench_curve.py.

A curve is T points x_0 .. x_{T-1}; with k_s = psi1(x_s), dk_s = k_{s+1} - k_s, dx_s = x_{s+1} - x_s, kappa_s = k(x_s, x_{s+1}), W = beta E,
dmu_s = dk_s^T W, da_s = Lk^-1 dk_s, db_s = La^-1 dk_s:
    seg[c, s]     = |dmu_s|^2 + D (|db_s|^2 - |da_s|^2) + 2 D (sf2 - kappa_s)
    energy[c]     = 1/2 (T - 1) sum_s seg[c, s]
    g_s           = W dmu_s - D (Lk^-T da_s - La^-T db_s),   g_{-1} = g_{T-1} = 0
    grad[c, t, q] = (T - 1) [(g_{t-1} - g_t) . dk_t,q + D alpha_q (kappa_{t-1} dx_{t-1,q} - kappa_t dx_{t,q})],   dk_t,q = -alpha_q (x_tq - z_q) o k_t
Every difference is formed first: dk_s = k_base expm1(-1/2 sum_q alpha_q dx_sq ((x_sq - z_q) + (x_{s+1,q} - z_q))) with the base the endpoint of
the larger k (the argument is <= 0), and sf2 - kappa_s = -sf2 expm1(-1/2 sum_q alpha_q dx_sq^2)."""
import numpy as np

from oracle import literal as L

import predict_ref as R


def _curves(X):
    X = np.asarray(X)
    if X.ndim == 2:
        X = X[None]
    assert X.ndim == 3 and X.shape[1] >= 2, 'X shape %s: (n_curves, T >= 2, Q) expected' % (X.shape,)
    return X


def _differences(Z, sf2, alpha, X):
    """k (n, T, M) and, per segment, dk (n, T-1, M), dx (n, T-1, Q), sf2 - kappa and kappa (n, T-1), in the dtype of X."""
    n, T, Q = X.shape
    k = L.psi1(Z, sf2, alpha, X.reshape(n * T, Q), np.zeros_like(X.reshape(n * T, Q))).reshape(n, T, -1)
    x0, x1 = X[:, :-1], X[:, 1:]
    dx = x1 - x0
    u = np.einsum('nsq,nsmq->nsm', alpha * dx, (x0[:, :, None, :] - Z[None, None]) + (x1[:, :, None, :] - Z[None, None]))
    v = np.where(u >= 0, k[:, :-1], k[:, 1:]) * np.expm1(-0.5 * np.abs(u))
    dk = np.where(u >= 0, v, -v)
    w = -0.5 * np.einsum('nsq,nsq->ns', alpha * dx, dx)
    return k, dk, dx, -(sf2 * np.expm1(w)), sf2 * np.exp(w)


def _assemble(Z, alpha, X, D, k, dx, prior, kappa, dmu, quad, g):
    """dmu (n, T-1, D), quad (n, T-1) = |db|^2 - |da|^2 (or -dk^T B dk), g (n, T-1, M)."""
    n, T, Q = X.shape
    seg = np.sum(dmu * dmu, axis=2) + D * quad + 2 * D * prior
    energy = 0.5 * (T - 1) * np.sum(seg, axis=1)
    zero = np.zeros_like(g[:, :1])
    h = np.concatenate([zero, g], axis=1) - np.concatenate([g, zero], axis=1)               # (n, T, M): g_{t-1} - g_t
    diff = X[:, :, None, :] - Z[None, None]                                                  # (n, T, M, Q)
    data = -alpha * np.einsum('ntm,ntmq->ntq', h * k, diff)
    kd = kappa[:, :, None] * dx                                                              # (n, T-1, Q)
    zq = np.zeros_like(kd[:, :1])
    kt = np.concatenate([zq, kd], axis=1) - np.concatenate([kd, zq], axis=1)
    return dict(energy=energy, seg=seg, grad=(T - 1) * (data + D * alpha * kt))


def curve(Z, sf2, alpha, beta, Psi2, C, X):
    """The inverse-factor form (float64): dict energy (n,), seg (n, T-1), grad (n, T, Q)."""
    p = R.posterior_parts(Z, sf2, alpha, beta, Psi2, C)
    X, alpha = _curves(np.asarray(X, dtype=float)), np.asarray(alpha, dtype=float)
    k, dk, dx, prior, kappa = _differences(Z, sf2, alpha, X)
    n, S, M = dk.shape
    flat = dk.reshape(n * S, M)
    da, db = np.linalg.solve(p['Lk'], flat.T), np.linalg.solve(p['La'], flat.T)            # (M, n S)
    dmu = flat.dot(p['W'])
    g = dmu.dot(p['W'].T) - C.shape[1] * (np.linalg.solve(p['Lk'].T, da) - np.linalg.solve(p['La'].T, db)).T
    quad = (np.sum(db * db, axis=0) - np.sum(da * da, axis=0)).reshape(n, S)
    return _assemble(Z, alpha, X, C.shape[1], k, dx, prior, kappa, dmu.reshape(n, S, -1), quad, g.reshape(n, S, M))


def curve_B(Z, sf2, alpha, beta, Psi2, C, X):
    """The same with the quadratic form and g in B = Kmm^-1 - (Kmm + beta Psi2)^-1."""
    p = R.posterior_parts(Z, sf2, alpha, beta, Psi2, C)
    X, alpha = _curves(np.asarray(X, dtype=float)), np.asarray(alpha, dtype=float)
    k, dk, dx, prior, kappa = _differences(Z, sf2, alpha, X)
    n, S, M = dk.shape
    flat = dk.reshape(n * S, M)
    dB = flat.dot(p['B'])
    dmu = flat.dot(p['W'])
    g = dmu.dot(p['W'].T) - C.shape[1] * dB
    quad = -np.sum(dB * flat, axis=1).reshape(n, S)
    return _assemble(Z, alpha, X, C.shape[1], k, dx, prior, kappa, dmu.reshape(n, S, -1), quad, g.reshape(n, S, M))


def curve_ld(Z, sf2, alpha, beta, Psi2, C, X):
    """The inverse-factor form in 80-bit long double from the same float64 statistics (predict_ref's _chol_ld / _fwd_ld), every difference formed
    first.  Long-double arrays."""
    LD = R.LD
    Z, X = np.asarray(Z, dtype=LD), _curves(np.asarray(X, dtype=LD))
    alpha, sf2, beta = np.asarray(alpha, dtype=LD), LD(sf2), LD(beta)
    K = L.rbf_gram(Z, sf2, alpha)
    Lk, La = R._chol_ld(K), R._chol_ld(K + beta * np.asarray(Psi2, dtype=LD))
    back = lambda F, Y: R._fwd_ld(F.T[::-1, ::-1], Y[::-1])[::-1]                           # F^-T Y: the upper solve as a reversed lower one
    W = beta * back(La, R._fwd_ld(La, C))
    k, dk, dx, prior, kappa = _differences(Z, sf2, alpha, X)
    n, S, M = dk.shape
    flat = dk.reshape(n * S, M)
    da, db = R._fwd_ld(Lk, flat.T), R._fwd_ld(La, flat.T)
    dmu = flat.dot(W)
    g = dmu.dot(W.T) - C.shape[1] * (back(Lk, da) - back(La, db)).T
    quad = (np.sum(db * db, axis=0) - np.sum(da * da, axis=0)).reshape(n, S)
    return _assemble(Z, alpha, X, C.shape[1], k, dx, prior, kappa, dmu.reshape(n, S, -1), quad, g.reshape(n, S, M))
