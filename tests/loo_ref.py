"""numpy references of exact leave-one-out / leave-block-out scoring (gp_loo_score), for deterministic inputs and fixed Z, sf2, alpha, beta.

``loo_closed_form``: the rank-g downdate from tests/predict_ref.py's quantities -- with k_i = psi1(x_i), a_i = Lk^-1 k_i, b_i = La^-1 k_i,
e_i = y_i - k_i^T W, and for a block G of rows H = beta B_G B_G^T, S = I - H:
    E'_G = S^-1 E_G,   v'_i = sf2 - |a_i|^2 + ([S^-1]_ii - 1) / beta (+ 1/beta),   lev_i = beta |b_i|^2.
It is evaluated in numpy.longdouble from the statistics it is given, as predict_ref.predict_ld evaluates the prediction: a reference should not
carry an error of the size it is asked to judge, and in float64 the error of |b_i|^2 (cond(Kmm + beta Psi2) eps) reaches [S^-1]_ii through S^-1
TWICE, i.e. with the square of 1 / (1 - lambda_max(H)).  The results are returned rounded to float64.
``loo_refit``: brute force in numpy.longdouble -- per block the statistics of all rows but the block's (the block's k k^T, k y^T and y y^T taken
off the long-double statistics of all rows), q(u) rebuilt from scratch (predict_ref.predict_ld) and the block predicted.
Rows [j block, (j + 1) block) form block j; the last one may be short.  Shared by tests/test_loo_ref_cpu.py and tests/test_gpu_loo.py."""
import numpy as np

from oracle import literal as L
import predict_ref as R
import score_ref as S

LD = np.longdouble


def blocks(n, block):
    return [np.arange(s, min(s + block, n)) for s in range(0, n, block)]


def statistics_ld(Z, sf2, alpha, Y, X_mu):
    """(k (n, M), Psi2 = k^T k, C = k^T Y, sum y^2) of deterministic inputs in long double."""
    Xl, Yl = np.atleast_2d(np.asarray(X_mu, dtype=LD)), np.atleast_2d(np.asarray(Y, dtype=LD))
    k = L.psi1(np.asarray(Z, dtype=LD), LD(sf2), np.asarray(alpha, dtype=LD), Xl, np.zeros_like(Xl))
    assert k.dtype == LD
    return k, k.T.dot(k), k.T.dot(Yl), np.sum(Yl * Yl)


def parts_ld(Z, sf2, alpha, beta, Psi2, C, X_mu):
    """predict_ref.predict_ld's quantities at the rows X_mu, long double: k (n, M), a = Lk^-1 k^T and b = La^-1 k^T (M, n), mean = k W (n, D)."""
    Zl, al, sf2, beta = np.asarray(Z, dtype=LD), np.asarray(alpha, dtype=LD), LD(sf2), LD(beta)
    Xl = np.atleast_2d(np.asarray(X_mu, dtype=LD))
    K = L.rbf_gram(Zl, sf2, al)
    Lk, La = R._chol_ld(K), R._chol_ld(K + beta * np.asarray(Psi2, dtype=LD))
    W = beta * R._fwd_ld(La.T[::-1, ::-1], R._fwd_ld(La, np.asarray(C, dtype=LD))[::-1])[::-1]          # La^-T (La^-1 C), as predict_ld forms it
    k = L.psi1(Zl, sf2, al, Xl, np.zeros_like(Xl))
    return dict(k=k, a=R._fwd_ld(Lk, k.T), b=R._fwd_ld(La, k.T), mean=k.dot(W))


def loo_closed_form(Z, sf2, alpha, beta, Psi2, C, Y, X_mu, block=1, observed=None, include_noise=True):
    """dict (float64 arrays): ``e`` (n, D) the leave-out residuals, ``var`` (n,) their variance (with 1/beta under ``include_noise``), ``lev`` (n,),
    ``sinv`` (n,) [S^-1]_ii, ``mean`` (n, D) the full-data mean, the scores of score_ref.score_from on (e, var) -- row_logp, row_sse, row_chi2, cols,
    terms --, and per block ``lam_max`` (the largest eigenvalue of H) and ``cond_S``; ``not_pd``: the blocks whose S has no Cholesky factor (their
    rows are NaN, and no scores are formed).  Psi2 (M, M) and C (M, D) may be float64 (a device's statistics) or long double."""
    p = parts_ld(Z, sf2, alpha, beta, Psi2, C, X_mu)
    Yl = np.atleast_2d(np.asarray(Y, dtype=LD))
    n = Yl.shape[0]
    a, b, bl = p['a'], p['b'], LD(beta)
    E = Yl - p['mean']
    e, sinv = np.full(E.shape, np.nan, dtype=LD), np.full(n, np.nan, dtype=LD)
    lam, cond, not_pd = [], [], []
    for j, G in enumerate(blocks(n, block)):
        H = bl * b[:, G].T.dot(b[:, G])
        Sm = np.eye(len(G), dtype=LD) - H
        lam.append(np.linalg.eigvalsh(H.astype(float))[-1])
        try:
            Ls = R._chol_ld(Sm)
        except np.linalg.LinAlgError:
            not_pd.append(j)
            cond.append(np.inf)
            continue
        Xs = R._fwd_ld(Ls, np.eye(len(G), dtype=LD))
        e[G] = Xs.T.dot(Xs.dot(E[G]))
        sinv[G] = np.sum(Xs * Xs, axis=0)
        cond.append(np.linalg.cond(Sm.astype(float)))
    var = LD(sf2) - np.sum(a * a, axis=0) + (sinv - 1) / bl + (1 / bl if include_noise else 0)
    f = lambda x: np.asarray(x, dtype=float)          # noqa: E731
    out = dict(e=f(e), var=f(var), lev=f(bl * np.sum(b * b, axis=0)), sinv=f(sinv), mean=f(p['mean']), lam_max=np.array(lam), cond_S=np.array(cond),
               not_pd=not_pd)
    if np.isfinite(out['var']).all():
        out.update(S.score_from(out['e'], np.zeros_like(out['e']), out['var'][:, None], observed))
    return out


def loo_refit(Z, sf2, alpha, beta, Y, X_mu, block=1, include_noise=True):
    """dict: ``e`` (n, D) and ``var`` (n,) as long-double arrays, from one refit per block."""
    Xl, Yl = np.atleast_2d(np.asarray(X_mu, dtype=LD)), np.atleast_2d(np.asarray(Y, dtype=LD))
    n = Xl.shape[0]
    k, Psi2, C, yy = statistics_ld(Z, sf2, alpha, Y, X_mu)
    e, var = np.empty(Yl.shape, dtype=LD), np.empty(n, dtype=LD)
    for G in blocks(n, block):
        P2, Cg, yyg = Psi2 - k[G].T.dot(k[G]), C - k[G].T.dot(Yl[G]), yy - np.sum(Yl[G] * Yl[G])
        assert yyg >= 0
        m, v = R.predict_ld(Z, sf2, alpha, beta, P2, Cg, Xl[G])
        e[G] = Yl[G] - m
        var[G] = v[:, 0] + (LD(1) / LD(beta) if include_noise else 0)
    return dict(e=e, var=var)
