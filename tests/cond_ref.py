"""Long-double references of the posterior conditioned on extra observed rows (gp_condition_set / gp_condition_predict),
built on tests/predict_ref.py, and the error bounds the device is held to.  Shared by tests/test_cond_ref_cpu.py and tests/test_gpu_condition.py.

cond_closed_form: the rank-m update as the device forms it -- S = I + beta B_c B_c^T = L L^T, V = L^-1 B_c, T = L^-1 (Y_c - M_c), u = V b.
cond_refit: the same model the long way round -- K_c^T K_c and K_c^T Y_c added to the statistics, then predict_ld."""
import numpy as np

import predict_ref as R
from oracle import literal as L

LD = R.LD
EPS = np.finfo(float).eps


def _upper_solve(Lm, B):
    """Lm^-T B for lower-triangular Lm: the upper solve as a reversed lower one."""
    return R._fwd_ld(Lm.T[::-1, ::-1], np.asarray(B, dtype=LD)[::-1])[::-1]


def cond_closed_form(Z, sf2, alpha, beta, Psi2, C, Xc, Yc, X):
    """The formulas of the header in long double, from the float64 statistics.  A dict: mean, var (the model as it is; var (n,)), mean_c, var_c
    (conditioned), reduction = beta |u|^2, and what the bounds are made of: S (m, m), h = B_c b (m, n), Rs = S^-1 (Y_c - M_c) (m, D), Mc (m, D),
    a2, b2 (n,), abs_mean = |k| |W| and abs_upd = beta |u|^T |T| (n, D): the sums of the absolute values of the terms of mean and of its update."""
    Z, alpha = np.asarray(Z, dtype=LD), np.asarray(alpha, dtype=LD)
    Xc, X = np.atleast_2d(np.asarray(Xc, dtype=LD)), np.atleast_2d(np.asarray(X, dtype=LD))
    Yc = np.atleast_2d(np.asarray(Yc, dtype=LD))
    sf2, beta = LD(sf2), LD(beta)
    K = L.rbf_gram(Z, sf2, alpha)
    Lk, La = R._chol_ld(K), R._chol_ld(K + beta * np.asarray(Psi2, dtype=LD))
    W = beta * _upper_solve(La, R._fwd_ld(La, C))
    kc = L.psi1(Z, sf2, alpha, Xc, np.zeros_like(Xc))
    k = L.psi1(Z, sf2, alpha, X, np.zeros_like(X))
    Bc = R._fwd_ld(La, kc.T).T                                  # (m, M)
    Mc = kc.dot(W)
    a, b = R._fwd_ld(Lk, k.T), R._fwd_ld(La, k.T)               # (M, n)
    mean, a2, b2 = k.dot(W), np.sum(a * a, axis=0), np.sum(b * b, axis=0)
    var = sf2 - a2 + b2
    m = Xc.shape[0]
    S = np.eye(m, dtype=LD) + beta * Bc.dot(Bc.T)
    Ls = R._chol_ld(S)
    V, T = R._fwd_ld(Ls, Bc), R._fwd_ld(Ls, Yc - Mc)
    u = V.dot(b)                                                # (m, n)
    red = beta * np.sum(u * u, axis=0)
    return dict(mean=mean, var=var, mean_c=mean + beta * u.T.dot(T), var_c=var - red, reduction=red, S=S, h=Bc.dot(b), Rs=_upper_solve(Ls, T), Mc=Mc,
                a2=a2, b2=b2, abs_mean=np.abs(k).dot(np.abs(W)), abs_upd=beta * np.abs(u).T.dot(np.abs(T)))


def cond_refit(Z, sf2, alpha, beta, Psi2, C, Xc, Yc, X):
    """(mean (n, D), var (n,)) of the model whose statistics are Psi2 + K_c^T K_c and C + K_c^T Y_c, in long double (predict_ld)."""
    Zl, al = np.asarray(Z, dtype=LD), np.asarray(alpha, dtype=LD)
    Xc = np.atleast_2d(np.asarray(Xc, dtype=LD))
    kc = L.psi1(Zl, LD(sf2), al, Xc, np.zeros_like(Xc))
    Psi2c = np.asarray(Psi2, dtype=LD) + kc.T.dot(kc)
    Cc = np.asarray(C, dtype=LD) + kc.T.dot(np.atleast_2d(np.asarray(Yc, dtype=LD)))
    mean, var = R.predict_ld(Z, sf2, alpha, beta, Psi2c, Cc, X)
    return mean, var[:, 0]


def cond_bounds(ref, tol, sf2, beta, M):
    """The bounds on the device's mean', var' and reduction against ``ref`` (cond_closed_form), derived as DESIGN.md section 19 derives its own.
    ``tol`` is test_gpu_score._tol's bound on gp_predict: tol_m = tol max(1, |mean|) on a mean, tol_v = tol sf2 on a variance -- and on every
    product of two factor rows, so on every entry of h = B_c b and of B_c B_c^T.  Then |dh|_2 <= sqrt(m) tol_v, |dS|_2 <= m beta tol_v, and
    with |S^-1|_2 <= 1:
      reduction = beta h^T S^-1 h:     |d reduction| <= beta (2 |h|_2 sqrt(m) tol_v + |h|_2^2 m beta tol_v)
      var' = var - reduction:          |d var'| <= tol_v + |d reduction|
      Rs = S^-1 (Y_c - M_c):           |d Rs[:, d]|_2 <= sqrt(m) tol_m(M_c[:, d]) + m beta tol_v |Rs[:, d]|_2
      mean' = mean + beta h^T Rs:      |d mean'| <= tol_m + beta (sqrt(m) tol_v |Rs[:, d]|_2 + |h|_2 |d Rs[:, d]|_2)
    plus c eps times the sum of the absolute values of the terms of each sum (c = the number of terms + 16: one rounding per addition, a few for
    the products), as section 18 adds them: var' sums sf2, |a|^2, |b|^2 and beta |u|^2 (2 M + m terms), mean' its M + m products.
    Returns (b_mean (n, D), b_var (n,), b_red (n,)) as float64."""
    f = lambda x: np.asarray(x, dtype=np.float64)       # noqa: E731
    m = ref['S'].shape[0]
    tol_v = tol * sf2
    hn = f(np.sqrt(np.sum(ref['h'] ** 2, axis=0)))                       # (n,)
    Rn = f(np.sqrt(np.sum(ref['Rs'] ** 2, axis=0)))                      # (D,)
    tol_mc = tol * np.maximum(1.0, f(np.max(np.abs(ref['Mc']), axis=0)))  # (D,)
    d_red = beta * (2 * hn * np.sqrt(m) * tol_v + hn ** 2 * m * beta * tol_v)
    c_var = (2 * M + m + 16) * EPS * f(sf2 + ref['a2'] + ref['b2'] + ref['reduction'])
    b_red = d_red + c_var
    b_var = tol_v + d_red + c_var
    d_Rs = np.sqrt(m) * tol_mc + m * beta * tol_v * Rn
    tol_m = tol * np.maximum(1.0, np.abs(f(ref['mean'])))
    b_mean = tol_m + beta * (np.sqrt(m) * tol_v * Rn[None, :] + hn[:, None] * d_Rs[None, :]) + (M + m + 16) * EPS * f(ref['abs_mean'] + ref['abs_upd'])
    return b_mean, b_var, b_red


# ---- the cases both test files run: (N_s, M, Q, D) of the two models, the set sizes, and the seeded inputs -----------------------------------
SHAPES = [(300, 20, 2, 3), (520, 130, 3, 130)]
MS = [1, 5, 128, 129, 300]
NS = [1, 300]


def model_seed(shape):
    """The seed of test_gpu_score._model for a shape: M + Q + D, as test_gpu_score._Case takes it (25 and 263).  With these and cond_inputs'
    seed 1000 m + n the long-double reference satisfies the condition of test 1 (the bound on var' below 1e-3 of the smallest var') at every
    case: tests/test_cond_ref_cpu.py checks it."""
    return shape[1] + shape[2] + shape[3]


def cond_inputs(Q, D, m, n):
    """Seeded conditioning rows (Xc (m, Q), Yc (m, D)) and queries X (n, Q): the queries spread like the training embeddings, the conditioning
    inputs at half that spread -- in the middle of the training inputs, where the rows' leverages beta |b|^2 and with them |h|_2 are small: with
    rows spread like the data the m^2 term of the bound on var' reaches 5e-3 of the smallest var' at m = 300, and the bound would not be sharp.
    The outputs are a smooth function of the input plus noise of the model's size.  From m = 2 on the last conditioning input repeats the first
    (with its own output); from n = 2 on the last query IS the first conditioning input."""
    rs = np.random.RandomState(1000 * m + n)
    Xc, X = 0.5 * rs.randn(m, Q), rs.randn(n, Q)
    Yc = np.sin(Xc.dot(rs.randn(Q, D))) + 0.3 * rs.randn(m, D)
    if m >= 2:
        Xc[-1] = Xc[0]
    if n >= 2:
        X[-1] = Xc[0]
    return Xc, Yc, X
