"""Shift-exact extended-precision reference of every evaluation path (numpy long double, x86 80-bit: eps 1.08e-19).

The RBF-ARD statistics depend on the latent points X_mu and the inducing points Z only through differences, so adding one constant c to every
coordinate of both changes nothing but the mu^2 term of the KL.  This module computes every quantity that way: each (mu - z) and (z_m - z_m') is
FORMED AS A DIFFERENCE FIRST, and only differences are multiplied.  With inputs on the 2^-24 grid of ``make_inputs`` and a shift of at most 2^16
those differences are exact (43 bits), so the evaluation at a shifted input is the evaluation of the same problem and the results do not move
(tests/test_shift_ref_cpu.py holds that to 1e-15).  The float64 oracle (oracle/factorised.py) expands the squares and cannot serve here.

Nothing is imported from oracle/; the formulas are those of SURVEY.md section 7, DESIGN.md sections 11 and 12 (tests/predict_ref.py,
tests/infer_ref.py), restated with differences.  Shared by tests/test_shift_ref_cpu.py and tests/test_gpu_translation.py."""
import numpy as np

LD = np.longdouble
SHIFTS = (0.0, 2.0 ** 6, 2.0 ** 12, 2.0 ** 16)
GRID = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ long-double linear algebra
def chol_ld(A):
    """Lower Cholesky factor (left-looking, one matrix-vector product per column)."""
    n = A.shape[0]
    L = np.zeros((n, n), dtype=A.dtype)
    for j in range(n):
        v = A[j:, j] - L[j:, :j].dot(L[j, :j])
        if not v[0] > 0:
            raise np.linalg.LinAlgError('not positive definite at column %d' % j)
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L


def tri_inv_ld(L):
    """Inverse of a lower-triangular matrix (forward substitution, row by row)."""
    n = L.shape[0]
    X = np.zeros((n, n), dtype=L.dtype)
    for i in range(n):
        r = -L[i, :i].dot(X[:i, :])
        r[i] += 1
        X[i, :] = r / L[i, i]
    return X


def spd_inv_logdet_ld(A):
    """(A^-1, ln det A, L^-1) of a symmetric positive definite matrix."""
    L = chol_ld(A)
    X = tri_inv_ld(L)
    return X.T.dot(X), 2 * np.sum(np.log(np.diag(L))), X


# ------------------------------------------------------------------------------------------------ inputs
def make_inputs(N, D, M, Q, regime, seed, n_new=16):
    """Seeded problem on the 2^-24 grid with |x| < 8: X_mu uniform in a box, Z = M of its rows chosen farthest-point first (spread over the data,
    well separated) plus a small offset, alpha from the closest pair of inducing points so that their correlation is exp(-2) -- K_mm and
    K_mm + beta Psi2 stay well conditioned at every Q -- and variances with alpha S in [0.05, 0.55].  ``n_new`` new rows (Xt, St, Yt) for
    predict / infer."""
    assert M <= N
    rs = np.random.RandomState(seed)
    snap = lambda x: np.round(x / GRID) * GRID
    X = snap(rs.uniform(-6.5, 6.5, size=(N, Q)))
    idx = [int(rs.randint(N))]
    dist = np.sum((X - X[idx[0]]) ** 2, axis=1)
    while len(idx) < M:
        idx.append(int(np.argmax(dist)))
        dist = np.minimum(dist, np.sum((X - X[idx[-1]]) ** 2, axis=1))
    pair2 = np.sum((X[idx][:, None, :] - X[idx][None, :, :]) ** 2, axis=2) + np.diag(np.full(M, np.inf))
    dmin2 = float(np.min(pair2)) if M > 1 else 1.0               # squared distance of the closest pair of inducing points
    Z = snap(X[idx] + rs.uniform(-0.05, 0.05, size=(M, Q)) * np.sqrt(dmin2 / Q))
    alpha = 4.0 / dmin2 * rs.uniform(0.8, 1.25, size=Q)
    W = rs.randn(Q, D) * np.sqrt(alpha)[:, None] / np.sqrt(Q)
    f = lambda x: np.sin(x.dot(W)) + 0.5 * np.cos(2.0 * x.dot(W))
    Y = f(X) + 0.1 * rs.randn(N, D)
    X_S = np.zeros((N, Q)) if regime == 'A' else rs.uniform(0.05, 0.55, size=(N, Q)) / alpha[None, :]
    pick = rs.randint(N, size=n_new)
    Xt = snap(np.clip(X[pick] + rs.uniform(-0.5, 0.5, size=(n_new, Q)) * np.sqrt(dmin2 / Q), -7.5, 7.5))
    St = rs.uniform(0.05, 0.55, size=(n_new, Q)) / alpha[None, :]
    Yt = f(Xt) + 0.1 * rs.randn(n_new, D)
    for a in (X, Z, Xt):
        assert np.max(np.abs(a)) < 8.0 and np.all(a == snap(a))
    return dict(N=N, D=D, M=M, Q=Q, regime=regime, shift=0.0, Y=Y, X_mu=X, X_S=X_S, Z=Z, sf2=1.0, alpha=alpha, beta=10.0, Xt=Xt, St=St, Yt=Yt)


def shifted(d, c):
    """The same problem with c added to every coordinate of X_mu, Z and the new rows: exact in float64 (16 + 3 + 24 = 43 bits), asserted."""
    out = dict(d)
    out['shift'] = float(c)
    for k in ('X_mu', 'Z', 'Xt'):
        out[k] = d[k] + c
        assert np.all(out[k] - c == d[k]), '%s + %g is not exact' % (k, c)
    return out


# ------------------------------------------------------------------------------------------------ statistics
def _params(d, dtype):
    T = lambda x: np.asarray(x, dtype=dtype)
    return T(d['Z']), dtype(d['sf2']), T(d['alpha']), dtype(d['beta'])


def kmm(Z, sf2, alpha):
    dz = Z[:, None, :] - Z[None, :, :]
    return sf2 * np.exp(-np.sum(alpha * dz * dz, axis=2) / 2), dz


def psi1(Z, sf2, alpha, mu, S):
    """(Psi1 (n, M), u (n, Q), d = mu - z (n, M, Q))."""
    d = mu[:, None, :] - Z[None, :, :]
    d1 = alpha * S + 1
    u = alpha / d1
    c1 = sf2 / np.sqrt(np.prod(d1, axis=1))
    return c1[:, None] * np.exp(-np.einsum('nq,nmq->nm', u, d * d) / 2), u, d


def psi2_points(sf2, alpha, S, d, dz2):
    """psi2_n (n, M, M) of the points whose differences d = mu - z (n, M, Q) are given; dz2 = (z_m - z_m')^2 as (Q, M*M).
    exponent = lnE_nm + lnE_nm' - 1/4 sum_q (alpha_q - w_nq)(z_mq - z_m'q)^2, lnE_nm = -1/2 sum_q w_nq (mu_nq - z_mq)^2."""
    n, M, _ = d.shape
    d2 = 2 * alpha * S + 1
    w = alpha / d2
    c2 = sf2 * sf2 / np.sqrt(np.prod(d2, axis=1))
    lnE = -np.einsum('nq,nmq->nm', w, d * d) / 2
    coup = -(alpha - w).dot(dz2).reshape(n, M, M) / 4
    return c2[:, None, None] * np.exp(lnE[:, :, None] + lnE[:, None, :] + coup), w, d2


def statistics(d, dtype=LD, chunk=32):
    """Psi1, Psi2 = sum_n psi2_n, C = Psi1^T Y, Psi0 = N sf2, KL and sum_YYT, in ``dtype`` (long double: the reference; float64: the plain
    direct-difference evaluation the CPU test holds against it)."""
    Z, sf2, alpha, _ = _params(d, dtype)
    mu, S, Y = (np.asarray(d[k], dtype=dtype) for k in ('X_mu', 'X_S', 'Y'))
    N, M = mu.shape[0], Z.shape[0]
    regA = bool(np.all(d['X_S'] == 0))
    P1, _, dd = psi1(Z, sf2, alpha, mu, S)
    out = dict(Psi1=P1, C=P1.T.dot(Y), Psi0=sf2 * N, sum_YYT=np.sum(Y * Y), regime_A=regA)
    if regA:
        out['Psi2'], out['KL'] = P1.T.dot(P1), dtype(0)
        return out
    _, dz = kmm(Z, sf2, alpha)
    dz2 = np.ascontiguousarray((dz * dz).reshape(M * M, -1).T)
    Psi2 = np.zeros((M, M), dtype=dtype)
    for lo in range(0, N, chunk):
        p2, _, _ = psi2_points(sf2, alpha, S[lo:lo + chunk], dd[lo:lo + chunk], dz2)
        Psi2 += p2.sum(0)
    out['Psi2'] = Psi2
    out['KL'] = np.sum(S - np.log(S) + mu * mu - 1) / 2
    return out


def kl_shift(d0, c):
    """KL(shifted by c) - KL(unshifted) in closed form: sum_nq ((mu + c)^2 - mu^2) / 2 = c sum mu + N Q c^2 / 2 (zero for fixed embeddings)."""
    if np.all(d0['X_S'] == 0):
        return LD(0)
    mu, c = np.asarray(d0['X_mu'], dtype=LD), LD(c)
    return c * np.sum(mu) + mu.size * c * c / 2


# ------------------------------------------------------------------------------------------------ the full evaluation
def evaluate(d, chunk=32):
    """F and every gradient of one evaluation on a single shard, long double.  grad_X_mu carries the -mu of the KL term in BOTH regimes, as the
    library and the reference do (the per-point gradient is only meaningful for free embeddings); grad_X_S is None for fixed embeddings."""
    Z, sf2, a, b = _params(d, LD)
    mu, S, Y = (np.asarray(d[k], dtype=LD) for k in ('X_mu', 'X_S', 'Y'))
    N, D = Y.shape
    M, Q = Z.shape
    st = statistics(d, LD, chunk)
    regA = st['regime_A']
    Psi2, C, Psi0, KL, sumYY = st['Psi2'], st['C'], st['Psi0'], st['KL'], st['sum_YYT']
    K, dz = kmm(Z, sf2, a)
    A = K + b * Psi2
    Ki, ldK, _ = spd_inv_logdet_ld(K)
    P, ldA, _ = spd_inv_logdet_ld(A)
    E = P.dot(C)
    two_pi = 2 * np.arccos(LD(-1))
    trKi, trP, trCE = np.sum(Ki * Psi2), np.sum(P * Psi2), np.sum(C * E)
    F = (-N * D * np.log(two_pi) / 2 + D * N * np.log(b) / 2 + D * ldK / 2 - D * ldA / 2 - b * sumYY / 2 - b * D * Psi0 / 2 + b * D * trKi / 2
         + b * b * trCE / 2 - KL)
    EEt = E.dot(E.T)
    Abar = b * b * E
    Bbar = b * D * (Ki - P) / 2 - b ** 3 * EEt / 2
    dFdK = D * (Ki - P) / 2 - b * D * Ki.dot(Psi2).dot(Ki) / 2 - b * b * EEt / 2
    grad_beta = (N * D / b / 2 - D * trP / 2 - sumYY / 2 - D * Psi0 / 2 + D * trKi / 2 + b * trCE - b * b * np.sum(E * Psi2.dot(E)) / 2)
    V = dFdK * K
    dz2 = dz * dz
    gZ = -a[None, :] * np.einsum('ab,abq->aq', V + V.T, dz)
    ga = -np.einsum('ab,abq->q', V, dz2) / 2
    grad_sf2 = (np.sum(V) + np.sum(Abar * C) + 2 * np.sum(Bbar * Psi2) - b * D * Psi0 / 2) / sf2
    # ---- Psi1 part
    P1, u, dd = psi1(Z, sf2, a, mu, S)
    d1 = a * S + 1
    G = Y.dot(Abar.T)
    if regA:
        G = G + P1.dot(Bbar + Bbar.T)
    H = G * P1
    h = H.sum(1)
    Hd = np.einsum('nm,nmq->nq', H, dd)
    Hd2 = np.einsum('nm,nmq->nq', H, dd * dd)
    gZ = gZ + np.einsum('nm,nq,nmq->mq', H, u, dd)
    ga = ga - np.sum(Hd2 / (d1 * d1) + (S / d1) * h[:, None], axis=0) / 2
    gmu = -mu - u * Hd
    gS = None
    if not regA:
        gS = -(1 - 1 / S) / 2 + u * u * Hd2 / 2 - u * h[:, None] / 2
        dz2f = np.ascontiguousarray(dz2.reshape(M * M, Q).T)
        Tsum = np.zeros((M, M), dtype=LD)
        for lo in range(0, N, chunk):
            hi = min(N, lo + chunk)
            p2, w, d2 = psi2_points(sf2, a, S[lo:hi], dd[lo:hi], dz2f)
            T = p2 * Bbar[None, :, :]
            Ts = T + T.transpose(0, 2, 1)                       # both orders of a pair
            Tsum += T.sum(0)
            rs_ = Ts.sum(2)                                     # (n, M)
            sr = T.sum((1, 2))                                  # (n,)
            dn = dd[lo:hi]
            Pd = np.matmul(Ts, dn)                              # (n, M, Q): sum_b Ts[a, b] (mu - z_b)
            rd = np.einsum('nm,nmq->nq', rs_, dn)               # sum_ab Ts[a, b] (mu - z_a) = 2 sum_ab T (mu - zbar_ab)
            # sum_ab T (mu - zbar_ab)^2 with mu - zbar_ab = ((mu - z_a) + (mu - z_b)) / 2
            quad = (np.einsum('nm,nmq->nq', rs_, dn * dn) + np.einsum('nmq,nmq->nq', Pd, dn)) / 4
            gZ += np.einsum('nq,nmq->mq', w, rs_[:, :, None] * dn + Pd) / 2
            ga += np.sum(-quad / (d2 * d2) - (S[lo:hi] / d2) * sr[:, None], axis=0)
            gmu[lo:hi] += -w * rd
            gS[lo:hi] += 2 * w * w * quad - w * sr[:, None]
        gZ += -a[None, :] * np.einsum('ab,abq->aq', Tsum + Tsum.T, dz) / 2
        ga += -np.einsum('ab,abq->q', Tsum, dz2) / 4
    return dict(F=F, grad_Z=gZ, grad_alpha=ga, grad_sf2=grad_sf2, grad_beta=grad_beta, grad_X_mu=gmu, grad_X_S=gS, stats=st, Kmm=K, A=A,
                Ki=Ki, P=P, E=E, cond_Kmm=float(np.linalg.cond(K.astype(np.float64))), cond_A=float(np.linalg.cond(A.astype(np.float64))))


# ------------------------------------------------------------------------------------------------ predict and infer (q(u) frozen)
def model(d, st):
    """W = beta (K_mm + beta Psi2)^-1 C, B = K_mm^-1 - (K_mm + beta Psi2)^-1 and the two inverse factors, from the statistics ``st``."""
    Z, sf2, a, b = _params(d, LD)
    K, dz = kmm(Z, sf2, a)
    Ki, _, Lki = spd_inv_logdet_ld(K)
    P, _, Lai = spd_inv_logdet_ld(K + b * st['Psi2'])
    return dict(Z=Z, sf2=sf2, alpha=a, beta=b, W=b * P.dot(st['C']), B=Ki - P, Lki=Lki, Lai=Lai, dz2=np.ascontiguousarray((dz * dz).reshape(Z.shape[0] ** 2, -1).T))


def predict(mdl, X_mu, X_S=None, include_noise=False):
    """(mean (n, D), var): var (n, 1) for X_S None (sf2 - |Lk^-1 k|^2 + |La^-1 k|^2), (n, D) for uncertain inputs (tests/predict_ref.py)."""
    X_mu = np.atleast_2d(np.asarray(X_mu, dtype=LD))
    noise = 1 / mdl['beta'] if include_noise else LD(0)
    if X_S is None:
        k, _, _ = psi1(mdl['Z'], mdl['sf2'], mdl['alpha'], X_mu, np.zeros_like(X_mu))
        p, q = mdl['Lki'].dot(k.T), mdl['Lai'].dot(k.T)
        return k.dot(mdl['W']), (mdl['sf2'] - np.sum(p * p, axis=0) + np.sum(q * q, axis=0) + noise)[:, None]
    X_S = np.atleast_2d(np.asarray(X_S, dtype=LD))
    k, _, dd = psi1(mdl['Z'], mdl['sf2'], mdl['alpha'], X_mu, X_S)
    p2, _, _ = psi2_points(mdl['sf2'], mdl['alpha'], X_S, dd, mdl['dz2'])
    mean = k.dot(mdl['W'])
    var = mdl['sf2'] - np.einsum('ab,nab->n', mdl['B'], p2)[:, None] + np.einsum('ad,nab,bd->nd', mdl['W'], p2, mdl['W']) - mean * mean + noise
    return mean, var


def infer_objective(mdl, Y, cols, X_mu, X_S):
    """(L (n,), dL/dmu (n, Q), dL/dS (n, Q)) of new rows over the observed columns ``cols`` (None: all): tests/infer_ref.py objective_row."""
    Y, mu, S = (np.atleast_2d(np.asarray(x, dtype=LD)) for x in (Y, X_mu, X_S))
    c = np.arange(Y.shape[1]) if cols is None else np.asarray(cols, dtype=int).reshape(-1)
    Do, b, sf2, a = len(c), mdl['beta'], mdl['sf2'], mdl['alpha']
    Wo = mdl['W'][:, c]
    G = Wo.dot(Wo.T) - Do * mdl['B']
    yo = Y[:, c]
    k, u, dd = psi1(mdl['Z'], sf2, a, mu, S)
    p2, w, _ = psi2_points(sf2, a, S, dd, mdl['dz2'])
    v = yo.dot(Wo.T)                                                 # (n, M)
    T = G[None, :, :] * p2
    two_pi = 2 * np.arccos(LD(-1))
    val = (-Do * np.log(two_pi / b) / 2 - b * (np.sum(yo * yo, axis=1) - 2 * np.sum(k * v, axis=1) + T.sum((1, 2)) + Do * sf2) / 2
           - np.sum(mu * mu + S - np.log(S) - 1, axis=1) / 2)
    kv = k * v
    dk_mu = -u * np.einsum('nm,nmq->nq', kv, dd)
    dk_S = (u * u * np.einsum('nm,nmq->nq', kv, dd * dd) - u * kv.sum(1)[:, None]) / 2
    Ts = T + T.transpose(0, 2, 1)
    rs_ = Ts.sum(2)
    Pd = np.matmul(Ts, dd)
    quad = (np.einsum('nm,nmq->nq', rs_, dd * dd) + np.einsum('nmq,nmq->nq', Pd, dd)) / 4      # sum_ab T (mu - zbar_ab)^2
    dp_mu = -w * np.einsum('nm,nmq->nq', rs_, dd)                                                # -2 w sum_ab T (mu - zbar_ab)
    dp_S = 2 * w * w * quad - w * T.sum((1, 2))[:, None]
    gmu = -b * (-2 * dk_mu + dp_mu) / 2 - mu
    gS = -b * (-2 * dk_S + dp_S) / 2 - (1 - 1 / S) / 2
    return val, gmu, gS


def rel_err(x, truth):
    """max |x - truth| / max |truth| of a block, in long double."""
    x, truth = np.asarray(x, dtype=LD), np.asarray(truth, dtype=LD)
    s = np.max(np.abs(truth))
    return float(np.max(np.abs(x - truth)) / (s if s > 0 else 1))


# ------------------------------------------------------------------------------------------------ the shapes both test files use
# (name, N, D, M, Q, regime, want_embedding_grads): one shape per kernel family that a width or size switch of the library selects.  N = 300 is ragged
# against the 128-row granule with more than one granule; M = 65 / 130 leave a ragged second / third 64-column slab.
CASES = [
    # fixed embeddings, no per-point gradients: psi1_kernel (Q <= 16), psi1_wide_kernel (17 .. 64), psi1_generic_kernel (beyond); phase 1 on p1v2_kernel,
    # phase 2 on p2_fast8_kernel (Q <= 11) or p2_gen8_kernel on [mu | 1 | mu^2]; D > 104 puts phase 1 on p1_kernel8
    ('fixed_q1', 300, 3, 130, 1, 'A', False), ('fixed_q3', 300, 3, 65, 3, 'A', False), ('fixed_q10', 300, 3, 130, 10, 'A', False),
    ('fixed_q17', 300, 3, 65, 17, 'A', False), ('fixed_q64', 300, 3, 130, 64, 'A', False), ('fixed_q65', 300, 3, 65, 65, 'A', False),
    ('fixed_q10_d105', 300, 105, 130, 10, 'A', False), ('fixed_q17_d105', 300, 105, 130, 17, 'A', False),
    # every variance zero with per-point gradients: the general phase 2 and its point kernel
    ('zero_var_q3', 300, 3, 130, 3, 'A', True),
    # free embeddings: psi2_pairs + psi2_sym (Q <= 12, three slabs), psi2_cols (two slabs, or Q = 13 .. 16), psi2_pairs_mfma + psi2_tile (17 .. 63, table
    # widths 24 / 32 / 64), psi2_generic (Q >= 64)
    ('free_q10', 300, 3, 130, 10, 'B', True), ('free_q12', 300, 3, 130, 12, 'B', True), ('free_q14', 300, 3, 65, 14, 'B', True),
    ('free_q16', 300, 3, 130, 16, 'B', True), ('free_q17', 300, 3, 65, 17, 'B', True), ('free_q25', 300, 3, 130, 25, 'B', True),
    ('free_q52', 300, 3, 65, 52, 'B', True), ('free_q63', 300, 3, 65, 63, 'B', True), ('free_q64', 300, 3, 65, 64, 'B', True),
]
PREDICT_CASES = [('predict_fixed_q10', 300, 3, 130, 10, 'A', False), ('predict_free_q25', 300, 3, 130, 25, 'B', True)]


def case_inputs(case):
    name, N, D, M, Q, regime, _ = case
    return make_inputs(N, D, M, Q, regime, seed=1000 + 7 * Q + M + D)
