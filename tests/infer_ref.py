"""numpy reference of latent inference for new rows (gp_infer_objective / gp_infer_latent): the per-row bound with q(u) frozen at the trained
optimum, its gradients, and a CPU engine with ShardEngine's inference surface for the host-logic tests.  Built on tests/predict_ref.py
(posterior_parts, predict) and oracle/literal.py (psi1, psi2_point).  Shared by tests/test_infer_cpu.py and tests/test_gpu_infer.py."""
import numpy as np

from oracle import literal as L
import predict_ref as R

softplus = lambda r: np.log1p(np.exp(r))
softplus_inv = lambda s: np.log(np.expm1(s))
sigmoid = lambda r: 1.0 / (1.0 + np.exp(-r))


class Model(object):
    """The frozen model: Z, sf2, alpha, beta and the training statistics Psi2, C -> W = beta P C and B = Ki - P."""

    def __init__(self, Z, sf2, alpha, beta, Psi2, C):
        self.Z, self.sf2, self.alpha, self.beta = np.asarray(Z, dtype=float), float(sf2), np.asarray(alpha, dtype=float).reshape(-1), float(beta)
        self.Psi2, self.C = np.asarray(Psi2, dtype=float), np.asarray(C, dtype=float)
        p = R.posterior_parts(self.Z, self.sf2, self.alpha, self.beta, self.Psi2, self.C)
        self.W, self.B = p['W'], p['B']
        self.D = self.C.shape[1]

    def cols(self, cols):
        return np.arange(self.D) if cols is None else np.asarray(cols, dtype=int).reshape(-1)


def objective_row(mdl, y, cols, mu, S, drop=None):
    """(L, dL/dmu, dL/dS) of one row: the formulas of DESIGN.md section 12, term by term.  ``drop`` (tests of the tests): 'kl_grad' leaves the KL
    term out of the gradients, 'psi2' the psi2 term out of the value."""
    Z, sf2, alpha, beta = mdl.Z, mdl.sf2, mdl.alpha, mdl.beta
    c = mdl.cols(cols)
    Do = len(c)
    Wo = mdl.W[:, c]
    G = Wo.dot(Wo.T) - Do * mdl.B
    yo = y[c]
    k = L.psi1(Z, sf2, alpha, mu[None], S[None])[0]
    P2 = L.psi2_point(Z, sf2, alpha, mu, S)
    v = Wo.dot(yo)
    T = G * P2
    val = -0.5 * Do * np.log(2 * np.pi / beta) - 0.5 * beta * (yo.dot(yo) - 2 * k.dot(v) + (0.0 if drop == 'psi2' else np.sum(T)) + Do * sf2) \
        - 0.5 * np.sum(mu ** 2 + S - np.log(S) - 1)
    u, w = alpha / (alpha * S + 1), alpha / (2 * alpha * S + 1)
    d = mu[None, :] - Z
    dk_mu = (k * v).dot(-u * d)
    dk_S = (k * v).dot(0.5 * (u * u * d * d - u))
    db = mu - (Z[:, None, :] + Z[None, :, :]) / 2
    dp_mu = np.einsum('ab,abq->q', T, -2 * w * db)
    dp_S = np.einsum('ab,abq->q', T, 2 * w * w * db * db - w)
    gmu = -0.5 * beta * (-2 * dk_mu + dp_mu)
    gS = -0.5 * beta * (-2 * dk_S + dp_S)
    if drop != 'kl_grad':
        gmu = gmu - mu
        gS = gS - 0.5 * (1 - 1 / S)
    return val, gmu, gS


def objective(mdl, Y, cols, X_mu, X_S, xs_is_raw=False, drop=None):
    """(L (n,), grad_mu (n, Q), grad_S (n, Q)); grad_S with respect to the raw value when ``xs_is_raw``."""
    Y, X_mu, X_S = np.atleast_2d(Y), np.atleast_2d(X_mu), np.atleast_2d(X_S)
    n, Q = X_mu.shape
    Lv, gm, gs = np.empty(n), np.empty((n, Q)), np.empty((n, Q))
    for i in range(n):
        S = softplus(X_S[i]) if xs_is_raw else X_S[i]
        Lv[i], gm[i], g = objective_row(mdl, Y[i], cols, X_mu[i], S, drop)
        gs[i] = g * sigmoid(X_S[i]) if xs_is_raw else g
    return Lv, gm, gs


def objective_via_predict(mdl, Y, cols, X_mu, X_S):
    """The same L from the posterior predictive: -D_o/2 ln(2 pi/beta) - beta/2 sum_{d in O} [(y_d - mean_d)^2 + var_d] - KL (the first oracle)."""
    c = mdl.cols(cols)
    mean, var = R.predict(mdl.Z, mdl.sf2, mdl.alpha, mdl.beta, mdl.Psi2, mdl.C, X_mu, X_S)
    e = ((np.atleast_2d(Y)[:, c] - mean[:, c]) ** 2 + var[:, c]).sum(1)
    KL = 0.5 * (X_mu ** 2 + X_S - np.log(X_S) - 1).sum(1)
    return -0.5 * len(c) * np.log(2 * np.pi / mdl.beta) - 0.5 * mdl.beta * e - KL


def objective_ld(mdl, Y, cols, X_mu, X_S):
    """L in 80-bit long double from the same float64 statistics (predict_ref.predict_ld gives mean and variance)."""
    LD = np.longdouble
    c = mdl.cols(cols)
    mean, var = R.predict_ld(mdl.Z, mdl.sf2, mdl.alpha, mdl.beta, mdl.Psi2, mdl.C, X_mu, X_S)
    Y, X_mu, X_S = np.asarray(np.atleast_2d(Y), dtype=LD), np.asarray(X_mu, dtype=LD), np.asarray(X_S, dtype=LD)
    e = ((Y[:, c] - mean[:, c]) ** 2 + var[:, c]).sum(1)
    KL = (X_mu ** 2 + X_S - np.log(X_S) - 1).sum(1) / 2
    return -LD(len(c)) / 2 * np.log(2 * LD(np.pi) / LD(mdl.beta)) - LD(mdl.beta) / 2 * e - KL


def optimise_row(mdl, y, cols, mu0, S0, method='L-BFGS-B', maxiter=500):
    """Reference optimiser over (mu, softplus-raw S) from the start (mu0, S0): (mu, S, L)."""
    import scipy.optimize as so
    Q = len(mu0)

    def f(x):
        val, gm, gs = objective_row(mdl, y, cols, x[:Q], softplus(x[Q:]))
        return -val, -np.concatenate((gm, gs * sigmoid(x[Q:])))
    x0 = np.concatenate((mu0, softplus_inv(np.asarray(S0, dtype=float))))
    opts = dict(maxiter=maxiter, gtol=1e-9, ftol=1e-15) if method == 'L-BFGS-B' else dict(maxiter=4 * maxiter, gtol=1e-8)
    r = so.minimize(f, x0, jac=True, method=method, options=opts)
    return r.x[:Q], softplus(r.x[Q:]), -r.fun


class NumpyInferEngine(object):
    """ShardEngine's inference surface on the CPU (tests of Predictor.infer's host logic): the same calls in the same order, every infer_latent
    call recorded in ``calls`` (a class attribute: the Predictor creates the engine itself)."""
    calls = []

    def __init__(self, N_s, D, M, Q, device=0):
        self.D, self.M, self.Q = D, M, Q
        self.state = 'new'

    def set_globals(self, Z, sf2, alpha, beta, N_global=None, step_size=0.0):
        self.g = (Z, sf2, alpha, beta)
        self.state = 'globals'

    def set_local_statistics(self, sum_YYT, Psi2, C, sum_exp_K_ii, KL):
        assert self.state == 'globals'
        self.stats = (Psi2, C)
        self.state = 'stats'

    def global_step(self, sync=True, jitter=0):
        assert self.state == 'stats'
        self.mdl = Model(*(self.g + self.stats))
        self.state = 'ready'

    def infer_latent(self, Y, X_mu, X_S, cols=None, xs_is_raw=False, max_iters=100, gtol=1e-5):
        assert self.state == 'ready' and not xs_is_raw
        Y, X_mu, X_S = np.atleast_2d(Y), np.atleast_2d(X_mu), np.atleast_2d(X_S)
        c = self.mdl.cols(cols)
        assert np.all(np.isfinite(Y[:, c])), 'NaN in an observed column'
        type(self).calls.append(dict(Y=Y.copy(), X_mu=X_mu.copy(), X_S=X_S.copy(), cols=None if cols is None else np.array(cols), max_iters=max_iters))
        out = [optimise_row(self.mdl, Y[i], cols, X_mu[i], X_S[i], maxiter=max_iters) for i in range(Y.shape[0])]
        return (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]), np.zeros(len(out), dtype=np.int32))

    def predict(self, X_mu, X_S=None, include_noise=False, xs_is_raw=False):
        assert self.state == 'ready'
        m = self.mdl
        return R.predict(m.Z, m.sf2, m.alpha, m.beta, m.Psi2, m.C, X_mu, X_S, include_noise)

    def close(self):
        self.state = 'closed'


def issue_problem(seed=5):
    """The optimiser test's model and new rows: N 600, M 16 (Z = 16 training latents), Q 2, D 8, sf2 1, alpha (1, 1), beta 50, X_S 0.02,
    Y = sin(XA) + XA/2 + noise; 40 new rows, columns 0-4 observed, started at the nearest training output, variance 0.5."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(seed)
    M, Q, D, N = 16, 2, 8, 600
    sf2, alpha, beta = 1.0, np.array([1.0, 1.0]), 50.0
    Xm = rng.normal(size=(N, Q))
    Xs = np.full((N, Q), 0.02)
    A = rng.normal(size=(Q, D))
    f = lambda X: np.sin(X.dot(A)) + 0.5 * X.dot(A)
    Y = f(Xm) + rng.normal(size=(N, D)) / np.sqrt(beta)
    Z = Xm[rng.choice(N, M, replace=False)].copy()
    n = 40
    Xt = rng.normal(size=(n, Q)) * 0.8
    Yt = f(Xt) + rng.normal(size=(n, D)) / np.sqrt(beta)
    cols = [0, 1, 2, 3, 4]
    _, ind = cKDTree(Y[:, cols]).query(Yt[:, cols])
    return dict(M=M, Q=Q, D=D, N=N, sf2=sf2, alpha=alpha, beta=beta, X_mu=Xm, X_S=Xs, Y=Y, Z=Z, Yt=Yt, Xt=Xt, cols=cols, hidden=[5, 6, 7], X0=Xm[ind],
                S0=np.full((n, Q), 0.5))
