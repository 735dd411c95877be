"""Reference for gparml_amd.lbfgs: a DENSE numpy L-BFGS on the concatenated vector -- explicit s, y arrays and the classical two-loop recursion --
with the line search and the keep / skip / restart rules of ``LBFGS`` stated once more, independently (``dense_lbfgs``); ``HostVectors``, the per-point
part of an L-BFGS history held in numpy, so that the split between host globals and "local" vectors runs without a GPU; and the test problems."""
import numpy as np

from gparml_amd.lbfgs import LbfgsHistory

C1, MAX_HALVINGS, CURVATURE = 1e-4, 20, 1e-10
U = 2.0 ** -53


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u) (the convention of tests/gemm_ref.py)."""
    return n * U / (1.0 - n * U)


def dense_direction(pairs, g):
    """Classical two-loop recursion: ``pairs`` = [(s, y), ...] oldest first; returns d = -H g with H0 = (s.y / y.y of the newest pair) I."""
    q = np.array(g, dtype=np.float64)
    a = []
    for s, y in reversed(pairs):
        ai = np.dot(s, q) / np.dot(s, y)
        a.append(ai)
        q = q - ai * y
    if pairs:
        s, y = pairs[-1]
        q = q * (np.dot(s, y) / np.dot(y, y))
    for (s, y), ai in zip(pairs, reversed(a)):
        q = q + (ai - np.dot(y, q) / np.dot(s, y)) * s
    return -q


def dense_lbfgs(f_and_grad, x0, m=10, maxiters=500, max_f_eval=500, xtol=1e-6, ftol=1e-6, gtol=1e-5, perturbed=False, seed=0):
    """L-BFGS on the whole vector ``x0`` with f_and_grad(x) -> (f, g).  Returns (x, flog, evaluations, status, trace); the trace has the
    tuples of ``LBFGS``'s.  ``perturbed``: every gradient entry is multiplied by 1 + 1e-13 u, u uniform in [-1, 1] (seeded)."""
    rng = np.random.RandomState(seed)

    def evaluate(x):
        f, g = f_and_grad(x)
        g = np.array(g, dtype=np.float64)
        if perturbed:
            g = g * (1.0 + 1e-13 * rng.uniform(-1.0, 1.0, g.shape))
        return float(f), g

    x = np.array(x0, dtype=np.float64)
    f, g = evaluate(x)
    evaluations, pairs, trace, flog, iteration, status = 1, [], [], [f], 0, 'Not converged'
    d = -g
    while True:
        if iteration >= maxiters:
            status = 'maxiter exceeded'
            break
        slope = float(np.dot(g, d))
        if slope >= 0:
            if not pairs:
                status = 'converged'
                break
            trace.append(('restart', 'slope'))
            pairs, d = [], -g
            continue
        a = min(1.0, 1.0 / np.sqrt(np.dot(g, g))) if not pairs else 1.0
        accepted = False
        for _ in range(MAX_HALVINGS + 1):
            f_t, g_t = evaluate(x + a * d)
            evaluations += 1
            if evaluations >= max_f_eval:
                break
            accepted = bool(f_t <= f + C1 * a * slope)
            trace.append(('trial', a, f_t, f + C1 * a * slope, accepted))
            if accepted:
                break
            a *= 0.5
        if evaluations >= max_f_eval and not accepted:
            status = 'Maximum number of function evaluations exceeded'
            break
        if not accepted:
            if not pairs:
                status = 'line search failed'
                break
            trace.append(('restart', 'line search'))
            pairs, d = [], -g
            continue
        s, y = a * d, g_t - g
        sy, ss, yy = float(np.dot(s, y)), float(np.dot(s, s)), float(np.dot(y, y))
        kept = bool(sy > CURVATURE * np.sqrt(ss * yy))
        trace.append(('pair', sy, ss, yy, kept))
        if kept:
            pairs = (pairs + [(s, y)])[-m:]
        move = float(np.max(np.abs(s)))
        x, g = x + s, g_t
        flog.append(f_t)
        iteration += 1
        small = move < xtol or abs(f_t - f) < ftol
        f = f_t
        if small or np.dot(g, g) <= gtol:
            status = 'converged'
            break
        d = dense_direction(pairs, g)
    return x, flog, evaluations, status, trace


def decisions(trace):
    """The accept / halve / keep / skip / restart sequence of a trace, without its numbers."""
    out = []
    for ev in trace:
        if ev[0] == 'trial':
            out.append('accept' if ev[4] else 'halve')
        elif ev[0] == 'pair':
            out.append('keep' if ev[4] else 'skip')
        else:
            out.append('restart:' + ev[1])
    return out


def margins(trace):
    """(smallest relative Armijo margin over the trials, smallest relative distance of a pair's s.y from its threshold) of a trace: how far every
    decision is from flipping.  A trial's margin is |bound - f_trial| / |bound|; a pair's is |s.y - thr| / sqrt(s.s y.y) with thr = 1e-10 sqrt(s.s y.y)."""
    arm = min([abs(ev[3] - ev[2]) / abs(ev[3]) for ev in trace if ev[0] == 'trial'] or [np.inf])
    cur = min([abs(ev[1] - CURVATURE * np.sqrt(ev[2] * ev[3])) / np.sqrt(ev[2] * ev[3]) for ev in trace if ev[0] == 'pair'] or [np.inf])
    return arm, cur


class HostVectors(LbfgsHistory):
    """``ResidentLBFGS`` in numpy: the "local" part of the variables, its direction, its latest gradient and its slice of the basis are arrays
    here.  ``problem`` supplies them: the test function evaluates at ``X + step * dir`` and leaves the local gradient in ``grad_latest``."""

    def __init__(self, X):
        self.X = np.array(X, dtype=np.float64)
        self.dir = np.zeros_like(self.X)
        self.grad_latest = None

    def _local_start(self, n_slots):
        self.basis = np.full((2 * n_slots + 1, self.X.size), np.nan)        # as the device's poison mode: only filled vectors may be read
        self.filled = np.zeros(2 * n_slots + 1, dtype=bool)
        self.basis[-1] = self.grad_latest
        self.filled[-1] = True

    def _local_reset(self, n_slots):
        self.filled[:-1] = False

    def _local_dots(self, slot):
        n = (len(self.filled) - 1) // 2
        out = np.zeros((3, 2 * n + 1))
        rows = [2 * n] if slot < 0 else [slot, n + slot, 2 * n]
        for r, i in zip(range(3 - len(rows), 3), rows):
            for j in np.nonzero(self.filled)[0]:
                out[r, j] = np.dot(self.basis[i], self.basis[j])
        return out

    def _local_push(self, slot, step):
        n = (len(self.filled) - 1) // 2
        self.basis[slot] = step * self.dir
        self.basis[n + slot] = self.grad_latest - self.basis[-1]
        self.basis[-1] = self.grad_latest
        self.filled[slot] = self.filled[n + slot] = True

    def _local_direction(self, coef):
        d = np.zeros_like(self.X)
        for j in np.nonzero(self.filled & (coef != 0.0))[0]:
            d = d + coef[j] * self.basis[j]
        self.dir = d

    def _local_update_X(self, step):
        self.X = self.X + step * self.dir

    def _local_largest_move(self, step):
        return float(np.max(np.abs(step * self.dir)))


# ---- problems: f_and_grad(x) on the whole vector
def quadratic(n, cond, seed):
    """f = 1/2 (x - c)^T A (x - c) with A SPD, eigenvalues log-spaced in [1, cond]."""
    rng = np.random.RandomState(seed)
    Qm, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Qm * np.logspace(0.0, np.log10(cond), n)) @ Qm.T
    A = 0.5 * (A + A.T)
    c = rng.standard_normal(n)

    def f_and_grad(x):
        r = x - c
        return 0.5 * float(r @ A @ r), A @ r
    return f_and_grad, A


def rosenbrock_chain(x):
    """sum_i 100 (x_{i+1} - x_i^2)^2 + (1 - x_i)^2."""
    x = np.asarray(x, dtype=np.float64)
    a, b = x[:-1], x[1:]
    f = float(np.sum(100.0 * (b - a * a) ** 2 + (1.0 - a) ** 2))
    g = np.zeros_like(x)
    g[:-1] += -400.0 * a * (b - a * a) - 2.0 * (1.0 - a)
    g[1:] += 200.0 * (b - a * a)
    return f, g


def split_problem(f_and_grad, x0, n_host):
    """The whole-vector problem as LBFGS sees a GPLVM: the first ``n_host`` variables are the optimiser's x, the rest live in a ``HostVectors``
    and are reached through the trial mechanism.  Returns (callback(x, iteration, step) -> (f, g_host), ops, x_host0)."""
    x0 = np.asarray(x0, dtype=np.float64)
    ops = HostVectors(x0[n_host:])

    def callback(x, iteration, step):
        local = ops.X + step * ops.dir if step != 0 else ops.X
        f, g = f_and_grad(np.concatenate([x, local]))
        ops.grad_latest = np.array(g[n_host:])
        return f, np.array(g[:n_host])
    return callback, ops, x0[:n_host].copy()
