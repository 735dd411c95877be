"""Limited-memory BFGS over a parameter vector that is split in two, like ``scg_adapted.SCG_adapted``: the small global part (Z, sf2,
alpha, beta) lives on the host, the big per-point part stays on the shards.  The form is the vector-free L-BFGS of Chen, Wang and Zhou
("Large-scale L-BFGS using MapReduce", NIPS 2014): with the basis b = [s_0 .. s_{n-1}, y_0 .. y_{n-1}, g] every inner product the two-loop
recursion needs is an entry of the Gram matrix G = b b^T, the two loops run on the host on COEFFICIENTS, and the new direction is one linear
combination of the basis.  Per iteration the per-point part costs one pass that refreshes three rows of G (one small collective) and one pass
that writes the direction, whatever the memory is (``gparml_amd.resident.ResidentLBFGS`` on the device vectors of csrc/lbfgs.hip).

``LbfgsHistory`` is the host half: the ring of pairs, G, the host part of every basis vector and the two loops.  Its ``_local_*`` hooks do nothing;
a subclass adds the per-point part behind them.  The optimiser itself is host logic, as SCG and GD are."""
import numpy as np

from .scg_adapted import safe_f_and_grad_f

C1 = 1e-4                 # Armijo: f(x + a d) <= f(x) + C1 a g.d
MAX_HALVINGS = 20
CURVATURE = 1e-10         # a pair is kept only if s.y > CURVATURE sqrt(s.s y.y)


def two_loop_coefficients(G, order, n_slots):
    """The coefficients delta (2 n_slots + 1) of the L-BFGS direction d = sum_j delta_j b_j from the Gram matrix ``G`` alone.  Basis order:
    s_k at k, y_k at n_slots + k, g last; ``order``: the slots that hold a pair, oldest first.  With p = sum_j delta_j b_j every product the
    classical recursion takes is a product of delta with a column of G: start p = -g; newest to oldest a_k = s_k.p / s_k.y_k, p -= a_k y_k;
    p *= s_n.y_n / y_n.y_n of the newest pair; oldest to newest p += (a_k - y_k.p / s_k.y_k) s_k.  The sums delta . G[:, k] cancel where p is
    short next to its terms, so the few hundred operations here run in the host's long double."""
    n, gi = n_slots, 2 * n_slots
    G = np.asarray(G, dtype=np.longdouble)
    delta = np.zeros(2 * n + 1, dtype=np.longdouble)
    delta[gi] = -1.0
    if not order:
        return delta.astype(np.float64)
    a = {}
    for k in reversed(order):
        a[k] = np.dot(delta, G[:, k]) / G[k, n + k]
        delta[n + k] -= a[k]
    new = order[-1]
    delta *= G[new, n + new] / G[n + new, n + new]
    for k in order:
        delta[k] += a[k] - np.dot(delta, G[:, n + k]) / G[k, n + k]
    return delta.astype(np.float64)


class LbfgsHistory(object):
    """Ring, Gram matrix and host part of an L-BFGS history of ``m`` pairs.  ``m + 1`` slots are held: a new pair is written into the spare slot
    before its curvature is known, so a skipped pair never costs a kept one.  The interface ``LBFGS`` drives: start, push, direction, slope,
    reset, update_X, largest_move, grad_norm2, n_pairs, finish."""

    def start(self, g_host, m):
        """An empty history at the point whose gradient is ``g_host`` on the host and grad_latest on the shards."""
        self.n_mem = int(m)
        assert self.n_mem >= 1, 'm must be >= 1'
        self.n_slots = self.n_mem + 1
        W = 2 * self.n_slots + 1
        self.host = np.zeros((W, np.size(g_host)))           # the host part of every basis vector (empty slots: zeros, never used)
        self.host[-1] = g_host
        self.G = np.zeros((W, W))
        self.order = []                                      # slots that hold a kept pair, oldest first
        self.delta = None                                    # coefficients of the direction last written
        self._local_start(self.n_slots)
        self._refresh(-1)

    @property
    def n_pairs(self):
        return len(self.order)

    def _live(self, extra=None):
        n = self.n_slots
        live = np.zeros(2 * n + 1, dtype=bool)
        live[-1] = True
        for k in self.order + ([] if extra is None else [extra]):
            live[k] = live[n + k] = True
        return live

    def _refresh(self, slot):
        """Replaces the rows and columns of G that belong to s[slot], y[slot] (slot >= 0) and g: one pass over the per-point vectors."""
        n = self.n_slots
        idx = [2 * n] if slot < 0 else [slot, n + slot, 2 * n]
        rows = np.asarray(self._local_dots(slot), dtype=np.float64).reshape(3, 2 * n + 1)[3 - len(idx):]
        rows = rows + self.host[idx] @ self.host.T
        rows[:, ~self._live(slot if slot >= 0 else None)] = 0.0
        for i, r in zip(idx, rows):
            self.G[i, :] = r
            self.G[:, i] = r

    def _forget(self, slot):
        n = self.n_slots
        for i in (slot, n + slot):
            self.G[i, :] = 0.0
            self.G[:, i] = 0.0
            self.host[i] = 0.0

    def push(self, step, g_host=None):
        """The pair of an accepted step: s = step * direction, y = the new gradient - g, g = the new gradient (``g_host`` its host part, grad_latest
        on the shards).  Returns True if the pair is kept: s.y > CURVATURE sqrt(s.s y.y); a kept pair displaces the oldest of a full ring."""
        n = self.n_slots
        slot = min(k for k in range(n) if k not in self.order)
        self._local_push(slot, step)
        if g_host is not None:
            self.host[slot] = step * self.d_host
            self.host[n + slot] = g_host - self.host[-1]
            self.host[-1] = g_host
        self._refresh(slot)
        sy, ss, yy = self.G[slot, n + slot], self.G[slot, slot], self.G[n + slot, n + slot]
        self.last_pair = (sy, ss, yy)
        kept = bool(sy > CURVATURE * np.sqrt(ss * yy))
        if kept:
            if len(self.order) == self.n_mem:
                self._forget(self.order.pop(0))
            self.order.append(slot)
        else:
            self._forget(slot)
        return kept

    def direction(self, coef=None):
        """Writes the direction sum_j coef_j b_j (``coef`` None: the L-BFGS direction of the history as it is) and returns its host part."""
        self.delta = two_loop_coefficients(self.G, self.order, self.n_slots) if coef is None else np.array(coef, dtype=np.float64)
        self._local_direction(self.delta)
        self.d_host = self.delta @ self.host
        return self.d_host

    def slope(self):
        """g . d of the direction last written, from the Gram matrix: no pass over the vectors."""
        return float(np.dot(self.delta, self.G[:, -1]))

    def grad_norm2(self):
        return float(self.G[-1, -1])

    def reset(self):
        """Drops every pair; g stays."""
        for k in list(self.order):
            self._forget(k)
        self.order = []
        self._local_reset(self.n_slots)

    def update_X(self, step):
        self._local_update_X(step)

    def largest_move(self, step):
        """max |step * d| over the host and the per-point part (call it before the next ``direction``)."""
        host = float(np.max(np.abs(step * self.d_host))) if self.d_host.size else 0.0
        return max(host, self._local_largest_move(step))

    def finish(self):
        self._local_finish()

    # ---- the per-point part: nothing here
    def _local_start(self, n_slots):
        pass

    def _local_dots(self, slot):
        return np.zeros((3, 2 * self.n_slots + 1))

    def _local_push(self, slot, step):
        pass

    def _local_direction(self, coef):
        pass

    def _local_reset(self, n_slots):
        pass

    def _local_update_X(self, step):
        pass

    def _local_largest_move(self, step):
        return 0.0

    def _local_finish(self):
        pass


def LBFGS(f_and_gradf, x, ops, fixed_embeddings=False, optargs=(), maxiters=500, max_f_eval=500, display=False, xtol=None, ftol=None, gtol=None,
          m=10, trace=None):
    """Returns (x, flog, function_eval, status), the shape of ``SCG_adapted`` / ``GD``; ``ops`` holds the per-point part of the history
    (``resident.ResidentLBFGS``).  With ``fixed_embeddings`` or ``ops`` None it is a plain host L-BFGS over ``x`` (sparse GP regression).

    The algorithm, decision by decision:
      * f, g = f_and_gradf(x, 0, 0); the history is empty and the direction is d = -g.
      * An iteration starts from the slope g.d.  If g.d >= 0 the history is cleared and d = -g (a restart).
      * Line search: the first trial step is a = min(1, 1 / |g|) while the history is empty (the start, and after a restart), else a = 1.  Every trial is
        ONE evaluation f_and_gradf(x + a d, iteration + 1, a) -- the per-point part through the trial mechanism, step_size = a along the resident
        direction.  It is accepted when f(x + a d) <= f(x) + 1e-4 a g.d (Armijo); otherwise a is halved, at most 20 times.  When the 21st trial fails too the
        history is cleared and the search starts again from d = -g -- once: with an empty history the run ends ('line search failed').
      * On acceptance, in this order: ``push`` (s = a d, y = g_new - g, g = g_new), the embeddings move (``gp_cg_update(2, a)``), then the new direction.
        The pair is kept only if s.y > 1e-10 sqrt(s.s y.y); a skipped pair leaves the history as it was.
      * The direction is the two-loop recursion on the Gram matrix with the scaling gamma = s.y / y.y of the newest kept pair.
      * Stopping, after an accepted step as in SCG: the largest move max |a d| < xtol or |f_new - f| < ftol, then g.g <= gtol ('converged'); maxiters
        accepted steps ('maxiter exceeded'); max_f_eval evaluations ('Maximum number of function evaluations exceeded', the trial that reaches the count
        is not used).
    ``flog`` holds the bound at the start and after every accepted step.  ``trace`` (a list, tests): every decision is appended as a tuple --
    ('trial', a, f_trial, f + 1e-4 a g.d, accepted), ('pair', s.y, s.s, y.y, kept), ('restart', reason)."""
    xtol = 1e-6 if xtol is None else xtol
    ftol = 1e-6 if ftol is None else ftol
    gtol = 1e-5 if gtol is None else gtol
    note = (lambda *ev: trace.append(ev)) if trace is not None else (lambda *ev: None)
    hist = LbfgsHistory() if (fixed_embeddings or ops is None) else ops
    x = np.array(x, dtype=np.float64)

    f, g = safe_f_and_grad_f(f_and_gradf, x, 0, 0, *optargs)
    assert f != float('inf')
    evaluations = 1
    hist.start(g, m)
    d = hist.direction()
    status, flog, iteration = 'Not converged', [f], 0
    try:
        while iteration < maxiters:
            slope = hist.slope()
            if slope >= 0:
                if hist.n_pairs == 0:                          # -g itself is no descent direction: g = 0
                    status = 'converged'
                    break
                note('restart', 'slope')
                hist.reset()
                d = hist.direction()
                continue
            a = min(1.0, 1.0 / np.sqrt(hist.grad_norm2())) if hist.n_pairs == 0 else 1.0
            accepted = False
            for _ in range(MAX_HALVINGS + 1):
                f_trial, g_trial = safe_f_and_grad_f(f_and_gradf, x + a * d, iteration + 1, a, *optargs)
                evaluations += 1
                if evaluations >= max_f_eval:
                    break
                accepted = bool(f_trial <= f + C1 * a * slope)
                note('trial', a, f_trial, f + C1 * a * slope, accepted)
                if accepted:
                    break
                a *= 0.5
            if evaluations >= max_f_eval and not accepted:
                status = 'Maximum number of function evaluations exceeded'
                break
            if not accepted:
                if hist.n_pairs == 0:
                    status = 'line search failed'
                    break
                note('restart', 'line search')
                hist.reset()
                d = hist.direction()
                continue
            kept = hist.push(a, g_trial)
            note('pair', *(tuple(hist.last_pair) + (kept,)))
            hist.update_X(a)
            x = x + a * d
            move = hist.largest_move(a)
            flog.append(f_trial)
            iteration += 1
            if display:
                print(' %4d   %.6e   %.3e   %.3e' % (iteration, f_trial, a, hist.grad_norm2()))
            small = move < xtol or abs(f_trial - f) < ftol
            f = f_trial
            if small or hist.grad_norm2() <= gtol:
                status = 'converged'
                break
            d = hist.direction()
        else:
            status = 'maxiter exceeded'
    finally:
        hist.finish()
    return x, flog, evaluations, status
