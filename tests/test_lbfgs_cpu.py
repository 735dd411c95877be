"""gparml_amd.lbfgs without a GPU: the coefficient-space (vector-free) recursion against the classical two-loop on explicit vectors, ``LBFGS`` with its
variables split between the host and a numpy stand-in for the resident vectors (tests/lbfgs_ref.py, HostVectors) against a dense L-BFGS that states the
same rules independently, the plain host form, and the properties of the trace."""
import numpy as np
import pytest

import lbfgs_ref as R
from gparml_amd.lbfgs import LBFGS, two_loop_coefficients

N_HOST = 6


def _history(m, n, n_host, pushes, skip, seed):
    """Pushes ``pushes`` pairs of an SPD quadratic (condition 100: every s.y > 0) into a HostVectors and, next to it, into a plain list; the pushes in
    ``skip`` get a y orthogonal to s, which both sides must drop.  Yields (history, pairs, g) after every push."""
    rng = np.random.RandomState(seed)
    _, A = R.quadratic(n, 100.0, seed + 1)
    g = rng.standard_normal(n)
    hist = R.HostVectors(np.zeros(n - n_host))
    hist.grad_latest = g[n_host:]
    hist.start(g[:n_host], m)
    hist.direction()
    pairs = []
    for i in range(pushes):
        s = rng.standard_normal(n)
        if i in skip:
            v = rng.standard_normal(n)
            y = v - (np.dot(v, s) / np.dot(s, s)) * s
        else:
            y = A @ s
        g_old, g = g, g + y
        hist.dir, hist.d_host, hist.grad_latest = s[n_host:].copy(), s[:n_host].copy(), g[n_host:].copy()
        kept = hist.push(1.0, g[:n_host].copy())
        y = g - g_old                                         # the y both sides hold: the difference of the gradients as rounded
        assert kept == (i not in skip)
        if kept:
            pairs = (pairs + [(s, y)])[-m:]
        yield hist, pairs, g


@pytest.mark.parametrize('m', [1, 3, 10])
def test_coefficient_space_direction_equals_the_dense_two_loop(m):
    """Relative 1e-12 in the max norm after every push: empty, filling, wrapped ring (m + 5 pushes), two skipped pairs."""
    n = 30
    worst = 0.0
    for hist, pairs, g in _history(m, n, 7, m + 5, {2, m + 2}, seed=10 + m):
        assert hist.n_pairs == len(pairs)
        d = np.concatenate([hist.direction(), hist.dir])
        ref = R.dense_direction(pairs, g)
        err = np.max(np.abs(d - ref)) / np.max(np.abs(ref))
        worst = max(worst, err)
        assert err <= 1e-12, (m, len(pairs), err)
        assert abs(hist.slope() - np.dot(g, ref)) <= 1e-12 * np.dot(np.abs(g), np.abs(ref))
        assert abs(hist.grad_norm2() - np.dot(g, g)) <= 1e-14 * np.dot(g, g)
    print('m = %d: worst relative direction error %.3g' % (m, worst))


def test_empty_history_is_steepest_descent():
    delta = two_loop_coefficients(np.zeros((7, 7)), [], 3)
    assert delta.tolist() == [0, 0, 0, 0, 0, 0, -1.0]


def _problems():
    fq, _ = R.quadratic(20, 100.0, 3)
    xq = np.random.RandomState(4).standard_normal(20)
    xr = np.where(np.arange(20) % 2 == 0, -1.2, 1.0)
    # 30 accepted steps: an L-BFGS run amplifies a rounding-level difference of one direction roughly tenfold every seven steps on these problems (the dense
    # reference against its own ``perturbed`` run shows the same growth), so relative 1e-10 is a statement about the first few dozen steps, not the hundredth
    return {'quadratic': (fq, xq, 30), 'rosenbrock': (R.rosenbrock_chain, xr, 30)}


@pytest.mark.parametrize('name', ['quadratic', 'rosenbrock'])
def test_split_lbfgs_makes_the_dense_reference_s_decisions(name):
    """20 variables, 6 on the host and 14 "local": the same accept / halve / keep / skip / restart sequence as the dense reference, flog to relative 1e-10."""
    f, x0, iters = _problems()[name]
    kw = dict(maxiters=iters, max_f_eval=10 * iters, xtol=1e-12, ftol=1e-13, gtol=1e-16)
    xr, flog_r, ev_r, st_r, tr_r = R.dense_lbfgs(f, x0, m=5, **kw)
    cb, ops, xh = R.split_problem(f, x0, N_HOST)
    trace = []
    x, flog, ev, st = LBFGS(cb, xh, ops, m=5, trace=trace, **kw)
    assert R.decisions(trace) == R.decisions(tr_r)
    assert (ev, st) == (ev_r, st_r)
    assert len(flog) == len(flog_r) > 10
    rel = np.max(np.abs(np.array(flog) - np.array(flog_r)) / np.abs(np.array(flog_r)))
    print('%s: %d accepted steps, %d evaluations, %s; flog within %.3g of the dense reference' % (name, len(flog) - 1, ev, st, rel))
    assert rel <= 1e-10
    assert np.max(np.abs(np.concatenate([x, ops.X]) - xr)) <= 1e-8 * np.max(np.abs(xr))
    assert 'halve' in R.decisions(trace) or name == 'quadratic'


@pytest.mark.parametrize('name', ['quadratic', 'rosenbrock'])
def test_fixed_embeddings_is_a_plain_host_lbfgs(name):
    f, x0, _ = _problems()[name]
    x, flog, ev, st = LBFGS(lambda x, it, step: f(x), x0, None, fixed_embeddings=True, maxiters=500, max_f_eval=2000, xtol=1e-14, ftol=1e-15, gtol=1e-18)
    assert flog[-1] <= 1e-9, (flog[-1], st)
    _, flog_r, ev_r, st_r, _ = R.dense_lbfgs(f, x0, m=10, maxiters=500, max_f_eval=2000, xtol=1e-14, ftol=1e-15, gtol=1e-18)
    assert len(flog) > 10 and st == 'converged'
    assert abs(flog[10] - flog_r[10]) <= 1e-10 * abs(flog_r[10])


def test_flog_never_increases_and_counts_accepted_steps():
    f, x0, _ = _problems()['rosenbrock']
    trace = []
    x, flog, ev, st = LBFGS(lambda x, it, step: f(x), x0, None, maxiters=80, max_f_eval=1000, xtol=0.0, ftol=0.0, gtol=0.0, trace=trace)
    assert all(b <= a for a, b in zip(flog, flog[1:]))
    assert len(flog) - 1 == sum(1 for ev_ in trace if ev_[0] == 'trial' and ev_[4]) == 80
    assert ev == 1 + sum(1 for ev_ in trace if ev_[0] == 'trial')
    assert st == 'maxiter exceeded'


def test_every_stopping_rule_reports_its_status():
    f, x0, _ = _problems()['quadratic']
    cb = lambda x, it, step: f(x)                     # noqa: E731
    off = dict(xtol=-1.0, ftol=-1.0, gtol=-1.0)
    # ftol: the last decrease is below it
    x, flog, ev, st = LBFGS(cb, x0, None, maxiters=500, max_f_eval=2000, **dict(off, ftol=1e-3))
    assert st == 'converged' and abs(flog[-1] - flog[-2]) < 1e-3 and all(abs(a - b) >= 1e-3 for a, b in zip(flog[:-1], flog[1:-1]))
    # gtol: the squared gradient norm at the end, and only there
    x, flog, ev, st = LBFGS(cb, x0, None, maxiters=500, max_f_eval=2000, **dict(off, gtol=1e-6))
    assert st == 'converged' and np.dot(f(x)[1], f(x)[1]) <= 1e-6
    # xtol: the largest move of the last step
    x2, flog2, ev, st = LBFGS(cb, x0, None, maxiters=500, max_f_eval=2000, **dict(off, xtol=1e-4))
    assert st == 'converged' and 2 < len(flog2) < 500
    # iterations and evaluations
    assert LBFGS(cb, x0, None, maxiters=3, max_f_eval=2000, **off)[3] == 'maxiter exceeded'
    x, flog, ev, st = LBFGS(cb, x0, None, maxiters=500, max_f_eval=4, **off)
    assert st == 'Maximum number of function evaluations exceeded' and ev == 4
    # a gradient that points uphill: no step is ever accepted
    x, flog, ev, st = LBFGS(lambda x, it, step: (f(x)[0], -f(x)[1]), x0, None, maxiters=500, max_f_eval=2000, **off)
    assert st == 'line search failed' and len(flog) == 1 and ev == 22


def test_line_search_failure_restarts_once_from_steepest_descent():
    """A function whose gradient turns wrong after a few steps: the history is cleared ('restart'), the search runs again from -g, then the run ends."""
    f, x0, _ = _problems()['quadratic']
    calls = [0]

    def cb(x, it, step):
        calls[0] += 1
        v, g = f(x)
        return (v, g) if calls[0] <= 6 else (v + 1e6, g)
    trace = []
    x, flog, ev, st = LBFGS(cb, x0, None, maxiters=500, max_f_eval=2000, xtol=-1.0, ftol=-1.0, gtol=-1.0, trace=trace)
    d = R.decisions(trace)
    assert st == 'line search failed' and d.count('restart:line search') == 1
    assert d[-21:] == ['halve'] * 21 and d[-22] == 'restart:line search'
