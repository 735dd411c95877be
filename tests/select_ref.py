"""The reference of the greedy conditional-variance selection (gp_select_*, csrc/select.hip): the pivoted Cholesky factorisation of K_nn, one pivot
per step, restated in numpy.

``select(X, sf2, alpha, K, tol)`` runs the algorithm of include/gparml_hip.h in ``numpy.longdouble`` (the 80-bit format: 64 bits of mantissa):
  k(x, z) = sf2 exp(-1/2 sum_q alpha_q (x_q - z_q)^2), the difference first, q ascending
  start d_n = sf2; step j: the pivot p is the unselected row of largest d, of equal ones the lowest; stop before the step when d_p <= tol sf2 or j = K
  c_n = (k(x_n, x_p) - sum_{i<j} L_ni L_pi) / sqrt(d_p), i ascending from 0;  L_nj = c_n;  d_n <- d_n - c_n^2 for every row, selected or not
  trace_j = sum max(d_n, 0) over the unselected rows after the step
and returns the pivots, L, d, the trace and, per step, the GAP: (best d - second-best d among the unselected rows) / sf2 before the step's choice
(inf when one row is left), and whether those two rows are exactly identical.  ``dtype=numpy.float64`` is the MIRROR: the same code in float64,
every product rounded where the device fuses it into a multiply-add, numpy's exp where the device has its own.

Why the gap matters: the device's float64 d differs from the reference's by rounding, and the pivots are compared exactly.  The comparison is
honest only where the choice is not within that rounding: every case of CASES satisfies, at every step actually run after step 0, gap >= MIN_GAP,
or the two best rows are identical (then the lowest index wins by the rule, in every arithmetic: identical rows carry identical bits).  The figure
1e-6 rests on a crude estimate of the float64 error of d, about K^2 u sf2 / (d_p / sf2)^(1/2) ~ 3e-9 at K = 512, d_p >= 1e-4 sf2; tests/test_select_cpu.py
asserts its consequence directly: the mirror's d is within gap / 100 of the reference's at every step of every case.  The seeds below were chosen so.
"""
import numpy as np

MIN_GAP = 1e-6


def kernel_column(X, z, sf2, alpha, dtype):
    """k(x_n, z) for every row of X, in ``dtype``: difference first, q ascending, each product and sum rounded."""
    s = np.zeros(X.shape[0], dtype=dtype)
    for q in range(X.shape[1]):
        e = X[:, q] - z[q]
        s = s + (alpha[q] * e) * e
    return dtype(sf2) * np.exp(dtype(-0.5) * s)


def select(X, sf2, alpha, K, tol, dtype=np.longdouble, pivots=None, keep_d=False):
    """The selection in ``dtype``.  ``pivots``: take these rows as pivots instead of the arg-max (the mirror is run on the reference's pivots,
    so that the two are compared step by step); the stopping rule then is the length of the list.  Returns a dict: pivots (K',) int64,
    L (n, K'), d (n,), trace (K',), gap (K',), same (K',) bool, and with ``keep_d`` d_steps (K' + 1, n): d before every step and at the end."""
    X = np.asarray(X, dtype=np.float64).astype(dtype)
    alpha = np.asarray(alpha, dtype=np.float64).astype(dtype)
    n = X.shape[0]
    sf2d = dtype(sf2)
    thr = dtype(np.float64(tol) * np.float64(sf2))           # the device compares with this float64 product
    d = np.full(n, sf2d, dtype=dtype)
    L = np.zeros((n, K), dtype=dtype)
    chosen = np.zeros(n, dtype=bool)
    out_p, trace, gap, same, d_steps = [], [], [], [], []
    for j in range(K):
        free = np.nonzero(~chosen)[0]
        if free.size == 0 or (pivots is not None and j >= len(pivots)):
            break
        df = d[free]
        order = np.argsort(-df, kind='stable')                # of equal values the lowest index first
        p = int(free[order[0]])
        if pivots is not None:
            p = int(pivots[j])
        elif not d[p] > thr:
            break
        if free.size > 1:
            q2 = int(free[order[1]])
            gap.append(float((df[order[0]] - df[order[1]]) / sf2d))
            same.append(bool(np.array_equal(X[p], X[q2])))
        else:
            gap.append(np.inf)
            same.append(False)
        if keep_d:
            d_steps.append(d.copy())
        acc = np.zeros(n, dtype=dtype)
        for i in range(j):
            acc = acc + L[:, i] * L[p, i]
        c = (kernel_column(X, X[p], sf2, alpha, dtype) - acc) / np.sqrt(d[p])
        L[:, j] = c
        d = d - c * c
        chosen[p] = True
        out_p.append(p)
        rest = d[~chosen]
        trace.append(np.maximum(rest, dtype(0)).sum(dtype=dtype) if rest.size else dtype(0))
    if keep_d:
        d_steps.append(d.copy())
    k = len(out_p)
    res = dict(pivots=np.array(out_p, dtype=np.int64), L=L[:, :k], d=d, trace=np.array(trace, dtype=dtype), gap=np.array(gap), same=np.array(same, dtype=bool))
    if keep_d:
        res['d_steps'] = np.array(d_steps, dtype=dtype).reshape(k + 1, n)
    return res


# name: (n, Q, K, seed, sf2, a, extra).  Rows: standard normal; alpha_q = a / Q * uniform(0.5, 1.5), so that the kernel stays well away from 0 and 1
# between most pairs of rows at every Q (far rows would all keep d = sf2 to the last bit: ties that are no duplicates).  extra: 'dup' = the rows
# are draws, with repeats, from 12 distinct ones; 'zero' = alpha_2 = 0.  tol = 1e-10 throughout.
CASES = {
    'n1_Q3_K2': (1, 3, 2, 1, 1.7, 1.0, None),
    'n2_Q3_K2': (2, 3, 2, 2, 1.7, 1.0, None),
    'n63_Q10_K33': (63, 10, 33, 3, 0.8, 1.0, None),
    'n64_Q16_K1': (64, 16, 1, 4, 2.5, 1.0, None),
    'n65_Q17_K33': (65, 17, 33, 5, 1.3, 1.0, None),
    'n65_Q1_K2': (65, 1, 2, 6, 1.1, 1.0, None),
    'n127_Q70_K33': (127, 70, 33, 7, 0.6, 1.0, None),
    'n129_Q10_K65': (129, 10, 65, 8, 1.9, 1.0, None),
    'n20000_Q10_K40': (20000, 10, 40, 9, 1.4, 1.0, None),
    'dup_n40_Q3_K20': (40, 3, 20, 10, 1.2, 2.0, 'dup'),
    'zero_alpha_n100_Q4_K10': (100, 4, 10, 11, 0.9, 1.0, 'zero'),
    'xcheck_n300_Q2_K12': (300, 2, 12, 12, 1.5, 1.0, None),
}
TOL = 1e-10
DUP_DISTINCT = 12


def make_case(name):
    """(X (n, Q), sf2, alpha (Q,), K) of a case."""
    n, Q, K, seed, sf2, a, extra = CASES[name]
    rs = np.random.RandomState(seed)
    X = rs.randn(n, Q)
    alpha = a / Q * rs.uniform(0.5, 1.5, Q)
    if extra == 'dup':
        X = X[:DUP_DISTINCT][np.concatenate([np.arange(DUP_DISTINCT), rs.randint(0, DUP_DISTINCT, n - DUP_DISTINCT)])]
        X = X[rs.permutation(n)]
    if extra == 'zero':
        alpha[2] = 0.0
    return X, sf2, alpha, K


_cache = {}


def reference(name):
    """(ref, mirror, err) of a case, computed once: the long-double selection (with d before every step), the float64 mirror on the same
    pivots, and the mirror's worst error against the reference as ONE figure per case -- the largest of max |dL| / sqrt(sf2), max |dd| / sf2
    and max |dtrace| / (n sf2): every quantity on the scale of a conditional variance of one row."""
    if name not in _cache:
        X, sf2, alpha, K = make_case(name)
        ref = select(X, sf2, alpha, K, TOL, keep_d=True)
        mir = select(X, sf2, alpha, K, TOL, dtype=np.float64, pivots=ref['pivots'], keep_d=True)
        _cache[name] = (ref, mir, deviation(ref, mir['L'], mir['d'], mir['trace'], sf2))
    return _cache[name]


def deviation(ref, L, d, trace, sf2):
    """The figure of ``reference`` for any (L (n, K'), d (n,), trace (K',)) against the long-double ``ref``."""
    n = ref['d'].shape[0]
    ld = np.longdouble
    eL = np.max(np.abs(np.asarray(L).astype(ld) - ref['L'])) / np.sqrt(ld(sf2)) if ref['L'].size else ld(0)
    ed = np.max(np.abs(np.asarray(d).astype(ld) - ref['d'])) / ld(sf2)
    et = np.max(np.abs(np.asarray(trace).astype(ld) - ref['trace'])) / (n * ld(sf2)) if ref['trace'].size else ld(0)
    return float(max(eL, ed, et))


def identities(X, sf2, alpha, pivots, L, d):
    """The two identities of the factorisation on a given (L, d), in long double, as errors relative to sf2:
    max over selected j and rows n of |sum_i L_ni L_{p_j i} - k(x_n, x_{p_j})|, and max_n |d_n - (sf2 - sum_i L_ni^2)|."""
    ld = np.longdouble
    Xl, al = np.asarray(X, dtype=np.float64).astype(ld), np.asarray(alpha, dtype=np.float64).astype(ld)
    Ll, dl = np.asarray(L).astype(ld), np.asarray(d).astype(ld)
    e1 = ld(0)
    for j, p in enumerate(pivots):
        e1 = max(e1, np.max(np.abs(Ll @ Ll[p] - kernel_column(Xl, Xl[p], sf2, al, ld))))
    e2 = np.max(np.abs(dl - (ld(sf2) - (Ll * Ll).sum(axis=1))))
    return float(e1 / ld(sf2)), float(e2 / ld(sf2))
