"""The per-row scaled conjugate gradient of gp_infer_latent (csrc/infer.hip: inf_scg_init_kernel, inf_scg_probe_kernel, inf_scg_trial_kernel,
inf_scg_update_kernel) on the host, exactly: the same fields (IS_*, II_*), the same branches and the same ascending-index fma chains.  Every
fma(a, b, c) is float(Fraction(a) * Fraction(b) + Fraction(c)), which is correctly rounded; every plain product, sum, difference and quotient the
source spells is the IEEE float64 operation of Python, which is correctly rounded as well.  Shared by tests/test_infer_scg_ref_cpu.py (numpy
evaluator) and tests/test_gpu_infer_scg.py (the device's own evaluations).

A state is a dict: x, gn, go, d, ge (lists of 2Q floats; ge = the gradient of L the last evaluation left behind), sc (IS_COUNT floats) and si
(II_COUNT ints).  An evaluator maps a point xe = (mu | softplus-raw S) to (L, gradient of L with respect to xe).  One iteration is
probe_point -> evaluation -> trial_point -> evaluation -> update, so that a caller can batch the evaluations of many rows; step() strings them
together for one row.

What is not reproducible bit for bit:
  sigma = 1e-4 / sqrt(kappa).  HIP's math API reference lists the double-precision sqrt with a maximum error of 1 ulp, not as correctly rounded.  One
    ulp is at most 2^-52 relative; the division is IEEE (the library is built with -O3 and no fast-math flag: __graft_entry__.HIPCC_FLAGS), so it
    passes that on and adds one rounding of 2^-53:  |sigma_dev - sigma| <= SIGMA_REL sigma,  SIGMA_REL = 2^-52 + 2^-53 + 2^-60 (the last term
    covers the product of the two and the long-double reference's own rounding).  probe_point therefore takes the device's stored sigma as given
    when the caller has one, and sigma_check() holds it to that bound.
  init with plain variances: x_raw = log(expm1(S)) and the slope 1 - exp(-S).  The same reference lists exp, expm1 and log at 1 ulp each.
    expm1 returns e (1 + t), |t| <= 2^-52, which shifts the logarithm by t; log adds an ulp of its result:  |x_raw_dev - x_raw| <= 2^-52 (1 + |x_raw|).
    exp(-S) = E (1 + t); 1 - E' is rounded once and the product with -ge once:  |gs_dev - gs| <= |gs| (2^-52 E / (1 - E) + 2^-52).
    Both carry the factor INIT_SLACK = 1 + 2^-20 for second-order terms.  With raw variances init is bit-exact.
  Scur = log(1 + exp(x_raw)) (csrc/varpoint.h softplus): exp returns E (1 + t), 1 + E' is rounded once (2^-53), log adds an ulp of its result:
    |S_dev - S| <= 2^-52 (E / (1 + E) + 1/2 + S) INIT_SLACK.
"""
import math
from fractions import Fraction

import numpy as np

IS_F, IS_LAM, IS_MU, IS_KAPPA, IS_SIGMA, IS_THETA, IS_ALPHA, IS_COUNT = range(8)
II_STATUS, II_SUCCESS, II_NSUCC, II_ITERS, II_COUNT = range(5)

SIGMA_REL = 2.0 ** -52 + 2.0 ** -53 + 2.0 ** -60
INIT_SLACK = 1.0 + 2.0 ** -20
MARGIN_ULPS = 4.0

# the mutations of tests/test_infer_scg_ref_cpu.py: each a flag of the one step below
MUTATIONS = ('lam_x2', 'thresholds_swapped', 'gamma_sign', 'no_restart_2q', 'theta_recomputed', 'sigma_x10', 'go_not_rotated', 'lam_not_stored',
             'iters_on_success', 'not_frozen')
DECISIONS = ('mu>=0', 'delta>0', 'Delta>=0', 'ft<=fp', 'Delta<0.25', 'Delta>0.75', 'gn<=gtol')
COUNTS = ('accepted', 'rejected', 'restart_2q', 'restart_mu', 'delta<=0', 'Delta<0.25', 'Delta_mid', 'Delta>0.75', 'gtol_stop', 'max_iters_stop')


def fma(a, b, c):
    """a * b + c with one rounding."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    p = Fraction(a) * Fraction(b)
    r = p + Fraction(c)
    if r == 0:
        return a * b + c if p == 0 else 0.0           # the sign of an exact zero: IEEE's own rules when the product is a zero, +0 on cancellation
    try:
        return float(r)
    except OverflowError:
        return math.inf if r > 0 else -math.inf


def div(a, b):
    """IEEE a / b, zero and non-finite operands included (Python raises on a zero divisor)."""
    return float(np.float64(a) / np.float64(b)) if (b == 0.0 or not math.isfinite(a) or not math.isfinite(b)) else a / b


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    return bool(np.array_equal(bits(a), bits(b)))


def ulps_apart(v, w, scale):
    """|v - w| in ulps of ``scale`` (the largest quantity that entered the comparison); inf when either is not finite (the branch is then forced)."""
    if not (math.isfinite(v) and math.isfinite(w) and math.isfinite(scale)):
        return math.inf
    s = float(np.spacing(abs(scale))) if scale != 0.0 else 5e-324
    return abs(v - w) / s


def maxabs(g):
    m = 0.0
    for v in g:
        if not math.isnan(v):                          # fmax drops a NaN
            m = max(m, abs(v))
    return m


def copy_state(s):
    return dict(x=list(s['x']), gn=list(s['gn']), go=list(s['go']), d=list(s['d']), ge=list(s['ge']), sc=list(s['sc']), si=list(s['si']))


def init(x_start, raw_in, L, g, gtol, max_iters):
    """inf_scg_init_kernel: the state after the evaluation (L, g) at the start x_start = (mu | S or raw S); g is with respect to S when not raw_in."""
    n2 = len(x_start)
    Q = n2 // 2
    x, gn = list(x_start), [0.0] * n2
    finite = math.isfinite(L)
    for q in range(Q):
        s = x_start[Q + q]
        if not raw_in:
            x[Q + q] = s if s > 40.0 else math.log(math.expm1(s))
        gn[q] = -g[q]
        gn[Q + q] = -g[Q + q] if raw_in else -g[Q + q] * (1.0 - math.exp(-s))
        finite = finite and math.isfinite(gn[q]) and math.isfinite(gn[Q + q]) and math.isfinite(x[Q + q])
    sc = [0.0] * IS_COUNT
    sc[IS_F], sc[IS_LAM] = -L, 1.0
    si = [0] * II_COUNT
    si[II_SUCCESS] = 1
    si[II_STATUS] = 1 if (finite and maxabs(gn) <= gtol) else 2 if (max_iters <= 0 or not finite) else 0
    return dict(x=x, gn=gn, go=list(gn), d=[-v for v in gn], ge=list(g), sc=sc, si=si)


def init_bounds(x_start, g):
    """Long-double x_raw and gs of a plain-variance start with the bounds of the module docstring: (x_raw, bound, gs, bound), each (Q,)."""
    LD = np.longdouble
    Q = len(x_start) // 2
    S = np.asarray(x_start[Q:], dtype=LD)
    xr = np.where(S > 40, S, np.log(np.expm1(S)))
    E = np.exp(-S)
    gs = -np.asarray(g[Q:], dtype=LD) * (1 - E)
    u = LD(2.0) ** -52
    return xr, u * (1 + np.abs(xr)) * INIT_SLACK, gs, np.abs(gs) * u * (E / (1 - E) + 1) * INIT_SLACK


def softplus_bounds(x_raw):
    """Long-double softplus and the bound of the module docstring."""
    LD = np.longdouble
    x = np.asarray(x_raw, dtype=LD)
    E = np.exp(x)
    S = np.log1p(E)
    return S, LD(2.0) ** -52 * (E / (1 + E) + LD(0.5) + S) * INIT_SLACK


def sigma_check(kappa, sigma):
    """|sigma - 1e-4 / sqrt(kappa)| / (SIGMA_REL sigma) against long double: at most 1 when the stored sigma is within the derived bound."""
    LD = np.longdouble
    ref = LD(1.0e-4) / np.sqrt(LD(kappa))
    return float(abs(LD(sigma) - ref) / (LD(SIGMA_REL) * ref))


def probe_point(s, sigma=None, mut=()):
    """inf_scg_probe_kernel for one row.  Returns (xe or None, info): None when the row takes no probe (finished, or its last step was rejected).
    ``sigma``: the device's stored value to take as given (None: computed here).  Updates s in place."""
    info = dict(margins={}, restart_mu=False)
    running = s['si'][II_STATUS] == 0 or 'not_frozen' in mut
    if not (running and s['si'][II_SUCCESS]):
        return None, info
    d, gn, x = s['d'], s['gn'], s['x']
    n2 = len(x)
    mu = 0.0
    for i in range(n2):
        mu = fma(d[i], gn[i], mu)
    info['margins']['mu>=0'] = ulps_apart(mu, 0.0, max(abs(d[i] * gn[i]) for i in range(n2)))
    if mu >= 0.0:
        info['restart_mu'] = True
        mu = 0.0
        for i in range(n2):
            d[i] = -gn[i]
            mu = fma(d[i], gn[i], mu)
    kappa = 0.0
    for i in range(n2):
        kappa = fma(d[i], d[i], kappa)
    if sigma is None:
        sigma = div(1.0e-3 if 'sigma_x10' in mut else 1.0e-4, math.sqrt(kappa) if kappa >= 0.0 else math.nan)
    xe = [fma(sigma, d[i], x[i]) for i in range(n2)]
    s['sc'][IS_MU], s['sc'][IS_KAPPA], s['sc'][IS_SIGMA] = mu, kappa, sigma
    return xe, info


def trial_point(s, ge_probe, mut=()):
    """inf_scg_trial_kernel for one row; ge_probe: the gradient of L at the probe point (None when the row took none).  Returns (xe or None, info)."""
    info = dict(margins={}, delta_nonpos=False)
    running = s['si'][II_STATUS] == 0 or 'not_frozen' in mut
    if not running:
        return None, info
    d, gn, x, sc = s['d'], s['gn'], s['x'], s['sc']
    n2 = len(x)
    probed = bool(s['si'][II_SUCCESS])
    if probed:
        s['ge'] = list(ge_probe)
    if probed or 'theta_recomputed' in mut:                # the mutation: the success flag forgotten, theta from whatever gradient lies there
        ge = s['ge']
        th = 0.0
        for i in range(n2):
            th = fma(d[i], -ge[i] - gn[i], th)
        sc[IS_THETA] = div(th, sc[IS_SIGMA])
    theta, kappa, lam = sc[IS_THETA], sc[IS_KAPPA], sc[IS_LAM]
    delta = fma(lam, kappa, theta)
    info['margins']['delta>0'] = ulps_apart(delta, 0.0, max(abs(theta), abs(lam * kappa)))
    lam_new = lam
    if not delta > 0.0:
        info['delta_nonpos'] = True
        delta = lam * kappa
        lam_new = lam - div(theta, kappa)
    alpha = div(-sc[IS_MU], delta)
    sc[IS_LAM] = lam if 'lam_not_stored' in mut else lam_new
    sc[IS_ALPHA] = alpha
    return [fma(alpha, d[i], x[i]) for i in range(n2)], info


def update(s, xe, L, ge, gtol, max_iters, mut=()):
    """inf_scg_update_kernel for one row after the evaluation (L, ge) at the trial point xe.  Returns info; updates s in place."""
    info = dict(margins={}, ok=False, restart_2q=False, band=None, stop=None)
    running = s['si'][II_STATUS] == 0 or 'not_frozen' in mut
    if not running:
        return info
    x, gn, go, d, sc, si = s['x'], s['gn'], s['go'], s['d'], s['sc'], s['si']
    n2 = len(x)
    s['ge'] = list(ge)
    ft, fp, mu, alpha = -L, sc[IS_F], sc[IS_MU], sc[IS_ALPHA]
    finite = math.isfinite(ft) and all(math.isfinite(v) for v in ge)
    Delta = div(2.0 * (ft - fp), alpha * mu)
    if not finite or not math.isfinite(Delta):
        Delta = -1.0
        info['margins']['Delta>=0'] = info['margins']['ft<=fp'] = math.inf
    else:
        # the sign of Delta is the sign of ft - fp over alpha mu; the difference is what can be close
        info['margins']['Delta>=0'] = info['margins']['ft<=fp'] = ulps_apart(ft, fp, max(abs(ft), abs(fp)))
    ok = Delta >= 0.0 and ft <= fp
    info['ok'] = ok
    nsucc = si[II_NSUCC]
    if ok:
        nsucc += 1
        for i in range(n2):
            x[i] = xe[i]
            if 'go_not_rotated' not in mut:
                go[i] = gn[i]
            gn[i] = -ge[i]
        sc[IS_F] = ft
    if ok or 'iters_on_success' not in mut:
        si[II_ITERS] += 1
    it = si[II_ITERS]
    if ok:
        m = maxabs(gn)
        info['margins']['gn<=gtol'] = ulps_apart(m, gtol, max(m, gtol))
    if ok and maxabs(gn) <= gtol:
        si[II_STATUS] = 1
        info['stop'] = 'gtol'
    elif it >= max_iters:
        si[II_STATUS] = 2
        info['stop'] = 'max_iters'
    lam = sc[IS_LAM]
    lo, hi = (0.75, 0.25) if 'thresholds_swapped' in mut else (0.25, 0.75)
    info['margins']['Delta<0.25'] = ulps_apart(Delta, 0.25, max(abs(Delta), 0.25))
    info['margins']['Delta>0.75'] = ulps_apart(Delta, 0.75, max(abs(Delta), 0.75))
    info['band'] = 'Delta<0.25' if Delta < 0.25 else 'Delta>0.75' if Delta > 0.75 else 'Delta_mid'
    if Delta < lo:
        lam = min((2.0 if 'lam_x2' in mut else 4.0) * lam, 1.0e100)
    if Delta > hi:
        lam = max(0.5 * lam, 1.0e-60)
    sc[IS_LAM] = lam
    if nsucc == n2 and 'no_restart_2q' not in mut:
        info['restart_2q'] = True
        for i in range(n2):
            d[i] = -gn[i]
        nsucc = 0
    elif ok:
        gg = og = 0.0
        for i in range(n2):
            gg = fma(gn[i], gn[i], gg)
            og = fma(go[i], gn[i], og)
        Gamma = div(gg - og, mu) if 'gamma_sign' in mut else div(og - gg, mu)
        for i in range(n2):
            d[i] = fma(Gamma, d[i], -gn[i])
    si[II_NSUCC] = nsucc
    si[II_SUCCESS] = 1 if ok else 0
    return info


def step(s, evaluate, gtol, max_iters, sigma=None, mut=()):
    """One iteration of one row from the state s (left untouched): (new state, info).  info: margins (decision -> ulps), the branch flags of the
    three kernels, and the points evaluated (xe_probe, xe_trial)."""
    t = copy_state(s)
    xp, ip = probe_point(t, sigma, mut)
    gp = evaluate(xp)[1] if xp is not None else None
    xt, itr = trial_point(t, gp, mut)
    info = dict(margins={}, restart_mu=ip['restart_mu'], delta_nonpos=itr['delta_nonpos'], ok=False, restart_2q=False, band=None, stop=None, ran=xt is not None,
                xe_probe=xp, xe_trial=xt)
    info['margins'].update(ip['margins'])
    info['margins'].update(itr['margins'])
    if xt is not None:
        L, g = evaluate(xt)
        iu = update(t, xt, L, g, gtol, max_iters, mut)
        info['margins'].update(iu.pop('margins'))
        info.update(iu)
    return t, info


def smallest_margin(info):
    m = info['margins']
    return min(m.values()) if m else math.inf


def count(counts, info):
    """Adds one step's branches to a dict of COUNTS."""
    if not info['ran']:
        return
    counts['accepted' if info['ok'] else 'rejected'] += 1
    counts['restart_2q'] += info['restart_2q']
    counts['restart_mu'] += info['restart_mu']
    counts['delta<=0'] += info['delta_nonpos']
    counts[info['band']] += 1
    counts['gtol_stop'] += info['stop'] == 'gtol'
    counts['max_iters_stop'] += info['stop'] == 'max_iters'


def run(x_start, raw_in, evaluate0, evaluate, gtol, max_iters, mut=()):
    """The free-running driver for one row: init from evaluate0(x_start) (gradient with respect to S when not raw_in), then steps until the row
    stops.  Returns (state, counts, trace): trace[k] = (state before iteration k, info of iteration k)."""
    L, g = evaluate0(x_start)
    s = init(list(x_start), raw_in, L, list(g), gtol, max_iters)
    counts = dict.fromkeys(COUNTS, 0)
    trace = []
    while s['si'][II_STATUS] == 0:
        t, info = step(s, evaluate, gtol, max_iters, mut=mut)
        count(counts, info)
        trace.append((s, info))
        s = t
    return s, counts, trace


EXACT_FIELDS = ('x', 'gn', 'go', 'd')
EXACT_SC = (IS_F, IS_LAM, IS_MU, IS_KAPPA, IS_THETA, IS_ALPHA)
EXACT_SI = (II_SUCCESS, II_NSUCC, II_ITERS)


def differing_fields(a, b):
    """The fields the lockstep compares exactly in which the states a and b differ (names)."""
    out = [f for f in EXACT_FIELDS if not same_bits(a[f], b[f])]
    out += ['sc[%d]' % j for j in EXACT_SC if not same_bits(a['sc'][j], b['sc'][j])]
    out += ['si[%d]' % j for j in EXACT_SI + (II_STATUS,) if a['si'][j] != b['si'][j]]
    return out


# ---- the committed cases on infer_ref.issue_problem() (tests/test_infer_scg_ref_cpu.py, tests/test_gpu_infer_scg.py) ------------------------------
K_STEPS = 12


def issue_cases(p):
    """name -> dict(Y, X0, S0, cols, K, gtol) on the problem p = infer_ref.issue_problem():
    issue      its 40 rows from their own start, gtol 1e-7: every row runs all 12 iterations;
    loose      the same with gtol 5: rows stop on the gradient from iteration 5 on, so finished rows exist within K;
    negcurv    found by a search over seeds 0-5 of starts drawn from Z (numpy's legacy randint, as test_restarts_are_rows draws them) and
               S0 in {1e-3, 0.5, 5}: seed 0, S0 = 5, the first 12 rows -- 17 steps with delta <= 0 and 15 restarts on mu >= 0 in 12 iterations
               (the 40 rows of `issue` take 8 and 24)."""
    n = 12
    starts = p['Z'][np.random.RandomState(0).randint(p['M'], size=(n,))]
    return dict(issue=dict(Y=p['Yt'], X0=p['X0'], S0=p['S0'], cols=p['cols'], K=K_STEPS, gtol=1e-7),
                loose=dict(Y=p['Yt'], X0=p['X0'], S0=p['S0'], cols=p['cols'], K=K_STEPS, gtol=5.0),
                negcurv=dict(Y=p['Yt'][:n], X0=starts, S0=np.full((n, p['Q']), 5.0), cols=p['cols'], K=K_STEPS, gtol=1e-7))
