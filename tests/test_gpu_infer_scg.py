"""gp_infer_latent's per-row SCG (csrc/infer.hip: inf_scg_init / probe / trial / update kernels) held to its algebra step by step, in lockstep:
for k = 0 .. K the optimiser runs max_iters = k from the same start and its state S_k is read back (gp_debug_peek 'infer_x', 'infer_sc', ...);
tests/infer_scg_ref.py then takes one step from the device's own S_k with the device's own evaluations (gp_infer_objective at the reference's
bit-exact probe and trial points) and must land on S_{k+1}: x, gn, go, d, f, lambda, mu, kappa, theta, alpha, the success flag, the success and
iteration counts and the status as bits; sigma = 1e-4 / sqrt(kappa), whose sqrt is not promised correctly rounded, is taken from the device and
held to the bound derived in infer_scg_ref's docstring, as are the libm-dependent entries of init with plain variances and Scur = softplus(raw).
Nothing here has a tolerance to tune.  tests/test_infer_scg_ref_cpu.py shows that the reference is an SCG, that these cases reach every branch,
and that ten plausible errors of the algebra each change a field compared here."""
import functools
import math

import numpy as np
import pytest

import infer_ref as I
import infer_scg_ref as S
from test_gpu_infer import _issue_predictor, _opt_setup

pytestmark = pytest.mark.gpu

ROWS = 128            # rows of the chunk (gp_debug_set_option 'infer_rows'): what the peeks are sized by; every case fits one chunk
STATE = (('x', 2), ('gn', 2), ('go', 2), ('d', 2), ('xe', 2), ('ge', 2), ('Scur', 1), ('sc', 0), ('si', 0), ('fe', 0))


@pytest.fixture(autouse=True)
def one_small_chunk():
    from gparml_amd import _lib
    lib = _lib.load()
    lib.gp_debug_set_option(b'infer_rows', ROWS)
    yield
    lib.gp_debug_set_option(b'infer_rows', 0)


@functools.lru_cache(maxsize=None)
def _problem():
    return I.issue_problem()


def _case(name):
    """(engine, case): the committed cases of infer_scg_ref.issue_cases on the issue's model, and `wide`: M 130, Q 17 (table width 32, the plain
    path; fma chains 34 long), D 3, regime B, 24 rows over all columns, K 8, through test_gpu_infer's model helper."""
    if name == 'wide':
        d, e, Y, mu, S0 = _opt_setup(seed=3, M=130, Q=17, D=3, N=400, n=24)
        return e, dict(Y=Y, X0=mu, S0=S0, cols=None, K=8, gtol=1e-7)
    p = _problem()
    return _issue_predictor(p)[0]._trained_engine(), S.issue_cases(p)[name]


def _peek(e, n):
    Q = e.Q
    out = {}
    for name, w in STATE:
        width = w * Q if w else dict(sc=S.IS_COUNT, si=S.II_COUNT, fe=1)[name]
        out[name] = e.peek('infer_' + name, ROWS * width).reshape(ROWS, width)[:n].copy()
    out['si'] = out['si'].astype(np.int64)
    out['fe'] = out['fe'][:, 0]
    return out


def _row_state(st, i):
    return dict(x=st['x'][i].tolist(), gn=st['gn'][i].tolist(), go=st['go'][i].tolist(), d=st['d'][i].tolist(), ge=st['ge'][i].tolist(),
                sc=st['sc'][i].tolist(), si=[int(v) for v in st['si'][i]])


def _calls(e, c, raw, ks):
    """[(outputs, state)] of infer_latent(max_iters = k) for k in ks, all from the case's start."""
    xs = I.softplus_inv(c['S0']) if raw else c['S0']
    res = []
    for k in ks:
        out = e.infer_latent(c['Y'], c['X0'], xs, cols=c['cols'], xs_is_raw=raw, max_iters=k, gtol=c['gtol'])
        res.append((out, _peek(e, c['Y'].shape[0])))
    return xs, res


def _evaluate(e, c, rows, pts, raw=True):
    """The device's own evaluation of the rows at the points pts (len(rows), 2Q): (L, gradient (len(rows), 2Q))."""
    Q = e.Q
    pts = np.asarray(pts, dtype=np.float64).reshape(len(rows), 2 * Q)
    L, gm, gs = e.infer_objective(c['Y'][rows], pts[:, :Q], pts[:, Q:], cols=c['cols'], xs_is_raw=raw)
    return L, np.hstack((gm, gs))


def _in_domain(pt, Q):
    """Well inside what gp_infer_objective accepts as a raw variance: log(1 + exp(raw)) finite and > 0 in float64 (it is 0 below raw = -36.7, where
    1 + exp(raw) rounds to 1; the optimiser's own evaluation then sees S = 0, a non-finite L, and rejects the step)."""
    return all(-36.0 < v < 700.0 for v in pt[Q:])


def _same(a, b):
    return S.same_bits(a, b)


def _check_outputs(name, c, raw, k, out, st):
    """The outputs of call k are (x | Scur or raw, -f, iters) of S_k as bits."""
    Q = st['Scur'].shape[1]
    m, s, L, it = out
    assert _same(m, st['x'][:, :Q]), (name, raw, k, 'X_mu')
    assert _same(s, st['x'][:, Q:] if raw else st['Scur']), (name, raw, k, 'X_S')
    assert _same(L, -st['sc'][:, S.IS_F]), (name, raw, k, 'L')
    assert np.array_equal(it, st['si'][:, S.II_ITERS]), (name, raw, k, 'iters')


def _check_scur(name, c, raw, k, st, st0, worst):
    """Scur of a row that has moved (or started raw) is within the softplus bound of long-double softplus(x_raw); a row that came in with plain
    variances and has not moved holds the caller's S."""
    Q = st['Scur'].shape[1]
    ref, bound = S.softplus_bounds(st['x'][:, Q:])
    err = np.abs(st['Scur'].astype(np.longdouble) - ref)
    moved = np.any(S.bits(st['x']) != S.bits(st0['x']), axis=1)
    for i in range(st['x'].shape[0]):
        if raw or moved[i]:
            worst['Scur'] = max(worst['Scur'], float(np.max(err[i] / bound[i])))
            assert np.all(err[i] <= bound[i]), (name, raw, k, i, 'Scur', st['Scur'][i], ref[i], bound[i])
        else:
            assert _same(st['Scur'][i], c['S0'][i]), (name, raw, k, i, 'Scur of a row that has not moved')


def _check_init(e, name, c, raw, xs, st, worst):
    """S_0 against inf_scg_init_kernel: bit-exact with raw variances; with plain ones the raw variance and its gradient within the derived bounds
    (log(expm1(S)) and 1 - exp(-S) go through libm), everything else exact."""
    n, Q = c['X0'].shape
    start = np.hstack((c['X0'], xs))
    L, g = _evaluate(e, c, np.arange(n), start, raw=raw)
    for i in range(n):
        ref = S.init(start[i].tolist(), raw, float(L[i]), g[i].tolist(), c['gtol'], 0)
        got = _row_state(st, i)
        what = (name, raw, 'init', i)
        assert got['si'] == ref['si'] and got['si'][S.II_STATUS] == 2, what + (got['si'], ref['si'])
        assert _same(got['sc'], ref['sc']), what + (got['sc'], ref['sc'])
        assert _same(got['go'], got['gn']) and _same(got['d'], [-v for v in got['gn']]), what
        if raw:
            assert _same(got['x'], ref['x']) and _same(got['gn'], ref['gn']), what + (got['x'], ref['x'], got['gn'], ref['gn'])
            continue
        assert _same(got['x'][:Q], ref['x'][:Q]) and _same(got['gn'][:Q], ref['gn'][:Q]), what
        xr, bx, gs, bg = S.init_bounds(start[i].tolist(), g[i].tolist())
        ex, eg = np.abs(np.asarray(got['x'][Q:], dtype=np.longdouble) - xr), np.abs(np.asarray(got['gn'][Q:], dtype=np.longdouble) - gs)
        worst['init_x'] = max(worst['init_x'], float(np.max(ex / bx)))
        worst['init_g'] = max(worst['init_g'], float(np.max(eg / np.maximum(bg, np.longdouble(5e-324)))))
        assert np.all(ex <= bx) and np.all(eg <= bg), what + (got['x'][Q:], xr, bx, got['gn'][Q:], gs, bg)


def _lockstep(name, raw, e, c):
    """Runs the K + 1 calls and every check of the module docstring on them; returns [(outputs, state)] and the figures measured."""
    n, Q = c['X0'].shape
    K, gtol = c['K'], c['gtol']
    xs, res = _calls(e, c, raw, range(K + 1))
    worst = dict(sigma=0.0, Scur=0.0, init_x=0.0, init_g=0.0, steps=0, left_out=[], margin=math.inf, outside=0)
    for k, (out, st) in enumerate(res):
        assert np.all(np.isfinite(st['sc'][:, S.IS_F])), (name, raw, k)
        _check_outputs(name, c, raw, k, out, st)
        _check_scur(name, c, raw, k, st, res[0][1], worst)
    _check_init(e, name, c, raw, xs, res[0][1], worst)
    for k in range(K):
        a, b = res[k][1], res[k + 1][1]
        # a row still running after call k shows status 2 at iters == k (init leaves a finite row at 2 with max_iters 0 as well)
        running = [i for i in range(n) if a['si'][i, S.II_STATUS] == 2 and a['si'][i, S.II_ITERS] == k]
        stopped = [i for i in range(n) if i not in running]
        assert all(a['si'][i, S.II_STATUS] == 1 for i in stopped), (name, raw, k, a['si'][stopped])
        for i in stopped:                                 # a finished row is frozen: its whole record and its outputs
            for f in ('x', 'gn', 'go', 'd', 'Scur', 'sc', 'si'):
                assert _same(a[f][i], b[f][i]), (name, raw, k, i, f, 'a finished row moved')
        rows = {i: _row_state(a, i) for i in running}
        for t in rows.values():
            t['si'][S.II_STATUS] = 0
        infos = {i: dict(margins={}) for i in running}
        # probe: the device's sigma of this step (it lies in S_{k+1}) is taken as given and held to its bound
        probes = {}
        for i in running:
            probed = bool(rows[i]['si'][S.II_SUCCESS])
            xp, info = S.probe_point(rows[i], sigma=float(b['sc'][i, S.IS_SIGMA]) if probed else None)
            infos[i]['margins'].update(info['margins'])
            if xp is not None:
                probes[i] = xp
                dev = S.sigma_check(rows[i]['sc'][S.IS_KAPPA], float(b['sc'][i, S.IS_SIGMA]))
                worst['sigma'] = max(worst['sigma'], dev)
                assert dev <= 1.0, (name, raw, k, i, 'sigma', float(b['sc'][i, S.IS_SIGMA]), rows[i]['sc'][S.IS_KAPPA], dev)
            else:
                assert _same(a['sc'][i, S.IS_SIGMA], b['sc'][i, S.IS_SIGMA]), (name, raw, k, i, 'sigma rewritten without a probe')
        gp = {}
        if probes:
            pr = sorted(probes)
            assert all(_in_domain(probes[i], Q) for i in pr), (name, raw, k, 'a probe point outside gp_infer_objective\'s domain')
            _, g = _evaluate(e, c, pr, [probes[i] for i in pr])
            gp = {i: g[j].tolist() for j, i in enumerate(pr)}
        trials = {}
        for i in running:
            xt, info = S.trial_point(rows[i], gp.get(i))
            infos[i]['margins'].update(info['margins'])
            trials[i] = xt
        # gp_infer_objective refuses a point whose variance is not a positive finite number; the optimiser itself evaluates such a trial point
        # (an overshoot in the raw variance) and rejects the step on the non-finite result.  There the device's own record of that evaluation
        # (fe, ge of S_{k+1}, once its xe is the reference's trial point bit for bit) stands in.
        inside = [i for i in running if _in_domain(trials[i], Q)]
        L, g = np.full(n, np.nan), np.full((n, 2 * Q), np.nan)
        if inside:
            L[inside], g[inside] = _evaluate(e, c, inside, [trials[i] for i in inside])
        for i in running:
            if i not in inside:
                assert _same(b['xe'][i], trials[i]), 'case %s raw=%d row %d k %d: trial point device %r reference %r' % (name, raw, i, k, b['xe'][i], trials[i])
                L[i], g[i] = b['fe'][i], b['ge'][i]
                worst['outside'] += 1
        for i in running:
            j = i
            info = S.update(rows[i], trials[i], float(L[j]), g[j].tolist(), gtol, k + 1)
            infos[i]['margins'].update(info['margins'])
            margin = S.smallest_margin(infos[i])
            worst['margin'] = min(worst['margin'], margin)
            if margin < S.MARGIN_ULPS:
                worst['left_out'].append((i, k, infos[i]['margins']))
                continue
            worst['steps'] += 1
            got = _row_state(b, i)
            where = 'case %s raw=%d row %d k %d' % (name, raw, i, k)
            for f in S.EXACT_FIELDS:
                assert _same(got[f], rows[i][f]), '%s: %s device %r reference %r margins %r' % (where, f, got[f], rows[i][f], infos[i]['margins'])
            for jf in S.EXACT_SC:
                assert _same(got['sc'][jf], rows[i]['sc'][jf]), '%s: sc[%d] device %r reference %r margins %r' % (where, jf, got['sc'][jf], rows[i]['sc'][jf],
                                                                                                                infos[i]['margins'])
            assert got['si'] == rows[i]['si'], '%s: si device %r reference %r margins %r' % (where, got['si'], rows[i]['si'], infos[i]['margins'])
            # the chunk's last evaluation is this step's trial point, evaluated as gp_infer_objective evaluates it
            assert _same(b['xe'][i], trials[i]) and _same(b['fe'][i], L[j]) and _same(b['ge'][i], g[j]), '%s: xe / fe / ge' % where
    assert len(worst['left_out']) <= 1, (name, raw, worst['left_out'])
    # frozen rows at output level: once a row shows status 1, its output triple never changes again
    for i in range(n):
        ks = [k for k in range(K + 1) if res[k][1]['si'][i, S.II_STATUS] == 1]
        for k in ks[1:]:
            assert all(_same(u[i], v[i]) for u, v in zip(res[ks[0]][0], res[k][0])), (name, raw, i, ks[0], k, 'the outputs of a finished row changed')
    print('[infer scg lockstep] %s raw=%d: %d steps compared as bits (%d on the device\'s record of a trial point outside the entry\'s domain), left out %r; sigma deviation / bound %.3g, Scur %.3g, init x_raw %.3g, init gs %.3g; '
          'smallest decision margin %.3g ulps' % (name, raw, worst['steps'], worst['outside'], worst['left_out'], worst['sigma'], worst['Scur'], worst['init_x'], worst['init_g'],
                                                  worst['margin']))
    return res, worst


@pytest.mark.parametrize('raw', [False, True])
@pytest.mark.parametrize('name', ['issue', 'loose', 'negcurv', 'wide'])
def test_lockstep(name, raw):
    e, c = _case(name)
    try:
        res, worst = _lockstep(name, raw, e, c)
    finally:
        e.close()
    assert worst['steps'] >= c['Y'].shape[0]
    if name == 'loose':                      # finished rows exist within K, so the frozen-row checks are not vacuous
        assert sum(res[c['K'] - 1][1]['si'][:, S.II_STATUS] == 1) >= 5


def test_lockstep_in_poison_mode():
    """The `issue` lockstep again with every buffer NaN-filled on allocation: the same bits in every call and every state."""
    from gparml_amd import _lib
    lib = _lib.load()
    e, c = _case('issue')
    try:
        _, plain = _calls(e, c, False, range(c['K'] + 1))
    finally:
        e.close()
    lib.gp_debug_set_option(b'poison_alloc', 1)
    try:
        e, c = _case('issue')
        try:
            res, _ = _lockstep('issue (poison)', False, e, c)
        finally:
            e.close()
    finally:
        lib.gp_debug_set_option(b'poison_alloc', 0)
    for k, ((o1, s1), (o2, s2)) in enumerate(zip(plain, res)):
        assert all(_same(u, v) for u, v in zip(o1, o2)), k
        for f, _ in STATE:
            assert _same(np.asarray(s1[f], dtype=np.float64), np.asarray(s2[f], dtype=np.float64)), (k, f)


def test_early_stop_returns_the_same_bits():
    """Every row of `loose` stops on the gradient long before 300 iterations: max_iters = 300 (the host polls the active-row count every 8
    iterations and breaks) returns the bits of max_iters = max(iters) + 1."""
    e, c = _case('loose')
    try:
        for raw in (False, True):
            xs = I.softplus_inv(c['S0']) if raw else c['S0']
            long = e.infer_latent(c['Y'], c['X0'], xs, cols=c['cols'], xs_is_raw=raw, max_iters=300, gtol=c['gtol'])
            top = int(np.max(long[3]))
            assert top + 1 + 8 < 300, top
            short = e.infer_latent(c['Y'], c['X0'], xs, cols=c['cols'], xs_is_raw=raw, max_iters=top + 1, gtol=c['gtol'])
            assert all(_same(u, v) for u, v in zip(long, short))
            assert np.all(_peek(e, c['Y'].shape[0])['si'][:, S.II_STATUS] == 1)
    finally:
        e.close()


def test_max_iters_zero_returns_the_start():
    e, c = _case('issue')
    try:
        for gtol, status in ((1e-7, 2), (1e9, 1)):          # no gradient is that large: the row is finished at once
            m, s, L, it = e.infer_latent(c['Y'], c['X0'], c['S0'], cols=c['cols'], max_iters=0, gtol=gtol)
            st = _peek(e, c['Y'].shape[0])
            assert _same(m, c['X0']) and _same(s, c['S0']) and np.all(it == 0)
            assert _same(L, e.infer_objective(c['Y'], c['X0'], c['S0'], cols=c['cols'], want_grads=False)[0])
            assert np.all(st['si'][:, S.II_STATUS] == status) and np.all(st['si'][:, S.II_ITERS] == 0)
    finally:
        e.close()


def test_a_row_with_a_non_finite_start_stays_and_disturbs_no_other():
    e, c = _case('issue')
    try:
        for raw in (False, True):
            xs = I.softplus_inv(c['S0']) if raw else c['S0']
            clean = e.infer_latent(c['Y'], c['X0'], xs, cols=c['cols'], xs_is_raw=raw, max_iters=12, gtol=c['gtol'])
            Y = c['Y'].copy()
            bad = 7
            Y[bad, c['cols']] = 1e200
            m, s, L, it = e.infer_latent(Y, c['X0'], xs, cols=c['cols'], xs_is_raw=raw, max_iters=12, gtol=c['gtol'])
            st = _peek(e, Y.shape[0])
            assert _same(m[bad], c['X0'][bad]) and _same(s[bad], xs[bad]) and it[bad] == 0 and not np.isfinite(L[bad])
            assert st['si'][bad, S.II_STATUS] == 2
            keep = np.arange(Y.shape[0]) != bad
            assert all(_same(u[keep], v[keep]) for u, v in zip(clean, (m, s, L, it)))
    finally:
        e.close()


def test_the_ragged_entry_point_gives_the_same_bits():
    """gp_infer_latent_rows with every row observing columns 0-4 against gp_infer_latent(cols = 0-4), outputs only."""
    e, c = _case('issue')
    try:
        obs = np.zeros(c['Y'].shape, dtype=np.uint8)
        obs[:, c['cols']] = 1
        for raw in (False, True):
            xs = I.softplus_inv(c['S0']) if raw else c['S0']
            for k in (1, 5, 12):
                a = e.infer_latent(c['Y'], c['X0'], xs, cols=c['cols'], xs_is_raw=raw, max_iters=k, gtol=c['gtol'])
                b = e.infer_latent_rows(c['Y'], c['X0'], xs, observed=obs, xs_is_raw=raw, max_iters=k, gtol=c['gtol'])
                for u, v, what in zip(a, b, ('X_mu', 'X_S', 'L', 'iters')):
                    assert _same(u, v), (raw, k, what, int(np.sum(S.bits(u) != S.bits(v))), float(np.max(np.abs(u - v))))
    finally:
        e.close()


def test_the_peeks_need_the_optimiser_state():
    from gparml_amd import _lib
    e, c = _case('issue')
    try:
        names = [n for n, _ in STATE]
        for n in names:
            with pytest.raises(_lib.GparmlHipError):
                e.peek('infer_' + n, ROWS * 8)
        e.infer_objective(c['Y'], c['X0'], c['S0'], cols=c['cols'])        # the chunk exists now, the optimiser's state does not
        for n in names:
            with pytest.raises(_lib.GparmlHipError):
                e.peek('infer_' + n, ROWS * 8)
        assert e.lib.gp_debug_peek(e.h, b'infer_x', np.empty(ROWS * 8).ctypes.data_as(_lib._dp), ROWS * 8) == _lib.GP_ERR_STATE
        assert e.lib.gp_debug_peek(e.h, b'infer_nothing', np.empty(ROWS * 8).ctypes.data_as(_lib._dp), ROWS * 8) == _lib.GP_ERR_BAD_ARG
        e.infer_latent(c['Y'], c['X0'], c['S0'], cols=c['cols'], max_iters=1)
        before = _peek(e, c['Y'].shape[0])
        again = _peek(e, c['Y'].shape[0])                                   # peeking changes nothing
        assert all(_same(np.asarray(before[f], dtype=np.float64), np.asarray(again[f], dtype=np.float64)) for f, _ in STATE)
        with pytest.raises(AssertionError):
            e.peek('infer_x', 3)                                            # too small a buffer: GP_ERR_BAD_ARG
    finally:
        e.close()
