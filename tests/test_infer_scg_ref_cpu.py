"""tests/infer_scg_ref.py, the host image of gp_infer_latent's per-row SCG kernels, on its own: it is an SCG (it reaches L-BFGS-B's optimum as the
device is required to), the committed cases reach every branch, each mutation of the algebra shows in a field the GPU lockstep compares exactly, and
no decision of the committed cases is within rounding of its threshold.  Evaluator: numpy's infer_ref.objective_row on issue_problem()."""
import numpy as np
import pytest

import infer_ref as I
import infer_scg_ref as S
import predict_ref as R


@pytest.fixture(scope='module')
def prob():
    p = I.issue_problem()
    Psi2, C = R.statistics(p['Z'], p['sf2'], p['alpha'], p['Y'], p['X_mu'], p['X_S'])
    return p, I.Model(p['Z'], p['sf2'], p['alpha'], p['beta'], Psi2, C)


def evaluator(mdl, y, cols, Q, raw=True):
    def ev(xe):
        L, gm, gs = I.objective(mdl, y[None], cols, np.array(xe[:Q])[None], np.array(xe[Q:])[None], xs_is_raw=raw)
        return float(L[0]), [float(v) for v in gm[0]] + [float(v) for v in gs[0]]
    return ev


def start(case, i, raw_in):
    return [float(v) for v in case['X0'][i]] + [float(v) for v in (I.softplus_inv(case['S0'][i]) if raw_in else case['S0'][i])]


def free_run(mdl, case, max_iters, raw_in=False, gtol=None):
    """[(state, counts, trace)] per row."""
    Q = case['X0'].shape[1]
    out = []
    for i in range(case['Y'].shape[0]):
        ev = evaluator(mdl, case['Y'][i], case['cols'], Q)
        out.append(S.run(start(case, i, raw_in), raw_in, evaluator(mdl, case['Y'][i], case['cols'], Q, raw=raw_in), ev, case['gtol'] if gtol is None else gtol,
                         max_iters))
    return out


def total(runs):
    return {k: sum(r[1][k] for r in runs) for k in S.COUNTS}


@pytest.fixture(scope='module')
def runs(prob):
    """The committed cases run freely for their K iterations (plain variances in), and `issue` for 300."""
    p, mdl = prob
    cases = S.issue_cases(p)
    out = {name: free_run(mdl, c, c['K']) for name, c in cases.items()}
    out['issue300'] = free_run(mdl, cases['issue'], 300)
    return cases, out


def test_the_reference_is_scg(prob, runs):
    """300 free-running iterations at gtol 1e-7 reach optimise_row's L-BFGS-B L to 1e-6 relative on at least 36 of the 40 rows (the bar
    tests/test_gpu_infer.py holds the device to); f never increases; iters counts attempts, accepted or not."""
    p, mdl = prob
    long = runs[1]['issue300']
    ref = np.array([I.optimise_row(mdl, p['Yt'][i], p['cols'], p['X0'][i], p['S0'][i])[2] for i in range(len(long))])
    got = np.array([-s['sc'][S.IS_F] for s, _, _ in long])
    good = got >= ref - 1e-6 * np.abs(ref)
    print('[scg ref vs L-BFGS-B] %d of %d rows match or exceed; worst shortfall %.3g' % (good.sum(), len(ref), np.max(ref - got)))
    assert good.sum() >= 36
    for s, c, trace in long:
        f = [t[0]['sc'][S.IS_F] for t in trace] + [s['sc'][S.IS_F]]
        assert all(b <= a for a, b in zip(f, f[1:]))
        assert s['si'][S.II_ITERS] == len(trace) == c['accepted'] + c['rejected']
        assert [t[0]['si'][S.II_ITERS] for t in trace] == list(range(len(trace)))


def test_the_committed_cases_reach_every_branch(runs):
    """K = 12 on `issue`: accepted 416, rejected 64, restarts after 2Q successes 93, restarts on mu >= 0 24, delta <= 0 8, Delta < 0.25 75,
    between 35, > 0.75 370, 40 rows stopped by max_iters; `negcurv`: 17 steps with delta <= 0, 15 restarts on mu >= 0; `loose`: rows stopped on
    the gradient within K; 300 iterations at gtol 1e-7: 4 rows stop on the gradient."""
    cases, r = runs
    t = total(r['issue'])
    print('[scg ref branches] issue', t, '\n[scg ref branches] negcurv', total(r['negcurv']), '\n[scg ref branches] loose', total(r['loose']))
    for k in ('accepted', 'rejected', 'restart_2q', 'Delta<0.25', 'Delta_mid', 'Delta>0.75', 'max_iters_stop'):
        assert t[k] >= 1, k
    assert total(r['issue300'])['gtol_stop'] >= 1
    assert total(r['negcurv'])['delta<=0'] >= 1 and total(r['negcurv'])['restart_mu'] >= 1
    assert total(r['loose'])['gtol_stop'] >= 1
    assert any(len(x[2]) < cases['loose']['K'] - 1 for x in r['loose'])        # a finished row with iterations of the lockstep still to come


def lockstep_states(mdl, case, i, raw_in=False):
    """S_0 .. S_K of row i as the device's calls max_iters = 0 .. K leave them, but for the status of a row still running (0 here, 2 there)."""
    Q = case['X0'].shape[1]
    ev = evaluator(mdl, case['Y'][i], case['cols'], Q)
    x0 = start(case, i, raw_in)
    L, g = evaluator(mdl, case['Y'][i], case['cols'], Q, raw=raw_in)(x0)
    s = S.init(x0, raw_in, L, g, case['gtol'], case['K'])
    states = [s]
    for _ in range(case['K']):
        s = S.step(s, ev, case['gtol'], case['K'])[0]
        states.append(s)
    return states, ev


@pytest.mark.parametrize('mut', S.MUTATIONS)
def test_every_mutation_shows_in_an_exactly_compared_field(prob, mut):
    """The lockstep has teeth: from some state S_k (k < 12) of some row of the committed cases the mutated step and the true step differ in a field
    the GPU test compares as bits.  sigma x10 additionally misses the sigma bound (the GPU lockstep takes the device's sigma as given, so there
    the bound is what catches it)."""
    p, mdl = prob
    cases = S.issue_cases(p)
    order = ('loose', 'issue', 'negcurv') if mut == 'not_frozen' else ('negcurv', 'issue', 'loose')
    for name in order:
        c = cases[name]
        for i in range(c['Y'].shape[0]):
            states, ev = lockstep_states(mdl, c, i)
            for k in range(c['K']):
                true, _ = S.step(states[k], ev, c['gtol'], c['K'])
                bad, _ = S.step(states[k], ev, c['gtol'], c['K'], mut=(mut,))
                diff = S.differing_fields(true, bad)
                if diff:
                    print('[scg ref mutation] %s: case %s row %d k %d differs in %s' % (mut, name, i, k, diff))
                    if mut == 'sigma_x10':
                        assert S.sigma_check(bad['sc'][S.IS_KAPPA], bad['sc'][S.IS_SIGMA]) > 1e6
                        assert S.sigma_check(true['sc'][S.IS_KAPPA], true['sc'][S.IS_SIGMA]) <= 1
                    return
    pytest.fail('mutation %s changes no exactly compared field in any (case, row, k)' % mut)


def test_no_decision_is_within_rounding_of_its_threshold(runs):
    """Over every (row, k) of the committed cases the smallest decision margin is 1.3e11 ulps of the compared quantity (`issue`, about 2.8e-5
    relative; `loose` 4.2e12, `negcurv` 2.7e12), measured with the numpy evaluator: none below 4 ulps, so the GPU lockstep need leave no step out
    on the reference's account."""
    cases, r = runs
    worst = {}
    for name in cases:
        ms = [S.smallest_margin(info) for _, _, trace in r[name] for _, info in trace]
        worst[name] = min(ms)
        assert sum(m < S.MARGIN_ULPS for m in ms) == 0, name
    print('[scg ref margins] smallest decision margin in ulps', worst)
