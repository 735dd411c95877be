"""Which gradient a batch row's (mu, S) takes a step along in gparml_amd.svi.ResidentSVI, settled without a GPU in svi_ref's long-double arithmetic.

The batch estimate of the uncollapsed bound is svi_ref.bound on the batch's statistics times N / |B| (gp_scale_stats scales every entry of the
statistics buffer: Psi2, C, sum_YYT, Psi0 and the rows' KL).  The driver steps along phase 2's per-row output g_n = dKL-part + the contraction of the
row's dPsi1 / dPsi2 with (Abar, Bbar), taken on the batch context AFTER the statistics were scaled.  Abar and Bbar are functions of q(u) and the
hyper-parameters alone -- a^T Gc and a^T G2 a, no statistic enters -- so g_n does not feel the scaling:

    d (batch estimate) / d x_n = N / |B| * g_n          d (full-data bound) / d x_n = g_n          (x_n a row of the batch)

The second is the gradient the local step wants (every row's term enters the full-data bound once), so the driver applies g_n as phase 2 leaves it,
without N / |B|; gp_scale_buffer('grads', N / |B|) touches the hyper-parameter sums only.  Both identities are held here by central differences of the
long-double bound, with the statistics built by the oracle's free-embedding Psi functions (oracle.factorised._psi1_chunk / _psi2_terms_chunk, which
compute in the type they are given).

Tolerance: 1e-6 of the largest entry of the derivative compared, tests/test_svi_ref_cpu.py's bound for partials, for its reasons (relative step
1e-6: truncation 1e-12, rounding 2^-64 / 1e-6 of the bound's magnitude)."""
import numpy as np

import svi_ref as R
from oracle import factorised as Fz

LD = np.longdouble
N, D, M, Q, B = 24, 3, 8, 2, 6
SCALE = LD(N) / LD(B)


def _case():
    d = Fz.synthetic_shard(N, D, M, Q, regime='B', seed=4, zseed=5, alpha_value=0.6)
    idx = np.sort(np.random.RandomState(6).permutation(N)[:B])
    rng = np.random.RandomState(7)
    G = rng.randn(M, M + 3)
    return d, idx, G.dot(G.T) / M + 0.3 * np.eye(M), rng.randn(M, D)      # q(u) far from any optimum: no envelope hides a wrong factor


def _stats(d, mu, S, Y, scale):
    """The statistics buffer of rows (mu, S, Y) after scale_stats(scale), in long double."""
    Z, a, s2 = np.asarray(d['Z'], LD), np.asarray(d['alpha'], LD), LD(d['sf2'])
    mu, S, Y = np.asarray(mu, LD), np.asarray(S, LD), np.asarray(Y, LD)
    P1, _ = Fz._psi1_chunk(Z, s2, a, mu, S)
    psi2, _, _ = Fz._psi2_terms_chunk(Z, s2, a, mu, S)
    assert P1.dtype == LD and psi2.dtype == LD
    KL = LD(0.5) * np.sum(S - np.log(S) + mu * mu - 1)
    return dict(Psi2=scale * psi2.sum(0), C=scale * P1.T.dot(Y), sum_YYT=scale * np.sum(Y * Y), Psi0=scale * s2 * len(mu), KL=scale * KL)


def _bound(d, st, Lam, H):
    return R.bound(R.kmm(d['Z'], d['sf2'], d['alpha'], True), st, Lam, H, d['beta'], N, D, True)


def _cd(f, x):
    h = LD(1e-6) * max(LD(1), abs(LD(x)))
    return (f(LD(x) + h) - f(LD(x) - h)) / (2 * h)


def test_a_batch_rows_gradient_carries_no_batch_factor():
    d, idx, Lam, H = _case()
    Yb, mub, Sb = d['Y'][idx], d['X_mu'][idx], d['X_S'][idx]
    # the per-row expression the driver steps along: phase 2 on (Abar, Bbar) of the step that saw the SCALED batch statistics
    s = R.step(d['Z'], d['sf2'], d['alpha'], d['beta'], _stats(d, mub, Sb, Yb, SCALE), Lam, H, N, D, regime_A=False, ld=True)
    p2 = Fz.phase2(d['Z'], d['sf2'], d['alpha'], Yb, mub, Sb, np.asarray(s['Abar'], np.float64), np.asarray(s['Bbar'], np.float64), want_embeddings=True)
    g = dict(mu=p2['grad_X_mu'], S=p2['grad_X_S'])
    # (Abar, Bbar) are the same on unscaled statistics: they do not depend on them
    s1 = R.step(d['Z'], d['sf2'], d['alpha'], d['beta'], _stats(d, d['X_mu'], d['X_S'], d['Y'], LD(1)), Lam, H, N, D, regime_A=False, ld=True)
    assert np.array_equal(s['Abar'], s1['Abar']) and np.array_equal(s['Bbar'], s1['Bbar'])
    worst = dict(batch=0.0, full=0.0)
    for which, arr_b, arr_f in (('mu', mub, d['X_mu']), ('S', Sb, d['X_S'])):
        top = float(np.max(np.abs(g[which])))
        for i in range(B):
            for q in range(Q):
                def batch(x, i=i, q=q):
                    mu, S = np.array(mub, LD), np.array(Sb, LD)
                    (mu if which == 'mu' else S)[i, q] = x
                    return _bound(d, _stats(d, mu, S, Yb, SCALE), Lam, H)

                def full(x, i=i, q=q):
                    mu, S = np.array(d['X_mu'], LD), np.array(d['X_S'], LD)
                    (mu if which == 'mu' else S)[idx[i], q] = x
                    return _bound(d, _stats(d, mu, S, d['Y'], LD(1)), Lam, H)
                eb = abs(float(_cd(batch, arr_b[i, q]) - SCALE * LD(g[which][i, q]))) / (float(SCALE) * top)
                ef = abs(float(_cd(full, arr_f[idx[i], q]) - LD(g[which][i, q]))) / top
                worst = dict(batch=max(worst['batch'], eb), full=max(worst['full'], ef))
                assert eb <= 1e-6, (which, i, q, eb)       # the batch estimate's derivative is N / |B| times the row's gradient ...
                assert ef <= 1e-6, (which, i, q, ef)       # ... and the row's gradient is the full-data bound's: no factor in the local step
    print('central differences against the per-row expression, relative to its largest entry: batch estimate %.2e, full-data bound %.2e'
          % (worst['batch'], worst['full']))


def test_the_raw_variance_step_is_the_chain_rule_of_the_softplus():
    """The resident update moves the RAW variance r, S = ln(1 + e^r): its direction is g_S dS/dr = g_S / (1 + e^-r) (gp_phase2's grad_latest)."""
    d, idx, Lam, H = _case()
    Yb, mub, Sb = d['Y'][idx], d['X_mu'][idx], d['X_S'][idx]
    raw = np.log(np.expm1(np.asarray(Sb, LD)))
    s = R.step(d['Z'], d['sf2'], d['alpha'], d['beta'], _stats(d, mub, Sb, Yb, SCALE), Lam, H, N, D, regime_A=False, ld=True)
    p2 = Fz.phase2(d['Z'], d['sf2'], d['alpha'], Yb, mub, Sb, np.asarray(s['Abar'], np.float64), np.asarray(s['Bbar'], np.float64), want_embeddings=True)
    want = np.asarray(p2['grad_X_S'], LD) / (1 + np.exp(-raw))
    top = float(np.max(np.abs(want)))
    for i in range(0, B, 2):
        for q in range(Q):
            def f(x, i=i, q=q):
                r = np.array(raw, LD)
                r[i, q] = x
                return _bound(d, _stats(d, mub, np.log1p(np.exp(r)), Yb, SCALE), Lam, H)
            assert abs(float(_cd(f, raw[i, q]) - SCALE * want[i, q])) <= 1e-6 * float(SCALE) * top, (i, q)
