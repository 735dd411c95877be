"""tests/svi_ref.py held to the mathematics of the whitened uncollapsed bound, without a GPU: the optimum against the reference's collapsed bound on a
golden case, every partial against central differences of the long-double bound, the natural step's fixed point, the 1/t partition identity and the
publish identity.  tests/test_gpu_svi.py then holds the device to svi_ref.

Tolerances.  The golden outputs are the reference's float64 (LU inverses): 1e-9 relative, the agreement the other golden comparisons of this suite
see at this size.  Central differences in long double with a relative step h = 1e-6 carry a truncation error of h^2 = 1e-12 and a rounding error of
2^-64 / h = 5e-14 of the bound's magnitude relative to the derivative's: the bound is ~1e3 here, so absolute 1e-7 on derivatives of size >= 1e-2
-- 1e-6 relative to the largest entry is asked.  The algebraic identities are asked in long double at 1e-14 relative (cond(K_mm) <= 1e3 at these
shapes, eps = 5e-20)."""
import numpy as np

import svi_ref as R
from conftest import load_golden

LD = np.longdouble


def _golden():
    inp, out = load_golden('regimeA_q10')
    st = dict(Psi2=out['sum_exp_K_mi_K_im'], C=out['exp_K_miY'], sum_YYT=float(out['sum_YYT']), Psi0=float(out['sum_exp_K_ii']), KL=float(out['KL']))
    return inp, out, st


def _random_state(M, D, seed):
    rng = np.random.RandomState(seed)
    G = rng.randn(M, M + 3)
    return G.dot(G.T) / M + 0.3 * np.eye(M), rng.randn(M, D)


def _rel(a, b):
    a, b = np.asarray(a, LD), np.asarray(b, LD)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def test_optimum_is_the_collapsed_bound_on_a_golden_case():
    inp, out, st = _golden()
    for ld in (False, True):
        K = R.kmm(inp['Z'], inp['sf2'], inp['alpha'], ld)
        Lam, H = R.optimum(K, st, inp['beta'], ld)
        s = R.step(inp['Z'], inp['sf2'], inp['alpha'], inp['beta'], st, Lam, H, inp['N'], inp['D'], ld=ld)
        assert abs(float(s['F']) - float(out['F'])) <= 1e-9 * abs(float(out['F'])), (ld, float(s['F']), float(out['F']))
        # the envelope theorem: at the optimum every partial is the collapsed one
        assert _rel(s['Abar'], out['dF_dexp_K_miY']) <= 1e-9
        assert _rel(s['Bbar'], out['dF_dexp_K_mi_K_im']) <= 1e-9
        assert _rel(s['dF_dKmm'] + s['dF_dKmm'].T, out['dF_dKmm'] + out['dF_dKmm'].T) <= 1e-9       # the reference's is not symmetrised; its use is
        assert abs(float(s['grad_beta']) - float(out['grad_beta'])) <= 1e-9 * abs(float(out['grad_beta']))
        assert abs(float(s['grad_sf2']) - float(out['grad_sf2'])) <= 1e-8 * abs(float(out['grad_sf2']))


def test_partials_match_central_differences_of_the_long_double_bound():
    inp, _, st = _golden()
    Z, sf2, alpha, beta, N, D = inp['Z'], inp['sf2'], inp['alpha'], inp['beta'], inp['N'], inp['D']
    M, Q = Z.shape
    Lam, H = _random_state(M, D, 3)                       # far from the optimum: no envelope to hide a wrong term
    s = R.step(Z, sf2, alpha, beta, st, Lam, H, N, D, ld=True)
    h = LD(1e-6)

    def L(Z=Z, sf2=sf2, alpha=alpha, beta=beta, st=st):
        return R.bound(R.kmm(Z, sf2, alpha, True), st, Lam, H, beta, N, D, True)

    def cd(f, x):
        step = h * max(LD(1), abs(LD(x)))
        return (f(LD(x) + step) - f(LD(x) - step)) / (2 * step)

    rng = np.random.RandomState(5)
    # Psi2 along random symmetric directions, C along random directions
    for _ in range(3):
        E = rng.randn(M, M)
        E = (E + E.T).astype(LD)
        got = cd(lambda t: L(st=dict(st, Psi2=np.asarray(st['Psi2'], LD) + t * E)), 0)
        assert abs(got - np.sum(s['Bbar'] * E)) <= 1e-6 * np.max(np.abs(s['Bbar'])) * np.sum(np.abs(E))
        Ec = rng.randn(M, D).astype(LD)
        got = cd(lambda t: L(st=dict(st, C=np.asarray(st['C'], LD) + t * Ec)), 0)
        assert abs(got - np.sum(s['Abar'] * Ec)) <= 1e-6 * np.max(np.abs(s['Abar'])) * np.sum(np.abs(Ec))
    # dL/dK_mm through a free symmetric dK ...
    Kl = R.kmm(Z, sf2, alpha, True)
    E = rng.randn(M, M)
    E = (E + E.T).astype(LD)
    got = cd(lambda t: R.bound(Kl + t * 1e-3 * E, st, Lam, H, beta, N, D, True), 0) / LD(1e-3)
    assert abs(got - np.sum(s['dF_dKmm'] * E)) <= 1e-6 * np.max(np.abs(s['dF_dKmm'])) * np.sum(np.abs(E))
    # ... and through perturbed Z and alpha with the statistics held: the K_mm parts of grad_Z and grad_alpha
    gZ = np.zeros((M, Q), LD)
    for m in range(0, M, 7):
        for q in range(0, Q, 3):
            def f(x, m=m, q=q):
                Zp = np.array(Z, LD)
                Zp[m, q] = x
                return L(Z=Zp)
            gZ[m, q] = cd(f, Z[m, q])
            assert abs(gZ[m, q] - s['grad_Z_K'][m, q]) <= 1e-6 * np.max(np.abs(s['grad_Z_K'])), (m, q)
    for q in range(Q):
        def f(x, q=q):
            ap = np.array(alpha, LD)
            ap[q] = x
            return L(alpha=ap)
        assert abs(cd(f, alpha[q]) - s['grad_alpha_K'][q]) <= 1e-6 * np.max(np.abs(s['grad_alpha_K'])), q
    assert abs(cd(lambda b: L(beta=b), beta) - s['grad_beta']) <= 1e-6 * abs(s['grad_beta'])

    # sf2 moves K_mm, C, Psi2 and Psi0 together (fixed embeddings: powers 1, 1, 2, 1)
    def f(x):
        r = LD(x) / LD(sf2)
        return L(sf2=x, st=dict(st, Psi2=np.asarray(st['Psi2'], LD) * r * r, C=np.asarray(st['C'], LD) * r, Psi0=LD(st['Psi0']) * r))
    assert abs(cd(f, sf2) - s['grad_sf2']) <= 1e-6 * abs(s['grad_sf2'])


def test_rate_one_from_a_random_start_is_the_optimum():
    inp, _, st = _golden()
    K = R.kmm(inp['Z'], inp['sf2'], inp['alpha'], True)
    w = R.whiten(K, st['Psi2'], st['C'], True)
    Lam0, H0 = _random_state(inp['M'], inp['D'], 11)
    Lam, H = R.natural_step(Lam0, H0, w, inp['beta'], 1.0, True)
    Lo, Ho = R.optimum(K, st, inp['beta'], True)
    assert _rel(Lam, Lo) <= 1e-14 and _rel(H, Ho) <= 1e-14
    assert np.array_equal(Lam, Lam.T)


def test_running_mean_over_a_partition_is_the_full_data_optimum():
    from oracle import factorised as Fz
    N, D, M, Q, T = 240, 4, 12, 2, 4
    d = Fz.synthetic_shard(N, D, M, Q, regime='A', seed=2, zseed=3, alpha_value=0.7)
    K = R.kmm(d['Z'], d['sf2'], d['alpha'], True)

    def stats(lo, hi, scale):
        s = Fz.phase1(d['Z'], d['sf2'], d['alpha'], d['Y'][lo:hi], d['X_mu'][lo:hi], d['X_S'][lo:hi])
        return dict(Psi2=scale * s['sum_exp_K_mi_K_im'], C=scale * s['exp_K_miY'])
    Lam, H = _random_state(M, D, 4)                       # rho_1 = 1 forgets the start
    batches = [stats((t - 1) * N // T, t * N // T, float(T)) for t in range(1, T + 1)]
    for t, b in enumerate(batches, 1):
        Lam, H = R.natural_step(Lam, H, R.whiten(K, ld=True, **b), d['beta'], LD(1) / t, True)
    # the full-data statistics as the long-double sum of the very batch statistics (a float64 phase 1 over all rows adds in another order and
    # differs by its own rounding, 6e-13 here after the whitening: not the identity's business)
    full = dict(Psi2=sum(np.asarray(b['Psi2'], LD) for b in batches) / T, C=sum(np.asarray(b['C'], LD) for b in batches) / T)
    Lo, Ho = R.optimum(K, full, d['beta'], True)
    assert _rel(Lam, Lo) <= 1e-14 and _rel(H, Ho) <= 1e-14


def test_publish_reproduces_the_posterior_of_lam():
    import predict_ref
    inp, _, st = _golden()
    Z, sf2, alpha, beta = inp['Z'], inp['sf2'], inp['alpha'], inp['beta']
    Lam, H = _random_state(inp['M'], inp['D'], 7)
    K = R.kmm(Z, sf2, alpha, True)
    P2e, Ce = R.publish(K, Lam, H, beta, True)
    # the publish identity: L_k L_l is the Cholesky factor of K_mm + beta Psi2_eff
    Lk, Ll = R.chol(K, True), R.chol(Lam, True)
    assert _rel(Lk.dot(Ll), R.chol(K + LD(beta) * P2e, True)) <= 1e-14
    Xs = np.random.RandomState(8).randn(9, inp['Q'])
    mean, var = R.predict(Z, sf2, alpha, Lam, H, Xs, True)
    m2, v2 = predict_ref.predict(Z, sf2, alpha, beta, np.asarray(P2e, np.float64), np.asarray(Ce, np.float64), Xs)
    # the collapsed predictive in float64 on the pseudo-statistics: its own error (cond(K_mm) eps) is the yardstick, 1e-10 is generous at M = 20
    assert _rel(m2, mean) <= 1e-10
    assert np.max(np.abs(v2[:, 0] - np.asarray(var, np.float64))) <= 1e-10 * sf2
    # the float64 path of the reference agrees with its long-double path
    m3, v3 = R.predict(Z, sf2, alpha, Lam, H, Xs, False)
    assert _rel(m3, mean) <= 1e-11 and np.max(np.abs(v3 - np.asarray(var, np.float64))) <= 1e-11 * sf2
