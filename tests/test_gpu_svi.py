"""gp_svi_* on the device (csrc/svi.hip) held to tests/svi_ref.py.  The statistics are the context's own phase 1, downloaded, so the reference sees
the same float64 inputs.

Shapes: M = 24 (one padded panel), D = 3, Q = 2, N = 200 in both regimes; M = 130 (two panels of the blocked Cholesky), D = 130 (two column
tiles), Q = 3, N = 300 with fixed embeddings.

Bounds.  The device runs the reference's algebra in float64 with other summation orders (the MFMA's k-chunks, the blocked factorisation), so the
yardstick is the float64 svi_ref against its own long-double evaluation ON THE SAME INPUTS, relative to the largest entry of each quantity; the
device gets 8x that, and never less than 8 gamma_M = 8 M 2^-53, the bound of one length-M float64 accumulation (a float64 reference that happens to
land closer than one accumulation's rounding is no licence to ask the device for more than the format gives).  Full gradients add phase 2, which is
linear in (Abar, Bbar) and unchanged: they get the largest relative error of the three partials, against the sum of the magnitudes of the parts."""
import ctypes

import numpy as np
import pytest

import svi_ref as R
from gparml_amd import _lib
from oracle import factorised as Fz

pytestmark = pytest.mark.gpu
LD = np.longdouble
SMALL, BIG = (24, 3, 2, 200), (130, 130, 3, 300)


def _engine(shape, regime, seed=0, N_global=None, rows=None):
    from gparml_amd.engine import ShardEngine
    M, D, Q, N = shape
    d = Fz.synthetic_shard(N, D, M, Q, regime=regime, seed=seed, zseed=seed + 1, alpha_value=0.5)
    if rows is not None:
        d = dict(d, Y=d['Y'][rows], X_mu=d['X_mu'][rows], X_S=d['X_S'][rows])
    eng = ShardEngine(d['Y'].shape[0], D, M, Q, device=0)
    eng.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'], N_global=N_global)
    eng.phase1()
    return eng, d


def _stats(eng):
    s = eng.scalars()
    return dict(Psi2=eng.download('PSI2_SUM'), C=eng.download('PSI1TY'), sum_YYT=s['sum_YYT'], Psi0=s['sum_exp_K_ii'], KL=s['KL'])


def _state(M, D, seed):
    rng = np.random.RandomState(seed)
    G = rng.randn(M, M + 3)
    return G.dot(G.T) / M + 0.3 * np.eye(M), rng.randn(M, D)


def _relerr(a, b):
    b = np.asarray(b, LD)
    return float(np.max(np.abs(np.asarray(a, LD) - b)) / np.max(np.abs(b)))


def _refs(d, st, Lam, H, N, D, regime_A):
    r64 = R.step(d['Z'], d['sf2'], d['alpha'], d['beta'], st, Lam, H, N, D, regime_A, ld=False)
    rld = R.step(d['Z'], d['sf2'], d['alpha'], d['beta'], st, Lam, H, N, D, regime_A, ld=True)
    return r64, rld


def _bound(r64, rld, key, M):
    """8 x the float64 reference's own error in `key`, floored at 8 gamma_M; the figures are printed before anything is asserted."""
    e = _relerr(r64[key], rld[key])
    return 8.0 * max(e, M * 2.0 ** -53), e


def _finish_ref(d, r, want_emb):
    """Full gradients of a step dict through the oracle's phase 2 and finish (float64), and the magnitudes of their parts."""
    g = {k: np.asarray(r[k], np.float64) for k in ('Abar', 'Bbar', 'grad_Z_K', 'grad_alpha_K', 'BbarPsi2')}
    regA = Fz.is_regime_A(d['X_S'])
    p2 = Fz.phase2(d['Z'], d['sf2'], d['alpha'], d['Y'], d['X_mu'], d['X_S'], g['Abar'], g['Bbar'], want_embeddings=want_emb)
    out = Fz.finish(d['Z'], d['sf2'], d['alpha'], dict(g, F=0.0, grad_sf2=0.0, grad_beta=0.0), p2, regA)
    scale = dict(grad_Z=np.max(np.abs(g['grad_Z_K'])) + np.max(np.abs(p2['grad_Z_data'])),
                 grad_alpha=np.max(np.abs(g['grad_alpha_K'])) + np.max(np.abs(p2['grad_alpha_data'])))
    return out, p2, scale


def _check_step(eng, d, st, Lam, H, shape, regime_A, want_emb, out):
    """out = finish() of svi_step -> phase2 on eng, whose state is (Lam, H): everything against svi_ref."""
    M, D, Q, N = shape
    r64, rld = _refs(d, st, Lam, H, N, D, regime_A)
    worst = 0.0
    for key, name in (('Abar', 'DF_DPSI1TY'), ('Bbar', 'DF_DPSI2'), ('dF_dKmm', 'DF_DKMM')):
        tol, e = _bound(r64, rld, key, M)
        got = _relerr(eng.download(name), rld[key])
        print('%s: reference %.2e device %.2e bound %.2e' % (key, e, got, tol))
        assert got <= tol, key
        worst = max(worst, tol)
    for key in ('F', 'grad_beta', 'grad_sf2'):
        tol, e = _bound(r64, rld, key, M)
        got = abs(out[key] - float(rld[key])) / abs(float(rld[key]))
        print('%s: reference %.2e device %.2e bound %.2e' % (key, e, got, tol))
        assert got <= tol, key
    ref, p2, scale = _finish_ref(d, rld, want_emb)
    for key in ('grad_Z', 'grad_alpha'):
        got = np.max(np.abs(out[key] - ref[key])) / scale[key]
        print('%s: device %.2e bound %.2e' % (key, got, worst))
        assert got <= worst, key
    if want_emb:
        got = _relerr(eng.download('GRAD_X_MU'), p2['grad_X_mu'])
        print('grad_X_mu: device %.2e bound %.2e' % (got, worst))
        assert got <= worst


@pytest.mark.parametrize('shape,regime,want_emb', [(SMALL, 'A', False), (SMALL, 'B', False), (SMALL, 'B', True), (BIG, 'A', False)])
def test_rate_one_on_full_statistics_is_the_collapsed_evaluation(shape, regime, want_emb):
    M, D, Q, N = shape
    eng, d = _engine(shape, regime)
    eng.global_step()
    eng.phase2(want_emb)
    col = eng.finish()
    col_gx = eng.download('GRAD_X_MU') if want_emb else None
    st = _stats(eng)
    eng.svi_begin()
    eng.svi_natural_step(1.0)
    eng.svi_step()
    eng.phase2(want_emb)
    out = eng.finish()
    # the yardstick: the float64 reference at ITS optimum (one float64 natural step, then the step) against the long-double one
    K = R.kmm(d['Z'], d['sf2'], d['alpha'])
    L64, H64 = R.optimum(K, st, d['beta'])
    Lld, Hld = R.optimum(R.kmm(d['Z'], d['sf2'], d['alpha'], True), st, d['beta'], True)
    r64 = R.step(d['Z'], d['sf2'], d['alpha'], d['beta'], st, L64, H64, N, D, regime == 'A')
    rld = R.step(d['Z'], d['sf2'], d['alpha'], d['beta'], st, Lld, Hld, N, D, regime == 'A', ld=True)
    # ... and, since the other side of the comparison is the collapsed step with a float64 error of its own, the float64 collapsed oracle against
    # the same long-double values (at the optimum they are the collapsed truth): the two errors add
    c64 = Fz.global_step(d['Z'], d['sf2'], d['alpha'], d['beta'], dict(sum_exp_K_mi_K_im=st['Psi2'], exp_K_miY=st['C'], sum_YYT=st['sum_YYT'],
                                                                      sum_exp_K_ii=st['Psi0'], KL=st['KL']), N, D)
    c64['dF_dKmm'] = 0.5 * (c64['dF_dKmm'] + c64['dF_dKmm'].T)          # the collapsed partial is used symmetrised (kmm_grads_row)

    def both(key):
        tol, e = _bound(r64, rld, key, M)
        return tol + 8.0 * _relerr(c64[key], rld[key]), e
    worst = max(both(k)[0] for k in ('Abar', 'Bbar', 'dF_dKmm'))
    for key in ('F', 'grad_beta', 'grad_sf2'):
        tol, e = both(key)
        got = abs(out[key] - col[key]) / abs(col[key])
        print('%s: reference %.2e device %.2e bound %.2e' % (key, e, got, tol))
        assert got <= tol, key
    _, _, scale = _finish_ref(d, rld, False)
    for key in ('grad_Z', 'grad_alpha'):
        got = np.max(np.abs(out[key] - col[key])) / scale[key]
        print('%s: device %.2e bound %.2e' % (key, got, worst))
        assert got <= worst, key
    if want_emb:
        got = _relerr(eng.download('GRAD_X_MU'), col_gx)
        print('grad_X_mu: device %.2e bound %.2e' % (got, worst))
        assert got <= worst
    eng.close()


@pytest.mark.parametrize('shape,regime,want_emb', [(SMALL, 'A', False), (SMALL, 'B', True), (BIG, 'A', False)])
def test_step_at_a_random_state_matches_the_reference(shape, regime, want_emb):
    M, D, Q, N = shape
    eng, d = _engine(shape, regime)
    st = _stats(eng)
    Lam, H = _state(M, D, 3)
    eng.svi_begin()
    eng.svi_set(Lam, H)
    eng.svi_step()
    eng.phase2(want_emb)
    out = eng.finish()
    _check_step(eng, d, st, Lam, H, shape, regime == 'A', want_emb, out)
    sc = eng.scalars()
    # the two log-determinant slots, by the same yardstick (ln|K_mm| of a nearly singular K_mm carries cond(K_mm) eps per pivot in any float64 factorisation)
    r64, rld = _refs(d, st, Lam, H, N, D, regime == 'A')
    for r in (r64, rld):
        r['logdet_A'] = r['logdet_K'] + r['logdet_Lam']
    for key, name in (('logdet_K', 'logdet_Kmm'), ('logdet_A', 'logdet_A')):
        tol, e = _bound(r64, rld, key, M)
        got = abs(sc[name] - float(rld[key])) / abs(float(rld[key]))
        print('%s: reference %.2e device %.2e bound %.2e' % (key, e, got, tol))
        assert got <= tol, key
    eng.close()


@pytest.mark.parametrize('shape', [SMALL, BIG])
def test_natural_step_and_get_match_the_reference(shape):
    M, D, Q, N = shape
    eng, d = _engine(shape, 'A')
    st = _stats(eng)
    Lam0, H0 = _state(M, D, 5)
    eng.svi_begin()
    eng.svi_set(Lam0, H0)
    eng.svi_natural_step(0.3)
    got = eng.svi_get()
    ref = {}
    for ld in (False, True):
        w = R.whiten(R.kmm(d['Z'], d['sf2'], d['alpha'], ld), st['Psi2'], st['C'], ld)
        Lam, H = R.natural_step(Lam0, H0, w, d['beta'], 0.3, ld)
        m = R.moments(Lam, H, ld)
        ref[ld] = dict(Lam=Lam, H=H, Mv=m['Mv'], Sv=m['Sv'])
    for key in ('Lam', 'H', 'Mv', 'Sv'):
        tol, e = _bound(ref[False], ref[True], key, M)
        err = _relerr(got[key], ref[True][key])
        print('%s: reference %.2e device %.2e bound %.2e' % (key, e, err, tol))
        assert err <= tol, key
    assert np.array_equal(got['Lam'], got['Lam'].T)
    eng.close()


def test_running_mean_over_four_batch_contexts_is_the_full_data_optimum():
    M, D, Q, N = SMALL
    T = 4
    full, d = _engine(SMALL, 'A')
    st = _stats(full)
    full.svi_begin()
    full.svi_set(*_state(M, D, 9))                       # rho_1 = 1 forgets it
    batches = []
    for t in range(1, T + 1):
        b, _ = _engine(SMALL, 'A', N_global=N, rows=slice((t - 1) * N // T, t * N // T))
        b.scale_stats(float(T))
        sb = _stats(b)
        batches.append(sb)
        full.set_local_statistics(sb['sum_YYT'], sb['Psi2'], sb['C'], sb['Psi0'], sb['KL'])      # the batch feeds the one SVI state
        full.svi_natural_step(1.0 / t)
        b.close()
    got = full.svi_get(moments=False)
    # the yardstick runs what the device ran: the same four batch statistics through four 1/t steps, in float64 and in long double
    seq, opt = {}, {}
    for ld in (False, True):
        K = R.kmm(d['Z'], d['sf2'], d['alpha'], ld)
        Lam, H = _state(M, D, 9)
        for t, sb in enumerate(batches, 1):
            Lam, H = R.natural_step(Lam, H, R.whiten(K, sb['Psi2'], sb['C'], ld), d['beta'], (LD(1) if ld else 1.0) / t, ld)
        seq[ld] = dict(Lam=Lam, H=H)
        Lo, Ho = R.optimum(K, st, d['beta'], ld)
        opt[ld] = dict(Lam=Lo, H=Ho)
    for key in ('Lam', 'H'):
        # the sequence itself: 8x the float64 sequence's error against the long-double sequence
        tol, e = _bound(seq[False], seq[True], key, M)
        err = _relerr(got[key], seq[True][key])
        print('%s sequence: reference %.2e device %.2e bound %.2e' % (key, e, err, tol))
        assert err <= tol, key
        # the identity: the full-data optimum on the full context's own statistics (another summation order than the batches'), by the distance of
        # the float64 SEQUENCE from the long-double optimum
        tol, e = _bound(seq[False], opt[True], key, M)
        err = _relerr(got[key], opt[True][key])
        print('%s optimum: reference %.2e device %.2e bound %.2e' % (key, e, err, tol))
        assert err <= tol, key
    full.close()


@pytest.mark.parametrize('shape', [SMALL, BIG])
def test_publish_makes_the_context_a_predictor_of_q(shape):
    M, D, Q, N = shape
    eng, d = _engine(shape, 'A')
    Lam, H = _state(M, D, 13)
    Xs = np.random.RandomState(14).randn(17, Q)
    eng.svi_begin()
    eng.svi_set(Lam, H)
    eng.svi_step()
    with pytest.raises(_lib.GparmlHipError):             # GP_ERR_STATE: the SVI step leaves no model
        eng.predict(Xs)
    eng.svi_publish()
    with pytest.raises(_lib.GparmlHipError):
        eng.predict(Xs)
    eng.global_step()
    mean, var = eng.predict(Xs)
    m64, v64 = R.predict(d['Z'], d['sf2'], d['alpha'], Lam, H, Xs)
    mld, vld = R.predict(d['Z'], d['sf2'], d['alpha'], Lam, H, Xs, True)
    # the float64 yardstick is the collapsed predictive on the published pseudo-statistics, what the device computes
    import predict_ref
    P2e, Ce = R.publish(R.kmm(d['Z'], d['sf2'], d['alpha']), Lam, H, d['beta'])
    mp, vp = predict_ref.predict(d['Z'], d['sf2'], d['alpha'], d['beta'], P2e, Ce, Xs)
    e_m = max(_relerr(mp, mld), _relerr(m64, mld), M * 2.0 ** -53)
    e_v = max(float(np.max(np.abs(vp[:, 0] - vld))), float(np.max(np.abs(v64 - vld))), M * 2.0 ** -53 * d['sf2']) / d['sf2']
    got_m, got_v = _relerr(mean, mld), float(np.max(np.abs(np.asarray(var).reshape(len(Xs), -1)[:, 0] - vld))) / d['sf2']
    print('mean: reference %.2e device %.2e; var: reference %.2e device %.2e' % (e_m, got_m, e_v, got_v))
    assert got_m <= 8 * e_m and got_v <= 8 * e_v
    eng.close()


def test_status_codes():
    M, D, Q, N = SMALL
    from gparml_amd.engine import ShardEngine
    eng = ShardEngine(N, D, M, Q, device=0)
    lib, h = eng.lib, eng.h
    z = np.zeros((M, max(M, D)))
    p = z.ctypes.data_as(_lib._dp)
    for rc in (lib.gp_svi_set(h, p, p), lib.gp_svi_get(h, p, None, None, None), lib.gp_svi_natural_step(h, 0.5), lib.gp_svi_step(h, 0),
               lib.gp_svi_publish(h), lib.gp_svi_end(h)):
        assert rc == _lib.GP_ERR_STATE
    assert lib.gp_svi_begin(h) == _lib.GP_OK
    assert lib.gp_svi_begin(h) == _lib.GP_ERR_STATE
    assert lib.gp_svi_step(h, 0) == _lib.GP_ERR_STATE                 # no statistics
    assert lib.gp_svi_natural_step(h, 0.5) == _lib.GP_ERR_STATE
    eng.close()
    eng, d = _engine(SMALL, 'A')
    lib, h = eng.lib, eng.h
    eng.svi_begin()
    for rho in (0.0, -0.1, 1.5, float('nan'), float('inf')):
        assert lib.gp_svi_natural_step(h, ctypes.c_double(rho)) == _lib.GP_ERR_BAD_ARG, rho
    Lam, H = _state(M, D, 1)
    bad = Lam.copy()
    bad[1, 0] += 1e-9
    for L_, H_ in ((bad, H), (np.where(np.eye(M) > 0, np.nan, Lam), H), (Lam, np.full_like(H, np.inf))):
        L_, pl = _lib.as_c(L_)
        H_, ph = _lib.as_c(H_)
        assert lib.gp_svi_set(h, pl, ph) == _lib.GP_ERR_BAD_ARG
    assert lib.gp_svi_step(h, 2) == _lib.GP_ERR_BAD_ARG
    eng.svi_set(-np.eye(M), H)
    assert lib.gp_svi_step(h, 0) == _lib.GP_OK                       # asynchronous: the outcome comes through the status
    mask = ctypes.c_int(7)
    assert lib.gp_global_status(h, ctypes.byref(mask)) == _lib.GP_ERR_NOT_PD and mask.value == 0
    with pytest.raises(np.linalg.LinAlgError):
        eng.svi_get()
    eng.svi_set(Lam, H)                                              # the state is the caller's: a good one and the step succeeds
    eng.svi_step()
    eng.close()


def test_an_svi_episode_leaves_the_evaluation_and_itself_reproducible():
    eng, d = _engine(SMALL, 'B')

    def evaluate():
        eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
        eng.phase1(); eng.global_step(); eng.phase2(True)
        o = eng.finish()
        return [o['F'], o['grad_sf2'], o['grad_beta'], o['grad_Z'].copy(), o['grad_alpha'].copy(), eng.download('GRAD_X_MU')]

    def episode():
        eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
        eng.phase1()
        eng.svi_begin()
        eng.svi_natural_step(0.7); eng.svi_step(); eng.phase2(True)
        o = eng.finish()
        s = eng.svi_get()
        res = [o['F'], o['grad_sf2'], o['grad_beta'], o['grad_Z'].copy(), o['grad_alpha'].copy(), eng.download('GRAD_X_MU'), s['Lam'], s['H'], s['Mv'], s['Sv']]
        eng.svi_publish(); eng.global_step()
        res += list(eng.predict(d['X_mu'][:5]))
        eng.svi_end()
        return res
    before = evaluate()
    e1 = episode()
    e2 = episode()
    after = evaluate()
    for a, b in zip(before, after):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    for a, b in zip(e1, e2):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    eng.close()


def test_svi_driver_on_a_toy_regression():
    from gparml_amd.engine import ShardEngine
    from gparml_amd.svi import SVI
    rng = np.random.RandomState(0)
    N, Q, D, M, T = 2000, 1, 1, 16, 10
    X = rng.uniform(-3, 3, (N, Q))
    Y = np.sin(2 * X) + 0.1 * rng.randn(N, D)
    Z = np.linspace(-3, 3, M)[:, None]
    hyp = dict(Z=Z, sf2=1.0, alpha=np.array([2.0]), beta=25.0)
    Xs = np.linspace(-2.5, 2.5, 40)[:, None]
    # the collapsed optimum's predictions
    col = ShardEngine(N, D, M, Q, device=0)
    col.upload_shard(Y, X, np.zeros_like(X))
    col.set_globals(hyp['Z'], hyp['sf2'], hyp['alpha'], hyp['beta'])
    col.phase1(); col.global_step()
    m_col, v_col = col.predict(Xs)
    svi = SVI((D, M, Q), Y, X, dict(batch=N // T, seed=1, **hyp))
    rows = []
    for t in range(1, 51):
        svi.step(1.0 / t)                                # 5 epochs over equal batches, fixed hyper-parameters
        rows.append(svi.last_batch)
    eng = svi.publish()
    m, v = eng.predict(Xs)
    # rho_t = 1/t makes the state the mean of the 50 scaled batch statistics = the full statistics (every row five times in 50 batches of five
    # permutation epochs).  Yardstick, from the reference alone: the truth is the long-double optimum on long-double full statistics; the float64
    # reference runs the device's 50 batches (float64 batch statistics, 1/t steps), the float64 collapsed predictive runs on float64 full
    # statistics; the two device paths may differ by 8x the sum of those two errors
    import predict_ref
    Z, sf2, alpha, beta = hyp['Z'], hyp['sf2'], hyp['alpha'], hyp['beta']
    Lt, Ht = R.optimum(R.kmm(Z, sf2, alpha, True), R.stats_fixed(Z, sf2, alpha, X, Y, ld=True), beta, True)
    mt, vt = R.predict(Z, sf2, alpha, Lt, Ht, Xs, True)
    K64 = R.kmm(Z, sf2, alpha)
    Lam, H = np.eye(M), np.zeros((M, D))
    for t, idx in enumerate(rows, 1):
        Lam, H = R.natural_step(Lam, H, R.whiten(K64, **R.stats_fixed(Z, sf2, alpha, X[idx], Y[idx], float(T))), beta, 1.0 / t)
    ms, vs = R.predict(Z, sf2, alpha, Lam, H, Xs)
    f64 = R.stats_fixed(Z, sf2, alpha, X, Y)
    mc, vc = predict_ref.predict(Z, sf2, alpha, beta, f64['Psi2'], f64['C'], Xs)
    scale_m = float(np.max(np.abs(mt)))
    e_m = (float(np.max(np.abs(ms - mt))) + float(np.max(np.abs(mc - mt)))) / scale_m
    e_v = (float(np.max(np.abs(vs - vt))) + float(np.max(np.abs(vc[:, 0] - vt)))) / sf2
    tol_m, tol_v = 8 * max(e_m, M * 2.0 ** -53), 8 * max(e_v, M * 2.0 ** -53)
    got_m = float(np.max(np.abs(m - m_col))) / scale_m
    got_v = float(np.max(np.abs(np.asarray(v).reshape(len(Xs), -1)[:, 0] - np.asarray(v_col).reshape(len(Xs), -1)[:, 0]))) / sf2
    print('mean: reference %.2e device %.2e bound %.2e; var: reference %.2e device %.2e bound %.2e' % (e_m, got_m, tol_m, e_v, got_v, tol_v))
    assert got_m <= tol_m and got_v <= tol_v
    # one Adam phase on the hyper-parameters raises the full-data bound
    before = svi.bound()
    for _ in range(30):
        svi.step(0.2, learn=True)
    assert svi.bound() > before
    col.close()
    svi.close()
