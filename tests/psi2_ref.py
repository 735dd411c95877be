"""Long-double reference of what a free-embedding (regime B) evaluation computes in its two phases, with an elementwise error bound.

The conventions are those of tests/compat_ref.py (read its docstring first): numpy long double for the reference, float64 for the "mirror" (float64
inputs, every sum ascending with one addition per term), point by point so that nothing of size N M M Q exists, every function returns
``(value, A, T)`` and the bound is ``compat_ref.bound``:

    |dev - ref| <= 2 (T + n_terms u A) + 2^-1022,        u = 2^-53; the float64 mirror must hold it WITHOUT the factor 2.

What is computed (``phase1`` and ``phase2``; oracle/factorised.py states the same formulas in float64).
  phase 1   psi2_sum (M, M) = sum_n psi2_n, psi1ty (M, D) = sum_n Psi1[n, m] Y[n, d], psi0 = N sf2, kl = 1/2 sum_nq (S + mu^2 - ln S - 1)
            (partial_terms.py:45-52, 74-87).
  phase 2   from float64 Bbar (M, M) = dF/dPsi2 and Abar (M, D) = dF/dC taken as exact inputs, with T_n = Bbar o psi2_n and H_n = Psi1_n o (Abar Y_n):
            grad_z_data (M, Q), grad_alpha_data (Q,): the contractions of dpsi1ty_dz, dpsi2_dz, dpsi1ty_dalpha, dpsi2_dalpha with Abar and Bbar
            (partial_terms.py:207-240, 286-299 without the K_mm terms), and grad_x_mu, grad_x_s (N, Q) (partial_terms.py:367-431) with their KL parts.

What the device arrays hold (read from finish_kernel, pt2_points_finish_kernel, point_kernel and p2_reduce_kernel).
  * ``grads`` (gp_debug_peek) = grad_z_data | grad_alpha_data: the sums over the points only.  gp_finish adds the global step's gK to it, and gK holds
    the K_mm parts AND the term -1/4 sum (Bbar o Psi2)(z - z')^2 of grad_alpha, which needs the reduced Psi2 only (csrc/linalg.hip).  So that term is
    NOT part of grad_alpha_data, exactly as oracle.factorised.phase2 leaves it to finish().
  * The symmetric Bbar is counted in both orders: the psi2 part of grad_Z is twice the one-sided contraction (partial_terms.py:238).  With
    r = T_n 1 and t = T_n Z (T_n symmetric) it is  -a (z r - t) + w (2 mu r - z r - t)  per point, no further factor.
  * GP_ARR_GRAD_X_MU = -mu - u (mu h - HZ) - w (2 mu sr - 2 zr): the sign is that of the bound's gradient (dF, not d(-F)); the KL part -mu is in the
    CALLER's coordinates, everything else in coordinates centred at the column mean of Z.
  * GP_ARR_GRAD_X_S is the derivative with respect to the variance S itself, not its raw (softplus-inverse) form, when the shard was uploaded with
    variances:  -1/2 (1 - 1/S) + 1/2 u^2 quad1 - 1/2 u h + 1/2 w^2 quad2 - w sr.  A row with S = 0 among free ones would have +inf there and in kl
    (log 0, partial_terms.py:85): gp_upload_shard refuses such a shard, so there is no device value to hold (the GPU test asserts the refusal).

The terms, A and n_terms.  The library evaluates every polynomial factor in EXPANDED form on centred coordinates (csrc/psi2.hip:375-377, psi.hip:1152-
1154): grad_Z as R1 - z R2, the quadratic forms as 4 mu^2 sr - 8 mu zr + 2 z2r + 2 zt, from running sums r, t, sr, zr, z2r, zt over the inducing
points.  An expanded evaluation rounds relative to the expanded magnitudes, so the terms of a sum are the expanded monomials: A is their absolute
sum, with |Bbar| and |Abar|, |Y| as factors, and the reference forms the value the same way (in long double, eleven bits below u of A).  n_terms is the
number of (n, m') resp. (n, d) pairs behind an element -- N (M + D) for grad_z, N M (M + D) for grad_alpha, M (M + D) for the per-point arrays, N for the
statistics, N Q for kl -- an upper bound on the additions whatever order a kernel takes them in (the monomials of one pair are counted in C_FAC).

T, derived.  tau of Psi1 and of the per-point psi2 are compat_ref's.  Added here:
  * The expanded pair exponent.  Every pair kernel but psi2_pairs_kernel forms the exponent as LEA[n, m] + LEA[n, m'] + sum_q z_mq v2_q z_m'q with
    LEA = LE - 1/2 sum_q v2_q z_mq^2, v2 = (alpha - w) / 2 (csrc/psi2.hip:44-45, 380): the coupling -1/4 sum (alpha - w)(z - z')^2 as three sums that
    cancel.  Each is a chain of Q fused multiply-adds, stored or added with one more rounding each: (Q + 3) u (1/2 sum_q v2_q (|z_mq| + |z_m'q|)^2)
    on centred z, in place of the (1 + Q) u coup that compat_ref counts for the difference form.  It is added to tau for every kernel (for
    psi2_pairs_kernel it is slack).
  * T_n = Bbar psi2_n and H_n = Psi1_n G_n: one rounding each; G_n = sum_d Abar Y is part of the sum (its D additions are in n_terms).
  * The rational factors of a monomial (u = alpha / (alpha S + 1), w, their squares, 1 / d^2, S / d, the centring of mu and z, the products and the
    few additions that join the monomials of one pair): at most sixteen roundings, C_FAC = 16, relative to the monomial.
  * kl: S + mu^2 - ln S - 1 per entry, four roundings and ln's own (C_KL = 6) relative to |S| + mu^2 + |ln S| + 1.
"""
import numpy as np

import compat_ref as R

LD = R.LD
C_FAC = 16
C_KL = 6
PHASE1 = ('psi2_sum', 'psi1ty', 'psi0', 'kl')
PHASE2 = ('grad_z_data', 'grad_alpha_data', 'grad_x_mu', 'grad_x_s')


def n_terms(name, N, D, M, Q):
    return {'psi2_sum': N, 'psi1ty': N, 'psi0': 1, 'kl': N * Q, 'grad_z_data': N * (M + D), 'grad_alpha_data': N * M * (M + D),
            'grad_x_mu': M * (M + D), 'grad_x_s': M * (M + D)}[name]


class _Pieces(R._Pieces):
    """compat_ref's pieces with the (M, M, Q) tables formed once per case, so that the per-point psi2 is two matrix-vector products and no temporary
    of that size, and with the expanded pair exponent's term in tau.  ``drop``: (n, m, m') of one term to leave out (the mutation of the CPU test)."""

    def __init__(self, Z, sf2, alpha, mu, S, full, drop=None):
        super(_Pieces, self).__init__(Z, sf2, alpha, mu, S, None, full)
        self.o = np.mean(self.Z, axis=0)
        self.zc, self.mc = self.Z - self.o, self.mu - self.o           # the centred coordinates the library works on
        self.dz2 = self.dz * self.dz
        self.drop = drop
        if full:
            self.dzc = np.abs(self.dz) * self.czz
            zs = self.cz[:, None, :] + self.cz[None, :, :]
            self.zs2 = zs * zs

    def psi2_point(self, n, d_n):
        a = self.alpha
        w = a / self.d2[n]
        v = a - w
        lnE = (d_n * d_n).dot(w) / 2
        coup = self.dz2.dot(v) / 4
        val = self.c2[n] * np.exp(-(lnE[:, None] + lnE[None, :] + coup))
        if self.drop is not None and self.drop[0] == n:
            val[self.drop[1], self.drop[2]] = 0
        if not self.full:
            return val, None
        cd = (np.abs(d_n) * (self.cm[n] + self.cz + np.abs(d_n))).dot(w)
        cc = self.dzc.dot(v) / 2
        E = self.lnc2[n] + lnE[:, None] + lnE[None, :] + coup
        tau = self.u * ((1 + self.Q) * E + self.Q * (lnE[:, None] + lnE[None, :]) + self.c_psi2 + cd[:, None] + cd[None, :] + cc
                        + (self.Q + 3) * self.zs2.dot(v) / 4)
        return val, tau


def _acc(acc, k, *terms):
    acc[k] = [t.copy() if np.ndim(t) else t for t in terms] if k not in acc else [x + t for x, t in zip(acc[k], terms)]


def _phase1(p, Y):
    acc = {}
    u = p.u
    for n in range(p.N):
        v, tau, _ = p.psi1_rows(slice(n, n + 1))
        v = v[0][:, None] * Y[n][None, :]
        if p.full:
            _acc(acc, 'psi1ty', v, np.abs(v), np.abs(v) * (tau[0][:, None] + u))
        else:
            _acc(acc, 'psi1ty', v)
        v, tau = p.psi2_point(n, p.mu[n] - p.Z)
        if p.full:
            _acc(acc, 'psi2_sum', v, v, v * tau)
        else:
            _acc(acc, 'psi2_sum', v)
        t = (p.S[n] + p.mu[n] * p.mu[n] - np.log(p.S[n]) - 1) / 2
        ta = (p.S[n] + p.mu[n] * p.mu[n] + np.abs(np.log(p.S[n])) + 1) / 2
        for q in range(p.Q):                                            # one addition per term, as every sum here
            _acc(acc, 'kl', t[q], ta[q], C_KL * u * ta[q])
    psi0 = p.sf2 * p.N
    acc['psi0'] = [psi0, psi0, u * psi0]
    return acc


def _phase2(p, Y, Bbar, Abar):
    acc = {}
    a, u, cf = p.alpha, p.u, C_FAC * p.u
    z, za = p.zc, np.abs(p.zc)
    z2 = z * z
    aB, aA = np.abs(Bbar), np.abs(Abar)
    gmu = np.empty((p.N, p.Q), dtype=p.Z.dtype)
    gs = np.empty_like(gmu)
    if p.full:
        gmuA, gmuT, gsA, gsT = (np.empty_like(gmu) for _ in range(4))
    for n in range(p.N):
        m, ma = p.mc[n], np.abs(p.mc[n])
        S, d1, d2 = p.S[n], p.d1[n], p.d2[n]
        u1, w = a / d1, a / d2
        # ---- the Psi1 part: H = Psi1_n o (Abar Y_n)
        v1, tau1, _ = p.psi1_rows(slice(n, n + 1))
        v1 = v1[0]
        H = v1 * Abar.dot(Y[n])
        sums = [(H, z, z2)]
        if p.full:
            Ha = v1 * aA.dot(np.abs(Y[n]))
            sums += [(Ha, za, z2), (Ha * (tau1[0] + u), za, z2)]
        out = []
        for X, zz, zz2 in sums:
            out.append((X, X.sum(), X.dot(zz), X.dot(zz2)))
        (H, h, HZ, HZ2) = out[0]
        gz = [H[:, None] * u1 * m - z * H[:, None] * u1]
        q1 = [m * m * h - 2 * m * HZ + HZ2]
        for X, xs, XZ, XZ2 in out[1:]:
            gz.append(X[:, None] * u1 * (ma + za))
            q1.append(m * m * xs + 2 * ma * XZ + XZ2)
        hs = [o[1] for o in out]
        hz = [o[2] for o in out]
        # ---- the psi2 part: T = Bbar o psi2_n, r = T 1, t = T Z
        v2, tau2 = p.psi2_point(n, p.mu[n] - p.Z)
        Ts = [(Bbar * v2, z, z2)]
        if p.full:
            Ta = aB * v2
            Ts += [(Ta, za, z2), (Ta * (tau2 + u), za, z2)]
        q2, srs, zrs = [], [], []
        for i, (X, zz, zz2) in enumerate(Ts):
            r, t = X.sum(axis=0), X.T.dot(zz)
            sr, zr, z2r, zt = r.sum(), r.dot(zz), r.dot(zz2), np.sum(t * zz, axis=0)
            if i == 0:
                gz[0] = gz[0] - a * (z * r[:, None] - t) + w * (2 * m * r[:, None] - z * r[:, None] - t)
                q2.append(4 * m * m * sr - 8 * m * zr + 2 * z2r + 2 * zt)
            else:
                gz[i] = gz[i] + a * (zz * r[:, None] + t) + w * (2 * ma * r[:, None] + zz * r[:, None] + t)
                q2.append(4 * m * m * sr + 8 * ma * zr + 2 * z2r + 2 * zt)
            srs.append(sr)
            zrs.append(zr)
        # ---- the sums over the points and the per-point arrays, each as (value, A, T)
        if p.full:
            _acc(acc, 'grad_z_data', gz[0], gz[1], gz[2] + cf * gz[1])
        else:
            _acc(acc, 'grad_z_data', gz[0])
        ga = [-(q1[0] / (d1 * d1) + S / d1 * hs[0]) / 2 - q2[0] / (d2 * d2) / 4 - S / d2 * srs[0]]
        gmu[n] = -p.mu[n] - u1 * (m * hs[0] - hz[0]) - w * (2 * m * srs[0] - 2 * zrs[0])
        kls, klsa = -(1 - 1 / S) / 2, (1 + 1 / S) / 2
        gs[n] = kls + u1 * u1 * q1[0] / 2 - u1 * hs[0] / 2 + w * w * q2[0] / 2 - w * srs[0]
        if p.full:
            for i in (1, 2):
                ga.append((q1[i] / (d1 * d1) + S / d1 * hs[i]) / 2 + q2[i] / (d2 * d2) / 4 + S / d2 * srs[i])
            gmuA[n] = np.abs(p.mu[n]) + u1 * (ma * hs[1] + hz[1]) + w * (2 * ma * srs[1] + 2 * zrs[1])
            gmuT[n] = u1 * (ma * hs[2] + hz[2]) + w * (2 * ma * srs[2] + 2 * zrs[2]) + cf * gmuA[n]
            gsA[n] = klsa + u1 * u1 * q1[1] / 2 + u1 * hs[1] / 2 + w * w * q2[1] / 2 + w * srs[1]
            gsT[n] = u1 * u1 * q1[2] / 2 + u1 * hs[2] / 2 + w * w * q2[2] / 2 + w * srs[2] + cf * gsA[n]
            _acc(acc, 'grad_alpha_data', ga[0], ga[1], ga[2] + cf * ga[1])
        else:
            _acc(acc, 'grad_alpha_data', ga[0])
    acc['grad_x_mu'] = [gmu, gmuA, gmuT] if p.full else [gmu]
    acc['grad_x_s'] = [gs, gsA, gsT] if p.full else [gs]
    return acc


def _both(fn, Z, sf2, alpha, mu, S, extra, drop):
    """{name: (value, A, T)}: the value in the type of the inputs; A and T from a float64 pass when the inputs are long double (compat_ref.all_arrays)."""
    Z = np.asarray(Z)
    if Z.dtype == np.float64:
        out = fn(_Pieces(Z, sf2, alpha, mu, S, True, drop), *extra)
        return {k: tuple(v) for k, v in out.items()}
    val = fn(_Pieces(Z, sf2, alpha, mu, S, False, drop), *extra)
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    err = fn(_Pieces(f64(Z), float(sf2), f64(alpha), f64(mu), f64(S), True), *[f64(x) for x in extra])
    return {k: (val[k][0], err[k][1], err[k][2]) for k in val}


def phase1(Z, sf2, alpha, mu, S, Y, drop=None):
    """{psi2_sum, psi1ty, psi0, kl: (value, A, T)}."""
    return _both(_phase1, Z, sf2, alpha, mu, S, (np.asarray(Y),), drop)


def phase2(Z, sf2, alpha, mu, S, Y, Bbar, Abar, drop=None):
    """{grad_z_data, grad_alpha_data, grad_x_mu, grad_x_s: (value, A, T)} for the given dF/dPsi2 (M, M) and dF/dC (M, D)."""
    return _both(_phase2, Z, sf2, alpha, mu, S, (np.asarray(Y), np.asarray(Bbar), np.asarray(Abar)), drop)


def hold(what, got, ref, shape, factor=2.0, tag='psi2 elementwise'):
    """Every array of ``got`` against the bound: prints the worst error / bound per array and returns the failures as strings."""
    N, D, M, Q = shape
    bad = []
    for k in got:
        v, A, T = ref[k]
        dev, v = np.asarray(got[k], dtype=np.float64), np.asarray(v)
        ratio, idx = R.worst(dev, v, A, T, n_terms(k, N, D, M, Q), factor)
        print('[%s] %-28s %-16s worst error / bound %.3g at %s' % (tag, what, k, ratio, idx))
        if not ratio <= 1.0:
            bad.append('%s: %.3g times the bound at %s (got %r, reference %r)' % (k, ratio, idx, float(dev[idx]), float(np.asarray(v)[idx])))
    return bad


# --------------------------------------------------------------------------------------------------------- the cases
# (name, N, D, M, Q, alpha, phase-2 family): the smallest shapes that reach each launch shape of run_phase1_b, run_phase2_b and choose_b_path
# (csrc/psi2.hip).  alpha as tests/test_gpu_parity.py chooses it for the latent width and the density of the inducing points, so that the global
# step factorises without jitter.  N stays small where M is large: the work of the reference is N M^2 Q.
def _alpha(Q, M):
    a = 0.5 if Q <= 4 else 0.8 if Q <= 6 else 0.5 if Q <= 8 else 0.3 if Q <= 10 else 0.3 if Q <= 13 else 0.15 if Q <= 16 else 0.1 if Q <= 24 else 0.08 if Q <= 32 else 0.05
    return 4.0 if (Q <= 4 and M >= 129) else a


def _case(N, D, M, Q, fam, tag=''):
    return ('%s_n%d_d%d_m%d_q%d%s' % (fam.lower(), N, D, M, Q, tag), N, D, M, Q, _alpha(Q, M), fam)


CASES = (
    # psi2_pairs_kernel and the column kernel in every width, Q odd and even, at N = 62 (a last trip of two points, S = 62 slices) and M = 33 (three tiles, the last ragged)
    [_case(62, 2, 33, q, 'COLS') for q in range(3, 17)]
    # the N and M edges at Q = 10 and 16: every N mod 4, one and several 16 x 16 tiles, one and two slabs
    + [_case(n, 2, m, q, 'COLS') for q in (10, 16) for n, m in ((61, 17), (63, 17), (61, 33), (63, 64), (62, 65), (61, 128))]
    # N = 531: slices of several trips (S = 64, nine points each: two trips and a tail), pb_blocks = 34 (pb2_reduce1_kernel with S2 = 2)
    + [_case(531, 2, 17, 10, 'COLS')]
    # five slabs in two slab groups, the second ragged
    + [_case(20, 2, 300, q, 'COLS') for q in (13, 14, 15, 16)]
    # the symmetric kernel: three slabs (two waves, a bye), four (no bye), five (a bye); Q = 8 and 12 are the widths with the constant ones quad
    + [_case(20, 2, m, q, 'SYM') for m, q in ((129, 3), (129, 8), (129, 12), (200, 6), (200, 10), (200, 12), (300, 11), (300, 12), (300, 6))]
    # the matrix-core pair kernel and the tile kernel: QB = 24, 32, 52, 64 (Q = 63: the spare ones column), three and six tiles of 64, S = 1
    + [_case(70, 2, 65, q, 'TILES') for q in (17, 24, 25, 31, 32, 51, 52, 63)]
    + [_case(70, 2, 130, q, 'TILES') for q in (17, 24, 31, 52, 63)]
    + [_case(531, 2, 65, 17, 'TILES')]                     # S = 2, the second slice ragged
    # the generic path: one chunk, and two chunks with a ragged second (P = 145 points at M = 240)
    + [_case(40, 2, 9, 64, 'GENERIC'), _case(40, 2, 9, 70, 'GENERIC'), _case(150, 2, 240, 64, 'GENERIC')]
    # edges
    + [_case(40, 2, 1, 3, 'COLS'), _case(1, 2, 5, 3, 'COLS'), _case(64, 1, 16, 2, 'COLS', '_far'),
       _case(50, 129, 20, 10, 'COLS')]
)
CASE_NAMES = [c[0] for c in CASES]
FORCED = {                                                 # environment of a child process -> cases
    'GPARML_B_PHASE2=tiles': [_case(70, 2, 65, q, 'TILES', '_forced') for q in (4, 10, 16)],
    'GPARML_B_SYM_MAXQ=10': [_case(20, 2, 200, 12, 'COLS', '_maxq10')],
}
REDUCED_N = {'cols_n531_d2_m17_q10': 131, 'tiles_n531_d2_m65_q17': 90, 'generic_n150_d2_m240_q64': 12}     # the CPU mirror's N for the long cases


def family(M, Q, forced_tiles=False, maxq=12):
    """The phase-2 family choose_b_path picks: this restates csrc/psi2.hip:733-754 (there is no query for it)."""
    if Q >= 64:
        return 'GENERIC'
    if Q >= 17 or forced_tiles:
        return 'TILES'
    QB = next(w for w in (4, 6, 8, 10, 12, 14, 16) if Q <= w)
    nslab, Mp = (M + 63) // 64, (M + 127) // 128 * 128
    smem = Mp * (QB + 1) * 8
    sym = QB <= min(maxq, 12) and 3 <= nslab <= 16 and smem <= 160 * 1024 and (160 * 1024 // smem) * ((nslab + 1) // 2) >= 12
    return 'SYM' if sym else 'COLS'


def case_inputs(case, N=None):
    """The float64 inputs of a case (oracle.factorised.synthetic_shard; inducing points around re-used rows where M > N); ``N``: fewer points."""
    from oracle import factorised as Fz
    name, N0, D, M, Q, alpha, fam = case
    N = N0 if N is None else N
    seed = 300 + sum(ord(ch) for ch in name) % 1000
    d = Fz.synthetic_shard(N, D, min(M, N), Q, regime='B', seed=seed, zseed=seed + 50, alpha_value=alpha)
    rs = np.random.RandomState(seed + 99)
    if M > N:
        d['Z'] = d['X_mu'][rs.randint(0, N, size=M)] + 0.5 * rs.randn(M, Q)
    if name.endswith('_far'):
        far = R.case_inputs(R.CASES[R.CASE_NAMES.index(R.FAR_FIELD)])
        assert (far['N'], far['D'], far['M'], far['Q']) == (N, D, M, Q)
        d = {k: far[k] for k in ('Y', 'X_mu', 'X_S', 'Z', 'sf2', 'alpha', 'beta')}
    d.update(N=N, D=D, M=M, Q=Q, name=name if N == N0 else '%s_at_n%d' % (name, N), family=fam)
    return d


def synthetic_partials(d):
    """A symmetric Bbar and an Abar of the sizes the global step produces, for the CPU tests (seeded; any float64 values serve as exact inputs)."""
    rs = np.random.RandomState(len(d['name']) + d['M'])
    B = rs.randn(d['M'], d['M'])
    return (B + B.T) / 2, rs.randn(d['M'], d['D'])
