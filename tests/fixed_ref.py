"""Reference of what a fixed-embedding (regime A, every variance zero) evaluation computes in its two phases, with an elementwise error bound.

The conventions are those of tests/compat_ref.py and tests/psi2_ref.py (read their docstrings first): every function returns ``(value, A, T)`` per
array and the bound is ``compat_ref.bound``:

    |dev - ref| <= 2 (T + n_terms u A) + 2^-1022,        u = 2^-53; the float64 mirror must hold it WITHOUT the factor 2.

Exact inputs.  Nothing is exponentiated here: the device's own Psi1 (GP_ARR_PSI1, a straight copy of Kaug's first M columns) is taken as the exact
float64 matrix K (N, M), next to Y, the device's Bbar and Abar (gp_debug_peek) for phase 2, and the centred coordinates zc = Z - o, mc = X_mu - o.
The origin o is the column mean of Z as choose_origin (csrc/api.hip) forms it on the host -- mean[q] += Z[m][q] / M in ascending m -- which
``origin`` repeats bit for bit; the GPU test asserts zc and mc against gp_debug_peek('Z') and ('mu'), so the origin's rounding is in no bound.
(That Psi1 itself is right is compat_ref's business: the GPU test holds it to compat_ref's own bound for the same inputs.)

Phase 1 (p1v2_kernel / p1v2_reduce_kernel; p1_kernel8 / p1_reduce_kernel / p1_scalars_kernel where p1v2 does not apply).
  psi2_sum[m, m'] = sum_n K[n, m] K[n, m'],  psi1ty[m, d] = sum_n K[n, m] Y[n, d].  The MFMA is fused, so a term has no rounding of its own, T = 0;
  any summation tree over N terms -- the slices, the eight chains of the reduce, the zero rows of the padding -- has N - 1 additions: the bound is
  2 N u A with A = sum_n |K K'| resp. sum_n |K Y|, nothing measured in it.  psi0 = sf2 N: one product, T = u psi0, n_terms 1.  sum_yyt = sum_nd
  Y^2 (sumsq_kernel and the host's sum of its 1024 partials): T = u A for the squares, n_terms N D.
  kl: p1v2_reduce_kernel writes 0.0 into every scalar slot but sum_YYT, psi0 and n, and p1_scalars_kernel writes ``regimeA ? 0.0 : kl``: the KL
  scalar of a fixed-embedding shard is DEFINED as exact zero (the reference's formula has log S with S = 0).  value 0, A = T = 0: the bound is the
  floor, i.e. only +-0 or a subnormal passes.

Phase 2 (csrc/psi.hip:646-649, 1143-1146), from Bbar (M, M) and Abar (M, D):
  G = [K | Y] [2 Bbar ; Abar^T],  W = G o K,  R0 = W^T 1,  R1 = W^T mc,  h = W 1,  HZ = W zc
  grad_z_data     = alpha (R1 - zc R0)
  grad_alpha_data = -1/2 (sum_n h_n mc_n^2 + sum_m (zc^2 R0 - 2 zc R1))
  grad_x_mu       = -(mc + o) - alpha (mc h - HZ),   grad_x_s = exact zero        (phase2(True): p2_gen8_kernel<true> + point_kernel)
  Both device forms evaluate these EXPANDED on the centred coordinates (p2_reduce_kernel: r1 - z r0 and z z r0 - 2 z r1, the mu^2 term from the wave's
  row sums; point_kernel: m m h - 2 m hz + hz2), so the terms of a sum are the expanded monomials and A is their absolute sum with |Bbar|, |Abar|,
  |Y| as factors: |W| <= K (K |2 Bbar| + |Y| |Abar|^T).  n_terms: the (n, m') and (n, d) pairs behind an element number N (M + D) for
  grad_z_data, N M (M + D) for grad_alpha_data and M (M + D) for grad_x_mu, but the kernels do not add them in one flat sum: G[n, m] is formed first
  (its M + D chain steps are counted in T below), and what is added afterwards is one W-term per point (N additions, whatever the tree: slices, wave
  partials, the reduce), for grad_alpha_data also one per inducing point (p2_reduce_kernel's gapart rows through colsum2_kernel, or point_kernel's
  sum over m before the points are added: N + M), and for grad_x_mu the M terms of a row.  So n_terms = N, N + M and M: the depth of the nested sums,
  not the pair count, which would be an upper bound three to seven orders looser at the larger cases (a Bm entry off by 1e-9 would pass it).
  T, counted from the kernels: one term K[n, m'] 2Bbar[m', m] K[n, m] x passes the M + D fused steps of G's accumulator chain (each rounds the
  partial sum it belongs to), ONE rounding for W = G o K, and the final combination: p2_reduce_kernel z * r0, the subtraction, alpha * (.) -- three;
  grad_alpha's z * z, (z z) * r0, (2 z) * r1 and the two additions resp. hs * x in front of the fused multiply-add -- at most four per monomial;
  point_kernel's m * m, (m m) * h, (2 m) * hzq, the two additions (the divisions by d1 = 1 are exact) -- four.  C_FIN = 4 covers all of them:
      T = (M + D + 1 + C_FIN) u A.
  (The additions over n, m' and d are in n_terms, as everywhere.)

The value.  It must be good to well below u A: long double matrix products (a sum of N terms in long double is off by at most N 2^-64 A, eleven bits
below the N u A it is compared with), or -- ``exact='dd'`` -- dd_ref's exact integer product in row chunks of at most 2048, added in Python integers
(exact; float64 BLAS underneath).  test_fixed_ref_cpu.py holds the two routes to 2^-60 A of each other.

The float64 mirror (``mirror``): the same inputs, every sum ascending with one addition per term (numpy's cumulative sum), products rounded before
they are added.  ``drop=(n, m, m')`` leaves the term K[n, m] K[n, m'] out of psi2_sum[m, m'] and the term K[n, m'] 2Bbar[m', m] out of G[n, m];
``drop_y=(n, m, d)`` leaves K[n, m] Y[n, d] out of psi1ty[m, d] and Y[n, d] Abar[m, d] out of G[n, m].

``family`` restates which launches a shape takes (p1v2.hip, psi.hip, p2_rem.hip: there is no query for the plan)."""

import numpy as np

import compat_ref as R
import dd_ref

LD = R.LD
U = R.U
C_FIN = 4


def M_D_FIN(d):
    """roundings of one term: T = M_D_FIN u A"""
    return d['M'] + d['D'] + 1 + C_FIN

PHASE1 = ('psi2_sum', 'psi1ty', 'psi0', 'sum_yyt', 'kl')
PHASE2 = ('grad_z_data', 'grad_alpha_data')
POINTS = ('grad_x_mu', 'grad_x_s')
SC_SUM_YYT, SC_PSI0, SC_KL, SC_NLOCAL, SC_COUNT = 0, 1, 2, 3, 8            # csrc/gp_common.h


def n_terms(name, N, D, M, Q):
    return {'psi2_sum': N, 'psi1ty': N, 'psi0': 1, 'sum_yyt': N * D, 'kl': 1, 'grad_z_data': N, 'grad_alpha_data': N + M, 'grad_x_mu': M,
            'grad_x_s': 1}[name]


def origin(Z):
    """choose_origin's column mean of Z, bit for bit: mean[q] += Z[m][q] / M in ascending m."""
    Z = np.asarray(Z, dtype=np.float64)
    o = np.zeros(Z.shape[1])
    Mf = float(Z.shape[0])
    for m in range(Z.shape[0]):
        o = o + Z[m] / Mf
    return o


def centred(Z, X_mu):
    """(zc, mc, o): what gp_set_globals and prep_elem_kernel store, one subtraction each."""
    o = origin(Z)
    return np.asarray(Z, dtype=np.float64) - o, np.asarray(X_mu, dtype=np.float64) - o, o


# --------------------------------------------------------------------------------------------------------- exact sums of products
_shl = np.frompyfunc(lambda n, s: n << int(s), 2, 1)


def _int_to_ld(n, e):
    """n 2^e (Python int, int) as a long double, rounded once per half"""
    if n == 0:
        return LD(0)
    s = max(0, abs(n).bit_length() - 120)
    m = n >> s
    hi = float(m)
    lo = float(m - int(hi))
    return np.ldexp(LD(hi), int(e + s)) + np.ldexp(LD(lo), int(e + s))


_to_ld = np.frompyfunc(_int_to_ld, 2, 1)


def atb_exact(A, B, rows=2048):
    """A^T B (A (N, a), B (N, b) float64) as long double from the EXACT value: dd_ref's integer product per row chunk, chunks added in Python integers."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    tot, te = None, None
    for i in range(0, A.shape[0], rows):
        n, e = dd_ref._exact_int(np.ascontiguousarray(A[i:i + rows].T), B[i:i + rows])
        if tot is None:
            tot, te = n, e
        else:
            e2 = np.minimum(te, e)
            tot, te = _shl(tot, te - e2) + _shl(n, e - e2), e2
    return _to_ld(tot, te.astype(object)).astype(LD)


def atb_ld(A, B, rows=4096):
    """A^T B in long double, row chunk by row chunk"""
    out = np.zeros((A.shape[1], B.shape[1]), dtype=LD)
    for i in range(0, A.shape[0], rows):
        out += np.asarray(A[i:i + rows], dtype=LD).T @ np.asarray(B[i:i + rows], dtype=LD)
    return out


def _atb(A, B, exact):
    return atb_exact(A, B) if exact == 'dd' else atb_ld(A, B)


def _asc(X):
    """sum over axis 0, ascending, one addition per term"""
    return np.cumsum(X, axis=0)[-1]


# --------------------------------------------------------------------------------------------------------- phase 1
def phase1(K, Y, sf2, exact='ld', mirror=False, drop=None, drop_y=None):
    """{psi2_sum, psi1ty, psi0, sum_yyt, kl: (value, A, T)} from the float64 K (N, M) and Y (N, D)."""
    K, Y = np.asarray(K, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    N, M = K.shape
    aK, aY = np.abs(K), np.abs(Y)
    out = {}
    if mirror:
        P2 = np.empty((M, M))
        for m in range(M):
            t = K[:, m:m + 1] * K
            if drop is not None and drop[1] == m:
                t[drop[0], drop[2]] = 0.0
            P2[m] = _asc(t)
        C = np.empty((M, Y.shape[1]))
        for m in range(M):
            t = K[:, m:m + 1] * Y
            if drop_y is not None and drop_y[1] == m:
                t[drop_y[0], drop_y[2]] = 0.0
            C[m] = _asc(t)
        syy = float(np.cumsum((Y * Y).reshape(-1))[-1])
    else:
        KY = _atb(K, np.concatenate([K, Y], axis=1), exact)
        P2, C = KY[:, :M], KY[:, M:]
        Yl = np.asarray(Y, dtype=LD)
        syy = np.sum(Yl * Yl)
    out['psi2_sum'] = (P2, aK.T @ aK, np.zeros((M, M)))
    out['psi1ty'] = (C, aK.T @ aY, np.zeros((M, Y.shape[1])))
    psi0 = float(sf2) * N if mirror else LD(sf2) * N
    out['psi0'] = (psi0, float(sf2) * N, U * float(sf2) * N)
    sa = float(np.sum(Y * Y))
    out['sum_yyt'] = (syy, sa, U * sa)
    out['kl'] = (0.0 if mirror else LD(0), 0.0, 0.0)
    return out


# --------------------------------------------------------------------------------------------------------- phase 2
def phase2(K, Y, Bbar, Abar, zc, mc, o, alpha, points=True, mirror=False, drop=None, drop_y=None):
    """{grad_z_data, grad_alpha_data[, grad_x_mu, grad_x_s]: (value, A, T)} for the given dF/dPsi2 (M, M) and dF/dC (M, D)."""
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    K, Y, Bbar, Abar, zc, mc, o, alpha = (f64(x) for x in (K, Y, Bbar, Abar, zc, mc, o, alpha))
    N, M = K.shape
    D = Y.shape[1]
    KY = np.concatenate([K, Y], axis=1)
    Bm = np.concatenate([2.0 * Bbar, Abar.T], axis=0)                  # (M + D, M): the Bm image without its padding
    az, am = np.abs(zc), np.abs(mc)
    # ---- A: the absolute sums of the expanded monomials (float64 is enough for a bound)
    WA = (np.abs(KY) @ np.abs(Bm)) * np.abs(K)
    R0A, R1A, hA, HZA = WA.sum(axis=0), WA.T @ am, WA.sum(axis=1), WA @ az
    A = {'grad_z_data': alpha * (R1A + az * R0A[:, None]),
         'grad_alpha_data': 0.5 * (hA @ (mc * mc) + np.sum(zc * zc * R0A[:, None] + 2 * az * R1A, axis=0))}
    if points:
        A['grad_x_mu'] = am + np.abs(o) + alpha * (am * hA[:, None] + HZA)
        A['grad_x_s'] = np.zeros((N, zc.shape[1]))
    tau = (M + D + 1 + C_FIN) * U
    # ---- the values
    if mirror:
        G = np.zeros((N, M))
        for k in range(M + D):
            t = KY[:, k:k + 1] * Bm[k]
            if drop is not None and k == drop[2]:
                t[drop[0], drop[1]] = 0.0
            if drop_y is not None and k == M + drop_y[2]:
                t[drop_y[0], drop_y[1]] = 0.0
            G = G + t
        W = G * K
        R0 = _asc(W)
        R1 = np.stack([_asc(W * mc[:, q:q + 1]) for q in range(mc.shape[1])], axis=1)
        h = np.cumsum(W, axis=1)[:, -1]
        hm2 = np.stack([_asc(h * (mc[:, q] * mc[:, q])) for q in range(mc.shape[1])])
        zz = zc * zc
        ga = -0.5 * (hm2 + _asc(zz * R0[:, None] - (2.0 * zc) * R1))
        gz = alpha * (R1 - zc * R0[:, None])
        if points:
            HZ = np.stack([np.cumsum(W * zc[:, q], axis=1)[:, -1] for q in range(zc.shape[1])], axis=1)
            gmu = -(mc + o) - alpha * (mc * h[:, None] - HZ)
    else:
        Kl, zl, ml, al = (np.asarray(x, dtype=LD) for x in (K, zc, mc, alpha))
        G = np.empty((N, M), dtype=LD)
        Bl = np.asarray(Bm, dtype=LD)
        for i in range(0, N, 4096):
            G[i:i + 4096] = np.asarray(KY[i:i + 4096], dtype=LD) @ Bl
        W = G * Kl
        R0, R1, h = W.sum(axis=0), W.T @ ml, W.sum(axis=1)
        gz = al * (R1 - zl * R0[:, None])
        ga = -(h @ (ml * ml) + np.sum(zl * zl * R0[:, None] - 2 * zl * R1, axis=0)) / 2
        if points:
            gmu = -(ml + np.asarray(o, dtype=LD)) - al * (ml * h[:, None] - W @ zl)
    out = {'grad_z_data': (gz, A['grad_z_data'], tau * A['grad_z_data']), 'grad_alpha_data': (ga, A['grad_alpha_data'], tau * A['grad_alpha_data'])}
    if points:
        out['grad_x_mu'] = (gmu, A['grad_x_mu'], tau * A['grad_x_mu'])
        out['grad_x_s'] = (np.zeros((N, zc.shape[1]), dtype=gmu.dtype), A['grad_x_s'], A['grad_x_s'])
    return out


def input_error_terms(K, eK, Y, Bbar, Abar, zc, mc, ez, em, alpha, points=True):
    """{array: the first-order effect of input perturbations |dK| <= eK (N, M), |dzc| <= ez (M, Q), |dmc| <= em (N, Q)}, to be added to T.  For the
    case at a shifted origin, held against the reference of the UN-shifted inputs: the shifted coordinates are rounded to float64 at magnitude 2^10,
    ez = u |z + c| and em = u |mu + c| (the subtraction of the origin is then exact, and a common error of the origin cancels: every output depends on
    mu - z alone), and eK is compat_ref's first-order bound of Psi1 with origin = -c plus the rounding of the reference's Psi1 to float64.  Each
    output is a polynomial in K, zc and mc; the terms below are |d output / d input| times the input's error, with the expanded magnitudes of A:
      G = K 2Bbar + Y Abar^T: eG = eK |2 Bbar|;   W = G o K: eW = eG K + |G| eK;   a sum_n W f(mu, z): sum eW |f| + sum |W| |f'| (em + ez)."""
    K, eK, Y, zc, mc, ez, em = (np.asarray(x, dtype=np.float64) for x in (K, eK, Y, zc, mc, ez, em))
    M = K.shape[1]
    aK, aY, aBm = np.abs(K), np.abs(Y), np.abs(np.concatenate([2.0 * Bbar, Abar.T], axis=0))
    GA = np.concatenate([aK, aY], axis=1) @ aBm
    eW, WA = (eK @ aBm[:M]) * aK + GA * eK, GA * aK
    az, am = np.abs(zc), np.abs(mc)
    e0, eh, R0A, hA = eW.sum(axis=0), eW.sum(axis=1), WA.sum(axis=0), WA.sum(axis=1)
    out = {'psi2_sum': eK.T @ aK + aK.T @ eK, 'psi1ty': eK.T @ aY,
           'grad_z_data': alpha * (eW.T @ am + az * e0[:, None] + WA.T @ em + ez * R0A[:, None]),
           'grad_alpha_data': 0.5 * (eh @ (am * am) + 2 * np.sum(az * (eW.T @ am), axis=0) + np.sum(az * az * e0[:, None], axis=0))
           + (hA @ (am * em) + np.sum(ez * (WA.T @ am), axis=0) + np.sum(az * (WA.T @ em), axis=0) + np.sum(az * ez * R0A[:, None], axis=0))}
    if points:
        out['grad_x_mu'] = em + alpha * (eh[:, None] * am + eW @ az + hA[:, None] * em + WA @ ez)
    return out


def hold(what, got, ref, shape, factor=2.0, tag='fixed elementwise'):
    """Every array of ``got`` against the bound: prints the worst error / bound per array and returns the failures as strings."""
    N, D, M, Q = shape
    bad = []
    for k in got:
        v, A, T = ref[k]
        dev, v = np.asarray(got[k], dtype=np.float64), np.asarray(v)
        ratio, idx = R.worst(dev, v, A, T, n_terms(k, N, D, M, Q), factor)
        print('[%s] %-30s %-16s worst error / bound %.3g at %s' % (tag, what, k, ratio, idx))
        if not ratio <= 1.0:
            bad.append('%s: %.3g times the bound at %s (got %r, reference %r)' % (k, ratio, idx, float(dev[idx]), float(v[idx])))
    return bad


# --------------------------------------------------------------------------------------------------------- the launches a shape takes
def _pack_slices(nF, SF, nG, SG):
    fill = [0] * 8
    for n, S in ((nF, SF), (nG, SG)):
        for _ in range(S):
            ok = [x for x in range(8) if fill[x] + n <= 64]
            if not ok:
                return False
            fill[min(ok, key=lambda x: (fill[x], x))] += n
    return True


def p2_rem_plan(ntiles, S, MT, nc, mode=1):
    """p2_rem.hip's plan: None, or (q, r, splits, RG)"""
    if not mode or S <= 0 or nc <= 0:
        return None
    q, r = divmod(ntiles, S)
    if q == 0 or r == 0 or r * MT > 512 or (mode == 1 and r * 16 > S):
        return None
    rg = 1
    while rg < 8 and 2 * rg * r * MT <= 256:
        rg *= 2
    return q, r, max(1, min(512 // (r * MT), nc)), rg


def family(N, D, M, Q, emb, p2_rem=1, p2_sync=True):
    """What run_phase1 / run_phase1_v2 (csrc/psi.hip, p1v2.hip) and run_phase2 / p2_rem_plan (psi.hip, p2_rem.hip) launch for a fixed-embedding
    shard: a dict of p1 ('p1v2' | 'tiles'), NBY, cap, SF, SG (p1v2 only); p2 ('fast8' | 'gen8_fixed' | 'gen8_points'), NRB (fast8 only), slices,
    S, tps, rem (None or (q, r)), wait."""
    Mp, Np = (M + 127) // 128 * 128, (N + 127) // 128 * 128
    MT, chunks, ntiles = Mp // 128, Np // 16, Np // 128
    f = dict(MT=MT)
    if D <= 104 and MT <= 11:                                           # p1v2_applicable
        nby = 8 if D <= 32 else 26
        nF, nG = MT * (MT - 1) // 2, MT
        wF, wG = 256, 144 + 8 * nby
        cap = 256 if (nF + nG) * chunks < 24 * 512 else 512
        SF = SG = 0
        for sg in range(min(min(cap // max(nG, 1), chunks), 2 * cap // (2 * nG + nF)), 0, -1):
            sf = min(max(1, int(sg * wF / wG + 0.5)), chunks) if nF > 0 else 0
            if nF * sf + nG * sg > cap:
                continue
            if _pack_slices(nF, sf, nG, sg):
                SF, SG = sf, sg
                break
        assert SG > 0
        f.update(p1='p1v2', NBY=nby, cap=cap, SF=SF, SG=SG)
    else:
        f.update(p1='tiles')
    fast, wide = (not emb) and Q + 1 <= 12, (not emb) and Q + 1 > 12
    f['p2'] = 'fast8' if fast else 'gen8_fixed' if wide else 'gen8_points'
    slices = max(1, min(8 * max(1, 64 // MT), ntiles))                 # P2State::alloc
    S0 = max(1, min(slices, ntiles))
    tps = (ntiles + S0 - 1) // S0
    S = (ntiles + tps - 1) // tps
    nc = (Mp + (D + 15) // 16 * 16) // 16
    rem = p2_rem_plan(ntiles, S0, MT, nc, p2_rem) if fast else None
    if rem:
        S, tps = S0, rem[0]
    blocks = 8 * ((S + 7) // 8) * MT
    f.update(slices=slices, S=S, tps=tps, rem=(rem[0], rem[1]) if rem else None, wait=bool(fast and p2_sync and MT > 1 and blocks <= 512),
             klast=((D - 1) % 16) // 4 + 1)
    if fast:
        f['NRB'] = (Q + 4) // 4
    return f


def identity(f):
    """the whole launch identity of a family() dict as one string: what LISTED holds per case"""
    p1 = '%s/%d cap%d SF%d SG%d' % (f['p1'], f['NBY'], f['cap'], f['SF'], f['SG']) if f['p1'] == 'p1v2' else f['p1']
    return 'MT%d klast%d %s %s%s S%d tps%d rem%s wait%d' % (f['MT'], f['klast'], p1, f['p2'], '/%d' % f['NRB'] if 'NRB' in f else '', f['S'], f['tps'],
                                                           '%d+%d' % f['rem'] if f['rem'] else '-', f['wait'])


# --------------------------------------------------------------------------------------------------------- the cases
# (name, N, D, M, Q, emb, what the case is listed for: the entries of family() it must land on).  The smallest shapes that reach each launch shape.
def _case(N, D, M, Q, emb=False, tag='', **fam):
    return ('n%d_d%d_m%d_q%d%s%s' % (N, D, M, Q, '_emb' if emb else '', tag), N, D, M, Q, emb, fam)


CASES = (
    # phase 1: p1v2_kernel<8> (D = 1, 5, 32; D = 4, 16, 17 for phase 2's last-chunk columns), <26> (33; 100: four padded columns in the last group; 104: its limit)
    [_case(129, d, 5, 3, p1='p1v2', NBY=8, klast=k) for d, k in ((1, 1), (4, 1), (5, 2), (16, 4), (17, 1), (32, 4))]
    + [_case(129, d, 5, 3, p1='p1v2', NBY=26, klast=k) for d, k in ((33, 1), (100, 1), (104, 2))]
    # the fall-back p1_kernel8 + p1_reduce_kernel + p1_scalars_kernel: D = 105, and MT = 12
    + [_case(129, 105, 5, 3, p1='tiles'), _case(150, 2, 1409, 2, p1='tiles', MT=12)]
    # row tiles: MT = 1 (M = 1, 5, 127, 128), 2 (one off-diagonal job), 3 (three), 11 (the planner's packing near its cap); phase 2: wait off / on
    + [_case(200, 2, m, 3, p1='p1v2', MT=1, wait=False) for m in (1, 127, 128)]
    + [_case(200, 2, 129, 3, p1='p1v2', MT=2, wait=True), _case(200, 2, 257, 3, p1='p1v2', MT=3, wait=True),
       _case(200, 2, 385, 7, p1='p1v2', MT=4, wait=True, NRB=2), _case(200, 2, 1281, 2, p1='p1v2', MT=11, cap=256, SF=4, SG=3)]
    # N edges (S = 1 .. 2 slices, not a multiple of 8: the blocks past the last slice zero their hgpart rows)
    + [_case(n, 2, 5, 3, p1='p1v2', S=s) for n, s in ((1, 1), (15, 1), (16, 1), (17, 1), (129, 2))]
    # slice boundaries at different k chunks for the F and G jobs: 128 chunks on SF = 97 and SG = 79 slices
    + [_case(2000, 2, 129, 3, p1='p1v2', cap=256, SF=97, SG=79)]
    # the 512-slot plan (12296 chunks on one G job per slice), tps = 3 and the remainder path at MT = 1 with r = 1
    + [_case(196609, 2, 5, 3, p1='p1v2', cap=512, SG=512, S=512, tps=3, rem=(3, 1))]
    # the remainder path at MT = 2, N not a multiple of 128
    + [_case(33074, 2, 129, 3, p1='p1v2', MT=2, S=256, tps=1, rem=(1, 3), wait=True)]
    # p2_fast8_kernel<1, 2, 3>
    + [_case(200, 2, 5, q, p2='fast8', NRB=nrb) for q, nrb in ((1, 1), (4, 2), (7, 2), (8, 3), (11, 3))]
    # p2_gen8_kernel<false> on [mu | 1 | mu^2]
    + [_case(150, 2, 5, q, p2='gen8_fixed') for q in (12, 16, 17, 30, 63, 64)]
    # ... and its last-chunk Y columns (p2_gen8_kernel skips the k-steps past klast; p2_fast8_kernel does not)
    + [_case(150, d, 5, 12, p2='gen8_fixed', klast=k) for d, k in ((5, 2), (16, 4), (17, 1), (100, 1))]
    + [_case(150, d, 5, 3, True, p2='gen8_points', klast=k) for d, k in ((5, 2), (12, 3), (100, 1))]
    # p2_gen8_kernel<true> + point_kernel on a fixed-embedding shard
    + [_case(150, 2, m, q, True, p2='gen8_points', MT=mt) for m, mt in ((5, 1), (129, 2)) for q in (3, 10, 20)]
    # edges: the far field (K = 0 exactly), columns of Y of very different scale, a common offset of 2^10 on (X, Z)
    + [_case(140, 3, 5, 3, True, '_far', p2='gen8_points'), _case(140, 3, 5, 3, False, '_far', p2='fast8'),
       _case(200, 8, 129, 3, False, '_yscale', wait=True), _case(200, 8, 5, 3, True, '_yscale'),
       _case(200, 2, 129, 3, False, '_shift', wait=True), _case(200, 2, 5, 3, True, '_shift')]
)
CASE_NAMES = [c[0] for c in CASES]
WAIT_CASES = [c for c in CASES if c[6].get('wait')]                    # once more free-running, GPARML_P2_SYNC=0, in one child process
REM_CASE = CASES[CASE_NAMES.index('n33074_d2_m129_q3')]                # at every value of gp_debug_set_option('p2_rem', .): 0, 1, 2
REM_LONG = _case(1023 * 128, 2, 5, 3, tag='_rem2', rem=(1, 511), S=512, tps=1)      # r = S - 1: only under p2_rem = 2 (the hard limits alone)
REDUCED_N = {'n196609_d2_m5_q3': 20001, 'n33074_d2_m129_q3': 3001, 'n130944_d2_m5_q3_rem2': 20001}     # the CPU mirror's N for the long cases
# The whole launch identity of every case in its default mode (REM_LONG: under p2_rem = 2), written out: a case that moves to another plan or kernel
# after a later planner change fails on this line, whatever entries its _case names.
LISTED = {
    'n129_d1_m5_q3': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 fast8/1 S2 tps1 rem- wait0',
    'n129_d4_m5_q3': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 fast8/1 S2 tps1 rem- wait0',
    'n129_d5_m5_q3': 'MT1 klast2 p1v2/8 cap256 SF0 SG16 fast8/1 S2 tps1 rem- wait0',
    'n129_d16_m5_q3': 'MT1 klast4 p1v2/8 cap256 SF0 SG16 fast8/1 S2 tps1 rem- wait0',
    'n129_d17_m5_q3': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 fast8/1 S2 tps1 rem- wait0',
    'n129_d32_m5_q3': 'MT1 klast4 p1v2/8 cap256 SF0 SG16 fast8/1 S2 tps1 rem- wait0',
    'n129_d33_m5_q3': 'MT1 klast1 p1v2/26 cap256 SF0 SG16 fast8/1 S2 tps1 rem- wait0',
    'n129_d100_m5_q3': 'MT1 klast1 p1v2/26 cap256 SF0 SG16 fast8/1 S2 tps1 rem- wait0',
    'n129_d104_m5_q3': 'MT1 klast2 p1v2/26 cap256 SF0 SG16 fast8/1 S2 tps1 rem- wait0',
    'n129_d105_m5_q3': 'MT1 klast3 tiles fast8/1 S2 tps1 rem- wait0',
    'n150_d2_m1409_q2': 'MT12 klast1 tiles fast8/1 S2 tps1 rem- wait1',
    'n200_d2_m1_q3': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 fast8/1 S2 tps1 rem- wait0',
    'n200_d2_m127_q3': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 fast8/1 S2 tps1 rem- wait0',
    'n200_d2_m128_q3': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 fast8/1 S2 tps1 rem- wait0',
    'n200_d2_m129_q3': 'MT2 klast1 p1v2/8 cap256 SF16 SG16 fast8/1 S2 tps1 rem- wait1',
    'n200_d2_m257_q3': 'MT3 klast1 p1v2/8 cap256 SF16 SG16 fast8/1 S2 tps1 rem- wait1',
    'n200_d2_m385_q7': 'MT4 klast1 p1v2/8 cap256 SF16 SG16 fast8/2 S2 tps1 rem- wait1',
    'n200_d2_m1281_q2': 'MT11 klast1 p1v2/8 cap256 SF4 SG3 fast8/1 S2 tps1 rem- wait1',
    'n1_d2_m5_q3': 'MT1 klast1 p1v2/8 cap256 SF0 SG8 fast8/1 S1 tps1 rem- wait0',
    'n15_d2_m5_q3': 'MT1 klast1 p1v2/8 cap256 SF0 SG8 fast8/1 S1 tps1 rem- wait0',
    'n16_d2_m5_q3': 'MT1 klast1 p1v2/8 cap256 SF0 SG8 fast8/1 S1 tps1 rem- wait0',
    'n17_d2_m5_q3': 'MT1 klast1 p1v2/8 cap256 SF0 SG8 fast8/1 S1 tps1 rem- wait0',
    'n129_d2_m5_q3': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 fast8/1 S2 tps1 rem- wait0',
    'n2000_d2_m129_q3': 'MT2 klast1 p1v2/8 cap256 SF97 SG79 fast8/1 S16 tps1 rem- wait1',
    'n196609_d2_m5_q3': 'MT1 klast1 p1v2/8 cap512 SF0 SG512 fast8/1 S512 tps3 rem3+1 wait0',
    'n33074_d2_m129_q3': 'MT2 klast1 p1v2/8 cap256 SF97 SG79 fast8/1 S256 tps1 rem1+3 wait1',
    'n200_d2_m5_q1': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 fast8/1 S2 tps1 rem- wait0',
    'n200_d2_m5_q4': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 fast8/2 S2 tps1 rem- wait0',
    'n200_d2_m5_q7': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 fast8/2 S2 tps1 rem- wait0',
    'n200_d2_m5_q8': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 fast8/3 S2 tps1 rem- wait0',
    'n200_d2_m5_q11': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 fast8/3 S2 tps1 rem- wait0',
    'n150_d2_m5_q12': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 gen8_fixed S2 tps1 rem- wait0',
    'n150_d2_m5_q16': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 gen8_fixed S2 tps1 rem- wait0',
    'n150_d2_m5_q17': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 gen8_fixed S2 tps1 rem- wait0',
    'n150_d2_m5_q30': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 gen8_fixed S2 tps1 rem- wait0',
    'n150_d2_m5_q63': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 gen8_fixed S2 tps1 rem- wait0',
    'n150_d2_m5_q64': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 gen8_fixed S2 tps1 rem- wait0',
    'n150_d5_m5_q12': 'MT1 klast2 p1v2/8 cap256 SF0 SG16 gen8_fixed S2 tps1 rem- wait0',
    'n150_d16_m5_q12': 'MT1 klast4 p1v2/8 cap256 SF0 SG16 gen8_fixed S2 tps1 rem- wait0',
    'n150_d17_m5_q12': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 gen8_fixed S2 tps1 rem- wait0',
    'n150_d100_m5_q12': 'MT1 klast1 p1v2/26 cap256 SF0 SG16 gen8_fixed S2 tps1 rem- wait0',
    'n150_d5_m5_q3_emb': 'MT1 klast2 p1v2/8 cap256 SF0 SG16 gen8_points S2 tps1 rem- wait0',
    'n150_d12_m5_q3_emb': 'MT1 klast3 p1v2/8 cap256 SF0 SG16 gen8_points S2 tps1 rem- wait0',
    'n150_d100_m5_q3_emb': 'MT1 klast1 p1v2/26 cap256 SF0 SG16 gen8_points S2 tps1 rem- wait0',
    'n150_d2_m5_q3_emb': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 gen8_points S2 tps1 rem- wait0',
    'n150_d2_m5_q10_emb': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 gen8_points S2 tps1 rem- wait0',
    'n150_d2_m5_q20_emb': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 gen8_points S2 tps1 rem- wait0',
    'n150_d2_m129_q3_emb': 'MT2 klast1 p1v2/8 cap256 SF16 SG16 gen8_points S2 tps1 rem- wait0',
    'n150_d2_m129_q10_emb': 'MT2 klast1 p1v2/8 cap256 SF16 SG16 gen8_points S2 tps1 rem- wait0',
    'n150_d2_m129_q20_emb': 'MT2 klast1 p1v2/8 cap256 SF16 SG16 gen8_points S2 tps1 rem- wait0',
    'n140_d3_m5_q3_emb_far': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 gen8_points S2 tps1 rem- wait0',
    'n140_d3_m5_q3_far': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 fast8/1 S2 tps1 rem- wait0',
    'n200_d8_m129_q3_yscale': 'MT2 klast2 p1v2/8 cap256 SF16 SG16 fast8/1 S2 tps1 rem- wait1',
    'n200_d8_m5_q3_emb_yscale': 'MT1 klast2 p1v2/8 cap256 SF0 SG16 gen8_points S2 tps1 rem- wait0',
    'n200_d2_m129_q3_shift': 'MT2 klast1 p1v2/8 cap256 SF16 SG16 fast8/1 S2 tps1 rem- wait1',
    'n200_d2_m5_q3_emb_shift': 'MT1 klast1 p1v2/8 cap256 SF0 SG16 gen8_points S2 tps1 rem- wait0',
    'n130944_d2_m5_q3_rem2': 'MT1 klast1 p1v2/8 cap256 SF0 SG256 fast8/1 S512 tps1 rem1+511 wait0',
}
GRID_H = 0.05
SHIFT = 2.0 ** 10


def case_inputs(case, N=None):
    """The float64 inputs of a case.  The inducing points' first coordinate sits on a jittered grid of spacing h = 0.05 with alpha_0 = 4 / h^2
    (neighbours correlate at exp(-2) at most: K_mm factorises without jitter at every M and Q, tests/test_gpu_p2_remainder.py's Q = 1 construction;
    the other coordinates are standard normal with alpha = 1 / (2 Q)); the latent means are spread over the whole grid, so every column of Psi1 has
    near and far rows.  ``N``: fewer points (the CPU mirror of the long cases)."""
    name, N0, D, M, Q, emb, fam = case
    N = N0 if N is None else N
    rs = np.random.RandomState(dd_ref._seed(name))
    h = GRID_H
    Z = rs.randn(M, Q)
    Z[:, 0] = (np.arange(M) - (M - 1) / 2.0) * h + rs.uniform(-0.1, 0.1, size=M) * h
    alpha = np.full(Q, 0.5 / Q)
    alpha[0] = 4.0 / (h * h)
    X_mu = rs.randn(N, Q)
    X_mu[:, 0] = rs.uniform(-(M / 2.0 + 1) * h, (M / 2.0 + 1) * h, size=N)
    Y = rs.randn(N, D)
    if name.endswith('_far'):
        X_mu[:, 0] += 1e3 / np.sqrt(alpha[0]) + M * h                   # 1e3 length scales from every inducing point: exp(-5e5) = 0
    if name.endswith('_yscale'):
        Y = Y * np.geomspace(0.01, 30.0, D)[None, :]
    extra = {}
    if name.endswith('_shift'):
        extra = dict(Z0=Z, X0=X_mu)                                     # the un-shifted inputs: the reference's
        Z, X_mu = Z + SHIFT, X_mu + SHIFT
    return dict(extra, N=N, D=D, M=M, Q=Q, emb=emb, family=fam, Z=Z, sf2=1.3, alpha=alpha, beta=10.0, X_mu=X_mu, X_S=np.zeros((N, Q)), Y=Y,
                name=name if N == N0 else '%s_at_n%d' % (name, N))


def host_psi1(d):
    """Psi1 of a case in float64 on the host (the CPU tests' stand-in for the device's array)"""
    zc, mc, _ = centred(d['Z'], d['X_mu'])
    e = np.zeros((d['N'], d['M']))
    for q in range(d['Q']):
        df = mc[:, q:q + 1] - zc[None, :, q]
        e += d['alpha'][q] * df * df
    return d['sf2'] * np.exp(-0.5 * e)


def synthetic_partials(d):
    """A symmetric Bbar and an Abar for the CPU tests (seeded; any float64 values serve as exact inputs)."""
    rs = np.random.RandomState(len(d['name']) + d['M'])
    B = rs.randn(d['M'], d['M'])
    return (B + B.T) / 2, rs.randn(d['M'], d['D'])
