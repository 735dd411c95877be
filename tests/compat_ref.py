"""Long-double reference of Psi1 and of the reference-shaped arrays (csrc/compat.hip), with an elementwise error bound.

What is computed.  The formulas of the reference's partial_terms.py:45-52, 146-205, 247-299 as oracle/literal.py restates them, in the reference's
layouts, in whatever floating-point type the inputs come in: numpy long double (x86 80-bit, eps 1.08e-19) for the reference, float64 for the
"mirror" (float64 inputs: every sum over the points in ascending order, one addition per point, as the kernels do).  Sums over n are taken point
by point, so the (N, M, M, Q) intermediate never exists.  Every function returns ``(value, A)``; with ``err=True`` it returns ``(value, A, T)``:

    value  the array
    A      the absolute sums: each output element is sum_n t_n (one term for Psi1, Kmm, the per-point psi2 and the two Kmm tensors), A = sum_n |t_n|
    T      sum_n tau_n |t_n| written out term by term (below): the first-order error of the terms themselves, before they are added

The bound.  With u = 2^-53 a float64 evaluation of the same formula may differ from the exact value by at most

    |dev - ref| <= 2 (T + n_terms u A) + floor,      T = tau A with tau the |t_n|-weighted mean of the per-term tau_n          (``bound``)

where n_terms is the length of the sum (n_terms u A: each of the n_terms additions rounds a partial sum that is at most A), floor = 2^-1022 (an
element that is zero or subnormal on either side is accepted against a zero or subnormal reference: gradual underflow rounds absolutely, not
relatively) and the factor 2 covers everything of second order.  The float64 mirror must hold it WITHOUT the factor 2 (test_compat_ref_cpu.py).

tau_n, derived.  Every term is a product of exponentials and rational factors of the inputs.
  * An exponential exp(e), e = l - 1/2 sum_q w_q d_q^2: an absolute error de of the argument is a relative error de of the value.  The argument is
    a sum of same-signed parts formed in float64, so de <= u (|e| + c): u |e| for the roundings that scale with the argument (|e| is taken as
    the sum of the magnitudes of its parts, |l| + 1/2 sum w d^2), and c for the roundings that do not: 2 Q + 8 for the Q fused multiply-adds
    of the exponent with the product in front of each, the scale factors and the logarithm's Q terms, plus 4 for exp itself (csrc/fexp.h: 1.7e-16
    relative for fexp, 3.3e-16 for the table form).  C_EXP = 2 Q + 12.
  * The chain of the exponent.  The Q fused multiply-adds each round a partial sum of the quadratic form, which is as large as the whole form
    as soon as one latent dimension dominates: Q u (1/2 sum w d^2) more, so u ((1 + Q) |e| + c) in all.  (Found on the device, not assumed: with
    the chain counted in c only, Psi1 at Q = 24, 52 and 65 with one steep dimension was 1.04 to 1.09 bounds off at |e| = 285 to 671 -- 11 u |e| --
    and an emulation of the kernel's arithmetic in numpy gave the device's bits: honest rounding, 23 additions onto a partial sum of 570.)
    The per-point psi2 has that chain three times: in each of its two LE entries and over the pair term on their sum.
  * The coordinate differences.  The library forms d = (mu - o) - (z - o) on coordinates centred at an origin o (the column mean of Z): the two
    centred values carry u |mu - o| and u |z - o| and the subtraction rounds once more, so d carries dd = u (|mu - o| + |z - o| + |d|) absolutely:
    three roundings, the first two whatever |d| is.  Through w d^2 / 2 that is w |d| dd in the argument; through the pair term V dz^2
    (V = -(alpha - w) / 4) it is 2 |V| |dz| u (|z - o| + |z' - o| + |dz|).  (The last part grows with the argument like u |e| does: for one
    dominant latent dimension it is 2 u |e|.  Left out, the float64 mirror exceeded the bound at |e| > 16 -- 4.1 u |e| at |e| = 65, Q = 2.)
    A rational factor that is linear in a difference (the derivative tensors) gets the same absolute error times its coefficient -- it is added
    to T as an ABSOLUTE error, because the factor itself may be zero (z_m = z_m').  ``origin`` replaces o: for inputs that were shifted by a
    constant before they were rounded to float64 (the translation test) the shifted magnitudes |mu + c|, |z + c| stand there, origin = -c.
  * The per-point psi2 has two such exponents (LE[n, m] + LE[n, m'], csrc/psi2.hip) and the pair term on DZ2 = fl(dz^2) (two roundings per entry,
    then one multiply-add): c = 2 (2 Q + 8) + 3 Q + 4, rounded up to C_PSI2 = 7 Q + 22 so that it also covers fixed embeddings, where the element is
    the rounded product of two Psi1 entries (2 C_EXP + 1).  All parts of its argument have one sign, so |e| is again the sum of the magnitudes.
  * The remaining factors of a term (alpha, 1 / (alpha S + 1), the squares, Y) cost one rounding each: the small constants next to tau below.
    In dpsi2_dz the factor is a sum of two parts that may cancel, f = f1 + f2; its roundings are relative to |f1| + |f2| and enter T that way.
  * The parts contractions (gp_grad_from_parts) multiply given float64 arrays: tau = 3 u (grad_Z: the symmetrised sum, the product, the factor)
    and 2 u (grad_alpha), n_terms = 2 M + D and 2 M^2 + M D.

This is a first-order bound with counted coefficients.  What makes it honest is the pair of tests around it: the float64 mirror shows that it is not too tight (ratio below 1 without the factor 2), and the measured
ratios that it is not vacuous (a wrong element is off by O(1), i.e. by 1e13 bounds)."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
FLOOR = 2.0 ** -1022

ARRAYS = ('psi1', 'kmm', 'psi2_points', 'dkmm_dz', 'dkmm_dalpha', 'dpsi1ty_dz', 'dpsi1ty_dalpha', 'dpsi2_dz', 'dpsi2_dalpha')
# gp_download's name of each array and the length of its sum
DEVICE_NAME = dict(psi1='PSI1', kmm='KMM', psi2_points='PSI2_POINTS', dkmm_dz='DKMM_DZ', dkmm_dalpha='DKMM_DALPHA', dpsi1ty_dz='DPSI1TY_DZ',
                   dpsi1ty_dalpha='DPSI1TY_DALPHA', dpsi2_dz='DPSI2_DZ', dpsi2_dalpha='DPSI2_DALPHA')
SUMMED = ('dpsi1ty_dz', 'dpsi1ty_dalpha', 'dpsi2_dz', 'dpsi2_dalpha')


def available():
    """True when numpy's long double has at least the 64-bit significand of the x86 extended format (its users skip otherwise)."""
    return np.finfo(LD).nmant >= 63


def to_ld(*arrays):
    return tuple(None if a is None else np.asarray(a, dtype=LD) for a in arrays)


def n_terms(name, N):
    return N if name in SUMMED else 1


def bound(A, T, nterms, factor=2.0):
    return factor * (np.asarray(T, dtype=LD) + LD(nterms) * LD(U) * np.asarray(A, dtype=LD)) + LD(FLOOR)


def worst(dev, ref, A, T, nterms, factor=2.0):
    """(ratio, index) of the element of ``dev`` that is worst against the bound; a NaN anywhere gives ratio inf at its index."""
    dev = np.asarray(dev)
    assert dev.shape == np.shape(ref), 'shape %s vs %s' % (dev.shape, np.shape(ref))
    r = np.abs(np.asarray(dev, dtype=LD) - ref) / bound(A, T, nterms, factor)
    r = np.where(np.isfinite(r), r, np.inf)
    i = int(np.argmax(r))
    return float(r.reshape(-1)[i]), tuple(int(k) for k in np.unravel_index(i, r.shape))


# --------------------------------------------------------------------------------------------------------- pieces
class _Pieces(object):
    """Everything the formulas share, in the type of the inputs.  ``full``: also the error terms tau (without it only the values are formed)."""

    def __init__(self, Z, sf2, alpha, mu, S, origin, full):
        self.full = full
        self.dt = dt = np.asarray(Z).dtype.type
        self.Z, self.alpha = np.asarray(Z), np.asarray(alpha).reshape(-1)
        self.sf2 = dt(sf2)
        self.M, self.Q = self.Z.shape
        self.u = dt(U)
        o = np.mean(self.Z, axis=0) if origin is None else np.asarray(origin, dtype=self.Z.dtype).reshape(-1)
        self.cz = np.abs(self.Z - o)                                    # (M, Q)
        self.c_exp = dt(2 * self.Q + 12)
        self.c_psi2 = dt(7 * self.Q + 22)
        self.dz = self.Z[:, None, :] - self.Z[None, :, :]               # (M, M, Q)
        self.czz = self.cz[:, None, :] + self.cz[None, :, :] + np.abs(self.dz)      # (M, M, Q): |z - o| + |z' - o| + |dz|, the three roundings of dz
        if mu is not None:
            self.mu, self.S = np.asarray(mu), np.asarray(S)
            self.N = self.mu.shape[0]
            assert self.mu.shape == self.S.shape == (self.N, self.Q) and np.all(self.S >= 0) and np.all(self.alpha >= 0)
            self.cm = np.abs(self.mu - o)                               # (N, Q)
            self.d1 = self.alpha * self.S + 1                           # (N, Q)
            self.d2 = 2 * self.alpha * self.S + 1
            self.c1 = self.sf2 / np.sqrt(self.d1).prod(axis=1)          # kernel_exp.py:80
            self.c2 = self.sf2 * self.sf2 / np.sqrt(np.prod(self.d2, axis=1))       # kernel_exp.py:143
            self.lnc1 = np.abs(np.log(self.sf2)) + np.sum(np.log(self.d1), axis=1) / 2      # magnitudes of the parts of ln c1, ln c2
            self.lnc2 = 2 * np.abs(np.log(self.sf2)) + np.sum(np.log(self.d2), axis=1) / 2

    def psi1_rows(self, sl):
        """Psi1 of the points ``sl`` (a slice): value (n, M), tau (n, M), d = mu - z (n, M, Q)."""
        a = self.alpha
        d = self.mu[sl, None, :] - self.Z[None, :, :]
        u1 = (a / self.d1[sl])[:, None, :]
        quad = np.sum(d * d * u1, axis=2)
        val = self.c1[sl, None] * np.exp(-quad / 2)
        if not self.full:
            return val, None, d
        coord = np.sum(u1 * np.abs(d) * (self.cm[sl, None, :] + self.cz[None, :, :] + np.abs(d)), axis=2)
        tau = self.u * (self.lnc1[sl, None] + (1 + self.Q) * quad / 2 + self.c_exp + coord)
        return val, tau, d

    def kmm(self):
        e = np.sum(self.alpha * self.dz * self.dz, axis=2) / 2
        val = self.sf2 * np.exp(-e)
        if not self.full:
            return val, None
        coord = np.sum(self.alpha * np.abs(self.dz) * self.czz, axis=2)
        return val, self.u * ((1 + self.Q) * e + self.c_exp + coord)

    def psi2_point(self, n, d_n):
        """psi2 of point n from its differences d_n (M, Q): value (M, M), tau (M, M).  kernel_exp.py:143-146 in the factorised form
        exponent = lnE_m + lnE_m' - 1/4 sum_q (alpha_q - w_q) dz_q^2, lnE_m = -1/2 sum_q w_q (mu_q - z_mq)^2 (algebraically the same)."""
        a = self.alpha
        w = a / self.d2[n]
        lnE = np.sum(w * d_n * d_n, axis=1) / 2                          # (M,) magnitudes
        coup = np.sum((a - w) * self.dz * self.dz, axis=2) / 4          # (M, M)
        val = self.c2[n] * np.exp(-(lnE[:, None] + lnE[None, :] + coup))
        if not self.full:
            return val, None
        cd = np.sum(w * np.abs(d_n) * (self.cm[n] + self.cz + np.abs(d_n)), axis=1)   # (M,)
        cc = np.sum((a - w) * np.abs(self.dz) * self.czz, axis=2) / 2
        E = self.lnc2[n] + lnE[:, None] + lnE[None, :] + coup
        tau = self.u * ((1 + self.Q) * E + self.Q * (lnE[:, None] + lnE[None, :]) + self.c_psi2 + cd[:, None] + cd[None, :] + cc)
        return val, tau


class _Sum(object):
    """(value, A, T) of a sum over the points, added point by point in ascending order -- one rounding per point, which is what the float64
    mirror is asked to do and harmless in long double."""

    def __init__(self):
        self.v = [None, None, None]

    def add(self, *terms):
        for i, t in enumerate(terms):
            self.v[i] = t.copy() if self.v[i] is None else self.v[i] + t


# --------------------------------------------------------------------------------------------------------- the arrays
def _psi1(p, chunk=64):
    val = np.empty((p.N, p.M), dtype=p.Z.dtype)
    T = np.empty((p.N, p.M), dtype=p.Z.dtype) if p.full else None
    for i in range(0, p.N, chunk):
        sl = slice(i, min(p.N, i + chunk))
        v, tau, _ = p.psi1_rows(sl)
        val[sl] = v
        if p.full:
            T[sl] = tau * v
    return val, val, T


def _kmm(p):
    val, tau = p.kmm()
    return val, val, tau * val if p.full else None


def _psi2_points(p):
    val = np.empty((p.N, p.M, p.M), dtype=p.Z.dtype)
    T = np.empty((p.N, p.M, p.M), dtype=p.Z.dtype) if p.full else None
    for n in range(p.N):
        v, tau = p.psi2_point(n, p.mu[n] - p.Z)
        val[n] = v
        if p.full:
            T[n] = tau * v
    return val, val, T


def _dkmm_dz(p):
    K, tau = p.kmm()
    dz = np.transpose(p.dz, (0, 2, 1))                                  # (M, Q, M')
    val = K[:, None, :] * (-p.alpha)[None, :, None] * dz
    if not p.full:
        return val, None, None
    A = np.abs(val)
    return val, A, A * (tau[:, None, :] + 3 * p.u) + K[:, None, :] * p.alpha[None, :, None] * p.u * np.transpose(p.czz, (0, 2, 1))


def _dkmm_dalpha(p):
    K, tau = p.kmm()
    dz = np.transpose(p.dz, (2, 0, 1))                                  # (Q, M, M')
    val = -K[None, :, :] * dz * dz / 2
    if not p.full:
        return val, None, None
    A = np.abs(val)
    return val, A, A * (tau[None, :, :] + 3 * p.u) + K[None, :, :] * np.abs(dz) * p.u * np.transpose(p.czz, (2, 0, 1))


def _psi1_sums(p, Y, want):
    """dexp_K_miY_dZ (M, Q, D) and dexp_K_miY_dalpha (Q, M, D), partial_terms.py:162-188, 256-271, one point at a time."""
    Y = np.asarray(Y)
    out = {k: _Sum() for k in want}
    a, u = p.alpha, p.u
    for n in range(p.N):
        v, tau, d = p.psi1_rows(slice(n, n + 1))
        v, d = v[0][:, None], d[0]                                      # (M, 1), (M, Q)
        y = Y[n]
        if p.full:
            tau, ay = tau[0][:, None], np.abs(Y[n])
            cc = p.cm[n] + p.cz + np.abs(d)                             # (M, Q)
        if 'dpsi1ty_dz' in want:
            g = a * d / p.d1[n]                                         # (M, Q)
            w = v * g
            if p.full:
                e = v * (np.abs(g) * (tau + 5 * u) + a / p.d1[n] * u * cc)
                out['dpsi1ty_dz'].add(w[:, :, None] * y, np.abs(w)[:, :, None] * ay, e[:, :, None] * ay)
            else:
                out['dpsi1ty_dz'].add(w[:, :, None] * y)
        if 'dpsi1ty_dalpha' in want:
            r = d / p.d1[n]
            h = r * r + p.S[n] / p.d1[n]                                # (M, Q), both parts >= 0
            w = -(v * h) / 2
            if p.full:
                e = v * (h * (tau + 6 * u) / 2 + np.abs(r) / p.d1[n] * u * cc)
                out['dpsi1ty_dalpha'].add(w.T[:, :, None] * y, np.abs(w).T[:, :, None] * ay, e.T[:, :, None] * ay)
            else:
                out['dpsi1ty_dalpha'].add(w.T[:, :, None] * y)
    return {k: tuple(o.v) for k, o in out.items()}


def _psi2_sums(p, want):
    """dexp_K_mi_K_im_dZ (M, Q, M) and dexp_K_mi_K_im_dalpha (Q, M, M), partial_terms.py:190-205, 273-284, one point at a time."""
    out = {k: _Sum() for k in want}
    a, u = p.alpha, p.u
    dzq = np.transpose(p.dz, (0, 2, 1))                                 # (M, Q, M')
    f1 = -a[None, :, None] * dzq / 2
    dz4 = dzq * dzq / 4
    tr = lambda x: np.transpose(x, (1, 0, 2))
    if p.full:
        czq = np.transpose(p.czz, (0, 2, 1))
        af1, ez, ea = np.abs(f1), a[None, :, None] / 2 * u * czq, np.abs(dzq) / 2 * u * czq
        czs = p.cz[:, :, None] + p.cz.T[None, :, :]
    for n in range(p.N):
        d = p.mu[n] - p.Z                                               # (M, Q)
        v, tau = p.psi2_point(n, d)                                     # (M, M')
        s2 = d[:, :, None] + d.T[None, :, :]                            # 2 mu - z_m - z_m'   (M, Q, M')
        w = (a / p.d2[n])[None, :, None]
        vq = v[:, None, :]
        if p.full:
            tq = tau[:, None, :]
            cs = 2 * p.cm[n][None, :, None] + czs + np.abs(s2)
        if 'dpsi2_dz' in want:
            f2 = w * s2 / 2
            f = f1 + f2
            t = vq * f
            if p.full:
                e = vq * (tq * np.abs(f) + 6 * u * (af1 + np.abs(f2)) + ez + w / 2 * u * cs)
                out['dpsi2_dz'].add(t, np.abs(t), e)
            else:
                out['dpsi2_dz'].add(t)
        if 'dpsi2_dalpha' in want:
            d2 = p.d2[n][None, :, None]
            r = s2 / d2
            f = -dz4 - r * r / 4 - (p.S[n] / p.d2[n])[None, :, None]    # three parts of one sign
            t = vq * f
            if p.full:
                e = vq * ((tq + 8 * u) * np.abs(f) + ea + np.abs(r) / d2 / 2 * u * cs)
                out['dpsi2_dalpha'].add(tr(t), tr(np.abs(t)), tr(e))
            else:
                out['dpsi2_dalpha'].add(tr(t))
    return {k: tuple(o.v) for k, o in out.items()}


def _compute(p, Y, names):
    out = {}
    for k, fn in (('psi1', _psi1), ('kmm', _kmm), ('psi2_points', _psi2_points), ('dkmm_dz', _dkmm_dz), ('dkmm_dalpha', _dkmm_dalpha)):
        if k in names:
            out[k] = fn(p)
    w1 = tuple(k for k in ('dpsi1ty_dz', 'dpsi1ty_dalpha') if k in names)
    w2 = tuple(k for k in ('dpsi2_dz', 'dpsi2_dalpha') if k in names)
    if w1:
        out.update(_psi1_sums(p, Y, w1))
    if w2:
        out.update(_psi2_sums(p, w2))
    return out


def all_arrays(Z, sf2, alpha, mu, S, Y, origin=None, names=ARRAYS):
    """{name: (value, A, T)} of the arrays ``names``; the sums that share a per-point quantity are formed in one pass over the points.  The values
    are formed in the type of the inputs.  A and T bound an error and need no more than float64 themselves: for long-double inputs they come from
    a second pass over the inputs rounded to float64 (a third of the long-double work), where an A or T below the float64 range becomes zero and
    leaves the element to the floor."""
    Z = np.asarray(Z)
    if Z.dtype == np.float64:
        return _compute(_Pieces(Z, sf2, alpha, mu, S, origin, True), Y, names)
    val = _compute(_Pieces(Z, sf2, alpha, mu, S, origin, False), Y, names)
    f64 = lambda x: None if x is None else np.asarray(x, dtype=np.float64)
    err = _compute(_Pieces(f64(Z), float(sf2), f64(alpha), f64(mu), f64(S), f64(origin), True), f64(Y), names)
    return {k: (val[k][0], err[k][1], err[k][2]) for k in val}


def _public(name, doc):
    def f(Z, sf2, alpha, mu=None, S=None, Y=None, origin=None, err=False):
        v, A, T = all_arrays(Z, sf2, alpha, mu, S, Y, origin=origin, names=(name,))[name]
        return (v, A, T) if err else (v, A)
    f.__name__, f.__doc__ = name, doc
    return f


psi1 = _public('psi1', 'exp_K_mi (N, M), partial_terms.py:49 / kernel_exp.py:80.')
kmm = _public('kmm', 'Kmm (M, M), kernels.py:72-113.')
psi2_points = _public('psi2_points', 'exp_K_mi_K_im (N, M, M), partial_terms.py:45-48.')
dkmm_dz = _public('dkmm_dz', "dKmm_dZ (M, Q, M): K[j, m'] (-alpha_k) (z_jk - z_m'k), partial_terms.py:146-160.")
dkmm_dalpha = _public('dkmm_dalpha', "dKmm_dalpha (Q, M, M): -1/2 K[m, m'] (z_mq - z_m'q)^2, partial_terms.py:247-254.")
dpsi1ty_dz = _public('dpsi1ty_dz', 'dexp_K_miY_dZ (M, Q, D), partial_terms.py:162-188.')
dpsi1ty_dalpha = _public('dpsi1ty_dalpha', 'dexp_K_miY_dalpha (Q, M, D), partial_terms.py:256-271.')
dpsi2_dz = _public('dpsi2_dz', 'dexp_K_mi_K_im_dZ (M, Q, M), partial_terms.py:190-205.')
dpsi2_dalpha = _public('dpsi2_dalpha', 'dexp_K_mi_K_im_dalpha (Q, M, M), partial_terms.py:273-284.')


# --------------------------------------------------------------------------------------------------------- parts contractions
def grad_z_from_parts(dF_dKmm, dKmm_dZ, dF_dC, dC_dZ, dF_dPsi2, dPsi2_dZ, err=False):
    """grad_Z (M, Q), partial_terms.py:207-240: for each (j, k) the (M, M) mask with row j AND column j set to dKmm_dZ[j, k, :] -- entry (j, j)
    is written twice and counted once --, the C term, and twice the psi2 term.  n_terms = 2 M + D."""
    A_, a3, B, b3, C, c3 = dF_dKmm, dKmm_dZ, dF_dC, dC_dZ, dF_dPsi2, dPsi2_dZ
    M = A_.shape[0]
    once = np.ones((M, M), dtype=A_.dtype)
    once[np.arange(M), np.arange(M)] = 0                                # the column pass adds nothing on the diagonal
    r = np.transpose(a3, (0, 2, 1))                                     # (j, m, k)
    val = (np.sum(A_[:, :, None] * r, axis=1) + np.sum((A_.T * once)[:, :, None] * r, axis=1)
           + np.sum(B[:, None, :] * b3, axis=2) + 2 * np.sum(C[:, None, :] * c3, axis=2))
    A = (np.sum((np.abs(A_) + np.abs(A_.T) * once)[:, :, None] * np.abs(r), axis=1)
         + np.sum(np.abs(B)[:, None, :] * np.abs(b3), axis=2) + 2 * np.sum(np.abs(C)[:, None, :] * np.abs(c3), axis=2))
    return (val, A, 3 * A_.dtype.type(U) * A) if err else (val, A)


def grad_alpha_from_parts(dF_dKmm, dKmm_dalpha, dF_dC, dC_dalpha, dF_dPsi2, dPsi2_dalpha, err=False):
    """grad_alpha (Q,), partial_terms.py:286-299: three Frobenius products per q.  n_terms = 2 M^2 + M D."""
    val = (np.sum(dF_dKmm[None] * dKmm_dalpha, axis=(1, 2)) + np.sum(dF_dC[None] * dC_dalpha, axis=(1, 2))
           + np.sum(dF_dPsi2[None] * dPsi2_dalpha, axis=(1, 2)))
    A = (np.sum(np.abs(dF_dKmm[None] * dKmm_dalpha), axis=(1, 2)) + np.sum(np.abs(dF_dC[None] * dC_dalpha), axis=(1, 2))
         + np.sum(np.abs(dF_dPsi2[None] * dPsi2_dalpha), axis=(1, 2)))
    return (val, A, 2 * dF_dKmm.dtype.type(U) * A) if err else (val, A)


# --------------------------------------------------------------------------------------------------------- the cases
# (name, N, D, M, Q, regime, alpha): alpha as tests/test_gpu_parity.py chooses it for the latent width (and, where M is large for its Q, for the
# density of the inducing points), so that the global step factorises without jitter
CASES = [
    ('B_q3_two_slabs', 131, 3, 70, 3, 'B', 0.5),          # QB 4, two 64-column slabs, Np 256, the tail group of the interleaved LE
    ('B_q10_Mp256', 129, 5, 130, 10, 'B', 0.3),
    ('B_q16_last_interleaved', 70, 2, 33, 16, 'B', 0.15),
    ('B_q17_first_point_major', 67, 2, 65, 17, 'B', 0.1),  # QB 24, psi1_kernel<24>
    ('B_q31', 60, 2, 40, 31, 'B', 0.08),                  # 32
    ('B_q40_Dp256', 50, 129, 20, 40, 'B', 0.05),          # psi1_wide_kernel<52>
    ('B_q63_spare_column', 45, 2, 12, 63, 'B', 0.05),     # 64
    ('B_q64_generic_psi2', 40, 2, 9, 64, 'B', 0.05),      # lea_rows_kernel + psi1_wide_kernel<64>
    ('B_q70_generic', 40, 2, 9, 70, 'B', 0.05),           # ... + psi1_generic_kernel
    ('A_q2_Mp384', 130, 4, 257, 2, 'A', 30.0),            # WC 2, the fixed-variance form; 257 inducing points in the plane
    ('A_q30', 100, 3, 40, 30, 'A', 0.05),
    ('A_q70', 60, 2, 20, 70, 'A', 0.03),
    ('B_far_field', 64, 1, 16, 2, 'B', 0.5),
]
CASE_NAMES = [c[0] for c in CASES]
FAR_FIELD = 'B_far_field'
FAR_EXPONENT = 780.0


def case_inputs(case):
    """The float64 inputs of a case: oracle.factorised.synthetic_shard, with the inducing points drawn around re-used rows where M > N (as
    test_gpu_parity.test_config4_shape does), and for the far-field case the latent means spread over a line so that the exponent of Psi1 runs from
    0 to below -760: |mu - z| up to r with 1/2 u r^2 = FAR_EXPONENT, u = alpha / (alpha S + 1) >= alpha / 1.55 -- the range follows from alpha and
    the spread of Z."""
    from oracle import factorised as Fz
    name, N, D, M, Q, regime, alpha = case
    seed = 100 + CASE_NAMES.index(name)
    d = Fz.synthetic_shard(N, D, min(M, N), Q, regime=regime, seed=seed, zseed=seed + 50, alpha_value=alpha)
    if M > N:
        rs = np.random.RandomState(seed + 99)
        d['Z'] = d['X_mu'][rs.randint(0, N, size=M)] + 0.3 * rs.randn(M, Q)
    if name == FAR_FIELD:
        rs = np.random.RandomState(seed + 98)
        zspread = float(np.max(np.abs(d['Z'] - d['Z'].mean(axis=0))))
        r = np.sqrt(2.0 * FAR_EXPONENT * 1.55 / alpha) + zspread
        d['X_mu'] = d['X_mu'].copy()
        # distances r sqrt(n / (N - 1)), alternating sides: the exponent is spread evenly over its range, not its square root
        d['X_mu'][:, 0] = d['Z'][:, 0].mean() + r * np.sqrt(np.arange(N) / (N - 1.0)) * np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
        d['X_mu'][:, 1] = d['Z'][:, 1].mean() + 0.1 * rs.randn(N)
    d.update(N=N, D=D, M=M, Q=Q, regime=regime, name=name)
    return d


def inputs_ld(d):
    return to_ld(d['Z'], d['sf2'], d['alpha'], d['X_mu'], d['X_S'], d['Y'])


PSI1_WIDTHS = (1, 2, 4, 6, 8, 10, 12, 14, 16, 24, 32, 52, 64, 65)


def psi1_case_inputs(q, regime, N=300, M=513):
    """Psi1 alone at WC = 4 (Mp >= 512): M = 513 inducing points whose first coordinate sits on a jittered grid of spacing h with alpha_0 = 4 / h^2
    (neighbours correlate at exp(-2) at most, so Kmm factorises at every q, the 513 points of q = 1 included; the other coordinates are standard
    normal with alpha = 1 / q) and latent means spread over the whole grid, so that every column has near and far rows."""
    rs = np.random.RandomState(7000 + 10 * q + (regime == 'B'))
    h = 0.05
    Z = rs.randn(M, q)
    Z[:, 0] = (np.arange(M) - M / 2.0) * h + rs.uniform(-0.1, 0.1, size=M) * h
    alpha = np.full(q, 1.0 / q)
    alpha[0] = 4.0 / (h * h)
    X_mu = rs.randn(N, q)
    X_mu[:, 0] = rs.uniform(-M / 2.0 * h, M / 2.0 * h, size=N)
    X_S = np.zeros((N, q)) if regime == 'A' else rs.uniform(0.05, 0.55, size=(N, q)) / alpha[None, :]
    Y = rs.randn(N, 2)
    return dict(N=N, D=2, M=M, Q=q, regime=regime, Z=Z, sf2=1.0, alpha=alpha, beta=10.0, X_mu=X_mu, X_S=X_S, Y=Y, name='psi1_q%d_%s' % (q, regime))
