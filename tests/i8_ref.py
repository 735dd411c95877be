"""The int8 phase 1 (gparml_amd/csrc/p1i8.hip, with the digit writer inside psi1_kernel, psi1.hip:110-122) restated on the host: its digits, its exact
integer sums, the exact value they stand for, the kernel's own float64 conversion bit for bit, and an elementwise bound on what the device may
return.  tests/test_i8_ref_cpu.py checks this file without a device (the truncation model, the fault table, the plan); tests/test_gpu_p1_i8_exact.py
holds the kernels to it.

INPUTS.  Psi1 (N, M) as the DEVICE generated it (gp_download PSI1 after a phase 1 with the path on: the very float64 values psi1_kernel digitised,
psi1.hip:99-122), Y (N, D) as uploaded, sf2.  Psi1 itself is held by test_gpu_compat_arrays.py; this reference isolates what the int8 path adds.
Nothing else measured on the device enters the value or the bound.

DIGITS (psi1.hip:114-121 for Psi1, p1i8.hip:259-266 for Y).  t = x * hscale with hscale = fl(0.5 / sf2) for Psi1 (psi1.hip:266) and 1 / yscale[d] (a
power of two: exact) for Y; then six rounds of  t <- 128 t,  g = rint(t),  t <- t - g.  The first multiply rounds once (IEEE: numpy rounds the same
way); 128 t is exact, g is an integer below 2^52 and t - g is exact (Sterbenz: |t - g| <= 1/2 and both are multiples of ulp(t)), so numpy float64
reproduces the device's digits bit for bit.  |t| <= 1/2 at the start gives |g| <= 64 in every round: `digits` asserts it.
yscale[d] (p1i8.hip:244-246): m = max |Y[:, d]| = f 2^e with f in [1/2, 1) -> yscale = 2^(e + 1): the unique power of two with 2 m < yscale <= 4 m
(m = 2^k exactly gives f = 1/2, e = k + 1, yscale = 4 m); 1 for a zero column.  The sign of the extreme entry plays no part (fabs, p1i8.hip:232).

INTEGER SUMS.  With d_a the a-th digit plane of Psi1 (N, M) and e_b the b-th of [Psi1 | Y] (N, M + D), a, b = 1 .. 6, the kernel keeps the 21 products
with a + b <= 7 (p1i8.hip:140-146), one int32 accumulator per order o = a + b = 2 .. 7:   I_o[i, j] = sum_n sum_{a + b = o} d_a[n, i] e_b[n, j].
Here they are float64 `@` on the digit planes: |d e| <= 4096, at most 6 pairs per order, so every partial sum is an integer below 6 * 4096 * N, exact
in float64 while 6 * 4096 * N < 2^53 (asserted; N < 3.6e11).  The B planes an A plane meets are stacked side by side: six GEMMs per slice.  Integer
sums do not depend on the split of the rows (test_i8_ref_cpu.py).  The device's accumulators are int32: a slice holds at most 81920 rows
(p1i8.hip:51) plus one k-step of rounding, and 6 * 4096 * 81952 = 2 014 052 352 < 2^31 = 2 147 483 648 even if every digit of every row were +-64 (real
Psi1 digits cannot be: a full first digit leaves |t| <= 1/256 for the rest); p1i8_prepare refuses a plan whose slices exceed 87000 rows
(p1i8.hip:328).  That edge needs N >= 655 360 and is not run on the device.

THE EXACT VALUE, in numpy long double (64-bit significand):
    Psi2[i, j] = 4 sf2^2 sum_o I_o[i, j] 128^-o   (i != j),        C[i, d] = 2 sf2 yscale_d sum_o I_o[i, M + d] 128^-o,
    Psi2[i, i] = sum_n Psi1[n, i]^2   -- the kernel takes the diagonal from psi1_kernel's float64 sums of squares, not from the digits (p1i8.hip:216-220).
I_o < 2^53 converts exactly; the six-term sum, sf2^2 and the two products round eight times at 2^-64, relative to the sum of the absolute terms.  The
diagonal is summed by an explicit pairwise tree (17 levels at N = 2^17, one rounding for each square): at most 18 roundings at 2^-64 of a sum of
positive terms.  Both are carried in the bound below (REF_ROUNDINGS, REF_DIAG_ROUNDINGS) and are 2^-11 of its float64 terms.

WHAT THE DEVICE ROUNDS, and the bound.  u = 2^-53.  The plan (`plan`, restating p1i8_prepare, p1i8.hip:315-356, and the workspace capacity it reads,
api.hip:91-100) gives the number of row slices S; slice s holds the k-steps [floor(s K / S), floor((s + 1) K / S)) of 32 rows, K = Np / 32
(p1i8.hip:343).  Per element:
  1. the conversion of a slice's six accumulators, v_s = fma(I_7 w_7, ... fma(I_2 w_2 ...)) from the small end (p1i8.hip:156-161): the weights are powers
     of two and I_o < 2^31, so every product is exact and the first fma adds to zero: 5 roundings, each at most u times a partial sum of |I_o| w_o;
  2. p1i8_reduce_kernel's eight interleaved sums (slice s goes to sum s mod 8, in order) and their tree (p1i8.hip:202-209): ceil(S / 8) - 1 additions
     on the longest chain (the first adds to zero) and 3 levels of the tree;
  3. the host's 4 * sf2 * sf2 (p1i8.hip:402: 4 sf2 is exact, the second product rounds once), Psi2 only -- 2 * sf2 is exact;
  4. one final product, s * kscale2 resp. s * kscale (p1i8.hip:212, 215); yscale is a power of two, so the second product of C is exact.
Every rounding is relative to a partial sum that is at most  P = sum_s sum_o |I_o,s| 128^-o  (the absolute per-slice terms, I_o,s the integer sum of
slice s), so with n = 5 + (ceil(S / 8) - 1) + 3 + 2 for Psi2 and one fewer for C, and A = scale * P (scale = 4 sf2^2 resp. 2 sf2 yscale_d),
      |dev - exact| <= (gamma_n + REF_ROUNDINGS 2^-64) A,        gamma_n = n u / (1 - n u)
(Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1: a product of n factors (1 + delta_i), |delta_i| <= u).  n = 18 at S = 72, 14 at
S = 40 -- the shape's own chain, not a guess.  P is a float64 expression with relative error below (S + 6) u; the factor 1 + 2^-40 on the bound
covers it.  Psi1 is positive and its leading digits dominate, so A is within a few parts in a thousand of |Psi2|; for C it is what the slices'
partial sums add up to in absolute value.
The diagonal: psi1_kernel adds the squares of a column over its workgroup's R rows with one fma each (psi1.hip:111; R = 16 * psi1_groups = 128 rows
below 2^17 padded rows, 512 from there on, psi1.hip:250-260): R roundings; p1i8_diag_kernel (p1i8.hip:171-191) adds the B = ceil(Np / R) block sums
into eight interleaved sums in order (ceil(B / 8) - 1 additions) and a 3-level tree.  All terms are positive, so with n_d = R + ceil(B / 8) + 2
      |dev_ii - exact_ii| <= (gamma_n_d + REF_DIAG_ROUNDINGS 2^-64) exact_ii.
n_d = 194 at N = 65536.  A digit-sum diagonal misses it by two orders of magnitude (fault 'diag', test_i8_ref_cpu.py).

THE CONVERSION BIT FOR BIT.  Every operation of 1 - 4 is either exact or ONE IEEE rounding of a float64 expression numpy evaluates the same way
(fma(I w, v) with an exact product is fl(I w + v)), so `emulate` -- the same sums in the same order -- is what the device must return bit for bit for
the off-diagonal of Psi2 and for C.  The GPU test asserts that too; the bound stays the statement that does not depend on the order.

FAULTS (`reference(..., fault=)`, applied to the emulated device value only; test_i8_ref_cpu.py holds each against the bound of the clean reference):
  'order7'  the order-7 products dropped            'order8'  order 8 included (26 products)       'floor'   floor in place of rint
  'kstep'   one k-step of 32 rows missing from one tile of one slice                               'slice2'  one slice added twice
  'diag'    the diagonal taken from the digits      'cshift'  a column block of C written one tile off (cyclic)
  'yscale2' yscale doubled (4 m < yscale <= 8 m): the last bit of a 42-bit Y is lost and every digit moves by one bit, so other products are dropped:
            the bound sees it (the kept products' exact value moves by the size of the truncation), and the exact probe (`probe_inputs`) bit for bit.

THE EXACT PROBE (`probe_inputs`).  sf2 = 1 (so that exp(ln sf2) is exactly sf2 and hscale = 1/2), alpha = 1, Z on a planar lattice of spacing 8: an
off-class entry is at most exp(-32) = 1.3e-14, t <= 6.4e-15 < 2^-43, and every one of its six digits rounds to zero.  Every row of X is bit-equal to
a row of Z (its class): Psi1 = 1, t = 1/2, first digit +64 -- the edge of the digit range -- and zeros behind it.  Y holds integers of at most 41
bits, odd ones included, times a power of two per column: 42 bits below yscale, exactly six digits, no remainder.  Then every sum above is a sum of
integers times one power of two, below 2^53 in those units: nothing rounds, and C = sf2 * the per-class sums of Y, Psi2 = sf2^2 diag(class counts),
bit for bit (`probe_expected`, plain integer arithmetic on the inputs).
"""
import zlib

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
DIGITS = 6                     # GP_I8_DIGITS, gp_common.h:21
KEPT = 7                       # I8L, p1i8.hip:56: digit products with a + b <= 7 (digits numbered from 1)
I8_MAX_ROWS = 81920            # p1i8.hip:51
REF_ROUNDINGS = 8
REF_DIAG_ROUNDINGS = 18
FAULTS = ('order7', 'order8', 'floor', 'kstep', 'slice2', 'diag', 'cshift', 'yscale2')


def pad(n):
    return -(-n // 128) * 128


# ---- the plan (p1i8_prepare) ------------------------------------------------------------------------------------------------------------------
def workspace_tiles(Np, Mp, Dp):
    """api.hip:91-100: the shared workspace's capacity in 128 x 128 tiles, a function of the shape alone"""
    mt, dt = Mp // 128, Dp // 128
    n_tiles = mt * (mt + 1) // 2 + mt * dt                   # psi.hip:216-220
    chunks = Np // 16                                        # KC = 16, mma_f64.h:32
    S = max(1, min(512 // max(1, n_tiles if mt * dt > 0 else 1), chunks))
    Tb = mt * dt
    Sb = max(1, min(512 // max(1, Tb), chunks))
    return max((S + 16) * n_tiles, (Sb + 16) * Tb, 1100)


def plan(N, D, M):
    """p1i8_prepare's slicing as a function of the shape: dict(T, s8, S (slices in all), n_shared, ksteps, bounds [(k0, k1)] per slice, tiles)"""
    Np, Mp, Dp = pad(N), pad(M), pad(D)
    MT, DT = Mp // 128, Dp // 128
    tiles = [(i, j) for i in range(MT) for j in range(i, MT)] + [(i, MT + j) for i in range(MT) for j in range(DT)]      # p1i8.hip:315-316
    T, SLOTS = len(tiles), 32
    ksteps = Np // 32
    s8min = max(1, (Np + 8 * I8_MAX_ROWS - 1) // (8 * I8_MAX_ROWS))                                                      # :320
    s8, best = s8min, 1e30
    for t in range(s8min, s8min + 9):                                                                                    # :322-325
        cost = float(-(-(t * T) // SLOTS)) / t
        if cost < best - 1e-9:
            best, s8 = cost, t
    Smax = workspace_tiles(Np, Mp, Dp) // T                                                                              # :326
    S = min(8 * s8, ksteps, Smax)                                                                                        # :327
    assert S >= 1 and (Np + S - 1) // S + 32 <= 87000, 'the path refuses this shape (p1i8.hip:328)'
    n_shared = 0
    if T <= SLOTS and S == 8 * (SLOTS // T) and s8 == SLOTS // T:                                                        # :336-340
        left = SLOTS - (SLOTS // T) * T
        n_shared = max(0, min((8 * left) // T, Smax - S, ksteps - S))
    Stot = S + n_shared
    bounds = [(s * ksteps // Stot, (s + 1) * ksteps // Stot) for s in range(Stot)]                                       # :343, :349
    return dict(T=T, s8=s8, S=Stot, n_shared=n_shared, ksteps=ksteps, bounds=bounds, tiles=tiles, MT=MT, DT=DT, Np=Np, Mp=Mp, Dp=Dp)


def diag_blocks(N):
    """(rows per psi1_kernel workgroup, number of workgroups along the rows): psi1.hip:250-260"""
    Np = pad(N)
    ngrp = 32 if Np >= (1 << 17) else 8
    return 16 * ngrp, (Np // 16 + ngrp - 1) // ngrp


def roundings(S):
    """(n for Psi2, n for C): the module docstring's count at S slices"""
    chain = 5 + (-(-S // 8) - 1) + 3
    return chain + 2, chain + 1


def diag_roundings(N):
    R, B = diag_blocks(N)
    return R + (-(-B // 8) - 1) + 3


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- digits -----------------------------------------------------------------------------------------------------------------------------------
def yscale(Y):
    m = np.max(np.abs(Y), axis=0)
    e = np.frexp(m)[1].astype(np.int64) + 1
    return np.where(m > 0.0, np.ldexp(1.0, np.where(m > 0.0, e, 0)), 1.0)


def digits(t, rnd=np.rint, check=True):
    """the six digit planes of t (already scaled: |t| <= 1/2), as float64 integers"""
    out = []
    t = np.array(t, dtype=np.float64)
    for _ in range(DIGITS):
        t = t * 128.0
        g = rnd(t)
        t = t - g
        if check:
            assert np.all(np.abs(g) <= 64.0), 'a digit outside [-64, 64]'
        out.append(g)
    return out


def _weights(kept):
    return [128.0 ** -(o + 2) for o in range(kept - 1)]        # order index o = (a - 1) + (b - 1): a + b = o + 2


def _order_sums(dA, dE, kept):
    """[kept - 1][M][W]: I_o of one block of rows; dA, dE: the digit planes of Psi1 and of [Psi1 | Y]"""
    n, M = dA[0].shape
    W = dE[0].shape[1]
    assert 6 * 4096 * max(n, 1) < 2 ** 53
    out = np.zeros((kept - 1, M, W))
    for a in range(DIGITS):
        nb = min(DIGITS, kept - 1 - a)
        if nb <= 0:
            continue
        G = dA[a].T @ np.concatenate(dE[:nb], axis=1)
        for b in range(nb):
            out[a + b] += G[:, b * W:(b + 1) * W]
    return out


def _pairwise_ld(x):
    """sum over axis 0 in long double by an explicit tree: ceil(log2 n) roundings"""
    x = np.asarray(x, dtype=LD)
    while x.shape[0] > 1:
        if x.shape[0] & 1:
            x = np.concatenate([x, np.zeros((1,) + x.shape[1:], dtype=LD)], axis=0)
        x = x[0::2] + x[1::2]
    return x[0]


def exact_diagonal(Psi1):
    N, M = Psi1.shape
    assert N <= 1 << 17
    out = np.empty(M, dtype=LD)
    for c0 in range(0, M, 64):
        x = np.asarray(Psi1[:, c0:c0 + 64], dtype=LD)
        out[c0:c0 + 64] = _pairwise_ld(x * x)
    return out


def emulate_diagonal(Psi1):
    """the device's sums of squares in float64, in its order; the fma of psi1.hip:111 is replaced by a rounded square and an addition (numpy has no fma),
    so this one is inside the bound but not bit for bit"""
    N, M = Psi1.shape
    R, B = diag_blocks(N)
    sq = np.zeros((B * R, M))
    sq[:N] = Psi1 * Psi1
    dpart = np.cumsum(sq.reshape(B, R, M), axis=1)[:, -1, :]
    acc = [np.cumsum(dpart[u::8], axis=0)[-1] if len(dpart[u::8]) else np.zeros(M) for u in range(8)]
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]))


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------
def reference(Psi1, Y, sf2, fault=None, bounds=None):
    """dict: Psi2, C (long double, exact), tol2, tolC (float64, the bound), emu2, emuC (float64: the device's conversion in its order), I (the integer
    sums [6][M][M + D]), yscale, plan.  ``fault`` changes the emulated value (and, for 'floor' and 'yscale2', the digits behind everything: take the
    exact value from a clean call).  ``bounds``: another split of the k-steps (the integer sums must not depend on it)."""
    assert fault is None or fault in FAULTS
    Psi1, Y = np.ascontiguousarray(Psi1, dtype=np.float64), np.ascontiguousarray(Y, dtype=np.float64)
    N, M = Psi1.shape
    D = Y.shape[1]
    W = M + D
    assert 6 * 4096 * N < 2 ** 53
    pl = plan(N, D, M)
    bnds = pl['bounds'] if bounds is None else bounds
    S = len(bnds)
    kept = {'order7': KEPT - 1, 'order8': KEPT + 1}.get(fault, KEPT)
    w = _weights(kept)
    rnd = np.floor if fault == 'floor' else np.rint
    ysc = yscale(Y) * (2.0 if fault == 'yscale2' else 1.0)
    hscale, yinv = 0.5 / sf2, 1.0 / ysc
    I = np.zeros((kept - 1, M, W))
    P = np.zeros((M, W))
    acc = [np.zeros((M, W)) for _ in range(8)]
    hit = S // 2                                             # the slice the 'kstep' and 'slice2' faults touch
    for s, (k0, k1) in enumerate(bnds):
        r0, r1 = min(32 * k0, N), min(32 * k1, N)            # the padded rows' digits are zeros (psi1.hip:99-100: v = 0 for n >= N; Y's padding is zero)
        dA = digits(Psi1[r0:r1] * hscale, rnd, check=fault is None)
        dE = [np.concatenate([a, y], axis=1) for a, y in zip(dA, digits(Y[r0:r1] * yinv, rnd, check=fault is None))]
        Is = _order_sums(dA, dE, kept)
        I += Is
        if fault == 'kstep' and s == hit:                    # the tile's first k-step of this slice: tile (0, last column block)
            cut = slice(r0, min(r0 + 32, r1))
            dA1 = digits(Psi1[cut] * hscale, rnd, check=False)
            dE1 = [np.concatenate([a, y], axis=1) for a, y in zip(dA1, digits(Y[cut] * yinv, rnd, check=False))]
            c0 = (W - 1) // 128 * 128
            Is[:, :128, c0:c0 + 128] -= _order_sums(dA1, dE1, kept)[:, :128, c0:c0 + 128]
        v = np.zeros((M, W))
        for o in range(kept - 2, -1, -1):
            v = Is[o] * w[o] + v                             # fma with an exact product
            P += np.abs(Is[o]) * w[o]
        acc[s % 8] = acc[s % 8] + v
        if fault == 'slice2' and s == hit:
            acc[s % 8] = acc[s % 8] + v
    assert np.max(np.abs(I)) < 2 ** 53
    tot = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]))
    k2, k1 = (4.0 * sf2) * sf2, 2.0 * sf2
    emu2 = tot[:, :M] * k2
    emuC = (tot[:, M:] * k1) * ysc
    if fault != 'diag':
        emu2[np.arange(M), np.arange(M)] = emulate_diagonal(Psi1)
    emu2 = np.triu(emu2) + np.triu(emu2, 1).T                # the device computes the upper tiles and mirrors them (p1i8.hip:221-222)
    if fault == 'cshift':
        Dp = pl['Dp']
        full = np.zeros((M, Dp))
        full[:, :D] = emuC
        emuC = np.roll(full, -128, axis=1)[:, :D] if Dp > 128 else np.roll(emuC, 1, axis=1)
    # the exact value
    val = np.zeros((M, W), dtype=LD)
    for o in range(kept - 2, -1, -1):
        val = val + np.asarray(I[o], dtype=LD) * (LD(128.0) ** -(o + 2))
    sf = LD(sf2)
    Psi2 = val[:, :M] * (LD(4.0) * sf * sf)
    C = val[:, M:] * (LD(2.0) * sf) * np.asarray(ysc, dtype=LD)
    dg = exact_diagonal(Psi1)
    Psi2[np.arange(M), np.arange(M)] = dg
    n2, nC = roundings(S)
    slack = 1.0 + 2.0 ** -40
    tol2 = (gamma(n2) + REF_ROUNDINGS * 2.0 ** -64) * slack * (k2 * P[:, :M])
    tolC = (gamma(nC) + REF_ROUNDINGS * 2.0 ** -64) * slack * (k1 * ysc[None, :] * P[:, M:])
    tol2[np.arange(M), np.arange(M)] = (gamma(diag_roundings(N)) + REF_DIAG_ROUNDINGS * 2.0 ** -64) * np.asarray(dg, dtype=np.float64) * slack
    return dict(Psi2=Psi2, C=C, tol2=tol2, tolC=tolC, emu2=emu2, emuC=emuC, I=I, yscale=ysc, plan=pl, n2=n2, nC=nC, nd=diag_roundings(N))


def ratios(dev, exact, tol):
    """|dev - exact| / tol per element (0 where both vanish, inf where only the tolerance does or the value is not finite)"""
    err = np.abs(np.asarray(dev, dtype=LD) - exact)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, np.asarray(err / np.asarray(tol, dtype=LD), dtype=np.float64))
    return np.where(np.isfinite(r), r, np.inf)


def hold(name, Psi2_dev, C_dev, ref, bits=True):
    """the problems of a device result as strings (empty: none); prints the worst error / bound per array"""
    bad = []
    M = ref['Psi2'].shape[0]
    off = ~np.eye(M, dtype=bool)
    r2, rC = ratios(Psi2_dev, ref['Psi2'], ref['tol2']), ratios(C_dev, ref['C'], ref['tolC'])
    parts = (('Psi2 off-diagonal', np.where(off, r2, 0.0)), ('Psi2 diagonal', np.where(off, 0.0, r2)), ('C', rC))
    same2 = bool(np.array_equal(np.where(off, Psi2_dev, 0.0), np.where(off, ref['emu2'], 0.0)))
    sameC = bool(np.array_equal(C_dev, ref['emuC']))
    print('%s: S = %d slices, n = %d / %d / %d roundings; worst error / bound: %s; bit-identical to the emulation: Psi2 off-diagonal %s, C %s' % (
        name, ref['plan']['S'], ref['n2'], ref['nd'], ref['nC'], ', '.join('%s %.4f' % (k, float(r.max())) for k, r in parts), same2, sameC))
    for k, r in parts:
        if r.max() > 1.0:
            i = np.unravel_index(int(np.argmax(r)), r.shape)
            bad.append('%s: %d elements outside the bound, worst %.3g of it at %s' % (k, int((r > 1.0).sum()), float(r.max()), i))
    if bits and not same2:
        bad.append('Psi2 off the diagonal differs from the conversion emulated in the device\'s order at %d elements' % int((np.where(off, Psi2_dev, 0.0) != np.where(off, ref['emu2'], 0.0)).sum()))
    if bits and not sameC:
        bad.append('C differs from the conversion emulated in the device\'s order at %d elements' % int((C_dev != ref['emuC']).sum()))
    return bad


def checksum(Psi1):
    return zlib.crc32(np.ascontiguousarray(Psi1).tobytes())


def save(path, ref, crc):
    np.savez(path, crc=np.int64(crc), Psi2=ref['Psi2'], C=ref['C'], tol2=ref['tol2'], tolC=ref['tolC'],
             emu2=ref['emu2'], emuC=ref['emuC'], counts=np.array([ref['plan']['S'], ref['n2'], ref['nC'], ref['nd']]))


def load(path, crc):
    """the reference a parent process saved, or None when it was made for another Psi1 (crc: checksum of the one at hand)"""
    z = np.load(path)
    if int(z['crc']) != crc:
        return None
    S, n2, nC, nd = (int(x) for x in z['counts'])
    return dict(Psi2=z['Psi2'], C=z['C'], tol2=z['tol2'], tolC=z['tolC'], emu2=z['emu2'], emuC=z['emuC'], plan=dict(S=S), n2=n2, nC=nC, nd=nd)


# ---- the truncation model (test_i8_ref_cpu.py) -------------------------------------------------------------------------------------------------
def truncation_bound(Psi1, Y, sf2, ysc):
    """|exact int8 value - K^T [K | Y]| per element, off the diagonal of Psi2: an operand entry x of scale s (2 sf2, yscale_d) is represented by
    x^ = s sum_j d_j 128^-j with |x - x^| <= s 2^-43 + 2 u |x| (six round-to-nearest digits leave 128^-6 / 2 = 2^-43; hscale and the first multiply round
    once each; for Y both are exact), so |x y - x^ y^| <= |x| dy + |y| dx + dx dy; the 15 products that are not formed have a + b = 8 .. 12, 5, 4, 3, 2, 1
    of them, |d e| <= 4096: at most 4096 (5 128^-8 + 4 128^-9 + ...) <= 5.04 2^-44 per row in units of s_x s_y.  The long-double product it is compared
    with rounds N + 1 times at 2^-64."""
    N = Psi1.shape[0]
    sx = 2.0 * sf2
    E = np.concatenate([Psi1, Y], axis=1)
    se = np.concatenate([np.full(Psi1.shape[1], sx), ysc])
    dX = sx * 2.0 ** -43 + 2 * U * np.abs(Psi1)
    dE = se[None, :] * 2.0 ** -43 + np.concatenate([2 * U * np.abs(Psi1), np.zeros_like(Y)], axis=1)
    aX, aE = np.abs(Psi1), np.abs(E)
    return aX.T @ dE + dX.T @ aE + dX.T @ dE + N * 5.04 * 2.0 ** -44 * sx * se[None, :] + (N + 1) * 2.0 ** -64 * (aX.T @ aE)


# ---- the exact probe ------------------------------------------------------------------------------------------------------------------------------
def probe_inputs(N=65536, M=512, seed=7):
    """D = 8, Q = 2 (module docstring); Y's columns: maximum 2^41 - 1 | maximum exactly 2^40 | a negative extreme | zeros | integers 2^-300 |
    integers 2^+300 | small odd integers | 20-bit integers"""
    rs = np.random.RandomState(seed)
    gx = 32 if M >= 32 else M
    Z = np.stack([8.0 * (np.arange(M) % gx), 8.0 * (np.arange(M) // gx)], axis=1)
    cls = rs.randint(0, M, size=N)
    cls[:M] = np.arange(M)                                   # no empty class
    top = 2 ** 41 - 1
    Y = np.zeros((N, 8))
    Y[:, 0] = rs.randint(-top, top + 1, size=N, dtype=np.int64); Y[5, 0] = top; Y[6, 0] = -(top - 2)
    Y[:, 1] = rs.randint(-2 ** 40 + 1, 2 ** 40, size=N, dtype=np.int64); Y[9, 1] = 2.0 ** 40
    Y[:, 2] = rs.randint(-2 ** 40 + 1, 2 ** 40, size=N, dtype=np.int64); Y[11, 2] = -top
    Y[:, 4] = rs.randint(-top, top + 1, size=N, dtype=np.int64) * 2.0 ** -300
    Y[:, 5] = rs.randint(-top, top + 1, size=N, dtype=np.int64) * 2.0 ** 300
    Y[:, 6] = 2 * rs.randint(-2, 2, size=N) + 1
    Y[:, 7] = rs.randint(-2 ** 20, 2 ** 20, size=N)
    return dict(N=N, D=8, M=M, Q=2, Z=Z, X_mu=Z[cls].copy(), X_S=np.zeros((N, 2)), Y=Y, sf2=1.0, alpha=np.ones(2), beta=1.0, cls=cls)


def probe_expected(d):
    """(Psi2, C) of the probe in plain integer arithmetic on the inputs: float64, exact"""
    M, cls, Y = d['M'], d['cls'], d['Y']
    counts = np.bincount(cls, minlength=M).astype(np.float64)
    C = np.zeros((M, Y.shape[1]))
    for col in range(Y.shape[1]):
        m = np.max(np.abs(Y[:, col]))
        unit = np.ldexp(1.0, int(np.frexp(m)[1]) - 41) if m > 0 else 1.0          # the column's integers are Y / unit, at most 41 bits
        q = Y[:, col] / unit
        assert np.array_equal(q, np.rint(q)) and np.max(np.abs(q)) < 2 ** 41
        sums = np.zeros(M, dtype=np.int64)
        np.add.at(sums, cls, q.astype(np.int64))
        assert np.max(np.abs(sums)) < 2 ** 53
        C[:, col] = sums.astype(np.float64) * unit
    return np.diag(counts) * d['sf2'] ** 2, C * d['sf2']
