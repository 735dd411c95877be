"""The global step's two extended-precision products -- G = K_mm^-1 Psi2 and the refinement residual R = C - (K_mm + beta Psi2) E -- restated exactly
on the host, with the error bound of each of their four device forms and the table of cases tests/test_gpu_dd_products.py runs through
gp_debug_dd_product (run_case at the end is the one caller of the hook).  tests/test_dd_ref_cpu.py checks the reference, numpy emulations of the
device arithmetic against the bounds, the checker and the hook's refusals without a device.

A case is a dict:
  form            1 dd-gemm (ddacc_gemm_kernel), 2 dd-residual (ddacc_residual_kernel), 3 row-residual (solve_residual_kernel), 4 int8 (gsi8.hip); 0 the step's choice
  product         0: out = P, 1: out = Csub - P, with P(i, j) = sum_k a(i, k) B[k][j]
  nA, nB, K       rows, columns, contraction length;   M, Mp, Dp for forms 0 and 3 (nA = K = Mp, nB = Mp or Dp)
  A               [nA][K] -- what the hook is given is A for forms 1 and 2, A^T ([K][nA]) for form 4, nothing for form 3
  B, Csub         [K][nB], [nA][nB]
  Keep, Psi2, beta, jitA   form 3: a(i, k) = fl(fl(beta Psi2[i][k] + Keep[i][k]) + (i == k ? jitA : 0)) for i, k < M -- the kernel's own rounding of its operand,
                  reproduced exactly (one FMA, one add); rows M .. Mp of the result are zeros
  check           'bound' (|out - exact| <= the form's bound at every element) or 'bits' (out == exact, which is then a float64)

THE EXACT VALUE.  Doubles are dyadic rationals.  exact_product cuts every row of A and every column of B into slices of 20 bits below the row's /
column's largest exponent (t <- 2^20 t, q = rint(t), t <- t - q until t = 0 everywhere: each step exact), so that every slice product q_l^T q_m is a
float64 matrix product of integers below 2^51 -- exact in any order -- and adds the slice products as Python integers.  The result, and Csub minus
it, are integers times a power of two per element; they are handed out as a double-double (hi, lo): hi the value rounded to nearest, lo the
remainder rounded to nearest (|value - hi - lo| <= 2^-106 |value|).  exact_fraction is the same value by fractions.Fraction, element by element,
and exact_fsum by math.fsum over error-free products (Veltkamp / Dekker): the three agree (test_dd_ref_cpu.py).  No longdouble, no device.

THE BOUNDS.  u = 2^-53, S(i, j) = sum_k |a(i, k)| |B[k][j]|, P the exact product, R = Csub - P.  Derived here, never measured.

dd-gemm.  ddacc_block is Dot2 of Ogita, Rump and Oishi (Accurate sum and dot product, SIAM J. Sci. Comput. 26, 2005, Algorithm 5.3): per term
pr + pe = a b exactly (FMA), t = fl(hi + pr) with its exact error q (Knuth's TwoSum), lo <- fl(lo + fl(q + pe)), result fl(hi + lo).  With the
exact lo* = sum (q + pe) one has hi + lo* = P; the computed lo differs from lo* by at most gamma_{K-1} gamma_K S (their Proposition 5.5's proof: K
additions of terms that are each below u times a partial sum of |a b|), gamma_n = n u / (1 - n u).  Hence
      |out - P| <= u |P| + gamma_K^2 S      and a fortiori      |out - P| <= 2 u |P| + (K + 2)^2 u^2 S,
since K u / (1 - K u) <= (K + 2) u for every K below 2^26.  The second form is the one used (DD_GEMM).

dd-residual (ddacc_block<.., SUB> and the int8 form's subtraction).  (hi, lo) as above with hi + lo = P + delta, |delta| <= gamma_K^2 S, and
out = fl(fl(c - hi) - lo).  Two roundings: out = ((c - hi)(1 + e1) - lo)(1 + e2) = (R - delta + e1 (c - hi))(1 + e2), so
      |out - R| <= u |R| + (1 + u)(|delta| + u |c - hi|),      |c - hi| <= |R| + |lo| + |delta|.
|lo| <= sum |q| + sum |pe| <= u K (1 + u)^(K+1) S + u S <= (K + 1)(1 + gamma_{K+1}) u S, so u |lo| <= 2 K u^2 S for K >= 2.  Together
      |out - R| <= 2 u |R| + (K + 2)^2 u^2 S + 4 K u^2 S,
the (1 + u) factors and u |delta| inside the slack (K + 2)^2 - K^2 / (1 - K u)^2 >= 4 K and 4 K - 2 K (DD_RESIDUAL).

row-residual (solve_residual_kernel).  Four chains of at most Kq = ceil(M / 4) terms, each a Dot2 without its last addition: quarter r has
h_r + l_r = P_r + delta_r with |delta_r| <= gamma_Kq^2 S_r, together at most (Kq + 1)^2 u^2 S.  Three double-double additions follow (residual_add:
t = fl(hi + x) with its exact error q, lo <- fl(lo + fl(q + xl))): two roundings each, of numbers that are sums of low-order parts.  Every low-order
part -- the four l_r, at most (Kq + 1)(1 + gamma) u S together, and the three q, at most u (1 + gamma) S each -- adds up to at most L = (Kq + 4)(1 + gamma) u S,
so the six roundings cost at most 6 u L, and the final |lo| is at most L.  With the two roundings of the subtraction as above,
      |out - R| <= 2 u |R| + (1 + u)^2 ((Kq + 1)^2 + 6 (Kq + 4) + (Kq + 4)) u^2 S (1 + gamma)  <=  2 u |R| + ((Kq + 2)^2 + 8 (Kq + 4)) u^2 S,
Kq = ceil(M / 4).  This is below the dd-residual bound at K = M for every M >= 5 and holds for M = 1 and 3, where quarters are empty and the constant
of the dd-residual bound would not cover the 8 (Kq + 4) of the additions (ROW_RESIDUAL).  S is taken over the rounded operand a.

int8 (gsi8.hip).  Worst case, whatever scale the kernel chooses, as long as scale is a power of two with 2 max < scale <= 4 max per column (amax_i for
row i of the result, bmax_j for column j).  Ten round-to-nearest base-128 digits leave |x - x^| <= scale 2^-71 per operand entry, so the digit
operands give sum_k |a b - a^ b^| <= K (4 amax 2^-71 bmax + 4 bmax 2^-71 amax (1 + 2^-69)) <= K 2^-68 amax bmax.  The digit products that are not
formed have da + db >= 12 (digits numbered from 1): 21 - o pairs of order o, |q q'| <= 4096, so per term at most 4096 (9 128^-12 + 8 128^-13 + ...)
<= 9.1 2^-72 in units of scale_a scale_b <= 16 amax bmax: K 9.1 2^-68 amax bmax.  The ten order sums are exact doubles; their two-sum chain rounds lo
ten times, each below u^2 times sum_o |x_o| <= 4.1 K amax bmax: 41 K 2^-106 amax bmax.  One final rounding of hi + lo.  In all
      |out - P| <= u |P| + (1 + u) K (10.1 2^-68 + 41 2^-106) amax_i bmax_j  <=  u |P| + K 2^-63 amax_i bmax_j           (10.1 2^-68 < 2^-64.6),
and with the subtraction (|lo| <= 41 K u amax bmax, so u |lo| vanishes in the slack)  |out - R| <= 2 u |R| + K 2^-63 amax_i bmax_j  (I8).

The comparison itself is float64 arithmetic on (out - hi) - lo: out - hi is exact wherever out is within a factor two of hi (Sterbenz) and an error
of the size of out elsewhere; S and the bound are float64 expressions with relative error below K u.  Both are orders of magnitude inside the slack
written out above.

INPUT CLASSES.  cancellation (full mantissas, k-rows k and k + K/2 carry a and -b (1 + 1e-9 g), permuted: median |P| / S about 5e-11, the regime of
K_mm^-1 Psi2; plain float64 `@` violates every bound above on most elements -- the condition test_dd_ref_cpu.py holds each such case to);
digit-order probes (int8: one digit position per operand, exact for da + db <= 11); integer-exact (float64 `@` is the answer, bit for bit); scale
edges (int8 column maxima: zero, a power of two, negative, 2^-300, 2^300)."""
import math
import zlib
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
DD_GEMM, DD_RESIDUAL, ROW_RESIDUAL, I8 = 1, 2, 3, 4
FORM_NAMES = {DD_GEMM: 'dd-gemm', DD_RESIDUAL: 'dd-residual', ROW_RESIDUAL: 'row-residual', I8: 'int8'}
SLICE_BITS = 20


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7fffffff


# ---- the exact value ----------------------------------------------------------------------------------------------------------------------
def _slices(X, axis):
    """X = 2^e * sum_l q_l 2^(-SLICE_BITS (l + 1)) along `axis` (e per row / column: the exponent of its largest entry), q_l integer-valued, |q_l| <= 2^SLICE_BITS"""
    mx = np.max(np.abs(X), axis=axis, keepdims=True)
    e = np.where(mx > 0, np.frexp(mx)[1], 0).astype(np.int64)
    t = np.ldexp(X, -e)                               # |t| <= 1, exact
    assert np.array_equal(np.ldexp(t, e), X), 'operand under- or overflows when scaled'
    q = []
    while t.any():
        assert len(q) < 64, 'operand has more than 1280 bits of dynamic range inside one row / column'
        t = t * 2.0 ** SLICE_BITS
        r = np.rint(t)
        t = t - r
        q.append(r)
    return e, q


def _exact_int(A, B):
    """(N, e): N object array of Python ints, e int64 array, with sum_k A[i][k] B[k][j] = N[i][j] 2^e[i][j] exactly"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    K = A.shape[1]
    assert K <= 2048 and B.shape[0] == K                 # 2^40 * 2^11 = 2^51: every slice product is exact in float64
    ea, qa = _slices(A, 1)
    eb, qb = _slices(B, 0)
    la, lb = max(len(qa), 1), max(len(qb), 1)
    orders = [np.zeros((A.shape[0], B.shape[1]), dtype=np.int64) for _ in range(la + lb - 1)]
    for l, x in enumerate(qa):
        for m, y in enumerate(qb):
            orders[l + m] += (x @ y).astype(np.int64)
    N = orders[0].astype(object)
    for T in orders[1:]:
        N = N * (1 << SLICE_BITS) + T.astype(object)     # Horner, in Python integers
    return N, ea + eb - SLICE_BITS * (la + lb)


def _dd_of(n, e):
    """the integer n times 2^e as (hi, lo): hi rounded to nearest, lo the remainder rounded to nearest"""
    hi = float(n)
    return math.ldexp(hi, e), math.ldexp(float(n - int(hi)), e)


def _sub_dd(n, e, c):
    if c != 0.0:
        m, ex = math.frexp(c)
        ci, ec = int(math.ldexp(m, 53)), ex - 53
        e2 = min(e, ec)
        n, e = (ci << (ec - e2)) - (n << (e - e2)), e2
    else:
        n = -n
    return _dd_of(n, e)


_dd_of_v = np.frompyfunc(_dd_of, 2, 2)
_sub_dd_v = np.frompyfunc(_sub_dd, 3, 2)


def exact_product(A, B, Csub=None):
    """(hi, lo), float64 arrays: sum_k A[i][k] B[k][j], or Csub minus it, exact to 2^-106 relative"""
    N, e = _exact_int(A, B)
    hi, lo = _dd_of_v(N, e.astype(object)) if Csub is None else _sub_dd_v(N, e.astype(object), np.asarray(Csub, dtype=np.float64).astype(object))
    return hi.astype(np.float64), lo.astype(np.float64)


def exact_fraction(A, B, Csub=None):
    """the same value as a Fraction per element (small cases)"""
    out = np.empty((A.shape[0], B.shape[1]), dtype=object)
    for i in range(A.shape[0]):
        fa = [Fraction(float(x)) for x in A[i]]
        for j in range(B.shape[1]):
            p = sum(fa[k] * Fraction(float(B[k, j])) for k in range(A.shape[1]))
            out[i, j] = p if Csub is None else Fraction(float(Csub[i, j])) - p
    return out


def split(a):
    """Veltkamp: a = hi + lo with 26-bit halves"""
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def two_product(a, b):
    """(p, e) with p = fl(a b) and p + e = a b exactly (Dekker; what fma(a, b, -p) returns on the device), barring under- and overflow"""
    p = a * b
    ah, al = split(a)
    bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def exact_fsum(A, B, Csub=None):
    """the value rounded to nearest by math.fsum over the error-free products (and Csub), per element"""
    out = np.empty((A.shape[0], B.shape[1]))
    for i in range(A.shape[0]):
        pr, pe = two_product(A[i][:, None], B)
        for j in range(B.shape[1]):
            terms = np.concatenate([pr[:, j], pe[:, j]])
            out[i, j] = math.fsum(terms) if Csub is None else math.fsum(np.concatenate([[Csub[i, j]], -terms]))
    return out


def rounded_operand(Keep, Psi2, beta, jitA, M):
    """solve_residual_kernel's a(i, k) = fma(beta, Psi2, Keep) + (i == k ? jitA : 0) on the leading M x M block, bit for bit: the FMA by one exact
    rational expression rounded once, then a float64 add"""
    fb = Fraction(float(beta))
    a = np.empty((M, M))
    for i in range(M):
        for k in range(M):
            a[i, k] = float(fb * Fraction(float(Psi2[i, k])) + Fraction(float(Keep[i, k])))
    a[np.arange(M), np.arange(M)] += jitA
    return a


# ---- the bounds (module docstring) ----------------------------------------------------------------------------------------------------------
def bound(case, a, B, hi):
    """elementwise tolerance of case['form'] on |out - exact|; a: the operand [rows][K] the sum runs over, hi: the exact value rounded"""
    form, K = case['form'], a.shape[1]
    if form == I8:
        amax, bmax = np.max(np.abs(a), axis=1), np.max(np.abs(B), axis=0)
        return (2.0 if case['product'] else 1.0) * U * np.abs(hi) + K * 2.0 ** -63 * amax[:, None] * bmax[None, :]
    S = np.abs(a) @ np.abs(B)
    if form == DD_GEMM:
        return 2 * U * np.abs(hi) + (K + 2) ** 2 * U * U * S
    if form == DD_RESIDUAL:
        return 2 * U * np.abs(hi) + ((K + 2) ** 2 + 4 * K) * U * U * S
    Kq = (case['M'] + 3) // 4
    return 2 * U * np.abs(hi) + ((Kq + 2) ** 2 + 8 * (Kq + 4)) * U * U * S


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def cancellation(rs, nA, nB, K, a_range_bits=0):
    """A [nA][K], B [K][nB]: k-rows k and k + K/2 carry a and -b (1 + 1e-9 g), k permuted; a_range_bits: per-entry dynamic range of A below its scale"""
    h = K // 2
    A, B = np.empty((nA, K)), np.empty((K, nB))
    A[:, :h] = rs.randn(nA, h)
    if a_range_bits:
        A[:, :h] *= np.exp2(rs.randint(-a_range_bits, 1, size=(nA, h)))
    A[:, h:2 * h] = A[:, :h]
    B[:h] = rs.randn(h, nB)
    B[h:2 * h] = -B[:h] * (1 + 1e-9 * rs.randn(h, nB))
    if K > 2 * h:                                        # odd K: one unpaired term
        A[:, 2 * h:] = rs.randn(nA, K - 2 * h) * 1e-9
        B[2 * h:] = rs.randn(K - 2 * h, nB)
    p = rs.permutation(K)
    return A[:, p], B[p]


def integers(rs, rows, cols, axis):
    """integers in [-64, 64] with +64 and -64 present in every row (axis = 1) or column (axis = 0)"""
    X = rs.randint(-64, 65, size=(rows, cols)).astype(np.float64)
    n = X.shape[axis]
    pos = np.argsort(rs.rand(rows, cols), axis=axis)
    for sign, which in ((64.0, 0), (-64.0, 1)):
        idx = np.take(pos, [which], axis=axis)
        np.put_along_axis(X, idx, sign, axis=axis)
    assert n >= 2
    return X


def _dd_case(name, form, nA, nB, K):
    rs = np.random.RandomState(_seed(name))
    A, B = cancellation(rs, nA, nB, K)
    case = dict(name=name, form=form, product=int(form != DD_GEMM), nA=nA, nB=nB, K=K, A=A, B=B, check='bound', cls='cancellation')
    if case['product']:
        # C = A E0 rounded, E0 = E (1 + 1e-9 g) would need a solve; a residual is small against both of its terms all the same with C = the rounded product + noise
        case['Csub'] = (A @ B) * (1 + 1e-12 * rs.randn(nA, nB))
    return case


ROW_M = (1, 3, 5, 127, 128, 130)
ROW_DP = (128, 384)
ROW_JIT = (0.0, 1e-7)


def row_case(M, Dp, jitA):
    """Keep, Psi2 [Mp][Mp] (identity padding, as build_kmm_kernel leaves it) whose columns k and k + M/2 are equal, so that the rounded operand's are
    (the diagonal's jitA aside); E's rows k and k + M/2 carry e and -e (1 + 1e-9 g); k permuted; C = the rounded product + noise"""
    name = 'row-M%d-Dp%d-jit%g' % (M, Dp, jitA)
    rs = np.random.RandomState(_seed('row-M%d' % M))      # Keep, Psi2 shared by the cases of one M: the Fraction work of rounded_operand is done once per (M, jitA)
    Mp = -(-M // 128) * 128
    beta, h = 1.7, M // 2
    p = rs.permutation(M)

    def paired(scale):
        b = rs.randn(M, h) * scale
        return np.concatenate([b, b, rs.randn(M, M - 2 * h) * scale], axis=1)[:, p]
    Keep, Psi2 = np.eye(Mp), np.zeros((Mp, Mp))
    Keep[:M, :M] = paired(1.0)
    Psi2[:M, :M] = paired(3.0)
    a = _rounded_cached(M, Keep, Psi2, beta, jitA)
    rs2 = np.random.RandomState(_seed(name))
    e = rs2.randn(h, Dp)
    E = np.zeros((Mp, Dp))
    E[:M] = np.concatenate([e, -e * (1 + 1e-9 * rs2.randn(h, Dp)), rs2.randn(M - 2 * h, Dp) * (1e-9 if h else 1.0)], axis=0)[p]
    C = np.zeros((Mp, Dp))
    C[:M] = (a @ E[:M]) * (1 + 1e-12 * rs2.randn(M, Dp))
    return dict(name=name, form=ROW_RESIDUAL, product=1, M=M, Mp=Mp, Dp=Dp, nA=Mp, nB=Dp, K=Mp, Keep=Keep, Psi2=Psi2, beta=beta, jitA=jitA, B=E, Csub=C,
                check='bound', cls='cancellation')


_ROUNDED = {}


def _rounded_cached(M, Keep, Psi2, beta, jitA):
    key = (M, jitA)
    if key not in _ROUNDED:
        _ROUNDED[key] = rounded_operand(Keep, Psi2, beta, jitA, M)
    return _ROUNDED[key]


I8_SHAPES = ((64, 64, 32), (64, 64, 64), (128, 64, 96), (192, 128, 128))


def _i8_case(nA, nB, K, product):
    name = 'i8-%dx%dx%d-%s' % (nA, nB, K, 'csub' if product else 'sum')
    rs = np.random.RandomState(_seed(name))
    A, B = cancellation(rs, nA, nB, K, a_range_bits=30)
    case = dict(name=name, form=I8, product=product, nA=nA, nB=nB, K=K, A=A, B=B, check='bound', cls='cancellation')
    if product:
        case['Csub'] = (A @ B) * (1 + 1e-12 * rs.randn(nA, nB))
    return case


def probe_case(da, db):
    """digit-order probe, 64 x 64 x 32, digits numbered from 1: k-row 0 holds A's anchors (0.5 in every column of A^T, zero in B), k-row 1 B's; every
    other entry is q 2 128^-d, q an integer in [-64, 64] with +-64 present, d = da for A and db for B.  The scales are pinned to 2, so every entry is
    ONE digit and the result sum_k qa qb 4 128^-(da + db) is a double: the output must be it bit for bit when the order da + db is kept (<= 11)."""
    name = 'probe-%d-%d' % (da, db)
    rs = np.random.RandomState(_seed(name))
    qa, qb = integers(rs, 64, 32, 1), integers(rs, 32, 64, 0)
    # d = 1: q 2 / 128 must stay at or below the anchor for the scale to stay 2 (the kernel's scale is above twice the maximum), so q is in [-32, 32]
    # there, +-32 present -- a first digit of +-64 arises by rounding only, which the cancellation cases produce
    if da == 1:
        qa = np.rint(qa / 2.0)
    if db == 1:
        qb = np.rint(qb / 2.0)
    A, B = qa * 2.0 * 128.0 ** -da, qb * 2.0 * 128.0 ** -db
    A[:, 0], B[0, :] = 0.5, 0.0
    A[:, 1], B[1, :] = 0.0, 0.5
    return dict(name=name, form=I8, product=0, nA=64, nB=64, K=32, A=A, B=B, check='bits' if da + db <= 11 else 'bound', cls='probe')


PROBES = [(da, db) for da in range(1, 11) for db in range(1, 11)]


def scale_edge_case(product):
    """int8, 128 x 64 x 64: columns of A^T (rows of A here) and of B whose maxima are zero, an exact power of two, negative, 2^-300 and 2^300"""
    name = 'i8-scale-edges-%s' % ('csub' if product else 'sum')
    rs = np.random.RandomState(_seed(name))
    A, B = cancellation(rs, 128, 64, 64, a_range_bits=30)
    for X, ax in ((A, 1), (B.T, 1)):                      # X's rows are W's columns
        X[3] = 0.0
        X[5] = np.clip(X[5], -0.7, 0.7); X[5, 7] = 1.0        # maximum exactly 2^0: frexp gives f = 1/2
        X[6] = np.clip(X[6], -0.7, 0.7); X[6, 9] = -4.0       # ... and negative
        X[8] = -np.abs(X[8]); X[8, 11] = -7.3                 # the largest entry by magnitude is negative
    A[10] *= 2.0 ** -300                                      # one side each, so that no product leaves the double range
    B[:, 12] *= 2.0 ** -300
    A[20] *= 2.0 ** 300
    B[:, 22] *= 2.0 ** 300
    case = dict(name=name, form=I8, product=product, nA=128, nB=64, K=64, A=A, B=B, check='bound', cls='edges')
    if product:
        case['Csub'] = (A @ B) * (1 + 1e-12 * rs.randn(128, 64))
    return case


def integer_case(name, form, product, nA, nB, K, symmetric=False):
    """integer-exact: float64 `@` is the answer.  symmetric: A = A^T (nA == K), so that the forms that read A by rows and the one that reads it by columns compute the same thing"""
    rs = np.random.RandomState(_seed(name))
    A = integers(rs, nA, K, 1)
    if symmetric:
        A = np.triu(A) + np.triu(A, 1).T
        A[np.arange(nA), np.arange(nA)] = 64.0 * (1 - 2 * (np.arange(nA) & 1))      # +-64 on the diagonal: present in every row and column
        if nA > 1:
            A[0, 1] = A[1, 0] = 64.0
            A[np.arange(2, nA), 0] = A[0, np.arange(2, nA)] = np.where(np.arange(2, nA) & 1, 64.0, -64.0)
    B = integers(rs, K, nB, 0)
    case = dict(name=name, form=form, product=product, nA=nA, nB=nB, K=K, A=A, B=B, check='bits', cls='integer', symmetric=symmetric)
    if product:
        case['Csub'] = rs.randint(-2 ** 20, 2 ** 20, size=(nA, nB)).astype(np.float64)
    return case


def all_cases():
    """name -> case: everything test_gpu_dd_products.py runs one by one (the probes and the form-0 production shapes have tests of their own)"""
    out = {}
    for c in (_dd_case('dd-gemm-128', DD_GEMM, 128, 128, 128), _dd_case('dd-gemm-256', DD_GEMM, 256, 256, 256),
              _dd_case('dd-residual-256x512', DD_RESIDUAL, 256, 512, 256), _dd_case('dd-residual-256x128', DD_RESIDUAL, 256, 128, 256)):
        out[c['name']] = c
    for M in ROW_M:
        for Dp in ROW_DP:
            for jit in ROW_JIT:
                c = row_case(M, Dp, jit)
                out[c['name']] = c
    for nA, nB, K in I8_SHAPES:
        for product in (0, 1):
            c = _i8_case(nA, nB, K, product)
            out[c['name']] = c
    for product in (0, 1):
        c = scale_edge_case(product)
        out[c['name']] = c
    c = integer_case('i8-64x64x2048-integer', I8, 0, 64, 64, 2048)
    out[c['name']] = c
    # the production shape of each double-double form, integer-exact (an exact rational reference would take minutes there)
    for c in (integer_case('dd-gemm-512-integer', DD_GEMM, 0, 512, 512, 512), integer_case('dd-residual-512x512-integer', DD_RESIDUAL, 1, 512, 512, 512)):
        out[c['name']] = c
    return out


def operand(case):
    """the [rows][K] operand the sum runs over (form 3: the kernel's rounded a, zero rows from M on), and B"""
    if case['form'] == ROW_RESIDUAL and 'A' not in case:
        M, Mp = case['M'], case['Mp']
        a = np.zeros((Mp, Mp))
        a[:M, :M] = _rounded_cached(M, case['Keep'], case['Psi2'], case['beta'], case['jitA']) if case.get('cls') == 'cancellation' else \
            rounded_operand(case['Keep'], case['Psi2'], case['beta'], case['jitA'], M)
        return a, case['B']
    return case['A'], case['B']


_REF = {}


def reference(case):
    """(hi, lo, tol) of a case, computed once per process and never changed: the exact value as a double-double and the form's bound (None for 'bits')"""
    if case['name'] not in _REF:
        a, B = operand(case)
        Csub = case.get('Csub') if case['product'] else None
        if case['check'] == 'bits' and case['cls'] == 'integer':
            hi = a @ B if Csub is None else Csub - a @ B
            lo = np.zeros_like(hi)
        else:
            hi, lo = exact_product(a, B, Csub)
        if case['form'] == ROW_RESIDUAL:
            hi[case['M']:] = 0.0; lo[case['M']:] = 0.0        # rows M .. Mp: exact zeros, whatever C holds there
        tol = None if case['check'] == 'bits' else bound(case, a, B, hi)
        for x in (hi, lo) + (() if tol is None else (tol,)):
            x.setflags(write=False)
        _REF[case['name']] = (hi, lo, tol)
    return _REF[case['name']]


# ---- the checker ------------------------------------------------------------------------------------------------------------------------------
def check(case, out, what='device'):
    """every element of out [rows][nB] against the case's reference; AssertionError naming the worst element and its error over tolerance"""
    hi, lo, tol = reference(case)
    out = np.asarray(out)
    assert out.shape == hi.shape, (out.shape, hi.shape)
    assert not np.isnan(out).any(), '%s %s: %d NaN in the result, first at %s' % (what, case['name'], np.isnan(out).sum(), np.argwhere(np.isnan(out))[0])
    if case['form'] == ROW_RESIDUAL:
        pad = out[case['M']:]
        assert not pad.any(), '%s %s: rows M .. Mp are not zeros (first at %s)' % (what, case['name'], np.argwhere(pad)[0] + [case['M'], 0])
    if tol is None:
        wrong = out != hi
        assert lo.any() == 0 and not wrong.any(), '%s %s: %d of %d elements differ from the exact value, first at %s: %r for %r' % (
            what, case['name'], wrong.sum(), wrong.size, np.argwhere(wrong)[0], out[tuple(np.argwhere(wrong)[0])], hi[tuple(np.argwhere(wrong)[0])])
        return 0.0
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        err = np.abs((out - hi) - lo)
        ratio = np.where(err == 0, 0.0, err / tol)            # a zero tolerance (a zero column) admits the exact value only
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    n_bad = int((ratio > 1.0).sum())
    assert n_bad == 0, '%s %s: %d of %d elements outside the bound; worst at %s: out %r, exact %r + %r, error %.3e = %.3g of the tolerance %.3e' % (
        what, case['name'], n_bad, ratio.size, worst, out[worst], hi[worst], lo[worst], err[worst], ratio[worst], tol[worst])
    return float(ratio[worst])


def share_outside(case, out):
    """the share of elements at which `out` misses the case's bound (the discrimination condition: float64 `@` must miss it at most elements)"""
    hi, lo, tol = reference(case)
    rows = case['M'] if case['form'] == ROW_RESIDUAL else case['nA']      # the rows below M are zeros by definition, not by arithmetic
    return float(np.mean((np.abs((out - hi) - lo) > tol)[:rows]))


# ---- numpy emulations of the device arithmetic ---------------------------------------------------------------------------------------------
def emulate_dot2(a, B, k0=0, k1=None, drop_lo=False, drop_pe=False):
    """(hi, lo) of ddacc_block / residual_chain over k in [k0, k1): elementwise the device's operations in the device's order"""
    k1 = a.shape[1] if k1 is None else k1
    hi, lo = np.zeros((a.shape[0], B.shape[1])), np.zeros((a.shape[0], B.shape[1]))
    for k in range(k0, k1):
        pr, pe = two_product(a[:, k:k + 1], B[k:k + 1, :])
        t = hi + pr
        bb = t - hi
        if not drop_lo:
            lo = lo + (((hi - (t - bb)) + (pr - bb)) + (0.0 if drop_pe else pe))
        hi = t
    return hi, lo


def emulate_dd(case, fault=None):
    """forms 1 - 3 as the kernels compute them; fault: None, 'lo' (never added), 'pe' (never added), 'sub' (Csub - (hi + lo) instead of (Csub - hi) - lo)"""
    a, B = operand(case)
    kw = dict(drop_lo=fault == 'lo', drop_pe=fault == 'pe')
    if case['form'] == ROW_RESIDUAL:
        M = case['M']
        kper = (M + 3) // 4
        hi, lo = emulate_dot2(a[:M], B, 0, min(M, kper), **kw)
        for r in (1, 2, 3):
            x, xl = emulate_dot2(a[:M], B, min(M, r * kper), min(M, (r + 1) * kper), **kw)
            t = hi + x
            bb = t - hi
            lo = lo + (((hi - (t - bb)) + (x - bb)) + xl)
            hi = t
        out = np.zeros((case['Mp'], case['Dp']))
        out[:M] = (case['Csub'][:M] - hi) - lo if fault != 'sub' else case['Csub'][:M] - (hi + lo)
        return out
    hi, lo = emulate_dot2(a, B, **kw)
    if not case['product']:
        return hi + lo
    return (case['Csub'] - hi) - lo if fault != 'sub' else case['Csub'] - (hi + lo)


def emulate_i8(case, fault=None):
    """gsi8.hip: column scales, ten digits, the 55 exact integer products by order, the two-sum chain; fault: None, 'order' (the last order dropped),
    'weight' (one order's weight off by 128), 'sub'"""
    At, B = case['A'].T, case['B']                        # W's columns: A^T-side and B-side, [K][n]

    def digits(X):
        mx = np.max(np.abs(X), axis=0)
        sc = np.where(mx > 0, np.ldexp(1.0, np.frexp(mx)[1] + 1), 1.0)
        t, q = X / sc, []
        for _ in range(10):
            t = t * 128.0
            r = np.rint(t)
            t = t - r
            q.append(r)
        return sc, q
    sa, qa = digits(At)
    sb, qb = digits(B)
    acc = [np.zeros((At.shape[1], B.shape[1])) for _ in range(10)]
    for da in range(10):
        for db in range(10 - da):
            acc[da + db] += qa[da].T @ qb[db]             # integers below 2^53: exact
    assert max(np.max(np.abs(x)) for x in acc) < 2 ** 31
    sc = sa[:, None] * sb[None, :]
    hi, lo, w = np.zeros_like(sc), np.zeros_like(sc), 2.0 ** -77
    for o in range(9, -1, -1):
        x = acc[o] * (w * (128.0 if fault == 'weight' and o == 6 else 1.0)) * sc
        if fault == 'order' and o == 9:
            x = np.zeros_like(x)
        t = hi + x
        bb = t - hi
        lo = lo + ((hi - (t - bb)) + (x - bb))
        hi = t
        w *= 128.0
    if not case['product']:
        return hi + lo
    return (case['Csub'] - hi) - lo if fault != 'sub' else case['Csub'] - (hi + lo)


def emulate(case, fault=None):
    return emulate_i8(case, fault) if case['form'] == I8 else emulate_dd(case, fault)


# ---- the hook -----------------------------------------------------------------------------------------------------------------------------
SENTINEL_BITS = np.uint64(0xFFFFFFFFFFFFFFFF)


def run_hook(product, form, dims, A=None, B=None, Csub=None, Keep=None, Psi2=None, beta=0.0, jitA=0.0, rows=None, cols=None):
    """gp_debug_dd_product: (status, form that ran, out [rows + 2][cols] or None)"""
    import ctypes
    from gparml_amd import _lib
    lib = _lib.load()
    keep = []

    def ptr(x):
        if x is None:
            return None
        keep.append(np.ascontiguousarray(x, dtype=np.float64))
        return keep[-1].ctypes.data_as(_lib._dp)
    out = np.zeros((max(rows or 0, 0) + 2, max(cols or 1, 1)))
    ran = ctypes.c_int32(-1)
    rc = lib.gp_debug_dd_product(0, int(product), int(form), (ctypes.c_int32 * 6)(*[int(x) for x in dims]), float(beta), float(jitA), ptr(A), ptr(B), ptr(Csub),
                                 ptr(Keep), ptr(Psi2), out.ctypes.data_as(_lib._dp), ctypes.byref(ran))
    return rc, ran.value, out


def run_case(case, form=None):
    """a case through the hook in its own form (or `form`): (status, form that ran, result [rows][nB], sentinel rows [2][nB])"""
    form = case['form'] if form is None else form
    step_shape = form in (0, ROW_RESIDUAL)
    assert form != 0 or case.get('symmetric'), 'the step chooses between forms that read A by rows and by columns: form 0 needs a symmetric A'
    dims = [case.get('M', case['nA']), case.get('Mp', case['nA']), case.get('Dp', case['nB'])] + ([0, 0, 0] if step_shape else [case['nA'], case['nB'], case['K']])
    A = case.get('A')
    if A is not None and form == I8:
        A = A.T
    rc, ran, out = run_hook(case['product'], form, dims, A=A, B=case['B'], Csub=case.get('Csub') if case['product'] else None, Keep=case.get('Keep'),
                            Psi2=case.get('Psi2'), beta=case.get('beta', 0.0), jitA=case.get('jitA', 0.0), rows=case['nA'], cols=case['nB'])
    return rc, ran, out[:-2], out[-2:]


def refusal_cases():
    """name -> (product, form, dims, operands present, a word of the message): what the hook refuses with GP_ERR_BAD_ARG before any HIP call"""
    x = np.zeros(4)
    ops = dict(A=x, B=x, Csub=x, Keep=x, Psi2=x)
    no_c = dict(A=x, B=x)
    return {
        'i8-K-not-32': (0, I8, [0, 0, 0, 64, 64, 48], no_c, 'K = 48'),
        'i8-K-over-2048': (0, I8, [0, 0, 0, 64, 64, 2080], no_c, 'K = 2080'),
        'i8-nA-not-64': (0, I8, [0, 0, 0, 96, 64, 64], no_c, 'nA = 96'),
        'i8-nB-not-64': (1, I8, [0, 0, 0, 64, 32, 64], ops, 'nB = 32'),
        'i8-plane-over-workspace': (0, I8, [0, 0, 0, 4096, 4096, 2048], no_c, 'workspace'),
        'dd-gemm-rows-not-8': (0, DD_GEMM, [0, 0, 0, 100, 64, 64], no_c, 'nA = 100'),
        'dd-gemm-cols-not-64': (0, DD_GEMM, [0, 0, 0, 64, 96, 64], no_c, 'nB = 96'),
        'dd-gemm-K-not-8': (0, DD_GEMM, [0, 0, 0, 64, 64, 12], no_c, 'K = 12'),
        'dd-residual-rows-not-8': (1, DD_RESIDUAL, [0, 0, 0, 12, 64, 64], ops, 'nA = 12'),
        'dd-residual-cols-not-64': (1, DD_RESIDUAL, [0, 0, 0, 64, 32, 64], ops, 'nB = 32'),
        'dd-residual-K-not-8': (1, DD_RESIDUAL, [0, 0, 0, 64, 64, 4], ops, 'K = 4'),
        'dd-residual-without-Csub': (1, DD_RESIDUAL, [0, 0, 0, 64, 64, 64], no_c, 'Csub'),
        'dd-gemm-for-the-residual': (1, DD_GEMM, [0, 0, 0, 64, 64, 64], ops, 'does not compute'),
        'row-for-G': (0, ROW_RESIDUAL, [5, 128, 128, 0, 0, 0], no_c, 'does not compute'),
        'row-Mp-not-128': (1, ROW_RESIDUAL, [5, 64, 128, 0, 0, 0], ops, 'Mp = 64'),
        'row-Dp-not-128': (1, ROW_RESIDUAL, [5, 128, 100, 0, 0, 0], ops, 'Dp = 100'),
        'row-M-over-Mp': (1, ROW_RESIDUAL, [129, 128, 128, 0, 0, 0], ops, 'M = 129'),
        'row-M-zero': (1, ROW_RESIDUAL, [0, 128, 128, 0, 0, 0], ops, 'M = 0'),
        'row-without-Keep': (1, ROW_RESIDUAL, [5, 128, 128, 0, 0, 0], dict(B=x, Csub=x, Psi2=x), 'Keep'),
        'row-with-free-sizes': (1, ROW_RESIDUAL, [5, 128, 128, 64, 64, 64], ops, 'nA, nB, K'),
        'form-5': (0, 5, [0, 0, 0, 64, 64, 64], no_c, 'form'),
        'product-2': (2, DD_GEMM, [0, 0, 0, 64, 64, 64], no_c, 'product'),
        'G-with-Csub': (0, DD_GEMM, [0, 0, 0, 64, 64, 64], ops, 'Csub'),
        'step-choice-at-the-one-panel-tail-G': (0, 0, [128, 128, 128, 0, 0, 0], no_c, 'tail'),
        'step-choice-at-the-one-panel-tail-residual': (1, 0, [128, 128, 128, 0, 0, 0], ops, 'tail'),
        'step-choice-Mp-not-128': (0, 0, [100, 200, 128, 0, 0, 0], no_c, 'Mp = 200'),
        'no-B': (0, DD_GEMM, [0, 0, 0, 64, 64, 64], dict(A=x), 'NULL'),
        'dd-gemm-without-A': (0, DD_GEMM, [0, 0, 0, 64, 64, 64], dict(B=x), 'needs A'),
    }
