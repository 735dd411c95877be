"""What one internal matrix product means (csrc/gp_common.h, GemmP), restated in plain numpy on host arrays, and the table of cases
tests/test_gpu_gemm_modes.py runs through gp_debug_gemm_modes (run_case at the end is the one caller of the hook).  tests/test_gemm_ref_cpu.py
checks the reference, the table and the hook's refusals on the CPU.

A case is a dict:
  la, lb          'K' (operand stored [free][k], k contiguous) or 'F' (stored [k][free])
  m, n, K         sizes of the product; inner, outer: the two batch counts (entry bz = i + inner * o)
  A, B, C         windows: dict(parent=name, off=element offset of entry 0, ld=, s=inner stride, o=outer stride)
  parents         name -> length in doubles (operands and result may share a parent)
  alpha, beta, tri, klow, mirror, splits, big
  amax, bmax      bound on |operand entries| (4 unless an operand is the result of an earlier product)

Semantics, as a statement about elements, for every batch entry:
  R = alpha * op(A) op(B) + beta * C0   on the m x n window of C
  tri = 0: C = R.   tri = 1: C(r,c) = R(r,c) for r >= c; for r < c it is R(r,c) or C0(r,c) (the kernels skip whole tiles of different sizes).
  tri = 2: the same with r <= c.   mirror (needs tri = 1, beta = 0, R symmetric): C = R everywhere, so C is exactly symmetric.
  klow promises that both operands are zero for k < free index and changes nothing about R.
  Nothing outside the C windows is written; nothing outside the operand windows is read.

Exact inputs: operands integer-valued in [-4, 4], C0 integer-valued, alpha and beta from {1, -1, 1.5, -0.5, 0}: every product and partial sum is
an integer (or half-integer) far below 2^53, so float64 `@` is the exact answer whatever the summation order, with or without FMA, split or not,
and the device must reproduce it bit for bit (the sign of an exact zero excepted: -1 * 0 and 0 - 0 differ there and it is no property of the product)."""
import numpy as np

NB = 128
SENTINEL = -12345.0


def win(parent, off, ld, s=0, o=0):
    return dict(parent=parent, off=int(off), ld=int(ld), s=int(s), o=int(o))


def shapes(case):
    """(rows, cols) of the stored A, B and C windows"""
    m, n, K = case['m'], case['n'], case['K']
    return {'A': (m, K) if case['la'] == 'K' else (K, m), 'B': (n, K) if case['lb'] == 'K' else (K, n), 'C': (m, n)}


def entries(case):
    return [(i, o) for o in range(case['outer']) for i in range(case['inner'])]          # bz = i + inner * o


def window_index(case, which, i, o):
    """flat indices (rows, cols) of batch entry (i, o)'s window inside its parent"""
    w = case[which]
    rows, cols = shapes(case)[which]
    return w['off'] + i * w['s'] + o * w['o'] + np.arange(rows)[:, None] * w['ld'] + np.arange(cols)[None, :]


def finish(case):
    """fills in the defaults and sizes every parent to hold its windows plus two rows of surroundings"""
    for k, v in dict(inner=1, outer=1, alpha=1.0, beta=0.0, tri=0, klow=0, mirror=0, splits=1, big=0, amax=4.0, bmax=4.0).items():
        case.setdefault(k, v)
    need = dict(case.get('parents', {}))
    for which in 'ABC':
        w = case[which]
        end = max(int(window_index(case, which, i, o)[-1, -1]) + 1 for i, o in entries(case))
        need[w['parent']] = max(need.get(w['parent'], 0), end + 2 * w['ld'])
    case['parents'] = need
    return case


def make_buffers(case, seed, exact=True, given=None):
    """parent name -> array.  NaN everywhere in a parent that holds an operand, SENTINEL in one that holds only C; the operand windows integer-valued
    in [-4, 4] (lower-triangular in k >= free under klow), C's windows integer-valued.  exact = False: standard normals instead.  given: parents to
    take as they are (the result of an earlier product)."""
    rs = np.random.RandomState(seed)
    given = given or {}
    bufs = {}
    op_parents = {case['A']['parent'], case['B']['parent']}
    for name, length in case['parents'].items():
        if name in given:
            assert given[name].size == length
            bufs[name] = given[name].copy()
        else:
            bufs[name] = np.full(length, np.nan if name in op_parents else SENTINEL)
    draw = (lambda shape: rs.randint(-4, 5, size=shape).astype(np.float64)) if exact else (lambda shape: rs.randn(*shape))
    for which in 'ABC':
        if case[which]['parent'] in given:
            continue
        if which == 'B' and case['B'] == case['A'] and shapes(case)['A'] == shapes(case)['B']:
            continue                                                  # the very same windows (X^T X, the trailing update): filled once
        rows, cols = shapes(case)[which]
        for i, o in entries(case):
            v = draw((rows, cols))
            if case['klow'] and which != 'C':
                v = np.tril(v)                                           # stored [k][free]: zero for k < free
            bufs[case[which]['parent']][window_index(case, which, i, o)] = v
    return bufs


def gemm_modes_ref(case, bufs, dtype=np.float64):
    """The C parent after the call as far as it is determined, and two masks over it:
    returns (ref, must, may).  ref: C's parent with R in every window (the initial content elsewhere); must: elements that have to equal ref;
    may: elements that equal ref or their initial value.  Everything else has to keep its initial bits."""
    C0 = bufs[case['C']['parent']]
    ref = C0.astype(dtype)
    must = np.zeros(C0.size, dtype=bool)
    may = np.zeros(C0.size, dtype=bool)
    m, n = case['m'], case['n']
    r, c = np.arange(m)[:, None], np.arange(n)[None, :]
    keep = {0: np.ones((m, n), dtype=bool), 1: r >= c, 2: r <= c}[case['tri']]
    if case['mirror']:
        assert case['tri'] == 1 and case['beta'] == 0 and m == n
        keep = np.ones((m, n), dtype=bool)
    for i, o in entries(case):
        a = bufs[case['A']['parent']][window_index(case, 'A', i, o)].astype(dtype)
        b = bufs[case['B']['parent']][window_index(case, 'B', i, o)].astype(dtype)
        opa = a if case['la'] == 'K' else a.T                            # (m, K)
        opb = b.T if case['lb'] == 'K' else b                            # (K, n)
        ci = window_index(case, 'C', i, o)
        R = dtype(case['alpha']) * opa.dot(opb)
        if case['beta'] != 0:
            R = R + dtype(case['beta']) * C0[ci].astype(dtype)
        ref[ci] = R
        must[ci[keep]] = True
        may[ci[~keep]] = True
    return ref, must, may


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same_value_bits(x, y):
    """bit equality with -0.0 read as 0.0 (x + 0.0 is +0.0 for either zero and x itself otherwise, NaN payloads included)"""
    return bits(x + 0.0) == bits(y + 0.0)


def check_exact(case, bufs, out):
    """out: C's parent as the device left it.  Asserts the four statements of the module docstring, bit for bit."""
    C0 = bufs[case['C']['parent']]
    ref, must, may = gemm_modes_ref(case, bufs)
    outside = ~(must | may)
    assert np.array_equal(bits(out)[outside], bits(C0)[outside]), 'an element outside the C windows changed (%d)' % np.sum(bits(out)[outside] != bits(C0)[outside])
    eq = same_value_bits(out, ref)
    assert eq[must].all(), '%d of %d required elements differ from the exact product (first flat index %d)' % (np.sum(~eq[must]), must.sum(), np.flatnonzero(must & ~eq)[0])
    free_ok = eq | (bits(out) == bits(C0))
    assert free_ok[may].all(), '%d elements of the skipped triangle are neither the product nor their initial value' % np.sum(~free_ok[may])
    if case['mirror']:
        for i, o in entries(case):
            w = out[window_index(case, 'C', i, o)]
            assert np.array_equal(bits(w), bits(w.T.copy())), 'mirrored result is not symmetric'


def rounding_bound(case, bufs):
    """elementwise bound on |device - exact| for real inputs, over C's parent (zero outside the windows): K products summed in any order, each
    rounded once or fused, then alpha and beta applied -- at most K + 2 roundings of relative size 2^-53 on a quantity bounded by
    |alpha| |A||B| + |beta| |C0| (Higham, Accuracy and Stability of Numerical Algorithms, section 3.5, with gamma_k ~ k u)"""
    C0 = bufs[case['C']['parent']]
    bound = np.zeros(C0.size)
    for i, o in entries(case):
        a = np.abs(bufs[case['A']['parent']][window_index(case, 'A', i, o)])
        b = np.abs(bufs[case['B']['parent']][window_index(case, 'B', i, o)])
        ci = window_index(case, 'C', i, o)
        mag = abs(case['alpha']) * (a if case['la'] == 'K' else a.T).dot(b.T if case['lb'] == 'K' else b) + abs(case['beta']) * np.abs(C0[ci])
        bound[ci] = (case['K'] + 2) * 2.0 ** -53 * mag
    return bound


def exactness_bound(case):
    """largest magnitude any partial sum or the result can reach with the case's integer-valued inputs; exact in float64 while below 2^53 (the factors 2
    keep the half-integers of alpha, beta = 1.5, -0.5 integer)"""
    return 2 * (abs(case['alpha']) * case['K'] * case['amax'] * case['bmax'] + abs(case['beta']) * 4.0)


# ---- the table --------------------------------------------------------------------------------------------------------------------------
LAYOUTS = [('K', 'K'), ('K', 'F'), ('F', 'K'), ('F', 'F')]
ALPHA_BETA = [(1.0, 0.0), (-1.0, 1.0), (1.5, -0.5)]


def windowed(la, lb, m, n, K, batch=1, **mode):
    """every operand a window of its own parent with ld = cols + 128, three rows and ten columns in, four rows between the batch entries"""
    case = dict(la=la, lb=lb, m=m, n=n, K=K, inner=batch, **mode)
    for which, (rows, cols) in shapes(case).items():
        ld = cols + 128
        case[which] = win('P' + which, 3 * ld + 10, ld, s=(rows + 4) * ld)
    return finish(case)


def grid_cases():
    """four layouts x both kernels x tri x alpha/beta at 384 x 384 (3 x 3 tiles of 128: a diagonal, a lower and an upper tile, an odd count), K = 400:
    three full chunks of the 32-tile kernel's 128 and a partial one"""
    out = {}
    for la, lb in LAYOUTS:
        for big in (0, 1):
            for tri in (0, 1, 2):
                for alpha, beta in ALPHA_BETA:
                    out['grid-%s%s-big%d-tri%d-a%g-b%g' % (la, lb, big, tri, alpha, beta)] = windowed(la, lb, 384, 384, 400, big=big, tri=tri, alpha=alpha, beta=beta)
    return out


def xtx_case(K, splits, big, plain=False):
    """A^-1 = X^T X as the blocked inverse launches it: both operands the same [k][free] windows, batch 2, lower tiles from their first non-zero k, mirrored;
    plain: the same operands as an ordinary full product"""
    ld = K + 128
    X = win('X', 3 * ld + 10, ld, s=(K + 4) * ld)
    case = dict(la='F', lb='F', m=K, n=K, K=K, inner=2, A=X, B=dict(X), C=win('PC', 3 * ld + 10, ld, s=(K + 4) * ld), splits=splits, big=big)
    if not plain:
        case.update(tri=1, klow=1, mirror=1)
    return finish(case)


XTX_SIZES = (384, 640, 1024)
XTX_RUNS = [(1, 1), (2, 1), (4, 1), (8, 1), (1, 0)]                     # (splits, big)


def xtx_cases():
    return {'xtx-%d-s%d-big%d' % (K, s, big): xtx_case(K, s, big) for K in XTX_SIZES for s, big in XTX_RUNS}


def splitk_beta_cases():
    out = {}
    for la, lb in (('K', 'F'), ('K', 'K')):                             # the global step's two
        for splits in (2, 8):
            for tri in (0, 1):
                out['splitk-%s%s-s%d-tri%d' % (la, lb, splits, tri)] = windowed(la, lb, 384, 384, 384, batch=2, big=1, splits=splits, tri=tri, alpha=1.5, beta=-0.5)
    return out


CHOL_MP = 640                                                            # five panels: a block count that is no power of two


def chol_panel_case(j, big=0):
    """panel solve j of the blocked Cholesky, batch 2: L[i,j] = A[i,j] inv(L_jj)^T into the packed work panel"""
    Mp, ld, bs = CHOL_MP, CHOL_MP, CHOL_MP * CHOL_MP
    rem = Mp // NB - j - 1
    return finish(dict(la='K', lb='K', m=rem * NB, n=NB, K=NB, inner=2, big=big, parents={'Amat': 2 * bs, 'Linv': 2 * bs, 'Twork': bs},
                       A=win('Amat', (j + 1) * NB * ld + j * NB, ld, s=bs), B=win('Linv', j * NB * ld + j * NB, ld, s=bs), C=win('Twork', 0, NB, s=rem * NB * NB)))


def chol_trailing_case(j, big=0):
    """trailing update j: A[i,k] -= L[i,j] L[k,j]^T on the lower tiles; A == B, and C a window of the same matrix"""
    Mp, ld, bs = CHOL_MP, CHOL_MP, CHOL_MP * CHOL_MP
    rem = Mp // NB - j - 1
    P = win('Amat', (j + 1) * NB * ld + j * NB, ld, s=bs)
    return finish(dict(la='K', lb='K', m=rem * NB, n=rem * NB, K=NB, inner=2, big=big, alpha=-1.0, beta=1.0, tri=1, parents={'Amat': 2 * bs},
                       A=P, B=dict(P), C=win('Amat', (j + 1) * NB * ld + (j + 1) * NB, ld, s=bs)))


def trtri_levels(Mp=CHOL_MP):
    """(h, p0, np, rows2) of every launch pair of the inverse factor by halves"""
    nt, out, h = Mp // NB, [], 1
    while h < nt:
        full, rem = nt // (2 * h), nt - (nt // (2 * h)) * 2 * h - h
        if full > 0:
            out.append((h, 0, full, h))
        if rem > 0:
            out.append((h, full, 1, rem))
        h *= 2
    return out


def trtri_cases(h, p0, np_, rows2):
    """the two launches of one level: T = L21 X11 into the packed work panel, then X21 = -X22 T from it; inner batch = the pairs of halves (np_), outer = 2"""
    Mp, ld, bs = CHOL_MP, CHOL_MP, CHOL_MP * CHOL_MP
    b, ps, m2 = h * NB, 2 * h * NB * (ld + 1), rows2 * NB
    o11 = 2 * p0 * h * NB * (ld + 1)
    o22, o21 = o11 + b * (ld + 1), o11 + b * ld
    T = win('Twork', 0, b, s=m2 * b, o=np_ * m2 * b)
    common = dict(la='K', lb='F', m=m2, n=b, inner=np_, outer=2)
    p = finish(dict(common, K=b, parents={'Amat': 2 * bs, 'Linv': 2 * bs, 'Twork': bs},
                    A=win('Amat', o21, ld, s=ps, o=bs), B=win('Linv', o11, ld, s=ps, o=bs), C=T))
    q = finish(dict(common, K=m2, alpha=-1.0, bmax=16.0 * b, parents={'Linv': 2 * bs, 'Twork': bs},
                    A=win('Linv', o22, ld, s=ps, o=bs), B=dict(T), C=win('Linv', o21, ld, s=ps, o=bs)))
    return p, q


def predict_case():
    """[Lk^-1 k* | La^-1 k*] = Psi1* Linv^T of gp_predict / gp_infer: n = 2 Mp"""
    return windowed('K', 'K', 128, 2 * 256, 256)


def rounding_case(la, lb, big):
    return windowed(la, lb, 256, 256, 272, big=big, alpha=1.5, beta=-0.5)


def all_exact_cases():
    out = {}
    out.update(grid_cases())
    out.update(xtx_cases())
    for K in XTX_SIZES:
        for big in (0, 1):
            out['xtx-plain-%d-big%d' % (K, big)] = xtx_case(K, 1, big, plain=True)
    out.update(splitk_beta_cases())
    for big in (0, 1):
        out['chol-panel-big%d' % big] = chol_panel_case(1, big)
        out['chol-trailing-big%d' % big] = chol_trailing_case(1, big)
    for lv in trtri_levels():
        p, q = trtri_cases(*lv)
        out['trtri-h%d-np%d-T' % (lv[0], lv[2])] = p
        out['trtri-h%d-np%d-X21' % (lv[0], lv[2])] = q
    out['predict'] = predict_case()
    return out


# ---- the hook -----------------------------------------------------------------------------------------------------------------------------
def run_case(case, bufs):
    """gp_debug_gemm_modes on copies of the parents: returns (status, C's parent afterwards).  Parents shared by name go in as one host pointer."""
    import ctypes
    from gparml_amd import _lib
    lib = _lib.load()
    host = {name: np.ascontiguousarray(bufs[name], dtype=np.float64).copy() for name in case['parents']}
    w = [case[x] for x in 'ABC']
    geom = [x['ld'] for x in w] + [x['s'] for x in w] + [x['o'] for x in w] + [x['off'] for x in w] + [host[x['parent']].size for x in w]
    mode = [case['tri'], case['klow'], case['mirror'], case['splits'], case['big']]
    ptr = [host[x['parent']].ctypes.data_as(_lib._dp) for x in w]
    rc = lib.gp_debug_gemm_modes(0, int(case['la'] == 'K'), int(case['lb'] == 'K'), case['m'], case['n'], case['K'], case['inner'], case['outer'],
                                 (ctypes.c_long * 15)(*geom), case['alpha'], case['beta'], (ctypes.c_int32 * 5)(*mode), *ptr)
    return rc, host[case['C']['parent']]


def refusal_cases():
    """name -> (case, a word of the message): everything the hook must refuse with GP_ERR_BAD_ARG before it touches a device"""
    base = lambda **kw: windowed('K', 'F', 384, 384, 384, **kw)
    out = {'m-unaligned': (dict(base(), m=320 + 32), 'unaligned'), 'n-unaligned': (dict(base(), n=100), 'unaligned'), 'k-unaligned': (dict(base(), K=376), 'unaligned'),
           'splits-5-of-24-chunks': (base(big=1, splits=5), 'splits'),
           'splits-3-under-klow': (dict(xtx_case(384, 1, 1), splits=3), 'splits'),            # 24 chunks on the first tile column, 16 on the second
           'splits-16-under-klow': (dict(xtx_case(384, 1, 1), splits=16), 'splits'),
           'mirror-with-beta': (dict(xtx_case(384, 1, 1), beta=1.0), 'mirror'),
           'mirror-with-beta-small-tiles': (dict(xtx_case(384, 1, 0), beta=-0.5), 'mirror')}
    inplace = chol_panel_case(1)
    inplace['C'] = dict(inplace['A'])                                                           # the panel solve in place, as before round 6
    out['panel-solve-in-place'] = (inplace, 'overlaps')
    trailing = chol_trailing_case(1)
    trailing['C'] = win('Amat', trailing['A']['off'] + 64, trailing['A']['ld'], s=trailing['A']['s'])   # half a panel to the right: shares 64 columns with it
    out['trailing-update-on-its-panel'] = (trailing, 'overlaps')
    other_ld = chol_panel_case(1)
    other_ld['C'] = win('Amat', other_ld['A']['off'] + NB, NB, s=other_ld['A']['s'])          # another leading dimension inside the operand's address range
    out['ranges-intersect-other-ld'] = (other_ld, 'overlaps')
    batches = base(batch=2)
    batches['C'] = dict(batches['C'], s=128 * batches['C']['ld'])
    out['c-windows-of-two-entries-overlap'] = (batches, 'overlap')
    past = base()
    past['parents'] = dict(past['parents'], PA=past['parents']['PA'] - 3 * past['A']['ld'])
    out['window-past-its-parent'] = (past, 'past')
    odd = base()
    odd['B'] = dict(odd['B'], off=odd['B']['off'] + 1)
    out['odd-offset'] = (odd, 'even')
    return out
