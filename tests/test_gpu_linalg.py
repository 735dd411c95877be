"""The library's dense FP64 building blocks against numpy (run with -m gpu): the MFMA GEMM core in all four operand layouts -- the
32x32-tile kernel the global step uses for small grids and the 128x128-tile kernel for large ones -- and the blocked Cholesky + inverse."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _gemm(ta, tb, m, n, k, alpha, A, B, beta, C):
    from gparml_amd import _lib
    lib = _lib.load()
    A, pa = _lib.as_c(A)
    B, pb = _lib.as_c(B)
    C = np.ascontiguousarray(C, dtype=np.float64).copy()
    rc = lib.gp_debug_gemm(0, ta, tb, m, n, k, alpha, pa, pb, beta, C.ctypes.data_as(_lib._dp))
    _lib.raise_for(rc, lib, None, 'gp_debug_gemm')
    return C


@pytest.mark.parametrize('ta,tb', [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize('m,n,k', [(100, 70, 50), (512, 512, 512), (300, 129, 1000), (3000, 3000, 40)])
def test_gemm_layouts(ta, tb, m, n, k):
    """(3000, 3000): 24 x 24 = 576 tiles of 128 -> the 128x128-tile kernel; the others (<= 256 such tiles) -> the 32x32-tile kernel."""
    rs = np.random.RandomState(m + n + k + 2 * ta + tb)
    A = rs.randn(k, m) if ta else rs.randn(m, k)
    B = rs.randn(n, k) if tb else rs.randn(k, n)
    C0 = rs.randn(m, n)
    ref = 1.5 * (A.T if ta else A).dot(B.T if tb else B) - 0.5 * C0
    out = _gemm(ta, tb, m, n, k, 1.5, A, B, -0.5, C0)
    assert np.max(np.abs(out - ref)) <= 1e-12 * np.max(np.abs(ref)) * np.sqrt(k)


@pytest.mark.parametrize('n', [1, 100, 128, 300, 640, 700, 900, 1100, 1400])     # 1, 1, 1, 3, 5, 6, 8, 9, 11 panels of 128: the inverse factor by halves meets truncated pairs at every level
def test_cholesky_and_inverse(n):
    from gparml_amd import _lib
    lib = _lib.load()
    rs = np.random.RandomState(n)
    X = rs.randn(n, n + 5)
    A = X.dot(X.T) / n + 0.1 * np.eye(n)
    A_c, pa = _lib.as_c(A)
    L, Ainv = np.zeros((n, n)), np.zeros((n, n))
    logdet = ctypes.c_double()
    rc = lib.gp_debug_potrf_inverse(0, n, pa, L.ctypes.data_as(_lib._dp), Ainv.ctypes.data_as(_lib._dp), ctypes.byref(logdet))
    _lib.raise_for(rc, lib, None, 'gp_debug_potrf_inverse')
    Lr = np.linalg.cholesky(A)
    assert np.max(np.abs(L - Lr)) <= 1e-11 * np.max(np.abs(Lr))
    assert np.max(np.abs(Ainv - np.linalg.inv(A))) <= 1e-9 * np.max(np.abs(Ainv))
    assert abs(logdet.value - np.linalg.slogdet(A)[1]) <= 1e-10 * max(1.0, abs(logdet.value))
    A[0, 0] = -1.0
    A_c, pa = _lib.as_c(A)
    assert lib.gp_debug_potrf_inverse(0, n, pa, None, None, None) == _lib.GP_ERR_NOT_PD


# ---- the blocked Cholesky + inverse as the global step runs it: batched, with the split-k workspace, under every switch -----------------
import contextlib      # noqa: E402

import linalg_cases as LC      # noqa: E402

from gemm_ref import bits      # noqa: E402


@contextlib.contextmanager
def _options(**kw):
    """process-wide switches (all 1 by default), restored whatever happens"""
    from gparml_amd import _lib
    lib = _lib.load()
    try:
        for k, v in kw.items():
            assert lib.gp_debug_set_option(k.encode(), int(v)) == _lib.GP_OK
        yield
    finally:
        for k in LC.OPTIONS:
            lib.gp_debug_set_option(k.encode(), 1)


def _potrf_batched(mats, workspace):
    """gp_debug_potrf_inverse_batched: (status, fail mask, L, Ainv, logdet), the arrays [batch][n][n] / [batch]"""
    from gparml_amd import _lib
    lib = _lib.load()
    A = np.ascontiguousarray(np.stack(mats), dtype=np.float64)
    batch, n = A.shape[0], A.shape[1]
    L, Ainv, logdet = np.full(A.shape, np.nan), np.full(A.shape, np.nan), np.full(batch, np.nan)
    mask = ctypes.c_int32(-1)
    rc = lib.gp_debug_potrf_inverse_batched(0, n, batch, int(workspace), A.ctypes.data_as(_lib._dp), L.ctypes.data_as(_lib._dp), Ainv.ctypes.data_as(_lib._dp),
                                            logdet.ctypes.data_as(_lib._dp), ctypes.byref(mask))
    return rc, mask.value, L, Ainv, logdet


def _same_bits(x, y):
    return np.array_equal(bits(x), bits(y))


@pytest.mark.parametrize('n,batch,workspace,rec,xtx,big', LC.MODES)
def test_cholesky_and_inverse_modes(n, batch, workspace, rec, xtx, big):
    """every combination of size, batch, workspace and switches that changes the launch sequence (linalg_cases.MODES says which and why), against float64
    LAPACK at the tolerances of test_cholesky_and_inverse, entry by entry"""
    mats = [LC.well_conditioned(n, b) for b in range(batch)]
    with _options(trtri_rec=rec, xtx_tri=xtx, gemm_big=big):
        rc, mask, L, Ainv, logdet = _potrf_batched(mats, workspace)
    assert (rc, mask) == (0, 0)
    for b in range(batch):
        Lr, Ar, ldr = LC.well_conditioned_ref(n, b)
        assert np.max(np.abs(L[b] - Lr)) <= 1e-11 * np.max(np.abs(Lr))
        assert np.max(np.abs(Ainv[b] - Ar)) <= 1e-9 * np.max(np.abs(Ainv[b]))
        assert abs(logdet[b] - ldr) <= 1e-10 * max(1.0, abs(logdet[b]))
        assert _same_bits(Ainv[b], Ainv[b].T.copy()) or not xtx        # the mirrored store makes the inverse exactly symmetric


@pytest.mark.parametrize('n,workspace', [(300, 1), (640, 0), (1100, 0), (1100, 1), (1537, 1)])
def test_xtx_tri_gives_the_same_bits(n, workspace):
    """linalg.hip, g_opt_xtx_tri: "bit-identical" -- the lower tiles from their first non-zero k, mirrored, against the full product (32-tile kernel at 300, 640 and
    1100 without the workspace; 128-tile kernel with 2 and 1 splits at 1100 and 1537 with it).
    [1100-1] is the one case with split-k, the production path at M >= 1024: the splits of a klow tile keep the full product's k boundaries (gemm128_kernel).
    When they shared the k that is left, K - klo, instead, 2000711 of 2420000 elements of the two inverses differed in bits (max 6.2e-15, entries ~10)."""
    mats = [LC.well_conditioned(n, b) for b in range(2)]
    with _options(xtx_tri=1):
        on = _potrf_batched(mats, workspace)
    with _options(xtx_tri=0):
        off = _potrf_batched(mats, workspace)
    assert on[:2] == (0, 0) and off[:2] == (0, 0)
    diff = bits(on[3]) != bits(off[3])
    print('xtx_tri on/off at n = %d, workspace %d: %d of %d elements of the inverse differ in bits, max |diff| %.3e' % (n, workspace, diff.sum(), diff.size, np.max(np.abs(on[3] - off[3]))))
    assert _same_bits(on[2], off[2]) and _same_bits(on[4], off[4])
    assert not diff.any()


@pytest.mark.parametrize('n,workspace', [(1, 0), (129, 1), (300, 1), (640, 1), (1100, 0), (1537, 1)])
def test_batch_entry_equals_the_matrix_alone_and_a_repeat_equals_itself(n, workspace):
    """entry b of a batch-2 call against the same matrix run alone, where both take the same kernels with the same split count (up to 896 rows always; at 1100 without
    the workspace: 32-tile kernel either way).  At 1537 with the workspace only the factor and the log-determinant: X^T X is split 2 ways alone and not at all
    in the batch, so the inverse may differ in rounding; the factor is the same bits although the first trailing update moves to the 128-tile kernel with the
    batch's tile count.  And the same call twice gives the same bits."""
    mats = [LC.well_conditioned(n, b) for b in range(2)]
    both = _potrf_batched(mats, workspace)
    again = _potrf_batched(mats, workspace)
    assert both[:2] == (0, 0) and again[:2] == (0, 0)
    for k in (2, 3, 4):
        assert _same_bits(both[k], again[k]), 'a repeated call differs in output %d' % k
    for b in range(2):
        solo = _potrf_batched([mats[b]], workspace)
        assert solo[:2] == (0, 0)
        same = [_same_bits(both[k][b], solo[k][0]) for k in (2, 3, 4)]
        print('n = %d, workspace %d, entry %d: L / Ainv / logdet equal to the solo run in bits: %s' % (n, workspace, b, same))
        assert same[0] and same[2]
        if n <= 1100:
            assert same[1]


def _indefinite(A, where):
    B = A.copy()
    i = 0 if where == 'first' else B.shape[0] - 1
    B[i, i] = -1.0
    return B


@pytest.mark.parametrize('where', ['first', 'last'])
@pytest.mark.parametrize('n,workspace', [(300, 1), (1100, 1)])
def test_fail_mask_and_the_neighbour_of_a_failing_entry(n, workspace, where):
    """bit b of the mask for batch entry b (a negative pivot in the first or in the last panel), GP_ERR_NOT_PD, and the other entry's L, Ainv and logdet
    bit-identical to a clean batch-2 call's (and, at 300 rows where the launch sequence is the same, to its solo run)"""
    from gparml_amd import _lib
    good = [LC.well_conditioned(n, b) for b in range(2)]
    bad = [_indefinite(a, where) for a in good]
    clean = _potrf_batched(good, workspace)
    assert clean[:2] == (0, 0)
    for mats, mask, ok in (([good[0], bad[1]], 2, 0), ([bad[0], good[1]], 1, 1)):
        rc, got, L, Ainv, logdet = _potrf_batched(mats, workspace)
        assert (rc, got) == (_lib.GP_ERR_NOT_PD, mask)
        assert 'fail mask %d' % mask in _lib.load().gp_last_error(None).decode()
        assert _same_bits(L[ok], clean[2][ok]) and _same_bits(Ainv[ok], clean[3][ok]) and _same_bits(logdet[ok], clean[4][ok])
        if n == 300:
            solo = _potrf_batched([good[ok]], workspace)
            assert _same_bits(L[ok], solo[2][0]) and _same_bits(Ainv[ok], solo[3][0]) and _same_bits(logdet[ok], solo[4][0])
    rc, got = _potrf_batched(bad, workspace)[:2]
    assert (rc, got) == (_lib.GP_ERR_NOT_PD, 3)


ILL_MARGIN = 4.0


@pytest.mark.parametrize('c', LC.ILL_C)
@pytest.mark.parametrize('n', LC.ILL_N)
def test_ill_conditioned_residuals(n, c):
    """A = Q diag(logspace(0, -c, n)) Q^T, condition 1e6, 1e8, 1e10 (the headline problem's matrix: 1.4e10), batch 2, with the workspace: a forward comparison
    means nothing here, so the residuals max|A - L L^T| / max|A| and max|A Ainv - I| against those of float64 LAPACK (dpotrf, dpotri) on the same matrix,
    times ILL_MARGIN.  The margin is not derived -- the panel solve multiplies by an explicit inv(L11), which has no textbook backward bound -- but measured
    on the MI355X and rounded up to the next power of two; a ratio above 16 would be a finding about the panel solve, not a reason to raise it.
    Measured device / LAPACK ratios (factor residual; inverse residual), worst of the two batch entries:
      n = 300:  cond 1e6 1.00; 1.72   cond 1e8 1.00; 1.88   cond 1e10 1.14; 2.53
      n = 1100: cond 1e6 2.29; 0.85   cond 1e8 2.80; 1.16   cond 1e10 1.78; 1.51
    Worst 2.80 -> margin 4.  (LAPACK itself: factor residual 8e-16 .. 1.4e-15, inverse residual 1e-11, 1e-9, 1e-7 by condition.)"""
    mats = [LC.ill_conditioned(n, c, b) for b in range(2)]
    rc, mask, L, Ainv, logdet = _potrf_batched(mats, 1)
    assert (rc, mask) == (0, 0)
    for b in range(2):
        dev = LC.residuals(mats[b], L[b], Ainv[b])
        lap = LC.lapack_residuals(n, c, b)
        print('ill-conditioned n = %d, cond 1e%d, entry %d: |A - LL^T| device %.3e LAPACK %.3e ratio %.2f; |A Ainv - I| device %.3e LAPACK %.3e ratio %.2f'
              % (n, c, b, dev[0], lap[0], dev[0] / lap[0], dev[1], lap[1], dev[1] / lap[1]))
        assert dev[0] <= ILL_MARGIN * lap[0] and dev[1] <= ILL_MARGIN * lap[1]
