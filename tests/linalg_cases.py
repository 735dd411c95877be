"""The matrices, the modes and the float64 LAPACK references of tests/test_gpu_linalg.py (numpy / scipy only: tests/test_linalg_cases_cpu.py runs this
file without a device)."""
import functools

import numpy as np

OPTIONS = ('trtri_rec', 'xtx_tri', 'gemm_big')         # gp_debug_set_option switches of potrf_inverse_batched; all 1 by default

# (n, batch, workspace, trtri_rec, xtx_tri, gemm_big): the combinations of n in {1, 129, 300, 640, 1100, 1537} x batch x workspace x the three switches that
# change which kernels potrf_inverse_batched launches.  Padded sizes 128, 256, 384, 640, 1152, 1664 = 1, 2, 3, 5, 9, 13 panels.
#  - one panel: no panel solve, no inverse by halves -- only X^T X and its three flags differ
#  - trtri_rec: any size with two panels or more; xtx_tri: every size (tri + klow + mirror on the last product)
#  - the workspace and gemm_big matter from 1024 padded rows on (the 128-tile kernel with split-k: 2 x 81 tiles -> 2 splits, 81 -> 4, 2 x 169 -> 1,
#    169 -> 2); below, the workspace only hands the 32-tile kernel a split count it must ignore
#  - without a workspace the tile count alone picks the kernel: <= 256 tiles of 128 go to the 32-tile kernel (2 x 81, 169), 2 x 169 to the 128-tile one,
#    and so do the trailing updates of the first panel there (2 x 144 tiles) while a single matrix of that size stays on the small tiles throughout
MODES = [
    (1, 1, 0, 1, 1, 1), (1, 2, 0, 1, 0, 1),
    (129, 2, 1, 1, 1, 1), (129, 1, 0, 0, 0, 1),
    (300, 2, 1, 1, 1, 1), (300, 2, 0, 0, 1, 1), (300, 1, 1, 1, 0, 1),
    (640, 2, 1, 1, 1, 1), (640, 1, 0, 0, 0, 1), (640, 2, 0, 1, 0, 1),
    (1100, 2, 1, 1, 1, 1), (1100, 1, 1, 1, 1, 1), (1100, 2, 1, 1, 0, 1), (1100, 2, 1, 1, 1, 0), (1100, 2, 0, 0, 1, 1),
    (1537, 2, 1, 1, 1, 1), (1537, 1, 1, 1, 1, 1), (1537, 2, 0, 1, 1, 1), (1537, 1, 0, 0, 0, 1),
]


@functools.lru_cache(maxsize=None)
def well_conditioned(n, b=0):
    """the family of test_cholesky_and_inverse (entry 0 is its matrix); read-only"""
    rs = np.random.RandomState(n + 1000 * b)
    X = rs.randn(n, n + 5)
    A = X.dot(X.T) / n + 0.1 * np.eye(n)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def well_conditioned_ref(n, b=0):
    """float64 LAPACK: (L, A^-1, log det)"""
    A = well_conditioned(n, b)
    return np.linalg.cholesky(A), np.linalg.inv(A), np.linalg.slogdet(A)[1]


ILL_C = (6, 8, 10)
ILL_N = (300, 1100)


@functools.lru_cache(maxsize=None)
def ill_conditioned(n, c, b=0):
    """A = Q diag(logspace(0, -c, n)) Q^T, symmetrised: condition number 10^c"""
    rs = np.random.RandomState(7 * n + c + 1000 * b)
    Q, _ = np.linalg.qr(rs.randn(n, n))
    A = (Q * np.logspace(0, -c, n)).dot(Q.T)
    A = (A + A.T) / 2
    A.setflags(write=False)
    return A


def residuals(A, L, Ainv):
    """(max|A - L L^T| / max|A|, max|A Ainv - I|)"""
    return np.max(np.abs(A - L.dot(L.T))) / np.max(np.abs(A)), np.max(np.abs(A.dot(Ainv) - np.eye(A.shape[0])))


@functools.lru_cache(maxsize=None)
def lapack_residuals(n, c, b=0):
    """the residuals of float64 LAPACK's own Cholesky factor and Cholesky-based inverse (dpotrf, dpotri) of the same matrix"""
    from scipy.linalg import lapack
    A = ill_conditioned(n, c, b)
    L, info = lapack.dpotrf(A, lower=1, clean=1)
    assert info == 0, 'LAPACK does not factorise the matrix (info %d)' % info
    Ai, info = lapack.dpotri(L, lower=1)
    assert info == 0
    Ai = np.tril(Ai) + np.tril(Ai, -1).T
    return residuals(A, L, Ai)
