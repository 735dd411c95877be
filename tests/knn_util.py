"""The reference of the neighbour search in latent space (gp_knn_rows, csrc/knn.hip; gparml_amd.init.knn): brute force in numpy.

``brute`` is the oracle of the tests: the squared distance of every pair in the direct form sum_q w_q (x_q - t_q)^2, then per query the k least
of the pairs (d2, row) by ``lexsort``.  On inputs with small integer coordinates and weights that are 0, 1 or powers of two every product and
sum is exact in float64, so the device must return these bits.  ``REAL`` is the real-valued case with its long-double distances and the gap rule
(tests/test_knn_merge.py checks, on the CPU, that the rule leaves out at most 1 % of its queries; tests/test_gpu_knn.py holds the device to it)."""
import numpy as np


def sqdist(X, T, weight=None, dtype=np.float64):
    """d2 (n, n_train) in the direct form: the difference first, then w e e summed over q ascending"""
    X, T = np.asarray(X, dtype=dtype), np.asarray(T, dtype=dtype)
    w = np.ones(X.shape[1], dtype=dtype) if weight is None else np.asarray(weight, dtype=dtype)
    d2 = np.zeros((X.shape[0], T.shape[0]), dtype=dtype)
    for q in range(X.shape[1]):
        e = X[:, q, None] - T[None, :, q]
        d2 += (w[q] * e) * e
    return d2


def lists_of(d2, k, skip=None):
    """(dist2 (n, k), rows (n, k)) of a distance table: per query the k least pairs (d2, row); the row ``skip[i]`` (>= 0) is left out; slots
    beyond the available rows hold inf and -1"""
    n, nt = d2.shape
    dist2, rows = np.full((n, k), np.inf), np.full((n, k), -1, dtype=np.int64)
    for i in range(n):
        keep = np.arange(nt)
        if skip is not None and skip[i] >= 0:
            keep = keep[keep != skip[i]]
        order = keep[np.lexsort((keep, d2[i, keep]))][:k]
        dist2[i, :len(order)], rows[i, :len(order)] = d2[i, order], order
    return dist2, rows


def brute(X, T, k, weight=None, skip=None):
    return lists_of(sqdist(X, T, weight), k, skip)


def integer_case(n_train, n, Q, seed):
    """small integer coordinates (|x| <= 8): exact arithmetic, and full of exact ties"""
    rs = np.random.RandomState(seed)
    return rs.randint(-8, 9, size=(n_train, Q)).astype(np.float64), rs.randint(-8, 9, size=(n, Q)).astype(np.float64)


# the real-valued case: (n_train, n, Q, k) and the seed of its normal data
REAL = (700, 300, 10, 8)
REAL_SEED = 11


def real_case():
    n_train, n, Q, k = REAL
    rs = np.random.RandomState(REAL_SEED)
    return rs.randn(n_train, Q), rs.randn(n, Q), k


def real_reference(T, X, k):
    """Long-double distances of the real-valued case: (d2 (n, n_train) longdouble, bound, rows (n, k), decided (n,)).  bound = (Q + 2) 2^-53 is the
    relative rounding bound of the direct form's float64 sum; a query's rows are decided when its k + 1 nearest long-double distances are pairwise
    further apart than twice that bound."""
    Q = X.shape[1]
    d2 = sqdist(X, T, dtype=np.longdouble)
    bound = (Q + 2) * 2.0 ** -53
    order = np.argsort(d2, axis=1, kind='stable')[:, :k + 1]
    near = np.take_along_axis(d2, order, axis=1)
    decided = np.all(near[:, 1:] - near[:, :-1] > 2 * bound * near[:, 1:], axis=1)
    return d2, bound, order[:, :k], decided
