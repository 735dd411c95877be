"""Shared by tests/test_kmeans_host.py and tests/test_gpu_kmeans.py: the blob data sets, a numpy stand-in for ShardEngine.kmeans_accumulate and the
numpy recomputation of a pass (float64, the direct form sum_q (x_q - z_q)^2)."""
import numpy as np

# (N, Q, K, B, RandomState seed): B blob centres 4 randn(B, Q), rows = a centre + 0.3 randn, seeds = K distinct rows.  Case 1 loses one empty
# cluster on the way (64 -> 63 centres).
BLOBS = [(20000, 10, 64, 40, 0), (5000, 3, 33, 12, 1), (3000, 2, 16, 16, 2)]


def blob_case(N, Q, K, B, seed):
    rs = np.random.RandomState(seed)
    centres = 4.0 * rs.randn(B, Q)
    X = centres[rs.randint(B, size=N)] + 0.3 * rs.randn(N, Q)
    seeds = X[rs.choice(N, K, replace=False)].copy()
    return X, seeds


def sqdist(X, C, block=4096):
    """(n, K) squared distances in the direct form, q ascending (never the expanded one)."""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    out = np.empty((X.shape[0], C.shape[0]))
    for i in range(0, X.shape[0], block):
        d = np.zeros((min(block, X.shape[0] - i), C.shape[0]))
        for q in range(X.shape[1]):
            t = X[i:i + block, q][:, None] - C[:, q][None, :]
            d += t * t
        out[i:i + block] = d
    return out


def relative_gap(d2):
    """Smallest (second best - best) / best squared distance over the rows (K >= 2): how far every label is from flipping."""
    part = np.partition(d2, 1, axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):        # a row ON its centre: inf, or nan for duplicated centres
        return float(np.min((part[:, 1] - part[:, 0]) / part[:, 0]))


def accumulate(X, C, labels=None):
    """What a pass returns for rows X and centres C: (sums, counts, [sum d^2, sum d], labels); with ``labels`` given, for those labels."""
    d2 = sqdist(X, C)
    if labels is None:
        labels = np.argmin(d2, axis=1)                  # the first of equal minima: ties go to the lowest index
    best = d2[np.arange(X.shape[0]), labels]
    K = C.shape[0]
    sums = np.zeros((K, X.shape[1]))
    np.add.at(sums, labels, X)
    counts = np.bincount(labels, minlength=K).astype(np.int64)
    return sums, counts, np.array([best.sum(), np.sqrt(best).sum()]), labels.astype(np.int32)


class NumpyEngine(object):
    """CPU stand-in with ShardEngine's constructor and kmeans_accumulate (tests only).  ``gaps`` collects the relative gap of every pass."""
    gaps = None
    made = []

    def __init__(self, N_s, D, M, Q, device=0):
        self.Q, self.device, self.closed = Q, device, False
        NumpyEngine.made.append(self)

    def kmeans_accumulate(self, centres, X=None, want_labels=False):
        centres = np.atleast_2d(np.asarray(centres, dtype=np.float64))
        if NumpyEngine.gaps is not None and centres.shape[0] > 1:
            NumpyEngine.gaps.append(relative_gap(sqdist(X, centres)))
        s, c, d, lab = accumulate(X, centres)
        return s, c, d, (lab if want_labels else None)

    def close(self):
        self.closed = True
