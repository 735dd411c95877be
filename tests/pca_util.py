"""Shared by tests/test_pca_host.py and tests/test_gpu_pca.py: the data sets, the 80-bit truths of the accumulation and projection passes, the SVD
form of supporting_functions.PCA restated, and a numpy stand-in for ShardEngine's two PCA methods."""
import numpy as np

U = 2.0 ** -53          # unit roundoff of float64


def gamma(k):
    """The constant of the standard bound of a float64 sum of k rounded terms in any order (Higham, Accuracy and Stability, section 3.1)."""
    return k * U / (1.0 - k * U)


def rows(n, D, seed=0):
    """(Y (n, D), centre (D,)): unit spread around column means up to 1e4 -- the unshifted Gram matrix Y^T Y - n c c^T would lose eight digits --
    and a centre near the mean that is not the mean."""
    rs = np.random.RandomState(1000 * D + n + seed)
    means = rs.uniform(-1e4, 1e4, D)
    Y = means + rs.randn(n, D)
    return Y, means + 0.3 * rs.randn(D)


_TRUTH = {}


def scatter_truth(Y, centre, key=None):
    """(sum, gram, abs_sum, abs_gram): sums of (y - c) and (y - c)(y - c)^T in numpy.longdouble from the float64 inputs, and the float64 sums of
    the absolute values of the terms (the scale of the bounds).  ``key``: computed once per key and shared."""
    if key is not None and key in _TRUTH:
        return _TRUTH[key]
    Yc = Y.astype(np.longdouble) - centre.astype(np.longdouble)
    A = np.abs(Yc).astype(np.float64)
    D = Y.shape[1]
    gram = np.zeros((D, D), dtype=np.longdouble)
    for i in range(0, D, 32):                    # numpy has no fast 80-bit product: the upper triangle in blocks of rows, then mirrored
        gram[i:i + 32, i:] = np.dot(Yc[:, i:i + 32].T, Yc[:, i:])
    gram = np.triu(gram) + np.triu(gram, 1).T
    out = (Yc.sum(axis=0), gram, A.sum(axis=0), A.T.dot(A))
    if key is not None:
        _TRUTH[key] = out
    return out


def project_truth(Y, mean, P):
    """((Y - mean) P, |Y - mean| |P|) in numpy.longdouble / float64."""
    Yc = Y.astype(np.longdouble) - mean.astype(np.longdouble)
    return np.dot(Yc, P.astype(np.longdouble)), np.abs(Yc).astype(np.float64).dot(np.abs(P))


def svd_pca(Y, Q):
    """supporting_functions.PCA (supporting_functions.py:102-121): thin SVD of the centred data, the first Q left singular vectors, each scaled to
    unit standard deviation; the sign of every component fixed by the project's rule (the largest entry of its axis is positive)."""
    Yc = Y - Y.mean(axis=0)
    Um, _, Vt = np.linalg.svd(Yc, full_matrices=False)
    X = Um[:, :Q]
    X = X / X.std(axis=0)
    V = Vt[:Q].T
    return X * np.sign(V[np.argmax(np.abs(V), axis=0), np.arange(Q)])[None, :]


def assert_columns_close(X, ref, tol=1e-9, signed=True, what=''):
    """Every column within tol relative to the column's largest entry; ``signed`` False: up to the sign of the column."""
    assert X.shape == ref.shape, (what, X.shape, ref.shape)
    for q in range(ref.shape[1]):
        s = 1.0 if signed else np.sign(np.dot(X[:, q], ref[:, q]))
        err = np.max(np.abs(s * X[:, q] - ref[:, q]))
        assert err <= tol * np.max(np.abs(ref[:, q])), (what, q, err)


class NumpyEngine(object):
    """CPU stand-in for a part of gparml_amd.init.pca (tests only): ShardEngine's scatter_accumulate / project_rows on its own rows."""

    def __init__(self, Y):
        self.Y = np.asarray(Y, dtype=np.float64)
        self.n_rows, self.D = self.Y.shape
        self.calls = []

    def scatter_accumulate(self, centre, want_gram=True):
        self.calls.append('gram' if want_gram else 'sum')
        Yc = self.Y - centre
        return Yc.sum(axis=0), (Yc.T.dot(Yc) if want_gram else None)

    def project_rows(self, mean, P):
        self.calls.append('project')
        return (self.Y - mean).dot(P)
