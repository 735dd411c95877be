"""Shared by tests/test_nearest_masked_host.py and tests/test_gpu_nearest_masked.py: the numpy recomputation of the masked nearest-row search (per
new row nearest_util.sqdist_cols over that row's own observed columns, ascending), a numpy stand-in for ShardEngine.nearest_rows(observed=) and a
counting stand-in engine class for Predictor."""
import numpy as np

from nearest_util import NumpyNearestEngine, sqdist_cols


def masked_sqdist(Y, T, observed):
    """(n, N): row i is sqdist_cols(Y[i], T, the observed columns of row i); the unobserved entries of Y are never read."""
    Y, T, observed = np.atleast_2d(np.asarray(Y, dtype=np.float64)), np.asarray(T, dtype=np.float64), np.atleast_2d(np.asarray(observed)) != 0
    assert observed.shape == Y.shape and observed.any(axis=1).all()
    out = np.empty((Y.shape[0], T.shape[0]))
    for i in range(Y.shape[0]):
        out[i] = sqdist_cols(Y[i:i + 1], T, np.flatnonzero(observed[i]))[0]
    return out


def masked_nearest(Y, T, observed):
    """(dist2 (n,), index (n,) int64) of the masked search by numpy: argmin takes the first of equal minima, the lowest row."""
    d2 = masked_sqdist(Y, T, observed)
    idx = np.argmin(d2, axis=1).astype(np.int64)
    return d2[np.arange(d2.shape[0]), idx], idx


def random_masks(rs, n, D, hidden=0.3):
    """(n, D) bool, about ``hidden`` of the entries unobserved, every row observing something; where n allows it the first rows observe only
    column 0, only column D - 1, all columns, and all but one column."""
    obs = rs.rand(n, D) >= hidden
    obs[np.arange(n), rs.randint(D, size=n)] = True
    special = [np.arange(D) == 0, np.arange(D) == D - 1, np.ones(D, dtype=bool), np.arange(D) != D // 2 if D > 1 else np.ones(D, dtype=bool)]
    for i, s in enumerate(special[:n]):
        obs[i] = s
    return obs


class NumpyMaskedNearestEngine(NumpyNearestEngine):
    """NumpyNearestEngine plus ``observed``; ``searches`` counts the calls of every instance of the class that is counted on."""
    searches = 0

    def nearest_rows(self, Y_test, cols=None, Y_train=None, want_x=True, observed=None):
        type(self).searches += 1
        if observed is None:
            return NumpyNearestEngine.nearest_rows(self, Y_test, cols=cols, Y_train=Y_train, want_x=want_x)
        assert cols is None
        T = self.Y if Y_train is None else np.asarray(Y_train, dtype=np.float64)
        n = np.atleast_2d(Y_test).shape[0]
        if T.shape[0] == 0:
            return np.full(n, np.inf), np.full(n, -1, dtype=np.int64), None
        d2, idx = masked_nearest(Y_test, T, observed)
        return d2, idx, (self.X_mu[idx] if (Y_train is None and want_x) else None)


class CountingPredictorEngine(NumpyMaskedNearestEngine):
    """What Predictor.infer(ragged=True) asks of its ``engine_class``, without a model: the masked numpy search, ``predict`` returning the class'
    ``Mz``, and an ``infer_latent_rows`` that records its arguments in ``rows_calls`` and returns the starts as they came."""
    rows_calls = []
    Mz = None

    def __init__(self, N, D, M, Q, device=None):
        NumpyMaskedNearestEngine.__init__(self)
        self.D, self.M, self.Q = D, M, Q

    def set_globals(self, *a, **k):
        pass

    def set_local_statistics(self, *a, **k):
        pass

    def global_step(self, **k):
        pass

    def close(self):
        pass

    def predict(self, X):
        return type(self).Mz, None

    def infer_latent_rows(self, Y, X_mu, X_S, observed=None, xs_is_raw=False, max_iters=100, gtol=1e-5):
        type(self).rows_calls.append(dict(X_mu=np.array(X_mu), observed=np.array(observed)))
        n = np.atleast_2d(X_mu).shape[0]
        return np.array(X_mu), np.array(X_S), np.zeros(n), np.zeros(n, dtype=np.int32)


def stub_predictor(Z, D, engine_class):
    """A Predictor over ``engine_class`` whose statistics are never looked at by the stand-ins above."""
    from gparml_amd.predict import Predictor
    M = Z.shape[0]
    gs = dict(Z=Z, sf2=1.0, alpha=np.ones(Z.shape[1]), beta=1.0)
    acc = dict(sum_YYT=1.0, sum_exp_K_mi_K_im=np.eye(M), sum_exp_K_miY=np.zeros((M, D)), sum_exp_K_ii=1.0, sum_KL=0.0)
    return Predictor(gs, acc, 1, D, engine_class=engine_class)
