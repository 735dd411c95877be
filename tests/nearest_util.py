"""Shared by tests/test_nearest_host.py and tests/test_gpu_nearest.py: the numpy recomputation of the nearest-row search (float64, the direct form
sum_j (y_j - t_j)^2 over the observed columns, j ascending), a numpy stand-in for ShardEngine.nearest_rows and emulated ranks for
init.nearest_start's ``allreduce``."""
import threading

import numpy as np


def sqdist_cols(Y, T, cols=None, block=2048):
    """(n, N) squared distances between the rows of Y and of T over ``cols`` (None: all), direct form, columns in the given order."""
    Y, T = np.asarray(Y, dtype=np.float64), np.asarray(T, dtype=np.float64)
    cols = list(range(Y.shape[1])) if cols is None else [int(c) for c in cols]
    out = np.empty((Y.shape[0], T.shape[0]))
    for i in range(0, Y.shape[0], block):
        d = np.zeros((min(block, Y.shape[0] - i), T.shape[0]))
        for c in cols:
            t = Y[i:i + block, c][:, None] - T[:, c][None, :]
            d += t * t
        out[i:i + block] = d
    return out


class NumpyNearestEngine(object):
    """CPU stand-in with ShardEngine's nearest_rows (tests only): resident rows (Y, X_mu) given at construction, or host rows per call."""

    def __init__(self, Y=None, X_mu=None):
        self.Y, self.X_mu = Y, X_mu

    def nearest_rows(self, Y_test, cols=None, Y_train=None, want_x=True):
        T = self.Y if Y_train is None else np.asarray(Y_train, dtype=np.float64)
        n = np.atleast_2d(Y_test).shape[0]
        if T.shape[0] == 0:
            return np.full(n, np.inf), np.full(n, -1, dtype=np.int64), None
        d2 = sqdist_cols(np.atleast_2d(Y_test), T, cols)
        idx = np.argmin(d2, axis=1).astype(np.int64)             # the first of equal minima: ties go to the lowest index
        x = self.X_mu[idx] if (Y_train is None and want_x) else None
        return d2[np.arange(n), idx], idx, x


class FakeRanks(object):
    """``world`` emulated ranks, one thread each: allreduce(rank) is that rank's summing function (the sum is taken in rank order on every rank)."""

    def __init__(self, world):
        self.world, self.buf, self.calls = world, [None] * world, 0
        self.barrier = threading.Barrier(world)

    def allreduce(self, rank):
        def f(v):
            self.buf[rank] = np.array(v, dtype=np.float64)
            self.barrier.wait()
            tot = self.buf[0].copy()
            for r in range(1, self.world):
                tot = tot + self.buf[r]
            if rank == 0:
                self.calls += 1
            self.barrier.wait()
            return tot
        return f

    def run(self, fn):
        """fn(rank, allreduce) on every rank at once; the list of results."""
        out, err = [None] * self.world, []

        def work(r):
            try:
                out[r] = fn(r, self.allreduce(r))
            except BaseException as e:      # noqa: BLE001
                err.append(e)
                self.barrier.abort()
        th = [threading.Thread(target=work, args=(r,)) for r in range(self.world)]
        for t in th:
            t.start()
        for t in th:
            t.join(60)
        if err:
            raise err[0]
        return out
