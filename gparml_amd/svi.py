"""Minibatch training of the sparse GP regression model (fixed embeddings) on the whitened uncollapsed bound: ShardEngine.svi_* (csrc/svi.hip) hold
q(u) on the device, this module draws the batches and moves the hyper-parameters.  DESIGN.md section 21.

One iteration on a batch B of the N host rows, in call order: set_globals(N_global = N), phase1, scale_stats(N / |B|), svi_natural_step(rho), svi_step,
phase2, scale_buffer('grads', N / |B|), finish.  The bound and its gradients are then unbiased estimates of the full-data ones at the current q(u).
The hyper-parameter update is a host-side Adam (or plain gradient) ascent step on driver.py's flat vector [Z, sf2, alpha, beta] with its softplus
transforms: optimiser logic stays off the device.  Free embeddings work at the C level (gp_svi_step covers both regimes) but need local parameters per
row, which this driver does not keep."""
import numpy as np

from .driver import positive_mask, split_flat, transform_grad_vec, transform_vec
from .engine import ShardEngine


class SVI(object):
    def __init__(self, engine_factory, Y, X, options):
        """``engine_factory``: (D, M, Q), or a callable rows -> ShardEngine.  ``Y`` (N, D), ``X`` (N, Q) host arrays.  ``options``: Z (M, Q), sf2, alpha
        (Q,), beta: the initial hyper-parameters; batch: rows per batch (must divide N: equal batches); seed: of the permutations; lr (0.01), adam
        (True; False: plain gradient ascent); device (0)."""
        self.Y = np.ascontiguousarray(Y, dtype=np.float64).reshape(len(Y), -1)
        self.X = np.ascontiguousarray(X, dtype=np.float64).reshape(len(X), -1)
        self.N = self.Y.shape[0]
        self.B = int(options.get('batch', self.N))
        assert 0 < self.B <= self.N and self.N % self.B == 0, 'batch must divide N: %d rows, batches of %d' % (self.N, self.B)
        Z = np.asarray(options['Z'], dtype=np.float64)
        self.M, self.Q = Z.shape
        if callable(engine_factory):
            make = engine_factory
        else:
            D, M, Q = engine_factory
            assert (D, M, Q) == (self.Y.shape[1], self.M, self.Q)
            make = lambda rows: ShardEngine(rows, D, M, Q, device=int(options.get('device', 0)))     # noqa: E731
        self.eng = make(self.B)           # the iteration's context: it holds q(u)
        self.aux = None                   # a second batch-sized context, made by bound() to add up the full-data statistics
        self._make = make
        self.mask = positive_mask([None] * (self.M * self.Q) + [(0, None)] * (self.Q + 2))
        pos = np.concatenate([[float(options['sf2'])], np.asarray(options['alpha'], dtype=np.float64).reshape(-1), [float(options['beta'])]])
        self.flat = np.concatenate([Z.reshape(-1), np.log(np.expm1(pos))])                             # softplus inverse, as driver.transform_back
        self.lr, self.adam = float(options.get('lr', 0.01)), bool(options.get('adam', True))
        self._m, self._v, self._k = np.zeros_like(self.flat), np.zeros_like(self.flat), 0
        self.rng = np.random.RandomState(int(options.get('seed', 0)))
        self._order, self._next = None, 0
        self.eng.svi_begin()

    def hyper(self):
        Z, sf2, alpha, beta = split_flat(transform_vec(self.mask, self.flat), self.M, self.Q)
        return dict(Z=Z.copy(), sf2=float(sf2), alpha=alpha.copy(), beta=float(beta))

    def _batch(self):
        if self._order is None or self._next >= self.N:
            self._order, self._next = self.rng.permutation(self.N), 0
        idx = np.sort(self._order[self._next:self._next + self.B])
        self._next += self.B
        self.last_batch = idx             # the rows of the latest batch, ascending
        return idx

    def _load(self, eng, idx):
        h = self.hyper()
        eng.upload_shard(self.Y[idx], self.X[idx], np.zeros((len(idx), self.Q)))
        eng.set_globals(h['Z'], h['sf2'], h['alpha'], h['beta'], N_global=self.N)
        eng.phase1()

    def step(self, rho, learn=False):
        """One iteration on the next batch; with ``learn`` the hyper-parameters then take one ascent step.  Returns the batch estimate of the bound."""
        scale = float(self.N) / self.B
        self._load(self.eng, self._batch())
        self.eng.scale_stats(scale)
        self.eng.svi_natural_step(rho)
        self.eng.svi_step()
        if not learn:
            return self.eng.scalars()['F']
        self.eng.phase2(False)
        self.eng.scale_buffer('grads', scale)
        out = self.eng.finish()
        g = np.concatenate([out['grad_Z'].reshape(-1), [out['grad_sf2']], out['grad_alpha'], [out['grad_beta']]]) * transform_grad_vec(self.mask, self.flat)
        if self.adam:
            self._k += 1
            self._m = 0.9 * self._m + 0.1 * g
            self._v = 0.999 * self._v + 0.001 * g * g
            g = (self._m / (1 - 0.9 ** self._k)) / (np.sqrt(self._v / (1 - 0.999 ** self._k)) + 1e-8)
        self.flat = self.flat + self.lr * g
        return out['F']

    def bound(self):
        """The full-data bound at the current q(u) and hyper-parameters: the statistics of every batch added up, then one svi_step."""
        if self.aux is None and self.N > self.B:
            self.aux = self._make(self.B)
        for k in range(self.N // self.B):
            idx = np.arange(k * self.B, (k + 1) * self.B)
            if k == 0:
                self._load(self.eng, idx)
            else:
                self._load(self.aux, idx)
                self.eng.combine(self.aux, 'stats', 'add')
        self.eng.svi_step()
        return self.eng.scalars()['F']

    def publish(self):
        """The iteration's context as a predictor of the trained model (engine.predict and every other new-input entry); the next step() goes on."""
        self.eng.svi_publish()
        self.eng.global_step()
        return self.eng

    def close(self):
        for e in (self.eng, self.aux):
            if e is not None:
                e.close()
        self.eng = self.aux = None
