"""Minibatch training of the sparse GP regression model (fixed embeddings) on the whitened uncollapsed bound: ShardEngine.svi_* (csrc/svi.hip) hold
q(u) on the device, this module draws the batches and moves the hyper-parameters.  DESIGN.md section 21.

One iteration on a batch B of the N host rows, in call order: set_globals(N_global = N), phase1, scale_stats(N / |B|), svi_natural_step(rho), svi_step,
phase2, scale_buffer('grads', N / |B|), finish.  The bound and its gradients are then unbiased estimates of the full-data ones at the current q(u).
The hyper-parameter update is a host-side Adam (or plain gradient) ascent step on driver.py's flat vector [Z, sf2, alpha, beta] with its softplus
transforms: optimiser logic stays off the device.

SVI draws its batches from host arrays and uploads each; ResidentSVI draws them from a shard that is already on the device (gather_from,
csrc/gather.hip) and, when that shard has free embeddings, keeps q(X) there: a batch's rows take a gradient step on the
batch context and go back by scatter_embeddings_to."""
import numpy as np

from .driver import positive_mask, split_flat, transform_grad_vec, transform_vec
from .engine import ShardEngine


class _Driver(object):
    """What the two drivers share: the hyper-parameters and their ascent step, the batches, the full-data bound, publish and close.  A subclass
    says how rows reach a context (_load) and makes self.eng."""

    def _setup(self, N, options):
        self.N = int(N)
        self.B = int(options.get('batch', self.N))
        assert 0 < self.B <= self.N and self.N % self.B == 0, 'batch must divide N: %d rows, batches of %d' % (self.N, self.B)
        Z = np.asarray(options['Z'], dtype=np.float64)
        self.M, self.Q = Z.shape
        self.aux = None                   # a second batch-sized context, made by bound() to add up the full-data statistics
        self.mask = positive_mask([None] * (self.M * self.Q) + [(0, None)] * (self.Q + 2))
        pos = np.concatenate([[float(options['sf2'])], np.asarray(options['alpha'], dtype=np.float64).reshape(-1), [float(options['beta'])]])
        self.flat = np.concatenate([Z.reshape(-1), np.log(np.expm1(pos))])                             # softplus inverse, as driver.transform_back
        self.lr, self.adam = float(options.get('lr', 0.01)), bool(options.get('adam', True))
        self._m, self._v, self._k = np.zeros_like(self.flat), np.zeros_like(self.flat), 0
        self.rng = np.random.RandomState(int(options.get('seed', 0)))
        self._order, self._next = None, 0

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

    def _ascend(self, out):
        """One ascent step of the hyper-parameters along finish()'s gradients ``out`` (Adam, or plain gradient ascent)."""
        g = np.concatenate([out['grad_Z'].reshape(-1), [out['grad_sf2']], out['grad_alpha'], [out['grad_beta']]]) * transform_grad_vec(self.mask, self.flat)
        if self.adam:
            self._k += 1
            self._m = 0.9 * self._m + 0.1 * g
            self._v = 0.999 * self._v + 0.001 * g * g
            g = (self._m / (1 - 0.9 ** self._k)) / (np.sqrt(self._v / (1 - 0.999 ** self._k)) + 1e-8)
        self.flat = self.flat + self.lr * g

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


class SVI(_Driver):
    def __init__(self, engine_factory, Y, X, options):
        """``engine_factory``: (D, M, Q), or a callable rows -> ShardEngine.  ``Y`` (N, D), ``X`` (N, Q) host arrays.  ``options``: Z (M, Q), sf2, alpha
        (Q,), beta: the initial hyper-parameters; batch: rows per batch (must divide N: equal batches); seed: of the permutations; lr (0.01), adam
        (True; False: plain gradient ascent); device (0)."""
        self.Y = np.ascontiguousarray(Y, dtype=np.float64).reshape(len(Y), -1)
        self.X = np.ascontiguousarray(X, dtype=np.float64).reshape(len(X), -1)
        self._setup(self.Y.shape[0], options)
        if callable(engine_factory):
            make = engine_factory
        else:
            D, M, Q = engine_factory
            assert (D, M, Q) == (self.Y.shape[1], self.M, self.Q)
            make = lambda rows: ShardEngine(rows, D, M, Q, device=int(options.get('device', 0)))     # noqa: E731
        self.eng = make(self.B)           # the iteration's context: it holds q(u)
        self._make = make
        self.eng.svi_begin()

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
        self._ascend(out)
        return out['F']


class ResidentSVI(_Driver):
    def __init__(self, full, options):
        """``full``: a ShardEngine that holds all N rows, with fixed embeddings or free ones (uploaded with xs_is_raw: the resident vector update
        works on raw variances).  ``options``: as SVI's, plus lr_x: the step of the local parameters (default: lr), and local_steps (1): gradient
        steps a batch's rows take per iteration.  Batches are gathered on the device; nothing of a batch crosses the bus but its indices."""
        self.full = full
        self._setup(full.N_s, options)
        assert self.Q == full.Q, 'Z has %d columns, the shard Q = %d' % (self.Q, full.Q)
        self.free = bool(full.xs_is_raw)
        self.lr_x, self.local_steps = float(options.get('lr_x', self.lr)), int(options.get('local_steps', 1))
        assert self.local_steps >= 1
        self._make = lambda rows: ShardEngine(rows, full.D, self.M, self.Q, device=full.device)     # noqa: E731
        self.eng = self._make(self.B)
        self.eng.svi_begin()

    def _load(self, eng, idx):
        h = self.hyper()
        eng.gather_from(self.full, idx)
        eng.set_globals(h['Z'], h['sf2'], h['alpha'], h['beta'], N_global=self.N)
        eng.phase1()

    def _local_step(self):
        """(X_mu, raw X_S) of the batch context += lr_x * their gradient, on the device: d = -grad_latest is the ascent direction (grad_latest
        holds the gradient of -F).  A row's gradient is that of the full-data bound at the current q(u): it carries no N / |B|
        (tests/test_svi_local_ref_cpu.py)."""
        self.eng.cg_set_grads()
        self.eng.cg_update(ShardEngine.CG_UPDATE_X, self.lr_x)

    def step(self, rho, learn=False):
        """One iteration on the next batch of the resident shard.  With ``learn`` the hyper-parameters then take one ascent step and, with free
        embeddings, the batch's rows take ``local_steps`` gradient steps (all but the last before the natural step, each on a fresh phase 1)
        and are written back into the shard.  Returns the batch estimate of the bound."""
        scale = float(self.N) / self.B
        idx = self._batch()
        self._load(self.eng, idx)
        self.eng.scale_stats(scale)
        if learn and self.free:
            for _ in range(self.local_steps - 1):
                self.eng.svi_step()
                self.eng.phase2(True)
                self._local_step()
                self.eng.phase1()
                self.eng.scale_stats(scale)
        self.eng.svi_natural_step(rho)
        self.eng.svi_step()
        if not learn:
            return self.eng.scalars()['F']
        self.eng.phase2(self.free)
        self.eng.scale_buffer('grads', scale)
        out = self.eng.finish()
        self._ascend(out)
        if self.free:
            self._local_step()
            self.eng.scatter_embeddings_to(self.full, idx)
        return out['F']

    def close(self):
        """Closes the batch contexts; ``full`` stays the caller's."""
        _Driver.close(self)
        self.full = None
