"""Device-resident model: every shard's data, embeddings, search direction and gradient vectors stay in HBM for the
whole optimisation -- the "full SCG loop that never touches the filesystem".

``ResidentModel.likelihood_and_gradient(x, iteration, step_size)`` has the optimiser callback contract of
parallel_GPLVM.py:222-279; ``ResidentCG`` offers the function names of scg_adapted_local_MapReduce.py:29-243 on the
resident vectors.  Across GPUs (one process per GPU) the local scalars are summed / maxed with torch.distributed.
"""
import numpy as np

from .driver import positive_mask, split_flat, transform_grad_vec, transform_vec
from .engine import ShardEngine
from .evaluation import BufferReduce, evaluate, refresh_statistics
from .lbfgs import LbfgsHistory


class ResidentModel(object):
    def __init__(self, shards, M, Q, D, fixed_embeddings=False, fixed_beta=False, device=0, dist_group=None, N_global=None,
                 engine_class=None):
        """shards: list of (Y, X_mu, X_S) held by THIS process (X_S raw = softplus-inverse space unless fixed_embeddings).  ``engine_class``
        (tests only) replaces ShardEngine."""
        self.M, self.Q, self.D = M, Q, D
        self.fixed_embeddings, self.fixed_beta = fixed_embeddings, fixed_beta
        self.engines = []
        # the variances as given, copied (N x Q doubles per shard on the host): init_X commits new means next to exactly what was uploaded
        self._X_S = [np.array(X_S, dtype=np.float64) for (_, _, X_S) in shards]
        for (Y, X_mu, X_S) in shards:
            e = (engine_class or ShardEngine)(Y.shape[0], D, M, Q, device=device)
            e.set_timing(0)            # an optimiser does not read per-kernel device timings: no timing events on the stream
            e.upload_shard(Y, X_mu, X_S, xs_is_raw=not fixed_embeddings)
            self.engines.append(e)
        self.group = dist_group
        self._dist = None
        self.version = 0            # bumped whenever the resident vectors may have changed (ResidentCG caches its reductions on it)
        self.last_jitter = 0        # the jitter mask the last evaluation ended with (0: none)
        self._n_small = 0           # collectives of _allreduce_vector so far
        if dist_group is not None or self._dist_ready():
            import torch.distributed as dist
            self._dist = dist
        # the two packed buffers of an evaluation: the shards of this process add into engines[0], the processes all-reduce
        self._reduce = BufferReduce(self.engines, dist=self._dist, group=self.group)
        n_local = sum(e.N_s for e in self.engines)
        self.N = int(N_global) if N_global is not None else int(self._allreduce_scalar(float(n_local)))
        self.bounds = [(None, None)] * (M * Q) + [(0, None)] + [(0, None)] * Q + [(0, None)]
        self._pos = positive_mask(self.bounds)

    @property
    def n_collectives(self):
        """All-reduces issued so far, buffers and small vectors (tests assert the per-iteration count)."""
        return self._n_small + self._reduce.n_collectives

    @staticmethod
    def _dist_ready():
        import sys
        if 'torch.distributed' not in sys.modules:     # nobody in this process can have initialised a group: do not pay the torch import
            return False
        try:
            import torch.distributed as dist
            return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        except Exception:
            return False

    def _allreduce_scalar(self, v, op='sum'):
        return float(self._allreduce_vector([v], op)[0])

    def _allreduce_vector(self, values, op='sum'):
        """One collective for a small vector of local scalars (sum or max over ranks)."""
        values = np.asarray(values, dtype=np.float64)
        if self._dist is None:
            return values
        import torch
        # the engine's own GPU, not torch's current device (a caller need not have run torch.cuda.set_device)
        t = torch.tensor(values, dtype=torch.float64,
                         device=torch.device('cuda', self.engines[0].device) if self._dist.get_backend() == 'nccl' else 'cpu')
        self._dist.all_reduce(t, op=self._dist.ReduceOp.SUM if op == 'sum' else self._dist.ReduceOp.MAX, group=self.group)
        self._n_small += 1
        return t.cpu().numpy()

    _stats_x = None
    _stats_version = -1

    def infer_start(self, Y, cols=None, cutoff=6.0, observed=None):
        """Starting means (n, Q) for the latent inference of the NEW rows Y: the resident base mean of the training row nearest to each over the
        output columns ``cols`` (None: all), zero for a row farther than ``cutoff`` from every training row -- predict.py:44-66 over the resident
        rows of every shard of every rank (gparml_amd.init.nearest_start on the engines: nothing is uploaded but Y).  ``observed`` (n, D) bool
        instead of ``cols``: every row is compared over its own observed columns (the start of ``infer_latent_rows``).  COLLECTIVE across ranks,
        with this model's group: every rank gets the same means."""
        from . import init
        kw = {}
        if self._dist is not None:
            kw = dict(allreduce=self._allreduce_vector, rank=self._dist.get_rank(self.group), world=self._dist.get_world_size(self.group))
        return init.nearest_start(self.engines, Y, cols=cols, cutoff=cutoff, observed=observed, **kw)[0]

    def infer(self, flat_array, Y, X_mu, X_S, cols=None, max_iters=100, gtol=1e-5):
        """Latent distributions of NEW rows Y for the model at ``flat_array`` (ShardEngine.infer_latent on the root engine: per-row SCG on the device
        from the start (X_mu, X_S) over the observed columns ``cols``; X_mu None: ``infer_start``, which is COLLECTIVE).  Returns
        (X_mu, X_S, L, iters).  The statistics are brought up to date as in ``predict``, with the same collective rule."""
        if X_mu is None:
            X_mu = self.infer_start(Y, cols=cols)
        self._refresh_statistics(flat_array)
        return self.engines[0].infer_latent(Y, X_mu, X_S, cols=cols, max_iters=max_iters, gtol=gtol)

    def predict(self, flat_array, X_mu, X_S=None, include_noise=False):
        """Posterior predictive mean and variance at new inputs for the model at the optimiser's parameter vector ``flat_array`` (ShardEngine.predict:
        var is (n, 1) for X_S None, (n, D) otherwise).  When ``flat_array`` is not, bit for bit, the vector of the last evaluation (SCG's last
        evaluation is a trial point, not the x it returns) or the resident embeddings moved since (an accepted step's update_X), the statistics
        part is run first at that point with the resident embeddings as they are (phase 1, the reduce, the global step).  That run is COLLECTIVE across ranks: every rank of a multi-GPU job must call predict with the same vector."""
        self._refresh_statistics(flat_array)
        return self.engines[0].predict(X_mu, X_S, include_noise=include_noise)

    def predict_joint(self, flat_array, X, include_noise=False):
        """Joint posterior mean (n, D) and covariance (n, n) at the new inputs X for the model at ``flat_array`` (ShardEngine.predict_joint on the
        root engine).  The statistics are brought up to date as in ``predict``, with the same collective rule."""
        self._refresh_statistics(flat_array)
        return self.engines[0].predict_joint(X, include_noise=include_noise)

    def predict_sample(self, flat_array, X, n_draws, include_noise=False, jitter=1e-8, eps=None, seed=None):
        """``n_draws`` coherent posterior samples (n_draws, n, D) and the mean (n, D) at X for the model at ``flat_array``
        (ShardEngine.predict_sample on the root engine).  The statistics are brought up to date as in ``predict``, with the same collective rule."""
        self._refresh_statistics(flat_array)
        return self.engines[0].predict_sample(X, n_draws, include_noise=include_noise, jitter=jitter, eps=eps, seed=seed)

    def sample_paths(self, flat_array, n_draws, n_features=1024, seed=None):
        """``n_draws`` posterior function draws of the model at ``flat_array`` as a callable ``draws(X) -> (n_draws, n, D)`` (predict.PathDraws on
        the root engine: the same functions at every call, any n).  The statistics are brought up to date as in ``predict``, with the same
        collective rule.  The draws belong to that model and the root engine holds one set at a time: after the next evaluation of the model, or a
        second ``sample_paths``, the earlier callable raises; call ``sample_paths`` again for new draws (nothing is redrawn by itself)."""
        from .predict import PathDraws
        self._refresh_statistics(flat_array)
        Z, _, alpha, _ = split_flat(transform_vec(self._pos, np.asarray(flat_array, dtype=np.float64)), self.M, self.Q)
        return PathDraws(self.engines[0], Z, alpha, n_draws, n_features=n_features, seed=seed)

    def score_training(self, use_S=True, flat_array=None, include_noise=True, want_rows=True):
        """Scores the training rows where they lie (ShardEngine.score on the resident rows of every shard of this process: per-row fit, outliers,
        calibration of the predictive variances): the resident Y under the prediction at the resident base means and, with ``use_S``, base
        variances, for the model at ``flat_array`` (None: the vector of the last evaluation or prediction).  Nothing of size N x D crosses the
        bus.  Returns the dict of ``ShardEngine.score``: the row values concatenated in shard order, the column sums of the shards added on the
        host.  Every engine needs the model: unless all of them hold it (the last evaluation was at this vector), phase 1, the reduce and a
        global step run on all of them first (COLLECTIVE across ranks, as ``predict``); across ranks the caller adds the ranks' ``cols`` and
        takes ``ShardEngine.score_summary`` of the sum.  A row's values do not depend on how the rows are split over shards as long as every
        shard's chunks stay on one side of gp_predict_score's kernel threshold (include/gparml_hip.h; 4096 rows per chunk at M = 512); beyond
        it they agree to rounding."""
        if flat_array is None:
            assert self._stats_x is not None, 'score_training: no evaluation or prediction yet: pass flat_array'
            flat_array = self._stats_x
        self._refresh_statistics(flat_array, all_engines=True)
        use_S = bool(use_S) and not self.fixed_embeddings          # fixed embeddings have no variances: the deterministic form, one variance per row
        parts = [e.score(None, use_resident_S=use_S, include_noise=include_noise, want_rows=want_rows) for e in self.engines]
        out = ShardEngine.score_summary(sum(p['cols'] for p in parts))
        for k in ('row_logp', 'row_sse', 'row_chi2'):
            out[k] = np.concatenate([p[k] for p in parts]) if want_rows else None
        return out

    def loo_training(self, block=1, flat_array=None, include_noise=True, want_rows=True):
        """Exact leave-one-out (``block`` = 1) or leave-block-out cross-validation of the training rows where they lie (ShardEngine.loo on every
        shard of this process), for the model at ``flat_array`` (None: the vector of the last evaluation or prediction) with its hyper-parameters
        and inducing points held fixed.  Blocks are PER SHARD: rows [j block, (j + 1) block) of a shard; for other folds order the rows before
        the upload.  The statistics are brought up to date on every engine as ``score_training`` does (COLLECTIVE across ranks).  Returns the dict
        of ``ShardEngine.loo``: row values, ``lev`` and ``var_loo`` concatenated in shard order (this process's rows); ``cols`` added over the
        shards and over the ranks (one vector all-reduce) with ``score_summary``'s figures of the sum.  Fixed embeddings only."""
        assert self.fixed_embeddings, 'loo_training: fixed embeddings only (leaving out a row with a free embedding is not a rank-one downdate)'
        if flat_array is None:
            assert self._stats_x is not None, 'loo_training: no evaluation or prediction yet: pass flat_array'
            flat_array = self._stats_x
        self._refresh_statistics(flat_array, all_engines=True)
        parts = [e.loo(block=block, include_noise=include_noise, want_rows=want_rows) for e in self.engines]
        cols = self._allreduce_vector(sum(p['cols'] for p in parts).reshape(-1)).reshape(self.D, 5)
        out = ShardEngine.score_summary(cols)
        for k in ('row_logp', 'row_sse', 'row_chi2', 'lev', 'var_loo'):
            out[k] = np.concatenate([p[k] for p in parts]) if (want_rows or k in ('lev', 'var_loo')) else None
        return out

    _stats_all = False          # every engine holds the model of _stats_x (an evaluation, or a refresh with all_engines), not the root alone

    def _refresh_statistics(self, flat_array, all_engines=False):
        """Brings the model up to date at ``flat_array`` unless it is: on the root engine, or (``all_engines``) on every engine of this process."""
        flat_array = np.asarray(flat_array, dtype=np.float64)
        last = self._stats_x
        if (last is None or last.shape != flat_array.shape or last.tobytes() != flat_array.tobytes()
                or self._stats_version != self.version or (all_engines and not self._stats_all and len(self.engines) > 1)):
            Z, sf2, alpha, beta = split_flat(transform_vec(self._pos, flat_array), self.M, self.Q)
            for e in self.engines:
                e.set_globals(Z, sf2, alpha, beta, N_global=self.N, step_size=0.0)
            refresh_statistics(self.engines, self._reduce, all_engines=all_engines)
            self._stats_x = np.array(flat_array, copy=True)
            self._stats_version = self.version
            self._stats_all = bool(all_engines)

    def init_Z(self, K=None, method='kmeans', **kw):
        """Inducing points for this model by k-means over the resident X_mu of every shard of every rank (gparml_amd.init.kmeans on the engines,
        X = None: nothing is uploaded): (centres (<= K, Q), mean distance, passes); K defaults to M.  The keyword arguments are init.kmeans'
        (seeds, thresh, max_iters, restarts, rng).  COLLECTIVE across ranks, with this model's group.  The caller tops up and adds the
        reference's noise (parallel_GPLVM.py:182-187) as driver.init_statistics does.
        ``method='greedy'``: the greedy conditional-variance selection instead (gparml_amd.init.greedy_select on the engines; keyword arguments
        sf2 = 1, alpha = ones(Q), tol): (Z (K', Q) of data rows, pivots (K', 2) as (shard, row), the trace after every step)."""
        from . import init
        if self._dist is not None:
            kw.setdefault('dist_group', True if self.group is None else self.group)
        K = self.M if K is None else int(K)
        if method == 'greedy':
            return init.greedy_select(self.engines, K, kw.pop('sf2', 1.0), kw.pop('alpha', np.ones(self.Q)), **kw)
        assert method == 'kmeans', "init_Z: method must be 'kmeans' or 'greedy', got %r" % (method,)
        return init.kmeans(self.engines, K, **kw)

    def knn_training(self, k, labels=None, weight='alpha', flat_array=None):
        """The ``k`` nearest neighbours of every training row among all the others, in latent space, over the resident X_mu of every shard of
        this process (gparml_amd.init.knn on the engines: nothing is downloaded but the shards' means, which the other shards search for).
        ``weight='alpha'``: the distance sum_q alpha_q (x_q - t_q)^2 in the kernel's own metric, with the ARD alpha of ``flat_array`` (None: the
        vector of the last evaluation or prediction), so that a dimension the model switched off counts for nothing; ``None``: Euclidean; or a
        (Q,) array.  Returns (dist2 (N, k), shard (N, k), row (N, k)) in shard order.  With ``labels`` (N,) in shard order, or one array per
        shard, it returns the leave-one-out k-NN classification error instead: the fraction of rows whose label differs from the majority label of
        their k neighbours (init.knn_vote's tie rule).  The shards of THIS process only: merging across the ranks of a dist_group is not done."""
        from . import init
        if isinstance(weight, str):
            assert weight == 'alpha', "knn_training: weight must be 'alpha', None or a (Q,) array, got %r" % (weight,)
            if flat_array is None:
                assert self._stats_x is not None, 'knn_training: no evaluation or prediction yet: pass flat_array (or a weight)'
                flat_array = self._stats_x
            weight = split_flat(transform_vec(self._pos, np.asarray(flat_array, dtype=np.float64)), self.M, self.Q)[2]
        d2, shard, row = init.knn(self.engines, None, k, weight=weight, skip_self=True)
        if labels is None:
            return d2, shard, row
        if isinstance(labels, (list, tuple)):
            per = [np.asarray(l).reshape(-1) for l in labels]
        else:
            cuts = np.cumsum([e.N_s for e in self.engines])[:-1]
            per = np.split(np.asarray(labels).reshape(-1), cuts)
        assert [len(l) for l in per] == [e.N_s for e in self.engines], 'knn_training: labels do not match the shards'
        allv, start = np.concatenate(per), np.concatenate([[0], np.cumsum([len(l) for l in per])])
        neigh = allv[np.where(row >= 0, start[np.maximum(shard, 0)] + row, 0)]
        return float(np.mean(init.knn_vote(neigh, d2) != allv))

    def init_X(self):
        """Initial embeddings for this model by PCA over the resident Y of every shard of every rank (gparml_amd.init.pca on the engines, Y = None:
        nothing is uploaded but the result): supporting_functions.PCA over ALL data, as the reference insists (local_MapReduce.py:50-65).  The
        means of every shard are replaced (upload_embeddings) and keep the variances the model was built with.  Returns (mean (D,), V (D, Q),
        std (Q,)): a new row y embeds as (y - mean) V / std.  COLLECTIVE across ranks, with this model's group: every rank gets the same axes."""
        from . import init
        mean, V, std, X = init.pca(self.engines, self.Q, allreduce=self._allreduce_vector if self._dist is not None else None)
        for e, x, s in zip(self.engines, X, self._X_S):
            e.upload_embeddings(x, s, xs_is_raw=not self.fixed_embeddings)
        self.version += 1                   # the resident embeddings moved: cached statistics and reductions are stale
        return mean, V, std

    def close(self):
        for e in self.engines:
            e.close()
        self.engines = []

    # ---- parallel_GPLVM.likelihood_and_gradient (:222-279) on resident shards
    def likelihood_and_gradient(self, flat_array, iteration, step_size=0):
        Z, sf2, alpha, beta = split_flat(transform_vec(self._pos, flat_array), self.M, self.Q)
        for e in self.engines:
            e.set_globals(Z, sf2, alpha, beta, N_global=self.N, step_size=step_size)
        res, self.last_jitter = evaluate(self.engines, self._reduce, not self.fixed_embeddings)
        self.version += 1                   # grad_latest changed
        # the vector whose statistics the root engine holds, and the resident vectors' version they were computed with (an optimiser's
        # update of the embeddings -- scg_adapted / gd after an accepted step -- bumps the version: the statistics are then recomputed)
        self._stats_x = np.array(flat_array, dtype=np.float64, copy=True)
        self._stats_version = self.version
        self._stats_all = True              # every engine ran the replicated global step
        grad = np.concatenate([res['grad_Z'].ravel(), [res['grad_sf2']], res['grad_alpha'], [0.0 if self.fixed_beta else res['grad_beta']]])
        grad = grad * transform_grad_vec(self._pos, flat_array)
        return -res['F'], -grad


class _ResidentVectors(object):
    """What ResidentCG and ResidentGD share: the model, a cache of reductions keyed on its version, the update of every shard's vectors."""

    def __init__(self, model):
        self.m = model
        self._cache = None      # (model.version, the reductions)

    def _upd(self, which, a=0.0):
        for e in self.m.engines:
            e.cg_update(which, a)
        self.m.version += 1


class ResidentCG(_ResidentVectors):
    """The helper functions of scg_adapted_local_MapReduce.py on the resident vectors (the ``folder`` argument of the
    reference's file-based helpers is accepted and ignored).  The cache holds the six reductions."""

    def _dots(self):
        """[mu, kappa, theta, |g_new|^2, g_new.g_old, max|d|] over all shards of all ranks: one pass over the resident vectors and
        two small collectives -- a packed SUM of five scalars and one MAX (scg_adapted_local_MapReduce.py:59-155 visits every
        shard's files once per quantity) -- cached until a vector changes (any update here, or a new evaluation's grad_latest)."""
        if self._cache is not None and self._cache[0] == self.m.version:
            return self._cache[1]
        tot = np.zeros(6)
        for e in self.m.engines:
            d = e.cg_dots()
            tot[:5] += d[:5]
            tot[5] = max(tot[5], d[5])
        if self.m._dist is not None:
            tot[:5] = self.m._allreduce_vector(tot[:5], 'sum')
            tot[5] = self.m._allreduce_vector(tot[5:6], 'max')[0]
        self._cache = (self.m.version, tot)
        return tot

    def embeddings_set_grads(self, folder=None):
        self._upd(ShardEngine.CG_SET_GRADS)

    def embeddings_get_grads_mu(self, folder=None):
        return self._dots()[0]

    def embeddings_get_grads_kappa(self, folder=None):
        return self._dots()[1]

    def embeddings_get_grads_theta(self, folder=None):
        return self._dots()[2]

    def embeddings_get_grads_current_grad(self, folder=None):
        return self._dots()[3]

    def embeddings_get_grads_gamma(self, folder=None):
        return self._dots()[4]

    def embeddings_get_grads_max_d(self, folder, alpha):
        return abs(alpha) * self._dots()[5]

    def embeddings_set_grads_reset_d(self, folder=None):
        self._upd(ShardEngine.CG_RESET_D)

    def embeddings_set_grads_update_d(self, folder, gamma):
        self._upd(ShardEngine.CG_UPDATE_D, gamma)

    def embeddings_set_grads_update_X(self, folder, alpha):
        self._upd(ShardEngine.CG_UPDATE_X, alpha)

    def embeddings_set_grads_update_grad_old(self, folder=None):
        self._upd(ShardEngine.CG_GRAD_OLD)

    def embeddings_set_grads_update_grad_new(self, folder=None):
        self._upd(ShardEngine.CG_GRAD_NEW)


class ResidentGD(_ResidentVectors):
    """The helper functions of gd_local_MapReduce.py:14-105 (the gradient-descent optimiser's vector algebra) on the
    resident vectors; ``grad_now`` is the library's grad_new array.  ``folder`` is accepted and ignored.  The cache holds
    (sum |grad_now|, max |grad_now|)."""

    def _abs(self):
        if self._cache is not None and self._cache[0] == self.m.version:
            return self._cache[1]
        s, mx = 0.0, 0.0
        for e in self.m.engines:
            a = e.cg_abs()
            s += a[0]
            mx = max(mx, a[1])
        if self.m._dist is not None:
            s = self.m._allreduce_scalar(s)
            mx = self.m._allreduce_scalar(mx, 'max')
        self._cache = (self.m.version, (s, mx))
        return s, mx

    def embeddings_set_grads(self, folder=None):                       # :14-32  grad_now = latest, d = -latest
        self._upd(ShardEngine.CG_SET_GRADS)

    def embeddings_get_grads_current_grad(self, folder=None):          # :38-47  sum |grad_now|
        return self._abs()[0]

    def embeddings_get_grads_max_gradnow(self, folder=None):           # :49-61  max |grad_now|
        return self._abs()[1]

    def embeddings_set_grads_update_d(self, folder, gamma):            # :63-74  d = -(grad_now + gamma d)
        self._upd(ShardEngine.CG_UPDATE_D, -gamma)

    def embeddings_set_grads_update_X(self, folder, step_size):        # :76-94  X += step d
        self._upd(ShardEngine.CG_UPDATE_X, step_size)

    def embeddings_set_grads_update_grad_now(self, folder=None):       # :96-105 grad_now = latest
        self._upd(ShardEngine.CG_GRAD_NEW)


class ResidentLBFGS(_ResidentVectors, LbfgsHistory):
    """The per-point part of an L-BFGS history on the resident vectors (csrc/lbfgs.hip, gp_lbfgs_*): the ring and the Gram matrix are
    ``lbfgs.LbfgsHistory``'s, on the host; here every shard keeps its slice of the 2 (m + 1) + 1 basis vectors in HBM.  Per accepted step: one
    fused ``push`` per shard, ONE ``lbfgs_dots`` per shard and ONE ``_allreduce_vector`` of 3 (2 (m + 1) + 1) doubles for the three rows of the
    Gram matrix that changed, one ``lbfgs_direction`` per shard.  ``slope()`` (g . d) is read from the matrix.  Use as the ``ops`` of
    ``lbfgs.LBFGS``; m <= 31 (the device holds at most 32 slots, one of them the spare)."""

    def __init__(self, model):
        _ResidentVectors.__init__(self, model)

    def _local_start(self, n_slots):
        for e in self.m.engines:
            e.lbfgs_begin(n_slots)
            e.lbfgs_grad()

    def _local_reset(self, n_slots):
        for e in self.m.engines:
            e.lbfgs_begin(n_slots)          # the same size: the pairs go, g stays

    def _local_dots(self, slot):
        tot = sum(e.lbfgs_dots(slot) for e in self.m.engines)
        if self.m._dist is not None:
            tot = self.m._allreduce_vector(tot.ravel(), 'sum').reshape(tot.shape)
        return tot

    def _local_push(self, slot, step):
        for e in self.m.engines:
            e.lbfgs_push(slot, step)

    def _local_direction(self, coef):
        for e in self.m.engines:
            e.lbfgs_direction(coef)
        self.m.version += 1                 # the direction changed: cached reductions and statistics are stale

    def _local_update_X(self, step):
        self._upd(ShardEngine.CG_UPDATE_X, step)

    def _local_largest_move(self, step):
        mx = max(e.cg_dots()[5] for e in self.m.engines)
        if self.m._dist is not None:
            mx = self.m._allreduce_scalar(mx, 'max')
        return abs(step) * mx

    def _local_finish(self):
        for e in self.m.engines:
            e.lbfgs_end()
