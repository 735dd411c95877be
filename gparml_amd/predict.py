"""Test-time latent inference on the GPU: Python-3 restatement of the reference's ``predict.py``.

``predict.likelihood_and_gradient`` (predict.py:116-144) optimises the variational mean and variance of NEW points against
the stored accumulated statistics of a trained model: the new points' local statistics are added to the stored global
sums, and the bound and ``grad_X_mu / grad_X_S`` are evaluated with the same ``partial_terms`` class.  Here that class is
``gparml_amd.partial_terms.partial_terms`` (all numbers from the HIP library); the optimiser is
``gparml_amd.scg_adapted.SCG_adapted`` with ``fixed_embeddings=True`` exactly as predict.py:82 does ("the globals are now
the embeddings").
"""
import numpy

from .driver import transform, transform_back, transform_grad
from .partial_terms import partial_terms
from .scg_adapted import SCG_adapted


class PathDraws(object):
    """``n_draws`` posterior function draws held on an engine: ``draws(X) -> (n_draws, n, D)``, the SAME functions at every call, any n.  A point's
    values are the same bits in every call, so a coarse grid and a finer one agree exactly where they share points.  ``close()`` (or a ``with``
    block) frees the draws -- and the engine, when the object owns it (Predictor.sample_paths).  An engine holds one set of draws at a time: once
    another ``paths_set`` or ``paths_clear`` has run on the engine (a second ``ResidentModel.sample_paths``), calling this object raises instead of
    returning the other set's functions, and its ``close()`` leaves the other set alone."""

    def __init__(self, engine, Z, alpha, n_draws, n_features=1024, seed=None, owns_engine=False):
        self.engine, self._owns = engine, owns_engine
        Z = numpy.asarray(Z, dtype=float)
        M, Q = Z.shape
        self.n_draws, self.n_features = int(n_draws), int(n_features)
        rs = numpy.random.RandomState(seed)
        # the order of the three draws is part of what ``seed`` means
        self.omega = rs.randn(self.n_features, Q) * numpy.sqrt(numpy.asarray(alpha, dtype=float).reshape(-1))
        w = rs.randn(self.n_draws, 2 * self.n_features, engine.D)
        eps_u = rs.randn(self.n_draws, M, engine.D)
        self.centre = Z.mean(axis=0)
        engine.paths_set(self.omega, w, eps_u, centre=self.centre)
        self._token = engine.paths_token

    def __call__(self, X, want_mean=False):
        return self._live().paths_eval(X, want_mean=want_mean)

    def _live(self):
        if self.engine is None or self.engine.paths_token != self._token:
            raise RuntimeError('these draws are gone: closed, or replaced by a later paths_set / paths_clear on the same engine -- draw again')
        return self.engine

    def jacobian(self, X):
        """d draws(X)[s, i, d] / d x_q: (n_draws, n, D, Q) (ShardEngine.paths_grad)."""
        return self._live().paths_grad(X, jac=True, metric=False)['jac']

    def metric(self, X):
        """The pull-back metric J_s^T J_s of every sampled surface at the points X: (n_draws, n, Q, Q), symmetric bit for bit -- a sampled
        Riemannian geometry where ``Predictor.metric`` gives the expected one."""
        return self._live().paths_grad(X, jac=False, metric=True)['metric']

    def value_and_grad(self, X, weights):
        """``(value, grad)`` of the scalarised draws ``sum_d weights[d] draws(X)[s, i, d]``: value (n_draws, n), grad (n_draws, n, Q) with respect
        to the point -- what climbing a drawn function (Thompson sampling) needs.  ``weights`` (D,), or (n_draws, n, D) for a weight per (draw,
        point).  Two device calls: the value from ``paths_eval``, the gradient from ``paths_grad``."""
        eng = self._live()
        weights = numpy.asarray(weights, dtype=float)
        out = eng.paths_eval(X)
        grad = eng.paths_grad(X, weights=weights, jac=False, metric=False)['grad']
        return numpy.einsum('snd,...d->sn', out, weights) if weights.ndim == 1 else numpy.einsum('snd,snd->sn', out, weights), grad

    def curve_energy(self, X):
        """Energy of discrete curves X (n_curves, T, Q) on every sampled surface, in ``ShardEngine.curve_energy``'s normalisation:
        ``energy[s, c] = 1/2 (T - 1) sum_t |f_s(x_{t+1}) - f_s(x_t)|^2`` (n_draws, n_curves) and its gradient with respect to the curve's points
        (n_draws, n_curves, T, Q).  One ``paths_eval`` for the surface's points and one ``paths_grad`` whose per-row weights are the derivative of
        the sum with respect to f_s(x_t), ``2 (2 f_t - f_{t-1} - f_{t+1})`` (one-sided at the two ends); the sums over t are formed on the host."""
        eng = self._live()
        X = numpy.asarray(X, dtype=float)
        assert X.ndim == 3 and X.shape[1] >= 2, 'X shape %s: (n_curves, T >= 2, Q) expected' % (X.shape,)
        C, T, Q = X.shape
        f = eng.paths_eval(X.reshape(C * T, Q)).reshape(self.n_draws, C, T, -1)
        df = f[:, :, 1:] - f[:, :, :-1]                                   # (S, C, T - 1, D)
        half = 0.5 * (T - 1)
        w = numpy.zeros_like(f)                                           # d sum_t |df_t|^2 / d f_t
        w[:, :, :-1] -= 2.0 * df
        w[:, :, 1:] += 2.0 * df
        grad = eng.paths_grad(X.reshape(C * T, Q), weights=w.reshape(self.n_draws, C * T, -1), jac=False, metric=False)['grad']
        return half * numpy.sum(df * df, axis=(2, 3)), half * grad.reshape(self.n_draws, C, T, Q)

    def close(self):
        if self.engine is not None:
            if self._owns:
                self.engine.close()
            elif self.engine.paths_token == self._token:
                self.engine.paths_clear()
            self.engine = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def straight_curves(x0, x1, T):
    """The equally spaced straight lines (n, T, Q) from the rows of x0 to the rows of x1 (n, Q); the endpoints carry the given bits."""
    x0, x1 = numpy.atleast_2d(numpy.asarray(x0, dtype=float)), numpy.atleast_2d(numpy.asarray(x1, dtype=float))
    assert x0.shape == x1.shape and x0.ndim == 2 and int(T) >= 2, 'x0 %s, x1 %s: two (n, Q) arrays and T >= 2 expected' % (x0.shape, x1.shape)
    t = (numpy.arange(int(T)) / (int(T) - 1.0))[None, :, None]
    X = x0[:, None, :] + t * (x1 - x0)[:, None, :]
    X[:, 0], X[:, -1] = x0, x1
    return X


def minimise_curves(energy_and_grad, X, iterations=200, gtol=1e-6):
    """Minimise the sum of the energies of the discrete curves X (n, T, Q) over their interior points, the endpoints held fixed, with
    scipy's L-BFGS-B.  ``energy_and_grad(X) -> (energy (n,), grad (n, T, Q))`` is called once per function evaluation with all curves (the
    device's ShardEngine.curve_energy, or a numpy reference).  Stops after ``iterations`` iterations or when the largest gradient component
    falls to ``gtol``.  Returns (X, info): the curves, and ``evaluations``, ``energy0`` (the energies at the start) and scipy's ``message``."""
    import scipy.optimize
    X = numpy.array(X, dtype=float, order='C')
    assert X.ndim == 3 and X.shape[1] >= 2, 'X shape %s: (n, T >= 2, Q) expected' % (X.shape,)
    info = {'evaluations': 0, 'energy0': None, 'message': 'nothing to optimise'}

    def fun(v):
        Y = X.copy()
        Y[:, 1:-1] = v.reshape(Y[:, 1:-1].shape)
        e, g = energy_and_grad(Y)
        e, g = numpy.asarray(e, dtype=float), numpy.asarray(g, dtype=float)
        if info['energy0'] is None:
            info['energy0'] = e.copy()
        info['evaluations'] += 1
        return float(numpy.sum(e)), g[:, 1:-1].reshape(-1).copy()

    if X.shape[0] == 0 or X.shape[1] == 2:
        info['energy0'] = numpy.asarray(energy_and_grad(X)[0], dtype=float)
        info['evaluations'] = 1
        return X, info
    res = scipy.optimize.minimize(fun, X[:, 1:-1].reshape(-1), jac=True, method='L-BFGS-B',
                                  options={'maxiter': int(iterations), 'gtol': float(gtol), 'ftol': 0.0})
    X[:, 1:-1] = res.x.reshape(X[:, 1:-1].shape)
    info['message'] = res.message if isinstance(res.message, str) else res.message.decode()
    return X, info


class Predictor(object):
    def __init__(self, global_statistics, accumulated_statistics, N_train, D, device=0, partial_terms_class=None, engine_class=None):
        """global_statistics: dict Z (M,Q), sf2, alpha, beta; accumulated_statistics: the five base sums of the trained model
        (the ``accumulated_statistics_*_f.npy`` files, predict.py:31-35).  ``partial_terms_class`` (tests only: a CPU class with the
        reference's constructor) replaces the GPU class so that the host logic can be checked without a device; ``engine_class`` (tests only: a
        CPU class with ShardEngine's constructor and its set_globals / set_local_statistics / global_step / infer_latent / predict / close) does the
        same for ``infer`` and ``impute``."""
        self._cls = partial_terms_class
        self._engine_cls = engine_class
        self.gs = global_statistics
        self.acc = accumulated_statistics
        Z = numpy.asarray(global_statistics['Z'], dtype=float)
        self.M, self.Q = Z.shape
        self.N, self.D = int(N_train), int(D)
        self.device = device
        self._pt = None

    def predict_outputs(self, X_mu, X_S, include_noise=False):
        """Reconstruct Y* from q(x*) = N(X_mu, diag X_S) (what ``test`` returns for new rows) with the trained model: the posterior predictive
        mean (n, D) and variance (n, D) of every output, against the stored accumulated statistics of the training data only (not the new
        rows' own statistics).  The columns a ``test(..., mask=...)`` call left out are the imputed ones.  ``include_noise`` adds 1/beta.
        X_S None predicts at the point X_mu (variance (n, 1))."""
        eng = self._trained_engine()
        try:
            return eng.predict(X_mu, X_S, include_noise=include_noise)
        finally:
            eng.close()

    def predict_joint(self, X, include_noise=False):
        """Joint posterior of the outputs at the points X (n, Q) with the trained model: mean (n, D) and the covariance (n, n) between the points,
        shared by all D outputs (ShardEngine.predict_joint), against the stored accumulated statistics of the training data."""
        eng = self._trained_engine()
        try:
            return eng.predict_joint(X, include_noise=include_noise)
        finally:
            eng.close()

    def predict_conditioned(self, X, Xc, Yc, include_noise=False, want_reduction=False):
        """The prediction at the points X (n, Q) of the trained model conditioned on the extra observed rows (Xc (m, Q), Yc (m, D)), m <= 1024,
        without a refit (ShardEngine.condition / condition_predict): (mean (n, D), var (n, 1)) and, with ``want_reduction``, the reduction
        (n, 1) of the variance.  Look-ahead posteriors, rows that arrived after training; the stored statistics are not changed."""
        eng = self._trained_engine()
        try:
            eng.condition(Xc, Yc)
            return eng.condition_predict(X, include_noise=include_noise, want_reduction=want_reduction)
        finally:
            eng.close()

    def predict_sample(self, X, n_draws, include_noise=False, jitter=1e-8, eps=None, seed=None):
        """``n_draws`` coherent samples (n_draws, n, D) of the outputs at the points X (n, Q), and the mean (n, D) (ShardEngine.predict_sample)."""
        eng = self._trained_engine()
        try:
            return eng.predict_sample(X, n_draws, include_noise=include_noise, jitter=jitter, eps=eps, seed=seed)
        finally:
            eng.close()

    def sample_paths(self, n_draws, n_features=1024, seed=None):
        """``n_draws`` posterior function draws of the trained model as a callable: ``draws(X) -> (n_draws, n, D)`` at any points X (n, Q), any n,
        the same functions at every call (ShardEngine.paths_set / paths_eval; Matheron's rule on ``n_features`` random Fourier frequency pairs
        drawn, like the normals, from numpy.random.RandomState(seed); the phases are centred on the column mean of Z).  The work of a call is
        linear in n.  The object holds an engine with the trained model: ``close()`` it (or use ``with``)."""
        eng = self._trained_engine()
        try:
            return PathDraws(eng, self.gs['Z'], self.gs['alpha'], n_draws, n_features=n_features, seed=seed, owns_engine=True)
        except Exception:
            eng.close()
            raise

    def _predict_grad(self, X, **which):
        eng = self._trained_engine()
        try:
            return eng.predict_grad(X, **which)
        finally:
            eng.close()

    def predict_jacobian(self, X):
        """(jac (n, D, Q), dvar (n, Q)): the derivatives of the predictive mean and of the variance of f with respect to the input, at the points
        X (n, Q) with the trained model (ShardEngine.predict_grad)."""
        out = self._predict_grad(X, jac=True, dvar=True, metric=False, logdet=False)
        return out['jac'], out['dvar']

    def predict_metric(self, X):
        """The expected metric tensor (n, Q, Q) of the mapping at the points X: E[J]^T E[J] + D Cov(J) (ShardEngine.predict_grad)."""
        return self._predict_grad(X, jac=False, dvar=False, metric=True, logdet=False)['metric']

    def predict_magnification(self, X):
        """The magnification factor sqrt(det metric) (n,) at the points X.  The log-determinant comes from the device for Q <= 64; beyond that it
        is numpy.linalg.slogdet of the returned metric."""
        if self.Q <= 64:
            return numpy.exp(0.5 * self._predict_grad(X, jac=False, dvar=False, metric=False, logdet=True)['logdet'])
        return numpy.exp(0.5 * numpy.linalg.slogdet(self.predict_metric(X))[1])

    def curve_energy(self, X, want_energy=True, want_segments=False, want_grad=True):
        """Expected energy 1/2 (T - 1) sum_s E|f(x_{s+1}) - f(x_s)|^2 of the discrete curves X (n_curves, T, Q) or (T, Q) under the trained model,
        its per-segment terms and its gradient with respect to the curve's points: a dict of ``energy``, ``seg``, ``grad`` as requested
        (ShardEngine.curve_energy)."""
        eng = self._trained_engine()
        try:
            return eng.curve_energy(X, want_energy=want_energy, want_segments=want_segments, want_grad=want_grad)
        finally:
            eng.close()

    @staticmethod
    def _length(seg):
        return numpy.sqrt(numpy.maximum(seg, 0.0)).sum(axis=-1)

    def curve_length(self, X):
        """The expected length sum_s sqrt(E|f(x_{s+1}) - f(x_s)|^2) of the discrete curves X (n_curves, T, Q) or (T, Q), from ``curve_energy``'s
        segments."""
        return self._length(self.curve_energy(X, want_energy=False, want_segments=True, want_grad=False)['seg'])

    def geodesic(self, x0, x1, T=32, X0=None, iterations=200, gtol=1e-6):
        """The discrete geodesics of T points between the latent points x0 and x1 ((Q,) or, batched, (n, Q)) under the expected metric of the
        trained model: the curves that minimise ``curve_energy`` with their endpoints held fixed (``minimise_curves``: L-BFGS-B on the host, one
        device call per function evaluation for all curves), started from the equally spaced straight lines or from ``X0`` (n, T, Q), whose
        end points are replaced by x0 and x1.  A curve whose energy did not fall keeps its start.  Returns a dict: ``curves`` (n, T, Q),
        ``energy`` (n,) and ``length`` (n,) from a final ``curve_energy`` call at the returned curves, and ``evaluations`` (a single pair:
        without the leading axis).  A local minimiser: curves between distant points may need a better start than the straight line."""
        single = numpy.asarray(x0).ndim == 1
        X = straight_curves(x0, x1, T)
        if X0 is not None:
            X0 = numpy.asarray(X0, dtype=float).reshape((-1,) + X.shape[1:])
            assert X0.shape == X.shape, 'X0 shape %s: %s expected' % (X0.shape, X.shape)
            X[:, 1:-1] = X0[:, 1:-1]
        eng = self._trained_engine()
        try:
            def f(Y):
                out = eng.curve_energy(Y)
                return out['energy'], out['grad']
            Xs, info = minimise_curves(f, X, iterations=iterations, gtol=gtol)
            out = eng.curve_energy(Xs, want_segments=True, want_grad=False)
            worse = ~(out['energy'] <= info['energy0'])
            if worse.any():
                Xs[worse] = X[worse]
                out = eng.curve_energy(Xs, want_segments=True, want_grad=False)
        finally:
            eng.close()
        res = {'curves': Xs, 'energy': out['energy'], 'length': self._length(out['seg'])}
        if single:
            res = {k: v[0] for k, v in res.items()}
        res['evaluations'] = info['evaluations']
        return res

    def knn(self, X, k, training, weight='alpha'):
        """The ``k`` nearest training embeddings of every latent point of ``X`` (n, Q): (dist2 (n, k), shard (n, k), row (n, k)), ascending in
        (dist2, shard, row) (gparml_amd.init.knn; csrc/knn.hip).  ``training``: the iterable of (Y_shard, X_shard) pairs ``infer`` takes (only
        the embeddings X_shard are read), shard = its position there.  ``weight='alpha'``: the distance sum_q alpha_q (x_q - t_q)^2 in the
        trained kernel's own metric; ``None``: Euclidean; or a (Q,) array.  The search is in latent space: starts for ``infer`` from several
        neighbours, geodesic graphs for ``geodesic``, local subsets.  The shards of this process only: nothing is merged across ranks."""
        from . import init
        cls = self._engine_cls
        if cls is None:
            from .engine import ShardEngine as cls
        if isinstance(weight, str):
            assert weight == 'alpha', "knn: weight must be 'alpha', None or a (Q,) array, got %r" % (weight,)
            weight = numpy.asarray(self.gs['alpha'], dtype=float).reshape(-1)
        eng = cls(1, self.D, self.M, self.Q, device=self.device)         # host rows on both sides: no model, no shard
        try:
            return init.knn([init.HostRows(eng, Xs) for _, Xs in training], X, k, weight=weight)
        finally:
            eng.close()

    def _trained_engine(self):
        """An engine that holds the trained model: the globals, the stored accumulated statistics of the training data and a global step on them."""
        cls = self._engine_cls
        if cls is None:
            from .engine import ShardEngine as cls
        g, a = self.gs, self.acc
        f = lambda x: float(numpy.asarray(x).reshape(-1)[0])
        eng = cls(1, self.D, self.M, self.Q, device=self.device)
        try:
            eng.set_globals(numpy.asarray(g['Z'], dtype=float), f(g['sf2']), numpy.asarray(g['alpha'], dtype=float).reshape(-1), f(g['beta']),
                            N_global=max(self.N, 1))
            eng.set_local_statistics(f(a['sum_YYT']), a['sum_exp_K_mi_K_im'], a['sum_exp_K_miY'], f(a['sum_exp_K_ii']), f(a['sum_KL']))
            eng.global_step(sync=True)
        except Exception:
            eng.close()
            raise
        return eng

    def infer(self, Y_test, mask=None, X_mu0=None, X_S0=None, training=None, is_random_init=False, random_restarts=0, iterations=100, gtol=1e-5,
              nearest='host', ragged=False, start=None):
        """q(x*) = N(X_mu, diag X_S) of every NEW row of ``Y_test`` (n, D) with q(u) frozen at the trained optimum: [X_mu (n, Q), X_S (n, Q), L (n,)],
        L the row's own bound (ShardEngine.infer_latent: every row is an independent problem, optimised on the device).

        Observed outputs of a row: the columns of ``mask`` (None: all) that are not NaN in it; only these enter the likelihood, so a row with
        missing outputs is embedded from what it has.  Rows are grouped by that pattern, one device call per pattern.  Starting mean: ``X_mu0``
        when given; else, as ``test``, the embedding of the nearest training output over the row's observed columns (``training`` = iterable of
        (Y_shard, X_shard) pairs, kept in memory and searched once per pattern: with a k-d tree on the host, or, with ``nearest='device'``, by
        ``init.nearest_start`` on the trained engine) or, with ``is_random_init``, a random inducing point for EVERY
        row followed by ``random_restarts`` further random inducing points per row; restarts are laid out as rows of the same call (row i's
        starts are rows i (R + 1) .. i (R + 1) + R) and the best L is kept per row (the earliest on ties).  Starting variance ``X_S0`` or
        0.5 + 0.01 randn clipped to [0.001, 1] (predict.py:71-72), shared by a row's restarts.

        ``ragged=True``: the observed set of a row is the same, but ALL rows and all their restarts go to ONE ``infer_latent_rows`` call, whatever
        the number of patterns (rows with holes in random places have a pattern each); restarts stay rows of that call and the best L per row is
        kept, the earliest on ties.  The starts work as above.  With ``training=...`` and ``nearest='device'`` ONE masked search per training
        shard serves all rows, each compared over its own observed columns (``init.nearest_start(observed=)``, gp_nearest_rows_masked); with
        ``nearest='host'`` the k-d trees are still built once per pattern.  ``start='inducing'`` (``ragged=True`` only) needs no training rows:
        every row starts at the inducing point whose predicted outputs are nearest to the row over its observed columns -- ``inducing_start`` on
        the host, or with ``nearest='device'`` the same choice by one masked search over the M predicted rows (no cut-off applies)."""
        Y = numpy.atleast_2d(numpy.asarray(Y_test, dtype=float))
        n, Q = Y.shape[0], self.Q
        assert Y.shape[1] == self.D, 'Y_test shape %s: (n, %d) expected' % (Y.shape, self.D)
        assert nearest in ('host', 'device'), "nearest must be 'host' or 'device'"
        assert start in (None, 'inducing'), "start must be None or 'inducing'"
        assert start is None or ragged, "start='inducing' needs ragged=True"
        Z = numpy.asarray(self.gs['Z'], dtype=float)
        cols = numpy.arange(self.D) if mask is None else numpy.unique(numpy.asarray(list(mask), dtype=int))
        observed = ~numpy.isnan(Y[:, cols])
        assert observed.any(axis=1).all(), 'a row of Y_test has no observed output among the columns of mask'
        if X_mu0 is not None:
            X_mu0 = numpy.atleast_2d(numpy.asarray(X_mu0, dtype=float))
            assert X_mu0.shape == (n, Q), 'X_mu0 shape %s: (%d, %d) expected' % (X_mu0.shape, n, Q)
            starts = X_mu0[:, None, :]
        elif is_random_init:
            starts = Z[numpy.random.randint(self.M, size=(n, int(random_restarts) + 1))]        # (n, R + 1, Q)
        elif start == 'inducing':
            starts, training = None, None
        else:
            if training is None:
                raise AssertionError('Predictor.infer needs the training shards (training=...), an initial mean (X_mu0=...) or is_random_init')
            training = list(training)
            starts = None
        if X_S0 is None:
            X_S0 = numpy.clip(numpy.ones((n, Q)) * 0.5 + 0.01 * numpy.random.randn(n, Q), 0.001, 1)
        X_S0 = numpy.atleast_2d(numpy.asarray(X_S0, dtype=float))
        assert X_S0.shape == (n, Q), 'X_S0 shape %s: (%d, %d) expected' % (X_S0.shape, n, Q)
        groups = {}
        for i in range(n):
            groups.setdefault(observed[i].tobytes(), []).append(i)
        X_mu, X_S, L = numpy.empty((n, Q)), numpy.empty((n, Q)), numpy.empty(n)
        eng = self._trained_engine()
        try:
            if ragged:
                return self._infer_ragged(eng, Y, cols, observed, groups, starts, X_S0, training, nearest, iterations, gtol)
            for key in sorted(groups, key=lambda k: groups[k][0]):
                rows = numpy.asarray(groups[key])
                c = cols[observed[rows[0]]]
                if starts is None and nearest == 'device':
                    s = self._nearest_on_device(eng, Y[rows], training, c)[:, None, :]
                elif starts is None:
                    s = self.nearest_training_embeddings(Y[rows], training, Q, c)[:, None, :]
                else:
                    s = starts[rows]
                k = s.shape[1]
                m, v, l, _ = eng.infer_latent(numpy.repeat(Y[rows], k, axis=0), s.reshape(-1, Q), numpy.repeat(X_S0[rows], k, axis=0),
                                              cols=None if c.size == self.D else c, max_iters=iterations, gtol=gtol)
                l = numpy.asarray(l).reshape(len(rows), k)
                best = numpy.argmax(l, axis=1)                                          # the earliest of equal maxima
                pick = numpy.arange(len(rows)) * k + best
                X_mu[rows], X_S[rows], L[rows] = numpy.asarray(m)[pick], numpy.asarray(v)[pick], l[numpy.arange(len(rows)), best]
        finally:
            eng.close()
        return [X_mu, X_S, L]

    def _infer_ragged(self, eng, Y, cols, observed, groups, starts, X_S0, training, nearest, iterations, gtol):
        """``infer`` with ``ragged=True`` on the trained engine: one ``infer_latent_rows`` call for every row and restart."""
        n, Q = Y.shape[0], self.Q
        obs = numpy.zeros((n, self.D), dtype=bool)
        obs[:, cols] = observed
        if starts is None and training is None:                                         # start='inducing'
            Z = numpy.asarray(self.gs['Z'], dtype=float)
            Mz = eng.predict(Z)[0]
            if nearest == 'device':                                                     # inducing_start's choice by one masked search over the M rows of Mz
                starts = Z[eng.nearest_rows(Y, observed=obs, Y_train=Mz, want_x=False)[1]][:, None, :]
            else:
                starts = self.inducing_start(Y, obs, Z, Mz)[:, None, :]
        elif starts is None and nearest == 'device':                                    # the nearest training output: one masked search per shard
            starts = self._nearest_on_device(eng, Y, training, observed=obs)[:, None, :]
        elif starts is None:                                                            # the nearest training output, searched per pattern
            starts = numpy.empty((n, 1, Q))
            for key in sorted(groups, key=lambda k: groups[k][0]):
                rows = numpy.asarray(groups[key])
                c = cols[observed[rows[0]]]
                starts[rows, 0] = self.nearest_training_embeddings(Y[rows], training, Q, c)
        k = starts.shape[1]
        m, v, l, _ = eng.infer_latent_rows(numpy.repeat(Y, k, axis=0), starts.reshape(-1, Q), numpy.repeat(X_S0, k, axis=0),
                                           observed=numpy.repeat(obs, k, axis=0), max_iters=iterations, gtol=gtol)
        l = numpy.asarray(l).reshape(n, k)
        best = numpy.argmax(l, axis=1)                                                  # the earliest of equal maxima
        pick = numpy.arange(n) * k + best
        return [numpy.asarray(m)[pick], numpy.asarray(v)[pick], l[numpy.arange(n), best]]

    @staticmethod
    def inducing_start(Y, observed, Z, Mz, block=None):
        """The start of ``infer(..., start='inducing')``: for every row of Y (n, D) the inducing point z_m (row of Z (M, Q)) that minimises
        sum over the row's observed d of (y_d - Mz[m, d])^2, Mz (M, D) the predicted mean at the inducing points; the lowest m on ties.  Entries of
        Y outside ``observed`` (n, D) are never used and may be NaN.  Host arithmetic in the direct form (differences first), ``block`` rows at a time (default: about 32 MB of
        differences): no (n, M, D) array is formed."""
        Y, Z, Mz = numpy.atleast_2d(numpy.asarray(Y, dtype=float)), numpy.asarray(Z, dtype=float), numpy.asarray(Mz, dtype=float)
        o = numpy.atleast_2d(numpy.asarray(observed)) != 0
        assert o.shape == Y.shape and Mz.shape == (Z.shape[0], Y.shape[1]), 'inducing_start: Y %s, observed %s, Mz %s' % (Y.shape, o.shape, Mz.shape)
        out = numpy.empty((Y.shape[0], Z.shape[1]))
        if block is None:
            block = max(1, (4 << 20) // max(1, Mz.size))
        for i0 in range(0, Y.shape[0], block):
            ob = o[i0:i0 + block]
            diff = numpy.where(ob[:, None, :], numpy.where(ob, Y[i0:i0 + block], 0.0)[:, None, :] - Mz[None, :, :], 0.0)      # (block, M, D)
            d2 = numpy.einsum('bmd,bmd->bm', diff, diff)
            out[i0:i0 + block] = Z[numpy.argmin(d2, axis=1)]                            # argmin: the first of equal minima
        return out

    def impute(self, Y_test, mask, include_noise=False, **infer_args):
        """Reconstruct the outputs of new rows from the observed columns ``mask``: ``infer`` (its keyword arguments pass through), then
        ``predict_outputs`` at the inferred q(x*).  Returns (mean (n, D), var (n, D), [X_mu, X_S, L]); the columns outside ``mask`` are the imputed ones."""
        res = self.infer(Y_test, mask=mask, **infer_args)
        mean, var = self.predict_outputs(res[0], res[1], include_noise=include_noise)
        return mean, var, res

    def score(self, Y_test, X_mu, X_S=None, observed=None, include_noise=True):
        """How well the trained model predicts the outputs ``Y_test`` (n, D) from q(x*) = N(X_mu, diag X_S) (X_S None: from the points X_mu): the
        Gaussian log predictive density and the errors of every observed entry, reduced on the device (ShardEngine.score: the dict of row values
        ``row_logp`` / ``row_sse`` / ``row_chi2`` and per-column and ``pooled`` ``count``, ``bias``, ``rmse``, ``chi2_mean``, ``nlpd``).
        ``observed`` (n, D): the entries to score; None: where Y_test is not NaN."""
        eng = self._trained_engine()
        try:
            return eng.score(Y_test, X_mu, X_S, observed=observed, include_noise=include_noise)
        finally:
            eng.close()

    def impute_score(self, Y_true, mask, include_noise=True, **infer_args):
        """The standard missing-data experiment: the rows of ``Y_true`` (n, D) are embedded from the columns ``mask`` alone, as ``impute`` does
        (``infer``; its keyword arguments pass through), and the model is scored on exactly the entries that were hidden from it and are known:
        the columns outside ``mask`` where Y_true is not NaN.  Returns (the dict of ``score``, [X_mu, X_S, L])."""
        Y = numpy.atleast_2d(numpy.asarray(Y_true, dtype=float))
        res = self.infer(Y, mask=mask, **infer_args)
        hidden = numpy.ones(Y.shape, dtype=bool)
        hidden[:, numpy.unique(numpy.asarray(list(mask), dtype=int))] = False
        return self.score(Y, res[0], res[1], observed=hidden & ~numpy.isnan(Y), include_noise=include_noise), res

    def _partial_terms(self):
        if self._pt is None:
            g = self.gs
            f = lambda x: float(numpy.asarray(x).reshape(-1)[0])
            args = (numpy.asarray(g['Z'], dtype=float), f(g['sf2']), numpy.asarray(g['alpha'], dtype=float).reshape(-1), f(g['beta']),
                    self.M, self.Q, self.N, self.D)
            if self._cls is not None:
                self._pt = self._cls(*args)
            else:
                self._pt = partial_terms(*args, update_global_statistics=False, device=self.device)
        return self._pt

    def likelihood_and_gradient(self, flat_array, iteration=0, step_size=0):
        """predict.py:116-144."""
        shape = self.shape
        bounds = self.bounds
        t = numpy.array([transform(b, x) for b, x in zip(bounds, flat_array)])
        half = len(t) // 2
        X_mu, X_S = t[:half].reshape(shape), t[half:].reshape(shape)
        pt = self._partial_terms()
        pt.set_data(self.Y_test, X_mu, X_S, is_set_statistics=True)
        new = pt.get_local_statistics()
        a = self.acc
        pt.set_local_statistics(a['sum_YYT'] + new['sum_YYT'], a['sum_exp_K_mi_K_im'] + new['sum_exp_K_mi_K_im'],
                                a['sum_exp_K_miY'] + new['exp_K_miY'], a['sum_exp_K_ii'] + new['sum_exp_K_ii'], a['sum_KL'] + new['KL'])
        likelihood = pt.logmarglik()
        gradient = numpy.concatenate((pt.grad_X_mu().flatten(), pt.grad_X_S().flatten()))
        gradient = numpy.array([g * transform_grad(b, x) for b, x, g in zip(bounds, flat_array, gradient)])
        return -1 * likelihood, -1 * gradient

    # ---- initialisation of the new points (predict.py:37-72) ------------------------------------------------------------------------
    @staticmethod
    def nearest_training_embeddings(Y_test, training, Q, mask=None):
        """predict.py:44-66: every new point starts at the trained embedding of the training output nearest to it (Euclidean distance over
        the output columns in ``mask``, all columns by default), searched shard by shard with a k-d tree (leaf size 100) and the
        reference's cut-off of 6: a new point farther than that from every training output keeps a zero mean.  ``training`` yields
        (Y_shard, X_shard) pairs -- one shard in memory at a time, ties between shards go to the first one as in the reference."""
        import scipy.spatial
        Y_test = numpy.atleast_2d(numpy.asarray(Y_test, dtype=float))
        cols = list(range(Y_test.shape[1])) if mask is None else list(mask)
        best = numpy.full(Y_test.shape[0], numpy.inf)
        X_mu = numpy.zeros((Y_test.shape[0], Q))
        for Y, X in training:
            Y = numpy.asarray(Y, dtype=float)
            if Y.ndim == 1:
                Y = numpy.atleast_2d(Y).T                                           # predict.py:55-56
            tree = scipy.spatial.cKDTree(Y[:, cols], leafsize=100)
            dist, ind = tree.query(Y_test[:, cols], k=1, distance_upper_bound=6)
            closer = dist < best                                                    # strict: an equally near point of a later shard does not win
            best[closer] = dist[closer]
            X_mu[closer] = numpy.asarray(X)[ind[closer]]
        return X_mu

    @staticmethod
    def _nearest_on_device(engine, Y_test, training, mask=None, observed=None):
        """``nearest_training_embeddings`` with the search on the device: every (Y_shard, X_shard) of ``training`` passes through ``engine`` as
        host rows (init.nearest_start), one shard in memory at a time; the same tie rule and cut-off.  ``observed`` (n, D) bool instead of
        ``mask``: every row over its own observed columns, still one search per shard."""
        from . import init
        return init.nearest_start(((engine, Ys, Xs) for Ys, Xs in training), Y_test, cols=None if mask is None else list(mask), observed=observed)[0]

    def _optimise(self, X_mu0, X_S0, iterations):
        x0 = numpy.concatenate((X_mu0.flatten(), X_S0.flatten()))
        x0 = numpy.array([transform_back(b, x) for b, x in zip(self.bounds, x0)])
        x, flog, nfe, status = SCG_adapted(self.likelihood_and_gradient, x0, None, fixed_embeddings=True, maxiters=iterations)
        t = numpy.array([transform(b, y) for b, y in zip(self.bounds, x)])
        n = len(t) // 2
        return [t[:n].reshape(self.shape), t[n:].reshape(self.shape), -flog[-1]]

    def test(self, Y_test, X_mu0=None, X_S0=None, iterations=100, training=None, mask=None, is_random_init=False, random_restarts=100,
             nearest='host'):
        """predict.test (predict.py:19-111) -> [X_mu, X_S, likelihood] of the new points.

        Starting mean: ``X_mu0`` when given; otherwise, as the reference, the embedding of the nearest training output (``training`` =
        iterable of (Y_shard, X_shard), ``mask`` = output columns to compare; no restarts, predict.py:43; ``nearest='device'`` searches on the
        GPU, the shards passing through an engine as host rows, instead of with k-d trees on the host) or, with ``is_random_init``, a
        random inducing point, followed by ``random_restarts`` further optimisations from other random inducing points that keep the best
        likelihood (predict.py:93-108; like the reference this branch starts ONE row of Z, so it serves a single new point).  Starting
        variance 0.5 + 0.01 randn clipped to [0.001, 1] (predict.py:71-72), drawn once; a restart begins at the best variances so far.  The global numpy
        random stream is consumed in the reference's order (index, variances, one index per restart)."""
        self.Y_test = numpy.atleast_2d(numpy.asarray(Y_test, dtype=float))
        Z = numpy.asarray(self.gs['Z'], dtype=float)
        if X_mu0 is not None:
            X_mu0, random_restarts = numpy.atleast_2d(numpy.asarray(X_mu0, dtype=float)), 0
        elif is_random_init:
            X_mu0 = numpy.atleast_2d(Z[numpy.random.randint(self.M)])               # predict.py:38-41
        else:
            if training is None:
                raise AssertionError('predict.test needs the training shards (training=...) or an initial mean (X_mu0=...)')
            random_restarts = 0                                                     # predict.py:43
            assert nearest in ('host', 'device'), "nearest must be 'host' or 'device'"
            if nearest == 'device':
                cls = self._engine_cls
                if cls is None:
                    from .engine import ShardEngine as cls
                eng = cls(1, self.D, self.M, self.Q, device=self.device)          # host rows pass through it: no model is needed
                try:
                    X_mu0 = self._nearest_on_device(eng, self.Y_test, training, mask)
                finally:
                    eng.close()
            else:
                X_mu0 = self.nearest_training_embeddings(self.Y_test, training, self.Q, mask)
        self.shape = X_mu0.shape
        if X_S0 is None:
            X_S0 = numpy.clip(numpy.ones(self.shape) * 0.5 + 0.01 * numpy.random.randn(*self.shape), 0.001, 1)   # predict.py:71-72
        X_S0 = numpy.asarray(X_S0, dtype=float)
        n = int(numpy.prod(self.shape))
        self.bounds = [(None, None)] * n + [(0, None)] * n
        best = self._optimise(X_mu0, X_S0, iterations)
        for _ in range(int(random_restarts) if is_random_init else 0):              # predict.py:93-108
            # the restart begins at the variances of the best result so far, not at the first draw (predict.py:87, 97-98, 105: X_S is rebound)
            trial = self._optimise(numpy.atleast_2d(Z[numpy.random.randint(self.M)]), best[1], iterations)
            if trial[2] > best[2]:
                best = trial
        return best


def test(options_, Y_test_, mask=None, is_random_init=False, random_iterations=100, random_restarts=100, device=0, map_reduce=None):
    """The reference's entry point (predict.test, predict.py:19-111) with its signature: mean, variance and likelihood of new points given
    the trained model that ``options`` describes (its ``statistics`` directory holds global_statistics_*_f.npy and
    accumulated_statistics_*_f.npy, its ``input`` / ``embeddings`` directories the training shards).  options['N'] must be populated."""
    import os
    from . import driver
    if map_reduce is None:
        from . import gpu_MapReduce as map_reduce
    options = dict(options_)
    options['load'] = True
    options, gs = driver.init_statistics(map_reduce, options)                       # predict.py:28-29 (the load branch)
    acc = {key: map_reduce.load(options['statistics'] + '/accumulated_statistics_' + key + '_f.npy')
           for key in ('sum_YYT', 'sum_exp_K_mi_K_im', 'sum_exp_K_miY', 'sum_exp_K_ii', 'sum_KL')}
    p = Predictor(gs, acc, options['N'], options['D'], device=device)

    def training():
        for name in sorted(os.listdir(options['input'] + '/')):                     # one shard in memory at a time
            yield (map_reduce._read_csv(options['input'] + '/' + name),
                   map_reduce.load(options['embeddings'] + '/' + name + '.embedding.npy'))

    return p.test(Y_test_, iterations=random_iterations, training=None if is_random_init else training(), mask=mask,
                  is_random_init=is_random_init, random_restarts=random_restarts)
