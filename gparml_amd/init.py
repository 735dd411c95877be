"""The initialisations on the device: the k-means and the greedy conditional-variance selection that place the inducing points, the PCA that turns
Y into the starting embeddings, and the nearest-training-row search that starts the latent inference of new rows.

k-means.  ``parallel_GPLVM.init_statistics`` calls ``scipy.cluster.vq.kmeans(embeddings, M)`` on the host, over the first shards that reach M rows
(parallel_GPLVM.py:179-186).  A pass of that loop is N K Q distance terms -- an hour of host time at N = 1e6, M = 512 with scipy's twenty
restarts -- and it has the map-reduce shape of an evaluation: every shard yields per-centre sums, counts and summed
distances (``ShardEngine.kmeans_accumulate``, csrc/kmeans.hip), which add over shards and ranks.  ``kmeans`` here is scipy's ``_kmeans``
loop restated on those sums: given the same seeds it returns what ``scipy.cluster.vq.kmeans(X_all, seeds, thresh=thresh)`` returns.

Greedy selection.  ``greedy_select`` is the kernel-aware placement: the pivoted Cholesky factorisation of K_nn (Burt, Rasmussen and van der Wilk
2019; csrc/select.hip), one deterministic pass of K steps whose every point is a data row and which reports, after every step, the Nystrom
residual tr(K_nn - K_nm K_mm^-1 K_mn) the collapsed bound is penalised by.  Each part updates its own rows; one pivot per step crosses parts.

PCA (the second half of this file).  ``supporting_functions.PCA`` (supporting_functions.py:102-121: left singular vectors of the centred data,
each scaled to unit standard deviation) runs over ALL data (local_MapReduce.py:50-65: per-subset PCA "gives rise to rotation problems").  The
same axes are the eigenvectors of the D x D scatter matrix, a SUM over shards and ranks: ``ShardEngine.scatter_accumulate`` (csrc/pca.hip) yields
per shard the column sums and the Gram matrix of the rows shifted by a centre, ``pca_axes`` is the eigen part on the host,
``ShardEngine.project_rows`` projects; ``pca`` drives the passes.

Nearest start (the end of this file).  ``predict.test`` starts every new point at the trained embedding of the training output nearest to it,
searched shard by shard with a k-d tree on the host (predict.py:44-66).  ``ShardEngine.nearest_rows`` (csrc/nearest.hip) yields per shard and new
row the least squared distance and its row; ``nearest_start`` takes the minimum over shards and ranks with the reference's tie rule and cut-off.

Neighbours in latent space (after it).  ``ShardEngine.knn_rows`` (csrc/knn.hip) yields per shard and query the k nearest rows of the embedding,
optionally in the ARD metric and without the query's own row; ``knn_merge`` / ``knn`` merge the shards' lists by (distance, shard, row) on the host
and ``knn_vote`` turns the neighbours' labels into the k-NN classification that GPLVM papers score an embedding by.
"""
import numpy


class HostRows(object):
    """A part of ``kmeans`` that passes host rows X (n, Q) through an engine (any object with ShardEngine's ``kmeans_accumulate``)."""

    def __init__(self, engine, X):
        self.engine = engine
        self.X = numpy.ascontiguousarray(X, dtype=numpy.float64)
        self.n_rows, self.Q = self.X.shape
        self.device = getattr(engine, 'device', 0)

    def kmeans_accumulate(self, centres, want_labels=False):
        return self.engine.kmeans_accumulate(centres, X=self.X, want_labels=want_labels)

    def take_rows(self, idx):
        return self.X[numpy.asarray(idx, dtype=numpy.int64)]

    # knn: the rows of this part are the training rows; without queries they are the queries too
    def knn_rows(self, X=None, k=1, weight=None, skip_self=False):
        assert X is None or not skip_self, 'knn_rows: skip_self needs the part\'s own rows as queries'
        skip = numpy.arange(self.n_rows, dtype=numpy.int64) if skip_self else None
        return self.engine.knn_rows(X=self.X if X is None else X, k=k, X_train=self.X, weight=weight, skip=skip)

    def knn_queries(self):
        return self.X

    # greedy_select: the selection lives in the engine, one at a time -- every part of one call needs an engine of its own
    def select_begin(self, K, sf2, alpha, tol=1e-10):
        return self.engine.select_begin(K, sf2, alpha, tol=tol, X=self.X)

    def select_run(self, steps):
        return self.engine.select_run(steps)

    def select_candidate(self, steps_done):
        return self.engine.select_candidate(steps_done)

    def select_apply(self, x_p, l_p, d_p, own_row=-1):
        return self.engine.select_apply(x_p, l_p, d_p, own_row=own_row)

    def select_end(self):
        return self.engine.select_end()


class _Ranks(object):
    """Sums over the ranks of a torch.distributed group, as ResidentModel._allreduce_vector does; the identity without one."""

    def __init__(self, dist_group, device):
        self.dist, self.group, self.device = None, dist_group, device
        self.rank, self.world = 0, 1
        if dist_group is not None:
            import torch.distributed as dist
            self.dist = dist
            if dist_group is True:                   # the default group
                self.group = None
            self.rank, self.world = dist.get_rank(self.group), dist.get_world_size(self.group)

    def sum(self, values):
        values = numpy.asarray(values, dtype=numpy.float64)
        if self.dist is None:
            return values
        import torch
        t = torch.tensor(values.ravel(), dtype=torch.float64,
                         device=torch.device('cuda', self.device) if self.dist.get_backend(self.group) == 'nccl' else 'cpu')
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group)
        return t.cpu().numpy().reshape(values.shape)


def _draw_seeds(parts, K, Q, rng, ranks):
    """K distinct rows over all parts of all ranks (scipy's _kpoints draws rows of its one matrix): global row indices in the order rank, part,
    row.  Every rank draws, so that equal generators stay in step; rank 0's draw is the one used."""
    local = [int(p.n_rows) for p in parts]
    per_rank = numpy.zeros(ranks.world)
    per_rank[ranks.rank] = sum(local)
    per_rank = ranks.sum(per_rank).astype(numpy.int64)
    total = int(per_rank.sum())
    assert total >= K, 'k-means: %d seeds wanted from %d rows' % (K, total)
    idx = numpy.asarray(rng.choice(total, K, replace=False), dtype=numpy.float64)
    idx = ranks.sum(idx if ranks.rank == 0 else numpy.zeros(K)).astype(numpy.int64)
    seeds = numpy.zeros((K, Q))
    start = int(per_rank[:ranks.rank].sum())
    for p, n in zip(parts, local):
        mine = numpy.nonzero((idx >= start) & (idx < start + n))[0]
        if mine.size:
            seeds[mine] = p.take_rows(idx[mine] - start)
        start += n
    return ranks.sum(seeds)


def _lloyd(parts, code, thresh, max_iters, ranks):
    """scipy.cluster.vq._kmeans: assign, average, drop the centres without members, until the mean distance moves by at most ``thresh``.  Returns
    the centres AFTER the last averaging and the mean distance BEFORE it, as scipy does, and the number of passes."""
    prev, passes = numpy.inf, 0
    while True:
        K, Q = code.shape
        acc = numpy.zeros(K * Q + K + 2)             # sums | counts | sum d^2, sum d: one vector, one collective per pass
        for p in parts:
            sums, counts, dist2 = p.kmeans_accumulate(code)[:3]
            acc[:K * Q] += numpy.asarray(sums, dtype=float).ravel()
            acc[K * Q:K * Q + K] += counts
            acc[K * Q + K:] += dist2
        acc = ranks.sum(acc)
        sums, counts = acc[:K * Q].reshape(K, Q), acc[K * Q:K * Q + K]
        avg = acc[K * Q + K + 1] / counts.sum()
        has = counts > 0
        code = sums[has] / counts[has, None]
        passes += 1
        diff, prev = abs(prev - avg), avg
        if not diff > thresh or passes >= max_iters:
            return code, avg, passes


def kmeans(parts, K, seeds=None, thresh=1e-5, max_iters=1000, restarts=1, rng=None, dist_group=None):
    """k-means over the rows of all ``parts``.  Returns (centres (<= K, Q), mean Euclidean distance of a row to its centre, passes).

    parts: objects with ``kmeans_accumulate(centres) -> (sums (K, Q), counts (K,), [sum d^2, sum d], ...)``: ShardEngines with resident embeddings,
    or ``HostRows(engine, X)``.  Drawing seeds also needs their ``Q``, ``n_rows`` and ``take_rows(idx)``.
    seeds (K, Q): the starting centres; ``restarts`` is then ignored, as scipy ignores ``iter`` with a guess.  None: K distinct rows over all
    parts, drawn with ``rng`` (``choice``; default: numpy's global stream), ``restarts`` times, keeping the run with the lowest mean distance.
    dist_group: a torch.distributed group (True: the default group) whose ranks each hold some of the parts: sums, counts and distances are
    all-reduced, every rank returns the same centres.  COLLECTIVE: every rank calls with the same K, seeds, thresh, max_iters and restarts.
    Centres that lose all their members are dropped (the caller tops up: driver.init_statistics)."""
    parts = list(parts)
    assert parts and int(K) >= 1
    ranks = _Ranks(dist_group, getattr(parts[0], 'device', 0))
    if seeds is not None:
        seeds = numpy.atleast_2d(numpy.asarray(seeds, dtype=numpy.float64))
        assert seeds.shape[0] == K, 'seeds shape %s: %d rows expected' % (seeds.shape, K)
        return _lloyd(parts, seeds, thresh, max_iters, ranks)
    if rng is None:
        rng = numpy.random
    Q = int(parts[0].Q)
    best = None
    for _ in range(max(1, int(restarts))):
        run = _lloyd(parts, _draw_seeds(parts, int(K), Q, rng, ranks), thresh, max_iters, ranks)
        if best is None or run[1] < best[1]:
            best = run
    return best


# ------------------------------------------------------------------------------------------------- greedy selection
def greedy_select(parts, K, sf2, alpha, tol=1e-10, dist_group=None):
    """Greedy conditional-variance selection of up to K rows over the rows of all ``parts`` under the kernel
    sf2 exp(-1/2 sum_q alpha_q (x_q - z_q)^2).  Returns (Z (K', Q), pivots (K', 2) int64, trace (K',)): the selected rows in the order they were
    chosen, each as (part, row) -- the part counted over all ranks in the order rank, part -- and after every step the trace of the Nystrom
    residual over all rows.  K' < K when the largest conditional variance left is <= ``tol`` sf2 (or the rows ran out): the data has no more than
    K' points the kernel tells apart.

    parts: as for ``kmeans`` -- ShardEngines with resident embeddings, or ``HostRows(engine, X)``, each with an engine of its OWN (an engine
    holds one selection).  One part and no ranks: every step runs on the device without a host round trip (``select_run``).  Several parts, or
    ranks: per step every part offers its best row (``select_candidate``), the largest conditional variance wins -- of equal ones the lowest
    (rank, part, row) -- and every part applies that pivot (``select_apply``); the same pivots and the same bits of L and d as one part.
    dist_group: a torch.distributed group (True: the default group) whose ranks each hold some of the parts.  COLLECTIVE then: every rank calls
    with the same K, sf2, alpha and tol, and every rank returns the same arrays."""
    parts = list(parts)
    K = int(K)
    assert parts and K >= 1
    owners = [id(getattr(p, 'engine', p)) for p in parts]
    assert len(set(owners)) == len(owners), 'greedy_select: every part needs an engine of its own (an engine holds one selection)'
    ranks = _Ranks(dist_group, getattr(parts[0], 'device', 0))
    alpha = numpy.asarray(alpha, dtype=numpy.float64).reshape(-1)
    Q = alpha.size
    begun = []
    try:
        for p in parts:
            p.select_begin(K, sf2, alpha, tol=tol)
            begun.append(p)
        if len(parts) == 1 and ranks.world == 1:
            rows, trace = parts[0].select_run(K)
            Z = numpy.asarray(parts[0].take_rows(rows), dtype=numpy.float64).reshape(len(rows), Q)
            return Z, numpy.stack([numpy.zeros(len(rows), dtype=numpy.int64), rows], axis=1), trace
        counts = numpy.zeros(ranks.world)
        counts[ranks.rank] = len(parts)
        first_part = int(round(ranks.sum(counts)[:ranks.rank].sum()))
        Z, pivots, trace = [], [], []
        for j in range(K):
            best = (-numpy.inf, -1, -1, None, None)                      # d, part, row, x, l
            for k, p in enumerate(parts):
                d, row, x, l = p.select_candidate(j)
                if row >= 0 and d > best[0]:                             # strict: of equal ones the lowest part
                    best = (d, k, row, x, l)
            slots = numpy.zeros(ranks.world)
            slots[ranks.rank] = best[0]
            slots = ranks.sum(slots)
            winner = int(numpy.argmax(slots))                            # the first of equal maxima: the lowest rank
            d_p = float(slots[winner])
            if not d_p > float(tol) * float(sf2):                        # the stopping rule, on the bits the device would compare
                break
            rec = numpy.full(2 + Q + j, -0.0)                            # -0.0: the identity of the sum, also for a winner's -0.0
            if winner == ranks.rank:
                rec[0], rec[1], rec[2:2 + Q], rec[2 + Q:] = first_part + best[1], best[2], best[3], best[4]
            rec = ranks.sum(rec)
            x_p, l_p = rec[2:2 + Q], rec[2 + Q:]
            t = 0.0
            for k, p in enumerate(parts):
                t += p.select_apply(x_p, l_p, d_p, own_row=best[2] if (winner == ranks.rank and k == best[1]) else -1)
            trace.append(float(ranks.sum(numpy.array([t]))[0]))
            Z.append(numpy.array(x_p))
            pivots.append((int(round(rec[0])), int(round(rec[1]))))
        return (numpy.array(Z, dtype=numpy.float64).reshape(len(Z), Q), numpy.array(pivots, dtype=numpy.int64).reshape(len(pivots), 2),
                numpy.array(trace, dtype=numpy.float64))
    finally:
        for p in begun:
            p.select_end()


# ------------------------------------------------------------------------------------------------- PCA
def pca_axes(n_tot, shift, ssum, gram, Q):
    """The eigen part of the streaming PCA.  n_tot rows; ``ssum`` (D,) and ``gram`` (D, D) are the sums over all rows of (y - shift) and of
    (y - shift)(y - shift)^T for a provisional centre ``shift`` (near the mean: the correction for the true mean then stays small against the
    scatter).  Returns (mean (D,), V (D, Q), std (Q,)): the embeddings are (Y - mean) V / std, identical to supporting_functions.PCA's SVD form up
    to the sign of a component (fixed here: the largest entry of every axis is positive) and rounding.  Raises LinAlgError when the data has fewer
    than Q principal directions."""
    delta = ssum / n_tot                                            # true mean - provisional centre
    scatter = gram - n_tot * numpy.outer(delta, delta)
    lam, V = numpy.linalg.eigh(scatter)
    order = numpy.argsort(lam)[::-1][:Q]
    lam, V = lam[order], V[:, order]
    # rank-deficient data (Q beyond the rank of the centred data, or cancellation in the mean correction) leaves zero or slightly negative
    # trailing eigenvalues: dividing by their root would write inf / nan embeddings without a word (the reference's SVD form divides by a
    # tiny standard deviation in the same case and returns noise)
    floor = numpy.finfo(float).eps * max(float(lam[0]), 0.0) * scatter.shape[0]
    if not (lam[-1] > floor):
        raise numpy.linalg.LinAlgError('PCA initialisation: the data has fewer than Q = %d principal directions (eigenvalue %d of the scatter '
                                       'matrix is %.3e against a largest one of %.3e)' % (Q, int(numpy.sum(lam > floor)) + 1, lam[-1], lam[0]))
    V = V * numpy.sign(V[numpy.argmax(numpy.abs(V), axis=0), numpy.arange(V.shape[1])])[None, :]
    return shift + delta, V, numpy.sqrt(lam / n_tot)                # std: X.std(axis=0) of the projected data (ddof = 0)


class HostY(object):
    """A part of ``pca`` that passes host rows through an engine (any object with ShardEngine's ``scatter_accumulate`` / ``project_rows``).
    ``Y``: the rows (n, D), or a callable returning them, called once per pass (a shard that is parsed from its file and not kept); ``n_rows`` is
    then required."""

    def __init__(self, engine, Y, n_rows=None):
        self.engine = engine
        self._Y = Y if callable(Y) else numpy.ascontiguousarray(numpy.atleast_2d(Y), dtype=numpy.float64)
        self.n_rows = int(n_rows) if callable(Y) else self._Y.shape[0]
        self.D = engine.D

    def _rows(self):
        return self._Y() if callable(self._Y) else self._Y

    def scatter_accumulate(self, centre, want_gram=True):
        return self.engine.scatter_accumulate(centre, Y=self._rows(), want_gram=want_gram)

    def project_rows(self, mean, P):
        return self.engine.project_rows(mean, P, Y=self._rows())


def pca(parts, Q, allreduce=None):
    """PCA over the rows of all ``parts`` of all ranks.  Returns (mean (D,), V (D, Q), std (Q,), X): X the list of this rank's projected parts,
    (Y_part - mean) V / std.

    parts: objects with ``scatter_accumulate(centre, want_gram=True) -> (sum, gram)``, ``project_rows(mean, P) -> X``, ``n_rows`` and ``D``:
    ShardEngines with resident data, or ``HostY(engine, Y)``.
    allreduce: a function that sums a float64 vector over the ranks holding the other parts (None: this process holds them all).  Its result
    is bit-identical on every rank, so every rank gets the same axes.  COLLECTIVE then: three calls, in this order.
    Pass 1 sums the rows (centre 0) for the global mean; pass 2 accumulates sums and Gram matrix centred on that mean -- the centre is
    subtracted before the products, so nothing cancels; pass 3 projects."""
    parts = list(parts)
    assert parts and int(Q) >= 1
    D = int(parts[0].D)
    red = allreduce if allreduce is not None else (lambda v: v)
    acc = numpy.zeros(D + 1)
    for p in parts:
        acc[:D] += p.scatter_accumulate(numpy.zeros(D), want_gram=False)[0]
        acc[D] += p.n_rows
    acc = numpy.asarray(red(acc), dtype=numpy.float64)
    n_tot = int(round(acc[D]))
    assert n_tot >= 1, 'PCA initialisation: no rows'
    centre = acc[:D] / n_tot
    acc = numpy.zeros(D + D * D)
    for p in parts:
        ssum, gram = p.scatter_accumulate(centre)
        acc[:D] += ssum
        acc[D:] += gram.ravel()
    acc = numpy.asarray(red(acc), dtype=numpy.float64)
    mean, V, std = pca_axes(n_tot, centre, acc[:D], acc[D:].reshape(D, D), int(Q))
    P = V / std
    return mean, V, std, [p.project_rows(mean, P) for p in parts]


# ------------------------------------------------------------------------------------------------- nearest start
def nearest_start(parts, Y_test, cols=None, cutoff=6.0, allreduce=None, rank=0, world=1, observed=None):
    """The starting means of latent inference: every row of ``Y_test`` (n, D) gets the embedding of the training row nearest to it over the
    output columns ``cols`` (None: all), as ``Predictor.nearest_training_embeddings`` (predict.py:44-66) does with a k-d tree per shard.
    Returns (X_mu0 (n, Q), dist (n,), owner (n,), index (n,)): the means, the Euclidean distance to the nearest training row (inf without one),
    the part that holds it (counted over all ranks in the order rank, part) and its row there; owner and index are -1 where the mean stayed zero.
    ``observed`` (n, D) bool instead of ``cols``: every row is compared over its own observed columns, in one masked search per part
    (``ShardEngine.nearest_rows(observed=)``); the part, rank and cut-off rules are the same.

    parts: an iterable (taken one at a time: a generator keeps one shard in memory) of engines whose resident rows and base means are searched
    (``ShardEngine.nearest_rows``), or of (engine, Y_shard, X_shard) for host rows passed through the engine.
    The rules are the reference's: inside a part the lowest row wins ties; a later part replaces the best only when strictly nearer
    (predict.py:63); a new row whose nearest distance is not < ``cutoff`` keeps a zero mean (cKDTree's distance_upper_bound is strict: a row at
    exactly 6.0 is not returned, one at nextafter(6, 0) is).
    allreduce: a function that sums a float64 vector over the ranks holding the other parts (None: this process holds them all), as
    ``pca`` takes; ``rank`` and ``world`` are then this process' place among them.  The minimum distance over the ranks wins, among the ranks that
    hold it the lowest, and that rank's row is summed out to all.  COLLECTIVE then: two calls -- every rank's distances (each in a slot of its
    own: a sum that gathers), then the winners' rows -- and every rank returns the same arrays."""
    Y_test = numpy.atleast_2d(numpy.asarray(Y_test, dtype=numpy.float64))
    n = Y_test.shape[0]
    assert cols is None or observed is None, 'nearest_start: cols and observed are alternatives'
    which = dict(cols=cols) if observed is None else dict(observed=observed)
    best = numpy.full(n, numpy.inf)
    owner, index = numpy.full(n, -1, dtype=numpy.int64), numpy.full(n, -1, dtype=numpy.int64)
    X, n_parts = None, 0
    for k, part in enumerate(parts):
        if isinstance(part, (tuple, list)):
            engine, Ys, Xs = part
            d2, idx, _ = engine.nearest_rows(Y_test, Y_train=Ys, want_x=False, **which)
            Xs = numpy.asarray(Xs, dtype=numpy.float64)
            x = numpy.zeros((n, Xs.shape[1]))
            x[idx >= 0] = Xs[idx[idx >= 0]]
        else:
            d2, idx, x = part.nearest_rows(Y_test, **which)
        if X is None:
            X = numpy.zeros((n, x.shape[1]))
        closer = (d2 < best) & (idx >= 0)                     # strict: an equally near row of a later part does not win
        best[closer], owner[closer], index[closer], X[closer] = d2[closer], k, idx[closer], x[closer]
        n_parts = k + 1
    if allreduce is not None:
        world, rank = int(world), int(rank)
        assert 0 <= rank < world, 'nearest_start: rank %d of %d' % (rank, world)
        slots = numpy.zeros((world, n + 2))                   # a rank's distances | its number of parts | its Q (0 without parts)
        slots[rank, :n], slots[rank, n], slots[rank, n + 1] = best, n_parts, 0 if X is None else X.shape[1]
        slots = numpy.asarray(allreduce(slots.ravel()), dtype=numpy.float64).reshape(world, n + 2)
        winner = numpy.argmin(slots[:, :n], axis=0)           # the first of equal minima: the lowest rank
        best = slots[winner, numpy.arange(n)]
        first_part, Q = int(round(slots[:rank, n].sum())), int(round(slots[:, n + 1].max()))
        mine = (winner == rank) & (index >= 0)
        row = numpy.full((n, Q + 2), -0.0)                    # -0.0: the identity of the sum, also for a winner's -0.0
        if mine.any():
            row[mine, :Q], row[mine, Q], row[mine, Q + 1] = X[mine], first_part + owner[mine], index[mine]
        row = numpy.asarray(allreduce(row.ravel()), dtype=numpy.float64).reshape(n, Q + 2)
        found = numpy.isfinite(best)
        X = numpy.where(found[:, None], row[:, :Q], 0.0)
        owner = numpy.where(found, numpy.round(row[:, Q]), -1).astype(numpy.int64)
        index = numpy.where(found, numpy.round(row[:, Q + 1]), -1).astype(numpy.int64)
    assert X is not None and X.shape[1] >= 1, 'nearest_start: no parts'
    dist = numpy.sqrt(best)
    far = ~(dist < cutoff)
    X[far], owner[far], index[far] = 0.0, -1, -1
    return X, dist, owner, index


# ------------------------------------------------------------------------------------------------- neighbours in latent space
def knn_merge(lists, k):
    """Merges per-shard neighbour lists into one: ``lists`` holds per shard (dist2 (n, k_s), rows (n, k_s)) as ``ShardEngine.knn_rows`` returns
    them (row -1: an empty slot).  Returns (dist2 (n, k), shard (n, k), row (n, k)): per query the k least of all pairs in the order
    (dist2, shard, row), ascending; slots beyond the available rows hold inf, -1, -1.  Pure numpy."""
    k = int(k)
    d2 = numpy.concatenate([numpy.asarray(d, dtype=numpy.float64).reshape(len(d), -1) for d, _ in lists], axis=1)
    row = numpy.concatenate([numpy.asarray(r, dtype=numpy.int64).reshape(len(r), -1) for _, r in lists], axis=1)
    shard = numpy.concatenate([numpy.full(numpy.asarray(r).reshape(len(r), -1).shape, s, dtype=numpy.int64) for s, (_, r) in enumerate(lists)], axis=1)
    empty = row < 0
    d2 = numpy.where(empty, numpy.inf, d2)
    # lexsort: the last key is the primary one; an empty slot comes behind every row, also behind one at an infinite distance
    order = numpy.lexsort((row, shard, empty, d2), axis=1)[:, :k]
    take = lambda a: numpy.take_along_axis(a, order, axis=1)
    d2, shard, row = take(d2), numpy.where(take(empty), -1, take(shard)), take(row)
    if d2.shape[1] < k:
        pad = ((0, 0), (0, k - d2.shape[1]))
        d2, shard, row = numpy.pad(d2, pad, constant_values=numpy.inf), numpy.pad(shard, pad, constant_values=-1), numpy.pad(row, pad, constant_values=-1)
    return d2, shard, row


def knn(parts, X, k, weight=None, skip_self=False):
    """The ``k`` nearest training rows of every query over all shards: (dist2 (n, k), shard (n, k), row (n, k)), ascending in
    (dist2, shard, row); slots beyond the available rows hold inf, -1, -1.

    parts: objects with ``knn_rows(X, k, weight=, skip_self=)`` and ``knn_queries()``: ShardEngines (their resident X_mu are the training rows),
    or ``HostRows`` for host rows passed through an engine.  ``X`` (n, Q): the queries.  ``X`` None: every shard's own rows are the queries, in
    shard order (n = all rows), each searched in every shard; with ``skip_self`` a query's own row is left out -- only in its own shard, where
    it is a row.  ``weight`` (Q,): the metric sum_q weight_q (x_q - t_q)^2 (None: Euclidean).
    The parts are those of THIS process: merging across the ranks of a dist_group is not done here."""
    parts = list(parts)
    assert parts, 'knn: no parts'
    if X is not None:
        assert not skip_self, 'knn: skip_self needs the shards\' own rows as queries (X None)'
        return knn_merge([p.knn_rows(X, k, weight=weight) for p in parts], k)
    out = []
    for i, p in enumerate(parts):
        Xi = p.knn_queries() if len(parts) > 1 else None
        out.append(knn_merge([q.knn_rows(None, k, weight=weight, skip_self=skip_self) if j == i else q.knn_rows(Xi, k, weight=weight)
                              for j, q in enumerate(parts)], k))
    return tuple(numpy.concatenate([o[a] for o in out], axis=0) for a in range(3))


def knn_vote(labels_of_neighbours, dist2=None):
    """k-NN classification from neighbour lists: ``labels_of_neighbours`` (n, k) holds the labels of every query's neighbours, nearest first;
    slots whose ``dist2`` (n, k) is not finite are empty (None: none is).  Returns (n,) the majority label of every query; a tie goes to the tied
    label whose nearest member comes first in the list; -1 for a query without neighbours."""
    L = numpy.asarray(labels_of_neighbours)
    L = L.reshape(len(L), -1)
    valid = numpy.ones(L.shape, dtype=bool) if dist2 is None else numpy.isfinite(numpy.asarray(dist2, dtype=numpy.float64).reshape(L.shape))
    # votes[i, j]: the members of query i's list that carry the label of slot j; argmax takes the first slot of the largest count
    votes = ((L[:, :, None] == L[:, None, :]) & valid[:, None, :]).sum(axis=2) * valid
    if L.shape[1] == 0:
        return numpy.full(len(L), -1, dtype=numpy.int64)
    best = numpy.argmax(votes, axis=1)
    out = L[numpy.arange(len(L)), best]
    return numpy.where(valid.any(axis=1), out, -1)
