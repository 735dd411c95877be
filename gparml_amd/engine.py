"""One data shard resident on one GPU: the two-phase bound+gradient evaluation.

    phase1 (statistics_mapper, local_MapReduce.py:183-248)  -> packed statistics  [all-reduce]
    global_step (parallel_GPLVM.py:302-369)                 -> F, dF_d*, grad_beta, Kmm parts
    phase2 (embeddings_mapper, local_MapReduce.py:310-363 + the Z/alpha sums) -> packed gradient sums [all-reduce]
    finish                                                  -> grad_Z, grad_alpha, grad_sf2, grad_beta
"""
import ctypes

import numpy as np

from . import _lib
from .evaluation import evaluate


class ShardEngine(object):
    def __init__(self, N_s, D, M, Q, device=0):
        self.lib = _lib.load()
        self.N_s, self.D, self.M, self.Q, self.device = int(N_s), int(D), int(M), int(Q), int(device)
        h = ctypes.c_void_p()
        rc = self.lib.gp_create(ctypes.byref(h), self.device, self.N_s, self.D, self.M, self.Q)
        _lib.raise_for(rc, self.lib, None, 'gp_create')
        self.h = h
        self._keep = []

    # ---- lifetime ---------------------------------------------------------------------------------
    def close(self):
        self.globals_key = None
        if getattr(self, 'h', None):
            self.lib.gp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        _lib.raise_for(rc, self.lib, self.h, what)

    def set_stream(self, stream_ptr):
        self._ck(self.lib.gp_set_stream(self.h, ctypes.c_void_p(stream_ptr)), 'gp_set_stream')

    # ---- data -------------------------------------------------------------------------------------
    def upload_shard(self, Y, X_mu, X_S, xs_is_raw=False):
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim == 1:
            Y = Y[:, None]
        assert Y.shape == (self.N_s, self.D), 'Y shape %s != (%d, %d)' % (Y.shape, self.N_s, self.D)
        X_mu = np.asarray(X_mu, dtype=np.float64)
        X_S = np.asarray(X_S, dtype=np.float64)
        assert X_mu.ndim == 2 and X_S.ndim == 2 and X_mu.shape == X_S.shape == (self.N_s, self.Q)   # kernel_exp.py:32-34
        Y, pY = _lib.as_c(Y)
        X_mu, pm = _lib.as_c(X_mu)
        X_S, ps = _lib.as_c(X_S)
        self.globals_key = None
        self._ck(self.lib.gp_upload_shard(self.h, pY, pm, ps, 1 if xs_is_raw else 0), 'gp_upload_shard')
        self.xs_is_raw = bool(xs_is_raw)

    def upload_embeddings(self, X_mu, X_S, xs_is_raw=False):
        X_mu = np.asarray(X_mu, dtype=np.float64)
        X_S = np.asarray(X_S, dtype=np.float64)
        assert X_mu.shape == X_S.shape == (self.N_s, self.Q)
        X_mu, pm = _lib.as_c(X_mu)
        X_S, ps = _lib.as_c(X_S)
        self.globals_key = None
        self._ck(self.lib.gp_upload_embeddings(self.h, pm, ps, 1 if xs_is_raw else 0), 'gp_upload_embeddings')
        self.xs_is_raw = bool(xs_is_raw)

    xs_is_raw = False         # the form the resident variances are stored in (the last upload's; gather_from takes the source's)

    @staticmethod
    def _rows_i64(rows, n):
        rows = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.int64)
        assert rows.shape == (n,), '%d rows for a context of %d' % (rows.size, n)
        return rows, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))

    def gather_from(self, src, rows):
        """This engine then holds what upload_shard(Y[rows], X_mu[rows], X_S[rows]) of ``src``'s resident arrays would leave, bit for bit, without
        a host copy (gp_gather_shard): ``rows`` (N_s,) indices into src, any order, repeats allowed; same device, same D and Q."""
        rows, pr = self._rows_i64(rows, self.N_s)
        self.globals_key = None
        self._ck(self.lib.gp_gather_shard(self.h, src.h, self.N_s, pr), 'gp_gather_shard')
        self.xs_is_raw = src.xs_is_raw

    def scatter_embeddings_to(self, dst, rows):
        """This engine's X_mu / X_S rows 0 .. N_s - 1 into ``dst``'s rows ``rows`` (strictly ascending), as dst.upload_embeddings of the edited
        arrays would (gp_scatter_embeddings); Y is never written back."""
        rows, pr = self._rows_i64(rows, self.N_s)
        dst.globals_key = None
        dst._ck(dst.lib.gp_scatter_embeddings(dst.h, self.h, self.N_s, pr), 'gp_scatter_embeddings')

    def set_direction(self, d):
        self.globals_key = None
        if d is None:
            self._ck(self.lib.gp_set_direction(self.h, None), 'gp_set_direction')
            return
        d = np.asarray(d, dtype=np.float64)
        assert d.shape == (2, self.N_s, self.Q)
        d, pd = _lib.as_c(d)
        self._ck(self.lib.gp_set_direction(self.h, pd), 'gp_set_direction')

    # What the device holds of the globals: the key of the last set_globals, None once anything has moved the context away from the evaluation that call
    # started (a new shard, new embeddings, a direction, a CG update, close).  set_globals itself never skips; a caller that wants to push each distinct
    # set once (partial_terms._push_globals) compares its own key with this one.
    globals_key = None

    @staticmethod
    def make_globals_key(Z, sf2, alpha, beta, N_global, step_size=0.0):
        return (np.ascontiguousarray(Z, dtype=np.float64).tobytes(), float(sf2), np.ascontiguousarray(alpha, dtype=np.float64).tobytes(), float(beta),
                int(N_global), float(step_size))

    def set_globals(self, Z, sf2, alpha, beta, N_global=None, step_size=0.0):
        Z = np.asarray(Z, dtype=np.float64)
        assert Z.shape == (self.M, self.Q)
        alpha = np.atleast_1d(np.asarray(alpha, dtype=np.float64).squeeze())
        assert alpha.shape == (self.Q,)
        Z, pZ = _lib.as_c(Z)
        alpha, pa = _lib.as_c(alpha)
        Ng = self.N_s if N_global is None else int(N_global)
        self.globals_key = None
        self._ck(self.lib.gp_set_globals(self.h, pZ, float(sf2), pa, float(beta), Ng, float(step_size)), 'gp_set_globals')
        self.globals_key = (Z.tobytes(), float(sf2), alpha.tobytes(), float(beta), Ng, float(step_size))     # make_globals_key on what as_c made

    # ---- evaluation ---------------------------------------------------------------------------------
    def phase1(self):
        self._ck(self.lib.gp_phase1(self.h), 'gp_phase1')

    def stats_packed_buffer(self):
        """Psi2 upper triangle | C (M*D) | scalars: the payload of the all-reduce across processes (stats_pack / stats_unpack)."""
        p, n = ctypes.c_void_p(), ctypes.c_int64()
        self._ck(self.lib.gp_stats_packed_buffer(self.h, ctypes.byref(p), ctypes.byref(n)), 'gp_stats_packed_buffer')
        return p.value, n.value

    def stats_pack(self):
        self._ck(self.lib.gp_stats_pack(self.h), 'gp_stats_pack')

    def stats_unpack(self):
        self._ck(self.lib.gp_stats_unpack(self.h), 'gp_stats_unpack')

    def stats_buffer(self):
        p, n = ctypes.c_void_p(), ctypes.c_int64()
        self._ck(self.lib.gp_stats_buffer(self.h, ctypes.byref(p), ctypes.byref(n)), 'gp_stats_buffer')
        return p.value, n.value

    def grads_buffer(self):
        p, n = ctypes.c_void_p(), ctypes.c_int64()
        self._ck(self.lib.gp_grads_buffer(self.h, ctypes.byref(p), ctypes.byref(n)), 'gp_grads_buffer')
        return p.value, n.value

    # ---- the reduce across GPUs inside the library (RCCL resolved with dlopen; include/gparml_hip.h gp_comm_*) -------------------------
    @staticmethod
    def comm_unique_id():
        """128-byte ncclUniqueId (rank 0 calls this and hands the bytes to every other rank)."""
        lib = _lib.load()
        buf = ctypes.create_string_buffer(_lib.GP_COMM_ID_BYTES)
        _lib.raise_for(lib.gp_comm_unique_id(ctypes.cast(buf, ctypes.c_void_p)), lib, None, 'gp_comm_unique_id')
        return buf.raw

    @staticmethod
    def comm_available():
        """True when RCCL can be resolved in this process (gp_comm_available; nothing collective happens)."""
        return _lib.load().gp_comm_available() == 0

    def comm_info(self, probe=False):
        """What this context's communicator saw: {'ranks', 'rank', 'stats_bytes', 'grads_bytes'[, 'probe_sum']}.  ``probe`` all-reduces one
        1.0 per rank (COLLECTIVE; synchronises the stream): the sum equals the rank count exactly when RCCL connected that many ranks."""
        nr, rk, sb, gb, ps = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_double()
        self._ck(self.lib.gp_comm_info(self.h, ctypes.byref(nr), ctypes.byref(rk), ctypes.byref(sb), ctypes.byref(gb),
                                       ctypes.byref(ps) if probe else None), 'gp_comm_info')
        out = {'ranks': nr.value, 'rank': rk.value, 'stats_bytes': sb.value, 'grads_bytes': gb.value}
        if probe:
            out['probe_sum'] = ps.value
        return out

    def comm_init(self, unique_id, nranks, rank):
        assert len(unique_id) == _lib.GP_COMM_ID_BYTES
        buf = ctypes.create_string_buffer(bytes(unique_id), _lib.GP_COMM_ID_BYTES)
        self._ck(self.lib.gp_comm_init(self.h, ctypes.cast(buf, ctypes.c_void_p), int(nranks), int(rank)), 'gp_comm_init')
        self.has_comm = True

    has_comm = False

    def allreduce(self, which='stats'):
        """statistics: pack -> RCCL all-reduce(sum) -> unpack; grads: all-reduce of the gradient sums.  Enqueued on the engine's stream."""
        self._ck(self.lib.gp_allreduce(self.h, 0 if which == 'stats' else 1), 'gp_allreduce')

    def comm_destroy(self):
        self._ck(self.lib.gp_comm_destroy(self.h), 'gp_comm_destroy')
        self.has_comm = False

    def combine(self, src, which='stats', op='add'):
        """dst (self) += src or dst = src for the packed statistics / gradient-sum buffers (same device)."""
        self._ck(self.lib.gp_buffer_combine(self.h, src.h, 0 if which == 'stats' else 1, 0 if op == 'add' else 1), 'gp_buffer_combine')
        if which == 'stats' and op == 'copy':
            # the reduced statistics come with what their owner learnt about their factorisation: only the engine that runs finish() sees a
            # retry request, and an engine without the hint would run phase 2 on the failed plain step its hinted owner has just repeated
            self._jitter_hint = src._jitter_hint

    # ---- resident CG vectors (scg_adapted_local_MapReduce.py:29-243) ----------------------------------
    CG_RESET_D, CG_UPDATE_D, CG_UPDATE_X, CG_GRAD_OLD, CG_GRAD_NEW, CG_SET_GRADS = range(6)

    def cg_set_grads(self):
        self._ck(self.lib.gp_cg_set_grads(self.h), 'gp_cg_set_grads')

    def cg_dots(self):
        """local sums [mu, kappa, theta, |g_new|^2, g_new.g_old, max|d|]"""
        out = np.zeros(6)
        self._ck(self.lib.gp_cg_dots(self.h, out.ctypes.data_as(_lib._dp)), 'gp_cg_dots')
        return out

    def cg_abs(self):
        """local [sum |grad_now|, max |grad_now|] (gd_local_MapReduce.py:38-61)"""
        out = np.zeros(2)
        self._ck(self.lib.gp_cg_abs(self.h, out.ctypes.data_as(_lib._dp)), 'gp_cg_abs')
        return out

    def cg_update(self, which, a=0.0):
        self.globals_key = None
        self._ck(self.lib.gp_cg_update(self.h, int(which), float(a)), 'gp_cg_update')

    # ---- resident L-BFGS history (gp_lbfgs_*, csrc/lbfgs.hip) ----------------------------------------------------
    _lbfgs_m = 0

    def lbfgs_begin(self, m):
        """Allocates (or clears) the history of ``m`` pairs: 2m + 1 resident vectors of 2 N_s Q doubles, basis order s_0.. | y_0.. | g."""
        self._ck(self.lib.gp_lbfgs_begin(self.h, int(m)), 'gp_lbfgs_begin')
        self._lbfgs_m = int(m)

    def lbfgs_grad(self):
        """g = grad_latest (the start, and after a restart)."""
        self._ck(self.lib.gp_lbfgs_grad(self.h), 'gp_lbfgs_grad')

    def lbfgs_push(self, slot, step):
        """s[slot] = step * direction, y[slot] = grad_latest - g, g = grad_latest in one pass; the embeddings do not move."""
        self._ck(self.lib.gp_lbfgs_push(self.h, int(slot), float(step)), 'gp_lbfgs_push')

    def lbfgs_dots(self, slot=-1):
        """(3, 2m+1): this shard's inner products of s[slot], y[slot] and g with every basis vector (slot -1: the g row only, zeros above)."""
        out = np.zeros((3, 2 * self._lbfgs_m + 1))
        self._ck(self.lib.gp_lbfgs_dots(self.h, int(slot), out.ctypes.data_as(_lib._dp)), 'gp_lbfgs_dots')
        return out

    def lbfgs_direction(self, coef):
        """direction = sum_j coef[j] b_j (empty slots and zero coefficients are skipped)."""
        self.globals_key = None
        coef, pc = _lib.as_c(np.asarray(coef, dtype=np.float64).reshape(-1))
        assert coef.shape == (2 * self._lbfgs_m + 1,), 'coef shape %s: (%d,) expected' % (coef.shape, 2 * self._lbfgs_m + 1)
        self._ck(self.lib.gp_lbfgs_direction(self.h, pc), 'gp_lbfgs_direction')

    def lbfgs_end(self):
        self._ck(self.lib.gp_lbfgs_end(self.h), 'gp_lbfgs_end')
        self._lbfgs_m = 0

    def lbfgs_peek(self, name):
        """A history vector or the direction as it lies on the device, (2, N_s, Q): 's<k>', 'y<k>', 'g' or 'dir' (gp_debug_peek; a test tool)."""
        n2 = 2 * self.N_s * self.Q
        return self.peek('dir' if name == 'dir' else 'lbfgs_' + name, n2)[:n2].reshape(2, self.N_s, self.Q).copy()

    def cg_peek(self, name):
        """A resident vector as it lies on the device (gp_debug_peek; a test tool): 'cg_g_new', 'cg_g_old', 'cg_g_latest' or 'dir' as (2, N_s, Q);
        'Xmu' or 'Xs' (the base embeddings as stored: raw variances when uploaded raw) as (N_s, Q)."""
        shape = (self.N_s, self.Q) if name in ('Xmu', 'Xs') else (2, self.N_s, self.Q)
        n = int(np.prod(shape))
        return self.peek(name, n)[:n].reshape(shape).copy()

    def cg_max_d(self, alpha):
        """local max |alpha d| (gp_cg_max_d, scg_adapted_local_MapReduce.py:142-155)"""
        out = ctypes.c_double()
        self._ck(self.lib.gp_cg_max_d(self.h, float(alpha), ctypes.byref(out)), 'gp_cg_max_d')
        return out.value

    def scale_stats(self, factor):
        self._ck(self.lib.gp_scale_stats(self.h, float(factor)), 'gp_scale_stats')

    def scale_buffer(self, which, factor):
        """Scale the packed statistics ('stats') or gradient-sum ('grads') buffer: node drop-out, local_MapReduce.py:119-129, 263-264."""
        self._ck(self.lib.gp_scale_buffer(self.h, 0 if which == 'stats' else 1, float(factor)), 'gp_scale_buffer')

    def global_step(self, sync=True, jitter=0):
        """Enqueue the global step.  ``sync=True`` (the class / MapReduce surfaces) also waits for its outcome, repeats it once with the
        reference's 1e-7 jitter when a factorisation failed (partial_terms.py:452-456) and raises LinAlgError if that fails too;
        ``sync=False`` (the evaluators) defers all of that to finish(), the evaluation's single host synchronisation."""
        self._ck(self.lib.gp_global_step_jitter(self.h, int(jitter)), 'gp_global_step')
        self._jitter_used = int(jitter)         # the mask this step ends up with (last_jitter reports it)
        # An evaluator whose previous evaluation needed the jitter (finish() saw the failed factorisation only after phase 2 had run on its
        # garbage: the whole phase 2 twice per evaluation, +62 % at N = 1e5, M = 512, Q = 5 with free embeddings) checks the outcome HERE the
        # next time: still the reference's order -- first without jitter, then with (partial_terms.py:452-456) -- for one extra host wait
        # instead of a wasted phase 2.  The hint is dropped as soon as a plain factorisation succeeds again.
        if sync or (jitter == 0 and self._jitter_hint):
            used = 0
            for _ in range(2):                  # at most one retry per matrix: the mask only grows (Kmm, then Kmm + beta Psi2)
                try:
                    self.global_status()
                    self._jitter_hint = used
                    return
                except _lib.JitterRetry as r:
                    used = self._jitter_used = r.mask
                    self._ck(self.lib.gp_global_step_jitter(self.h, r.mask), 'gp_global_step')
            self.global_status()                # a third failure is GP_ERR_NOT_PD -> LinAlgError
            self._jitter_hint = used

    # ---- explicit q(u), whitened (gp_svi_*, csrc/svi.hip) ----------------------------------------------------------
    def svi_begin(self):
        """q(v) := the prior (Lam = I, H = 0); the state lives until svi_end()."""
        self._ck(self.lib.gp_svi_begin(self.h), 'gp_svi_begin')

    def svi_set(self, Lam, H):
        """The natural parameters Lam (M, M), symmetric, and H (M, D)."""
        Lam, pl = _lib.as_c(Lam)
        H, ph = _lib.as_c(H)
        assert Lam.shape == (self.M, self.M) and H.shape == (self.M, self.D), 'svi_set: Lam (M, M) and H (M, D) expected'
        self._ck(self.lib.gp_svi_set(self.h, pl, ph), 'gp_svi_set')

    def svi_get(self, moments=True):
        """dict(Lam, H) and, with ``moments``, Mv = Lam^-1 H and Sv = Lam^-1 (LinAlgError when Lam does not factorise)."""
        out = dict(Lam=np.empty((self.M, self.M)), H=np.empty((self.M, self.D)))
        if moments:
            out.update(Mv=np.empty((self.M, self.D)), Sv=np.empty((self.M, self.M)))
        p = [out[k].ctypes.data_as(_lib._dp) if k in out else None for k in ('Lam', 'H', 'Mv', 'Sv')]
        self._ck(self.lib.gp_svi_get(self.h, *p), 'gp_svi_get')
        return out

    def svi_natural_step(self, rho):
        """Lam <- (1 - rho) Lam + rho (I + beta Psi2w), H <- (1 - rho) H + rho beta Cw on the statistics buffer as it stands."""
        self._ck(self.lib.gp_svi_natural_step(self.h, float(rho)), 'gp_svi_natural_step')
        self._svi_rhos = list(self._svi_rhos) + [float(rho)]

    _svi_rhos = ()

    def svi_step(self, sync=True, jitter=0):
        """The uncollapsed bound and its partials where global_step() leaves the collapsed ones; phase2() and finish() follow.  ``sync`` as in
        global_step(): waits for the outcome and, when K_mm did not factorise, repeats with the 1e-7 jitter on it.  The natural steps since the last
        svi_step left the state untouched in that case (gp_svi_natural_step skips on a failed K_mm): they are repeated on the jittered K_mm first."""
        self._ck(self.lib.gp_svi_step(self.h, int(jitter)), 'gp_svi_step')
        self._jitter_used = int(jitter)
        if sync:
            try:
                self.global_status()
            except _lib.JitterRetry as r:
                self._jitter_used = r.mask
                self._ck(self.lib.gp_svi_step(self.h, r.mask), 'gp_svi_step')       # the mask is the plan's from here on
                for rho in self._svi_rhos:
                    self._ck(self.lib.gp_svi_natural_step(self.h, rho), 'gp_svi_natural_step')
                if self._svi_rhos:
                    self._ck(self.lib.gp_svi_step(self.h, r.mask), 'gp_svi_step')
                self.global_status()
        self._svi_rhos = []          # (sync=False: the caller reads the outcome and repeats both steps itself)

    def svi_publish(self):
        """Pseudo-statistics of q(u) into the statistics buffer; global_step() next makes the context a predictor of the SVI-trained model."""
        self._ck(self.lib.gp_svi_publish(self.h), 'gp_svi_publish')

    def svi_end(self):
        self._ck(self.lib.gp_svi_end(self.h), 'gp_svi_end')

    def global_status(self):
        mask = ctypes.c_int(0)
        rc = self.lib.gp_global_status(self.h, ctypes.byref(mask))
        if rc == _lib.GP_RETRY_JITTER:
            raise _lib.JitterRetry(mask.value, 'gp_global_status: retry with jitter mask %d' % mask.value)
        self._ck(rc, 'gp_global_status')

    def phase2(self, want_embedding_grads=False):
        self._ck(self.lib.gp_phase2(self.h, 1 if want_embedding_grads else 0), 'gp_phase2')

    def finish(self):
        F = ctypes.c_double()
        gs = ctypes.c_double()
        gb = ctypes.c_double()
        gZ = np.empty((self.M, self.Q))
        ga = np.empty(self.Q)
        rc = self.lib.gp_finish(self.h, ctypes.byref(F), gZ.ctypes.data_as(_lib._dp), ctypes.byref(gs),
                                ga.ctypes.data_as(_lib._dp), ctypes.byref(gb))
        if rc == _lib.GP_RETRY_JITTER:
            try:
                self.global_status()    # raises JitterRetry carrying the mask
            except _lib.JitterRetry as r:
                self._jitter_hint = r.mask
                raise
        self._ck(rc, 'gp_finish')
        return dict(F=F.value, grad_Z=gZ, grad_sf2=gs.value, grad_alpha=ga, grad_beta=gb.value)

    def evaluate(self, want_embedding_grads=False):
        """Single-shard evaluation (no reduction across shards); one host synchronisation, in finish()."""
        out, self.last_jitter = evaluate([self], None, want_embedding_grads)     # 0, or the matrices that needed the reference's 1e-7 jitter
        if want_embedding_grads:
            out['grad_X_mu'] = self.download('GRAD_X_MU')
            if not self.regime_A_hint:
                out['grad_X_S'] = self.download('GRAD_X_S')
        return out

    # ---- prediction (gp_predict) ---------------------------------------------------------------------------
    def predict(self, X_mu, X_S=None, include_noise=False, xs_is_raw=False):
        """Posterior predictive at new inputs, after a successful global step of this engine (its reduced statistics: the whole model).
        Returns (mean (n, D), var): var is (n, 1) for deterministic inputs (X_S None: one variance per point) and (n, D) for uncertain inputs
        x ~ N(X_mu, diag X_S).  ``include_noise`` adds 1/beta (y instead of f).  The evaluation state is left untouched."""
        X_mu = np.atleast_2d(np.asarray(X_mu, dtype=np.float64))
        assert X_mu.ndim == 2 and X_mu.shape[1] == self.Q, 'X_mu shape %s: (n, %d) expected' % (X_mu.shape, self.Q)
        n = X_mu.shape[0]
        X_mu, pm = _lib.as_c(X_mu)
        ps = None
        if X_S is not None:
            X_S = np.atleast_2d(np.asarray(X_S, dtype=np.float64))
            assert X_S.shape == X_mu.shape, 'X_S shape %s != X_mu shape %s' % (X_S.shape, X_mu.shape)
            X_S, ps = _lib.as_c(X_S)
        mean = np.empty((n, self.D))
        var = np.empty((n, 1) if X_S is None else (n, self.D))
        self._ck(self.lib.gp_predict(self.h, n, pm, ps, 1 if xs_is_raw else 0, 1 if include_noise else 0, mean.ctypes.data_as(_lib._dp),
                                     var.ctypes.data_as(_lib._dp)), 'gp_predict')
        return mean, var

    # ---- held-out scoring (gp_predict_score) ---------------------------------------------------------------------
    @staticmethod
    def score_summary(cols):
        """The figures of ``score`` from the column sums ``cols`` (D, 5) = [count, sum e, sum e^2, sum e^2 / v, sum logp] (those of several shards
        add first): count, bias = sum e / count, rmse = sqrt(sum e^2 / count), chi2_mean = sum e^2 / v / count and nlpd = -sum logp / count, each
        per column (D,) and, under ``pooled``, over all columns; a column (or a pool) without a scored entry gives NaN."""
        cols = np.asarray(cols, dtype=np.float64)

        def figures(s):
            with np.errstate(invalid='ignore', divide='ignore'):
                cnt = np.where(s[..., 0] > 0, s[..., 0], np.nan)
                return dict(count=s[..., 0], bias=s[..., 1] / cnt, rmse=np.sqrt(s[..., 2] / cnt), chi2_mean=s[..., 3] / cnt, nlpd=-s[..., 4] / cnt)
        out = figures(cols)
        out['cols'] = cols
        out['pooled'] = figures(cols.sum(axis=0))
        return out

    def score(self, Y, X_mu=None, X_S=None, observed=None, include_noise=True, xs_is_raw=False, use_resident_S=False, want_rows=True):
        """Scores the outputs ``Y`` (n, D) under ``predict``'s mean and variance at the same inputs, on the device (gp_predict_score): per observed
        entry the Gaussian log density logp = -1/2 ln(2 pi v) - e^2 / (2 v), e = y - mean (uncertain inputs: of the moment-matched Gaussian).
        ``observed`` (n, D): non-zero where Y is scored; None: where Y is not NaN; the other entries are never read.  ``include_noise`` scores y
        (variance + 1/beta), the held-out convention; without it f.
        ``X_mu`` None scores the engine's resident rows at their base means -- with ``use_resident_S`` at their base variances as well -- and ``Y``
        None then means the resident Y: nothing of size n x D crosses the bus.
        Returns a dict: ``row_logp``, ``row_sse``, ``row_chi2`` (n,) (None without ``want_rows``), ``cols`` (D, 5) the column sums [count, sum e,
        sum e^2, sum e^2 / v, sum logp], and from them on the host ``count``, ``bias``, ``rmse``, ``chi2_mean``, ``nlpd`` per column (D,) and
        ``pooled`` (a dict of the same five over all columns).  FloatingPointError when a scored variance is not > 0 (possible without the noise)."""
        pm = ps = py = po = None
        flags = 1 if include_noise else 0
        if X_mu is None:
            assert X_S is None and not xs_is_raw, 'score: the resident rows take X_S from the engine (use_resident_S)'
            n = self.N_s
            if use_resident_S:
                flags |= 2
        else:
            assert not use_resident_S, 'score: use_resident_S needs the resident rows (X_mu None)'
            assert Y is not None, 'score: Y is needed with host inputs'
            X_mu = np.atleast_2d(np.asarray(X_mu, dtype=np.float64))
            assert X_mu.ndim == 2 and X_mu.shape[1] == self.Q, 'X_mu shape %s: (n, %d) expected' % (X_mu.shape, self.Q)
            n = X_mu.shape[0]
            X_mu, pm = _lib.as_c(X_mu)
            if X_S is not None:
                X_S = np.atleast_2d(np.asarray(X_S, dtype=np.float64))
                assert X_S.shape == X_mu.shape, 'X_S shape %s != X_mu shape %s' % (X_S.shape, X_mu.shape)
                X_S, ps = _lib.as_c(X_S)
        if Y is not None:
            Y = np.asarray(Y, dtype=np.float64)
            Y = Y[:, None] if Y.ndim == 1 else Y
            assert Y.shape == (n, self.D), 'Y shape %s: (%d, %d) expected' % (Y.shape, n, self.D)
            Y, py = _lib.as_c(Y)
            if observed is None and np.isnan(Y).any():
                observed = ~np.isnan(Y)
        if observed is not None:
            observed = np.ascontiguousarray(np.atleast_2d(np.asarray(observed)) != 0, dtype=np.uint8)
            assert observed.shape == (n, self.D), 'observed shape %s: (%d, %d) expected' % (observed.shape, n, self.D)
            po = observed.ctypes.data_as(_lib._u8p)
        rows = [np.empty(n) for _ in range(3)] if want_rows else [None] * 3
        cols = np.empty((self.D, 5))
        dp = lambda a: a.ctypes.data_as(_lib._dp) if a is not None else None          # noqa: E731
        rc = self.lib.gp_predict_score(self.h, n, pm, ps, 1 if xs_is_raw else 0, py, po, flags, dp(rows[0]), dp(rows[1]), dp(rows[2]), dp(cols))
        if rc != _lib.GP_ERR_NON_FINITE:
            self._ck(rc, 'gp_predict_score')
        out = self.score_summary(cols)
        out['row_logp'], out['row_sse'], out['row_chi2'] = rows
        try:
            self._ck(rc, 'gp_predict_score')
        except FloatingPointError as err:
            err.result = out            # every row but the named ones is valid: NaN marks the rows and columns of the bad variances
            raise
        return out

    # ---- leave-one-out / leave-block-out scoring of the resident rows (gp_loo_score) ----------------------------
    def loo(self, block=1, observed=None, include_noise=True, want_rows=True):
        """Exact leave-one-out (``block`` = 1) or leave-block-out cross-validation of the engine's resident rows, on the device (gp_loo_score): row i
        is predicted by the model that never saw the rows of its block -- rows [j block, (j + 1) block) of THIS shard form block j, 1 <= block <= 128;
        for other folds order the rows before the upload -- with the hyper-parameters and inducing points fixed, and scored as ``score`` scores.
        Fixed embeddings only; the engine's statistics must contain these rows (the caller's obligation: the library cannot tell).
        ``observed`` (N_s, D): non-zero where an entry is summed (it never enters the downdate); None: every entry.  ``include_noise`` scores y.
        Returns the dict of ``score`` -- ``row_logp``, ``row_sse``, ``row_chi2`` (None without ``want_rows``), ``cols`` (D, 5) and
        ``score_summary``'s figures of it -- with ``lev`` (N_s,) the leverages beta |La^-1 k_i|^2 and ``var_loo`` (N_s,) the leave-out variances.
        LinAlgError when a block cannot be left out (I - H does not factorise), FloatingPointError when a leave-out variance is not > 0: the
        exception's ``result`` holds the dict, NaN in the rows concerned."""
        n = self.N_s
        po = None
        if observed is not None:
            observed = np.ascontiguousarray(np.atleast_2d(np.asarray(observed)) != 0, dtype=np.uint8)
            assert observed.shape == (n, self.D), 'observed shape %s: (%d, %d) expected' % (observed.shape, n, self.D)
            po = observed.ctypes.data_as(_lib._u8p)
        rows = [np.empty(n) for _ in range(3)] if want_rows else [None] * 3
        lev, var, cols = np.empty(n), np.empty(n), np.empty((self.D, 5))
        dp = lambda a: a.ctypes.data_as(_lib._dp) if a is not None else None          # noqa: E731
        rc = self.lib.gp_loo_score(self.h, int(block), po, 1 if include_noise else 0, dp(rows[0]), dp(rows[1]), dp(rows[2]), dp(lev), dp(var), dp(cols))
        if rc not in (_lib.GP_ERR_NON_FINITE, _lib.GP_ERR_NOT_PD):
            self._ck(rc, 'gp_loo_score')
        out = self.score_summary(cols)
        out['row_logp'], out['row_sse'], out['row_chi2'] = rows
        out['lev'], out['var_loo'] = lev, var
        try:
            self._ck(rc, 'gp_loo_score')
        except (FloatingPointError, np.linalg.LinAlgError) as err:
            err.result = out
            raise
        return out

    # ---- joint prediction (gp_predict_joint, gp_predict_sample) ------------------------------------------------
    def _joint_X(self, X):
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        assert X.ndim == 2 and X.shape[1] == self.Q, 'X shape %s: (n, %d) expected' % (X.shape, self.Q)
        return _lib.as_c(X)

    def predict_joint(self, X, include_noise=False):
        """Joint posterior of f (``include_noise``: of y) at the new deterministic inputs X (n, Q), n <= 16384, after a successful global step as
        ``predict``.  Returns (mean (n, D), cov (n, n)): one covariance matrix shared by all D outputs, symmetric bit for bit, whose diagonal is
        ``predict``'s variance.  The evaluation state is left untouched."""
        X, px = self._joint_X(X)
        n = X.shape[0]
        mean, cov = np.empty((n, self.D)), np.empty((n, n))
        self._ck(self.lib.gp_predict_joint(self.h, n, px, 1 if include_noise else 0, mean.ctypes.data_as(_lib._dp), cov.ctypes.data_as(_lib._dp)),
                 'gp_predict_joint')
        return mean, cov

    def predict_sample(self, X, n_draws, include_noise=False, jitter=1e-8, eps=None, seed=None):
        """``n_draws`` coherent function samples at X (n, Q), n <= 8192: draws[s, :, d] = mean[:, d] + Lc eps[s, :, d] with Lc the lower Cholesky
        factor of cov + (noise + jitter sf2) I (``predict_joint``'s cov; ``jitter`` is relative to sf2).  ``eps`` (n_draws, n, D) standard normals,
        drawn with numpy.random.default_rng(seed) when not given.  Returns (draws (n_draws, n, D), mean (n, D))."""
        X, px = self._joint_X(X)
        n, n_draws = X.shape[0], int(n_draws)
        if eps is None:
            assert n_draws >= 0, 'n_draws must be >= 0'
            eps = np.random.default_rng(seed).standard_normal((n_draws, n, self.D))
        eps = np.asarray(eps, dtype=np.float64)
        assert eps.shape == (n_draws, n, self.D), 'eps shape %s: (%d, %d, %d) expected' % (eps.shape, n_draws, n, self.D)
        eps, pe = _lib.as_c(eps)
        draws, mean = np.empty((n_draws, n, self.D)), np.empty((n, self.D))
        self._ck(self.lib.gp_predict_sample(self.h, n, px, 1 if include_noise else 0, float(jitter), n_draws, pe, draws.ctypes.data_as(_lib._dp),
                                            mean.ctypes.data_as(_lib._dp)), 'gp_predict_sample')
        return draws, mean

    # ---- pathwise posterior function draws (gp_paths_set, gp_paths_eval, gp_paths_clear) ----------------------
    def paths_set(self, omega, w, eps_u, centre=None):
        """Fix ``n_draws`` posterior function draws, after a successful global step as ``predict``: ``omega`` (F, Q) the frequencies of the random
        Fourier prior (the caller draws omega[f, q] ~ N(0, alpha_q)), ``w`` (n_draws, 2F, D) and ``eps_u`` (n_draws, M, D) standard normals,
        ``centre`` (Q,) the origin of the phases (None: 0).  ``paths_eval`` then evaluates these same functions anywhere, any number of times,
        until the model changes (new globals, statistics or a global step drop the draws).  An engine holds ONE set of draws at a time: a second
        ``paths_set`` replaces the first (``paths_token`` changes with every ``paths_set`` and ``paths_clear``, so a holder of draws can tell)."""
        omega = np.atleast_2d(np.asarray(omega, dtype=np.float64))
        assert omega.ndim == 2 and omega.shape[1] == self.Q and omega.shape[0] >= 1, 'omega shape %s: (F, %d) expected' % (omega.shape, self.Q)
        F = omega.shape[0]
        w, eps_u = np.asarray(w, dtype=np.float64), np.asarray(eps_u, dtype=np.float64)
        assert w.ndim == 3 and w.shape[0] >= 1 and w.shape[1:] == (2 * F, self.D), 'w shape %s: (n_draws, %d, %d) expected' % (w.shape, 2 * F, self.D)
        S = w.shape[0]
        assert eps_u.shape == (S, self.M, self.D), 'eps_u shape %s: (%d, %d, %d) expected' % (eps_u.shape, S, self.M, self.D)
        pc = None
        if centre is not None:
            centre = np.asarray(centre, dtype=np.float64).reshape(-1)
            assert centre.shape == (self.Q,), 'centre shape %s: (%d,) expected' % (centre.shape, self.Q)
            centre, pc = _lib.as_c(centre)
        (omega, po), (w, pw), (eps_u, pe) = _lib.as_c(omega), _lib.as_c(w), _lib.as_c(eps_u)
        self._ck(self.lib.gp_paths_set(self.h, S, F, po, pc, pw, pe), 'gp_paths_set')
        self._paths_draws = S
        self.paths_token = getattr(self, 'paths_token', 0) + 1

    def paths_eval(self, X, want_mean=False):
        """The draws of ``paths_set`` at the new deterministic inputs X (n, Q), any n: (n_draws, n, D); with ``want_mean`` also ``predict``'s mean
        (n, D).  A point's values are the same bits alone, in any batch and in any call, so a draw evaluated on two grids agrees exactly where
        they share points.  The evaluation state is left untouched."""
        X, px = self._joint_X(X)
        n = X.shape[0]
        out = np.empty((getattr(self, '_paths_draws', 0), n, self.D))
        mean = np.empty((n, self.D)) if want_mean else None
        self._ck(self.lib.gp_paths_eval(self.h, n, px, 0, out.ctypes.data_as(_lib._dp), mean.ctypes.data_as(_lib._dp) if want_mean else None), 'gp_paths_eval')
        return (out, mean) if want_mean else out

    def paths_grad(self, X, weights=None, jac=True, metric=True, want_mean=False):
        """Derivatives of the draws of ``paths_set`` with respect to the input, at the new deterministic inputs X (n, Q).  Returns a dict of the
        requested arrays: ``jac`` (n_draws, n, D, Q) d out[s, i, d] / d x_q; ``metric`` (n_draws, n, Q, Q) the pull-back metric J_s^T J_s of every
        sampled surface (symmetric bit for bit); with ``weights`` also ``grad`` (n_draws, n, Q) = sum_d weights[d] jac[s, i, d, :] -- ``weights``
        (D,) scalarises every draw the same way, ``weights`` (n_draws, n, D) gives every (draw, point) its own (the vector-Jacobian product);
        with ``want_mean`` also ``mean_jac`` (n, D, Q), the Jacobian of the mean.  A point's values are the same bits alone, in any batch and
        for any subset of the outputs.  The evaluation state and the draws are left untouched."""
        X, px = self._joint_X(X)
        n, Q, S = X.shape[0], self.Q, getattr(self, '_paths_draws', 0)
        flags, pw = 0, None
        out = {}
        if weights is not None:
            weights = np.asarray(weights, dtype=np.float64)
            assert weights.shape in ((self.D,), (S, n, self.D)), 'weights shape %s: (%d,) or (%d, %d, %d) expected' % (weights.shape, self.D, S, n, self.D)
            flags = _lib.GP_PATHS_WEIGHTS_PER_ROW if weights.ndim == 3 else 0
            weights, pw = _lib.as_c(weights)
            out['grad'] = np.empty((S, n, Q))
        if jac:
            out['jac'] = np.empty((S, n, self.D, Q))
        if metric:
            out['metric'] = np.empty((S, n, Q, Q))
        if want_mean:
            out['mean_jac'] = np.empty((n, self.D, Q))
        p = lambda k: out[k].ctypes.data_as(_lib._dp) if k in out else None
        self._ck(self.lib.gp_paths_grad(self.h, n, px, flags, pw, p('jac'), p('grad'), p('metric'), p('mean_jac')), 'gp_paths_grad')
        return out

    def paths_clear(self):
        """Drop the draws of ``paths_set`` and free their device memory."""
        self._ck(self.lib.gp_paths_clear(self.h), 'gp_paths_clear')
        self._paths_draws = 0
        self.paths_token = getattr(self, 'paths_token', 0) + 1

    # ---- the posterior conditioned on extra observed rows (gp_condition_set, gp_condition_predict, gp_condition_clear) ----
    def condition(self, Xc, Yc):
        """Condition the model on ``m`` extra observed rows, after a successful global step as ``predict``: ``Xc`` (m, Q) their deterministic
        inputs, ``Yc`` (m, D) their outputs, 1 <= m <= 1024.  ``condition_predict`` then predicts as ``predict`` would after a refit on the shard
        with these rows appended (embeddings fixed), at the cost of one m x m factorisation here and two thin products per query chunk there.
        Nothing of the model or the evaluation state changes.  An engine holds ONE set at a time: a second ``condition`` replaces the first; a
        set goes stale when the model changes (new globals, statistics or a global step)."""
        Xc, Yc = np.atleast_2d(np.asarray(Xc, dtype=np.float64)), np.atleast_2d(np.asarray(Yc, dtype=np.float64))
        assert Xc.ndim == 2 and Xc.shape[1] == self.Q, 'Xc shape %s: (m, %d) expected' % (Xc.shape, self.Q)
        assert Yc.shape == (Xc.shape[0], self.D), 'Yc shape %s: (%d, %d) expected' % (Yc.shape, Xc.shape[0], self.D)
        (Xc, px), (Yc, py) = _lib.as_c(Xc), _lib.as_c(Yc)
        self._ck(self.lib.gp_condition_set(self.h, Xc.shape[0], px, py), 'gp_condition_set')

    def condition_predict(self, X, include_noise=False, want_reduction=False):
        """``predict`` at the new deterministic inputs X (n, Q) under the rows of ``condition``: (mean (n, D), var (n, 1)); with
        ``want_reduction`` also the reduction (n, 1) = var - var' >= 0 of the variance the rows bought.  ``include_noise`` adds 1/beta.  A point's
        values are the same bits alone and in any batch.  The evaluation state is left untouched."""
        X, px = self._joint_X(X)
        n = X.shape[0]
        mean, var = np.empty((n, self.D)), np.empty((n, 1))
        red = np.empty((n, 1)) if want_reduction else None
        self._ck(self.lib.gp_condition_predict(self.h, n, px, 1 if include_noise else 0, mean.ctypes.data_as(_lib._dp), var.ctypes.data_as(_lib._dp),
                                               red.ctypes.data_as(_lib._dp) if want_reduction else None), 'gp_condition_predict')
        return (mean, var, red) if want_reduction else (mean, var)

    def condition_clear(self):
        """Drop the rows of ``condition`` and free their device memory (no error without any)."""
        self._ck(self.lib.gp_condition_clear(self.h), 'gp_condition_clear')

    # ---- derivatives of the prediction with respect to the input (gp_predict_grad) ----------------------------
    def predict_grad(self, X, jac=True, dvar=True, metric=True, logdet=True):
        """Derivatives of ``predict`` at the new deterministic inputs X (n, Q), after a successful global step as ``predict``.  Returns a dict of the
        requested arrays: ``jac`` (n, D, Q) d mean_d / d x_q, ``dvar`` (n, Q) d var_f / d x_q, ``metric`` (n, Q, Q) the expected metric tensor
        E[J]^T E[J] + D Cov(J) (symmetric bit for bit) and ``logdet`` (n,) ln det metric (Q <= 64; the magnification factor is exp(logdet / 2)).
        The noise enters none of them.  The evaluation state is left untouched."""
        X, px = self._joint_X(X)
        n, Q = X.shape[0], self.Q
        out = {}
        if jac:
            out['jac'] = np.empty((n, self.D, Q))
        if dvar:
            out['dvar'] = np.empty((n, Q))
        if metric:
            out['metric'] = np.empty((n, Q, Q))
        if logdet:
            out['logdet'] = np.empty(n)
        p = lambda k: out[k].ctypes.data_as(_lib._dp) if k in out else None
        self._ck(self.lib.gp_predict_grad(self.h, n, px, 0, p('jac'), p('dvar'), p('metric'), p('logdet')), 'gp_predict_grad')
        return out

    # ---- energy of curves through latent space (gp_curve_energy) ----------------------------------------------
    def curve_energy(self, X, want_energy=True, want_segments=False, want_grad=True):
        """Expected energy of discrete curves X (n_curves, T, Q) -- or one curve (T, Q) -- under the posterior of f, after a successful global
        step as ``predict``.  Returns a dict of the requested arrays: ``energy`` (n_curves,) 1/2 (T - 1) sum_s seg_s, ``seg`` (n_curves, T - 1)
        the expected squared length E|f(x_{s+1}) - f(x_s)|^2 of every segment, ``grad`` (n_curves, T, Q) the derivative of ``energy`` with respect
        to the curve's points (one curve: without the leading axis).  A curve's values are the same bits alone and in any batch.  The noise
        enters nowhere.  The evaluation state is left untouched."""
        X = np.asarray(X, dtype=np.float64)
        single = X.ndim == 2
        if single:
            X = X[None]
        assert X.ndim == 3 and X.shape[2] == self.Q and X.shape[1] >= 2, 'X shape %s: (n_curves, T >= 2, %d) expected' % (X.shape, self.Q)
        X, px = _lib.as_c(X)
        n, T = X.shape[0], X.shape[1]
        out = {}
        if want_energy:
            out['energy'] = np.empty(n)
        if want_segments:
            out['seg'] = np.empty((n, T - 1))
        if want_grad:
            out['grad'] = np.empty((n, T, self.Q))
        p = lambda k: out[k].ctypes.data_as(_lib._dp) if k in out else None
        self._ck(self.lib.gp_curve_energy(self.h, n, T, px, 0, p('energy'), p('seg'), p('grad')), 'gp_curve_energy')
        return {k: v[0] for k, v in out.items()} if single else out

    # ---- latent inference for new rows (gp_infer_objective, gp_infer_latent) ---------------------------------
    def _infer_args(self, Y, X_mu, X_S, cols):
        Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
        assert Y.ndim == 2 and Y.shape[1] == self.D, 'Y shape %s: (n, %d) expected' % (Y.shape, self.D)
        n = Y.shape[0]
        X_mu = np.array(np.atleast_2d(np.asarray(X_mu, dtype=np.float64)), order='C', copy=True)
        X_S = np.array(np.atleast_2d(np.asarray(X_S, dtype=np.float64)), order='C', copy=True)
        assert X_mu.shape == (n, self.Q) and X_S.shape == (n, self.Q), 'X_mu %s / X_S %s: (%d, %d) expected' % (X_mu.shape, X_S.shape, n, self.Q)
        Y, py = _lib.as_c(Y)
        pc, nc = None, 0
        if cols is not None:
            cols = np.ascontiguousarray(np.asarray(cols).reshape(-1), dtype=np.int32)
            assert cols.size >= 1, 'cols is empty (None means every column)'
            pc, nc = cols.ctypes.data_as(_lib._ip), int(cols.size)
        return n, (Y, py), X_mu, X_S, (cols, pc, nc)

    def infer_objective(self, Y, X_mu, X_S, cols=None, xs_is_raw=False, want_grads=True):
        """The bound L of every NEW row of Y (n, D) under q(x) = N(X_mu, diag X_S) with q(u) frozen at the trained optimum (after a successful
        global step, as ``predict``), over the observed output columns ``cols`` (strictly increasing; None: all; the others may hold NaN).
        Returns (L (n,), grad_mu (n, Q), grad_S (n, Q)); grad_S is with respect to the raw value with ``xs_is_raw``.  Rows are independent."""
        n, (Y, py), X_mu, X_S, (cols, pc, nc) = self._infer_args(Y, X_mu, X_S, cols)
        L, gm, gs = np.empty(n), np.empty((n, self.Q)), np.empty((n, self.Q))
        dp = lambda a: a.ctypes.data_as(_lib._dp)
        self._ck(self.lib.gp_infer_objective(self.h, n, py, pc, nc, dp(X_mu), dp(X_S), 1 if xs_is_raw else 0, dp(L), dp(gm) if want_grads else None,
                                             dp(gs) if want_grads else None), 'gp_infer_objective')
        return (L, gm, gs) if want_grads else (L, None, None)

    def infer_latent(self, Y, X_mu, X_S, cols=None, xs_is_raw=False, max_iters=100, gtol=1e-5):
        """Maximise that bound per row over (X_mu, softplus-raw X_S) from the given start with the device's per-row scaled conjugate gradients.
        Returns (X_mu, X_S, L (n,), iters (n,) int32): X_S in the form it came in; a row with iters < max_iters stopped on max |gradient| <= gtol."""
        n, (Y, py), X_mu, X_S, (cols, pc, nc) = self._infer_args(Y, X_mu, X_S, cols)
        L, it = np.empty(n), np.zeros(n, dtype=np.int32)
        dp = lambda a: a.ctypes.data_as(_lib._dp)
        self._ck(self.lib.gp_infer_latent(self.h, n, py, pc, nc, dp(X_mu), dp(X_S), 1 if xs_is_raw else 0, int(max_iters), float(gtol), dp(L),
                                          it.ctypes.data_as(_lib._ip)), 'gp_infer_latent')
        return X_mu, X_S, L, it

    # ---- the same for rows that each observe their own columns (gp_infer_objective_rows, gp_infer_latent_rows) ---
    def _infer_rows_args(self, Y, X_mu, X_S, observed):
        n, (Y, py), X_mu, X_S, _ = self._infer_args(Y, X_mu, X_S, None)
        if observed is None:
            observed = ~np.isnan(Y)
        observed = np.ascontiguousarray(np.atleast_2d(np.asarray(observed)) != 0, dtype=np.uint8)
        assert observed.shape == (n, self.D), 'observed shape %s: (%d, %d) expected' % (observed.shape, n, self.D)
        return n, (Y, py), X_mu, X_S, (observed, observed.ctypes.data_as(_lib._u8p))

    def infer_objective_rows(self, Y, X_mu, X_S, observed=None, xs_is_raw=False, want_grads=True):
        """``infer_objective`` with the observed set of EVERY row: ``observed`` (n, D), non-zero where Y is observed (None: where Y is not NaN); the
        other entries of Y are never read.  One device call whatever the number of distinct patterns.  Returns (L, grad_mu, grad_S) as
        ``infer_objective``; a row's outputs do not depend on the other rows of the call or on their order, bit for bit."""
        n, (Y, py), X_mu, X_S, (observed, po) = self._infer_rows_args(Y, X_mu, X_S, observed)
        L, gm, gs = np.empty(n), np.empty((n, self.Q)), np.empty((n, self.Q))
        dp = lambda a: a.ctypes.data_as(_lib._dp)
        self._ck(self.lib.gp_infer_objective_rows(self.h, n, py, po, dp(X_mu), dp(X_S), 1 if xs_is_raw else 0, dp(L), dp(gm) if want_grads else None,
                                                  dp(gs) if want_grads else None), 'gp_infer_objective_rows')
        return (L, gm, gs) if want_grads else (L, None, None)

    def infer_latent_rows(self, Y, X_mu, X_S, observed=None, xs_is_raw=False, max_iters=100, gtol=1e-5):
        """``infer_latent`` with the observed set of every row (``observed`` as for ``infer_objective_rows``), all rows in one device call.
        Returns (X_mu, X_S, L (n,), iters (n,) int32) as ``infer_latent``."""
        n, (Y, py), X_mu, X_S, (observed, po) = self._infer_rows_args(Y, X_mu, X_S, observed)
        L, it = np.empty(n), np.zeros(n, dtype=np.int32)
        dp = lambda a: a.ctypes.data_as(_lib._dp)
        self._ck(self.lib.gp_infer_latent_rows(self.h, n, py, po, dp(X_mu), dp(X_S), 1 if xs_is_raw else 0, int(max_iters), float(gtol), dp(L),
                                               it.ctypes.data_as(_lib._ip)), 'gp_infer_latent_rows')
        return X_mu, X_S, L, it

    # ---- initialisation of the inducing points (gp_kmeans_accumulate) -----------------------------------------
    def kmeans_accumulate(self, centres, X=None, want_labels=False):
        """One Lloyd assignment pass of k-means (the vq + update_cluster_means pair inside scipy.cluster.vq.kmeans, parallel_GPLVM.py:179-186) over
        the host rows ``X`` (n, Q), or over the resident X_mu of this engine (``X`` None), against ``centres`` (K, Q), any K >= 1.  Returns
        (sums (K, Q), counts (K,) int64, dist2 = [sum d^2, sum d], labels (n,) int32 or None): per centre the sum and the number of the rows
        nearest to it (ties: the lowest index), and the summed squared / plain Euclidean distances.  Shards add; gparml_amd.init.kmeans drives the
        loop.  The evaluation state is left untouched."""
        centres = np.atleast_2d(np.asarray(centres, dtype=np.float64))
        assert centres.ndim == 2 and centres.shape[1] == self.Q, 'centres shape %s: (K, %d) expected' % (centres.shape, self.Q)
        K = centres.shape[0]
        centres, pc = _lib.as_c(centres)
        px, n = None, self.N_s
        if X is not None:
            X = np.atleast_2d(np.asarray(X, dtype=np.float64))
            assert X.ndim == 2 and X.shape[1] == self.Q, 'X shape %s: (n, %d) expected' % (X.shape, self.Q)
            n = X.shape[0]
            X, px = _lib.as_c(X)
        sums, counts, dist2 = np.empty((K, self.Q)), np.empty(K, dtype=np.int64), np.empty(2)
        labels = np.empty(n, dtype=np.int32) if want_labels else None
        self._ck(self.lib.gp_kmeans_accumulate(self.h, n, px, K, pc, sums.ctypes.data_as(_lib._dp), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                               dist2.ctypes.data_as(_lib._dp), labels.ctypes.data_as(_lib._ip) if want_labels else None),
                 'gp_kmeans_accumulate')
        return sums, counts, dist2, labels

    # ---- greedy conditional-variance selection of the inducing points (gp_select_*) ---------------------------
    def select_begin(self, K, sf2, alpha, tol=1e-10, X=None):
        """Starts a greedy conditional-variance selection (pivoted Cholesky of K_nn, csrc/select.hip) of up to ``K`` rows among the host rows
        ``X`` (n, Q), or among the resident X_mu of this engine (``X`` None), under the kernel sf2 exp(-1/2 sum_q alpha_q (x_q - z_q)^2); a step
        needs a conditional variance above ``tol`` sf2.  An engine holds one selection at a time; ``select_end`` frees it.  The evaluation state
        is left untouched.  Returns the number of rows."""
        alpha = np.asarray(alpha, dtype=np.float64).reshape(-1)
        assert alpha.shape == (self.Q,), 'alpha shape %s: (%d,) expected' % (alpha.shape, self.Q)
        alpha, pa = _lib.as_c(alpha)
        px, n = None, self.N_s
        if X is not None:
            X = np.atleast_2d(np.asarray(X, dtype=np.float64))
            assert X.ndim == 2 and X.shape[1] == self.Q, 'X shape %s: (n, %d) expected' % (X.shape, self.Q)
            n = X.shape[0]
            X, px = _lib.as_c(X)
        self._ck(self.lib.gp_select_begin(self.h, n, px, int(K), float(sf2), pa, float(tol)), 'gp_select_begin')
        self._select_n = n
        return n

    def select_run(self, steps):
        """Up to ``steps`` further steps of the selection on the device without a host round trip per step (the one-shard path).  Returns
        (rows (k,) int64, trace (k,)): the pivots found, k <= steps (fewer: the stopping rule, or K reached), and the trace of the Nystrom
        residual after each."""
        steps = int(steps)
        done = ctypes.c_int32(0)
        rows, trace = np.empty(max(steps, 1), dtype=np.int64), np.empty(max(steps, 1))
        self._ck(self.lib.gp_select_run(self.h, steps, ctypes.byref(done), rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), trace.ctypes.data_as(_lib._dp)),
                 'gp_select_run')
        return rows[:done.value].copy(), trace[:done.value].copy()

    def select_candidate(self, steps_done):
        """The best unselected local row after ``steps_done`` steps: (d, row, x (Q,), l (steps_done,)); row -1 and d -inf when every row is
        selected (or there are none)."""
        d, row = ctypes.c_double(0.0), ctypes.c_int64(-1)
        x, l = np.zeros(self.Q), np.zeros(max(int(steps_done), 1))
        self._ck(self.lib.gp_select_candidate(self.h, ctypes.byref(d), ctypes.byref(row), x.ctypes.data_as(_lib._dp), l.ctypes.data_as(_lib._dp)),
                 'gp_select_candidate')
        return d.value, row.value, x, l[:int(steps_done)]

    def select_apply(self, x_p, l_p, d_p, own_row=-1):
        """One step with the pivot (x_p (Q,), l_p (steps done,), d_p) given by the caller; ``own_row`` >= 0: the pivot is this local row.  Returns
        the local trace after the step.  The same kernels, the same bits as ``select_run``."""
        x_p, px = _lib.as_c(np.asarray(x_p, dtype=np.float64).reshape(-1))
        l_p, pl = _lib.as_c(np.asarray(l_p, dtype=np.float64).reshape(-1))
        assert x_p.shape == (self.Q,), 'x_p shape %s: (%d,) expected' % (x_p.shape, self.Q)
        t = ctypes.c_double(0.0)
        self._ck(self.lib.gp_select_apply(self.h, px, pl if l_p.size else None, float(d_p), int(own_row), ctypes.byref(t)), 'gp_select_apply')
        return t.value

    def select_end(self):
        self._ck(self.lib.gp_select_end(self.h), 'gp_select_end')

    def select_peek(self, steps_done):
        """(L (steps_done, n), d (n,)) of the selection in progress as they lie on the device (gp_debug_peek 'select_L', 'select_d'; a test tool)."""
        n, npad = self._select_n, (max(self._select_n, 1) + 63) // 64 * 64
        L = self.peek('select_L', max(int(steps_done) * npad, 1))[:int(steps_done) * npad].reshape(int(steps_done), npad)
        return L[:, :n].copy(), self.peek('select_d', npad)[:n].copy()

    # ---- initialisation of the embeddings (gp_scatter_accumulate, gp_project_rows) --------------------------------
    def _rows_arg(self, Y):
        if Y is None:
            return None, None, self.N_s
        Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
        assert Y.ndim == 2 and Y.shape[1] == self.D, 'Y shape %s: (n, %d) expected' % (Y.shape, self.D)
        Y, py = _lib.as_c(Y)
        return Y, py, Y.shape[0]

    def scatter_accumulate(self, centre, Y=None, want_gram=True):
        """The PCA initialisation's accumulation pass over the host rows ``Y`` (n, D), or over the resident Y of this engine (``Y`` None): returns
        (sum (D,), gram (D, D) or None) of the rows minus ``centre`` (D,), the centre subtracted before the products.  gram is bit-for-bit
        symmetric; results are bit-identical from run to run and between host and resident rows; ``want_gram`` False skips the D^2 work and
        returns the same sum.  Shards add; gparml_amd.init.pca drives the passes.  The evaluation state is left untouched."""
        centre = np.asarray(centre, dtype=np.float64).reshape(-1)
        assert centre.shape == (self.D,), 'centre shape %s: (%d,) expected' % (centre.shape, self.D)
        centre, pc = _lib.as_c(centre)
        Y, py, n = self._rows_arg(Y)
        ssum = np.empty(self.D)
        gram = np.empty((self.D, self.D)) if want_gram else None
        self._ck(self.lib.gp_scatter_accumulate(self.h, n, py, pc, ssum.ctypes.data_as(_lib._dp), gram.ctypes.data_as(_lib._dp) if want_gram else None),
                 'gp_scatter_accumulate')
        return ssum, gram

    def project_rows(self, mean, P, Y=None):
        """(Y - mean) P for the host rows ``Y`` (n, D) or the resident Y (``Y`` None): P (D, Q_out) with any Q_out >= 1 (the caller folds 1 / std
        into it); returns X (n, Q_out).  Rows are independent, bit for bit.  The resident X_mu is not written: ``upload_embeddings`` commits."""
        mean = np.asarray(mean, dtype=np.float64).reshape(-1)
        P = np.asarray(P, dtype=np.float64)
        if P.ndim == 1:
            P = P[:, None]
        assert mean.shape == (self.D,) and P.ndim == 2 and P.shape[0] == self.D and P.shape[1] >= 1, 'mean %s, P %s' % (mean.shape, P.shape)
        mean, pm = _lib.as_c(mean)
        P, pp = _lib.as_c(P)
        Y, py, n = self._rows_arg(Y)
        X = np.empty((n, P.shape[1]))
        self._ck(self.lib.gp_project_rows(self.h, n, py, pm, pp, P.shape[1], X.ctypes.data_as(_lib._dp)), 'gp_project_rows')
        return X

    # ---- the start of latent inference (gp_nearest_rows) ----------------------------------------------------
    def nearest_rows(self, Y_test, cols=None, Y_train=None, want_x=True, observed=None):
        """Per row of ``Y_test`` (n, D) the nearest training row in squared Euclidean distance over the output columns ``cols`` (None: all; the
        other columns may hold NaN) -- or, with ``observed`` (n, D) bool instead of ``cols``, over every row's own observed columns
        (gp_nearest_rows_masked: an unobserved entry may hold NaN; every row observes something) -- among the resident rows of this engine
        (``Y_train`` None) or the host rows ``Y_train`` (n_train, D).  Returns
        (dist2 (n,), index (n,) int64, x_near): of equally near rows the lowest index; x_near (n, Q) is the base mean X_mu[index] of the winner,
        None with host rows or ``want_x`` False.  Without training rows every index is -1 and every dist2 inf.  Shards combine by the minimum
        (gparml_amd.init.nearest_start).  The evaluation state is left untouched."""
        Y_test = np.atleast_2d(np.asarray(Y_test, dtype=np.float64))
        assert Y_test.ndim == 2 and Y_test.shape[1] == self.D, 'Y_test shape %s: (n, %d) expected' % (Y_test.shape, self.D)
        n = Y_test.shape[0]
        Y_test, py = _lib.as_c(Y_test)
        assert cols is None or observed is None, 'nearest_rows: cols and observed are alternatives'
        pc, nc = None, 0
        if observed is not None:
            observed = np.ascontiguousarray(np.atleast_2d(np.asarray(observed)) != 0, dtype=np.uint8)
            assert observed.shape == Y_test.shape, 'observed shape %s: %s expected' % (observed.shape, Y_test.shape)
        if cols is not None:
            cols = np.ascontiguousarray(np.asarray(cols).reshape(-1), dtype=np.int32)
            pc, nc = cols.ctypes.data_as(_lib._ip), int(cols.size)
        pt, n_train = None, 0
        if Y_train is not None:
            Y_train = np.asarray(Y_train, dtype=np.float64)
            if Y_train.ndim == 1:
                Y_train = Y_train[:, None]
            assert Y_train.ndim == 2 and Y_train.shape[1] == self.D, 'Y_train shape %s: (n_train, %d) expected' % (Y_train.shape, self.D)
            n_train = Y_train.shape[0]
            Y_train, pt = _lib.as_c(Y_train)
        dist2, index = np.empty(n), np.empty(n, dtype=np.int64)
        x = np.empty((n, self.Q)) if (want_x and Y_train is None) else None
        out = (dist2.ctypes.data_as(_lib._dp), index.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), x.ctypes.data_as(_lib._dp) if x is not None else None)
        if observed is not None:
            self._ck(self.lib.gp_nearest_rows_masked(self.h, n_train, pt, n, py, observed.ctypes.data_as(_lib._u8p), *out), 'gp_nearest_rows_masked')
        else:
            self._ck(self.lib.gp_nearest_rows(self.h, n_train, pt, n, py, pc, nc, *out), 'gp_nearest_rows')
        return dist2, index, x

    # ---- neighbours in latent space (gp_knn_rows) -----------------------------------------------------------------
    def knn_rows(self, X=None, k=1, X_train=None, weight=None, skip=None, skip_self=False):
        """Per query row the ``k`` (1 .. 32) nearest training rows in latent space (csrc/knn.hip): the queries ``X`` (n, Q), or the resident X_mu
        of this engine (``X`` None), against the host rows ``X_train`` (n_train, Q), or the resident X_mu (``X_train`` None), in the squared
        distance sum_q weight_q (x_q - t_q)^2 (``weight`` (Q,) finite and >= 0, None: Euclidean; the ARD alpha: the kernel's own metric).
        ``skip`` (n,) int: per query one training row that is left out (-1: none); ``skip_self`` (both sides resident): every query leaves out
        its own row.  Returns (dist2 (n, k), rows (n, k) int64): ascending in (dist2, row), an equal distance goes to the lower row; slots
        beyond the available rows hold -1 and inf.  A query's lists do not depend on the other queries, bit for bit.  Shards merge on the host
        (gparml_amd.init.knn).  The evaluation state is left untouched."""
        def rows_arg(A, name):
            if A is None:
                return None, None, self.N_s
            A = np.asarray(A, dtype=np.float64)
            if A.ndim == 1:
                A = A.reshape(-1, self.Q)
            assert A.ndim == 2 and A.shape[1] == self.Q, '%s shape %s: (n, %d) expected' % (name, A.shape, self.Q)
            A, pa = _lib.as_c(A)
            return A, pa, A.shape[0]
        X, px, n = rows_arg(X, 'X')
        X_train, pt, n_train = rows_arg(X_train, 'X_train')
        pw = None
        if weight is not None:
            weight = np.asarray(weight, dtype=np.float64).reshape(-1)
            assert weight.shape == (self.Q,), 'weight shape %s: (%d,) expected' % (weight.shape, self.Q)
            weight, pw = _lib.as_c(weight)
        ps = None
        if skip is not None:
            skip = np.ascontiguousarray(np.asarray(skip).reshape(-1), dtype=np.int64)
            assert skip.shape == (n,), 'skip shape %s: (%d,) expected' % (skip.shape, n)
            ps = skip.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        k = int(k)
        dist2, rows = np.empty((n, max(k, 0))), np.empty((n, max(k, 0)), dtype=np.int64)
        self._ck(self.lib.gp_knn_rows(self.h, n_train, pt, n, px, pw, k, ps, 1 if skip_self else 0, dist2.ctypes.data_as(_lib._dp),
                                      rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))), 'gp_knn_rows')
        return dist2, rows

    def knn_queries(self):
        """The rows ``knn_rows`` searches for with X None (init.knn passes them to the other shards)."""
        return self.download('X_MU')

    @property
    def n_rows(self):
        """Rows ``kmeans_accumulate`` clusters with X None (init.kmeans draws its seeds over them) and ``scatter_accumulate`` sums with Y None."""
        return self.N_s

    def take_rows(self, idx):
        """The rows ``idx`` of the resident X_mu (init.kmeans: the seeds)."""
        return self.download('X_MU')[np.asarray(idx, dtype=np.int64)]

    regime_A_hint = False
    _jitter_used = 0
    _jitter_hint = 0          # the jitter mask the previous evaluation ended up with (global_step)

    def set_local_statistics(self, sum_YYT, Psi2, C, sum_exp_K_ii, KL):
        Psi2, p2 = _lib.as_c(np.asarray(Psi2, dtype=np.float64).reshape(self.M, self.M))
        C, pc = _lib.as_c(np.asarray(C, dtype=np.float64).reshape(self.M, self.D))
        self._ck(self.lib.gp_set_local_statistics(self.h, float(sum_YYT), p2, pc, float(sum_exp_K_ii), float(KL)),
                 'gp_set_local_statistics')

    def i8_status(self):
        """The int8 phase-1 guard (gp_i8_status): {'state': -1 n/a | 0 unchecked | 1 accepted | 2 rejected, 'rel_psi2', 'rel_c', 'cond_lower_bound', 'checks'}."""
        st, ck = ctypes.c_int(), ctypes.c_int64()
        r2, rc, cl = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        self._ck(self.lib.gp_i8_status(self.h, ctypes.byref(st), ctypes.byref(r2), ctypes.byref(rc), ctypes.byref(cl), ctypes.byref(ck)), 'gp_i8_status')
        return {'state': st.value, 'rel_psi2': r2.value, 'rel_c': rc.value, 'cond_lower_bound': cl.value, 'checks': ck.value}

    def set_timing(self, level):
        """HIP timing events per evaluation: 2 = every stage and dominant kernel (default), 1 = first and last only (total_ms), 0 = none.
        Each event is ~4-7 us of idle stream; an optimiser on a small problem (BASELINE configs[1]) switches them off."""
        self._ck(self.lib.gp_set_timing(self.h, int(level)), "gp_set_timing")

    def timings(self):
        t = np.zeros(8)
        self._ck(self.lib.gp_last_timings(self.h, t.ctypes.data_as(_lib._dp)), 'gp_last_timings')
        return dict(generate_ms=t[0], phase1_ms=t[1], global_ms=t[2], phase2_ms=t[3], total_ms=t[4],
                    psi1_ms=t[5], p1_kernel_ms=t[6], p2_kernel_ms=t[7])

    def memory_info(self):
        """(free, total) bytes of the engine's device right now (hipMemGetInfo)."""
        f, t = ctypes.c_int64(), ctypes.c_int64()
        self._ck(self.lib.gp_memory_info(self.h, ctypes.byref(f), ctypes.byref(t)), 'gp_memory_info')
        return f.value, t.value

    # ---- results ------------------------------------------------------------------------------------
    _SHAPES = {
        'KMM': lambda s: (s.M, s.M), 'KMM_INV': lambda s: (s.M, s.M), 'PSI1': lambda s: (s.N_s, s.M),
        'PSI2_SUM': lambda s: (s.M, s.M), 'PSI1TY': lambda s: (s.M, s.D), 'KMM_PLUS_OP_INV': lambda s: (s.M, s.M),
        'DF_DKMM': lambda s: (s.M, s.M), 'DF_DPSI1TY': lambda s: (s.M, s.D), 'DF_DPSI2': lambda s: (s.M, s.M),
        'GRAD_X_MU': lambda s: (s.N_s, s.Q), 'GRAD_X_S': lambda s: (s.N_s, s.Q), 'SCALARS': lambda s: (8,),
        'PSI2_POINTS': lambda s: (s.N_s, s.M, s.M), 'DKMM_DZ': lambda s: (s.M, s.Q, s.M),
        'DPSI1TY_DZ': lambda s: (s.M, s.Q, s.D), 'DPSI2_DZ': lambda s: (s.M, s.Q, s.M),
        'DKMM_DALPHA': lambda s: (s.Q, s.M, s.M), 'DPSI1TY_DALPHA': lambda s: (s.Q, s.M, s.D),
        'DPSI2_DALPHA': lambda s: (s.Q, s.M, s.M), 'X_MU_TRIAL': lambda s: (s.N_s, s.Q), 'X_S_TRIAL': lambda s: (s.N_s, s.Q),
        'GRAD_LATEST': lambda s: (2, s.N_s, s.Q), 'X_MU': lambda s: (s.N_s, s.Q),
    }

    def download(self, name):
        shape = self._SHAPES[name](self)
        out = np.empty(shape, dtype=np.float64)
        self._ck(self.lib.gp_download(self.h, _lib.ARR[name], out.ctypes.data_as(_lib._dp), out.size), 'gp_download(%s)' % name)
        return out

    def peek(self, name, count):
        """The first ``count`` doubles of an internal device buffer as it lies in memory, padding included (gp_debug_peek: 'Bbar', 'Abar', 'stats',
        'grads', ...; a developer and test tool).  ``count`` must be at least the buffer's size; the rest of the result is left as allocated."""
        buf = np.empty(int(count))
        self._ck(self.lib.gp_debug_peek(self.h, name.encode(), buf.ctypes.data_as(_lib._dp), buf.size), 'gp_debug_peek(%s)' % name)
        return buf

    def scalars(self):
        s = self.download('SCALARS')
        return dict(sum_YYT=s[0], sum_exp_K_ii=s[1], KL=s[2], logdet_Kmm=s[3], logdet_A=s[4], F=s[5], grad_beta=s[6], grad_sf2=s[7])
