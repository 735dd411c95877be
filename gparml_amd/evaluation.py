"""The evaluation protocol, once, for every host surface (ShardEngine.evaluate, Driver's fast mode, ResidentModel, DistributedEvaluator):

    phase 1 on every engine -> reduce the packed statistics -> [ global step + phase 2 on every engine -> reduce the packed gradient
    sums -> finish on the root engine ], the bracket repeated with the jitter mask while finish() raises JitterRetry.

The engines are duck-typed (the methods of gparml_amd.engine.ShardEngine used below): the CPU tests drive the same code with stand-ins.
"""
from ._lib import JitterRetry


class BufferReduce(object):
    """How the packed buffers of this process's engines become the global sums.  ``engines``: every engine of this process;
    ``contributing``: the ones whose buffers enter the sums (node drop-out inside a process, local_MapReduce.py:119-129; default all) --
    the first of them is the root, which ends up holding the sums.  ``dist`` (torch.distributed or a stand-in; None: this process is
    alone) and ``group``: the collective across processes.  ``dropped``: this whole rank contributes nothing; ``fraction``:
    kept/(kept+dropped), both reduced buffers are divided by it (:263-264).  ``events``: None or four objects with record()."""

    def __init__(self, engines, contributing=None, fraction=None, dist=None, group=None, device=None):
        self.engines = engines
        self.contributing = engines if contributing is None else contributing
        self.root = self.contributing[0]
        self.fraction, self.dropped = fraction, False
        self.dist, self.group, self.device = dist, group, device
        self.events = None
        self.n_collectives = 0          # collectives across processes issued so far
        self._native = None
        self._tensors = None

    @property
    def native(self):
        """The root reduces through its own RCCL communicator (gp_allreduce): decided once, on first use -- COLLECTIVE across ``group``."""
        if self._native is None:
            from .dist import init_native_comm
            self._native = bool(self.dist is not None and init_native_comm(self.root, self.dist, self.group))
        return self._native

    def tensors(self):
        """(statistics, gradient sums) for torch.distributed, made once (the pointers never change): zero-copy views of the root's packed
        device buffers (Psi2's upper triangle, no padding: stats_pack / stats_unpack), or a CPU stand-in's host_buffers() as they are."""
        if self._tensors is None:
            import torch
            root = self.root
            self._host = hasattr(root, 'host_buffers')
            if self._host:
                s, g = root.host_buffers()
                self._tensors = torch.from_numpy(s), torch.from_numpy(g)
            else:
                from .dist import device_tensor
                # the engine's own GPU, not torch's current device (a caller need not have run torch.cuda.set_device)
                dev = self.device if self.device is not None else torch.device('cuda', root.device)
                p, n = root.stats_packed_buffer()
                g, m = root.grads_buffer()
                self._tensors = device_tensor(p, n, dev), device_tensor(g, m, dev)
        return self._tensors

    def _collective(self, which):
        root, ev = self.root, self.events
        first = 0 if which == 'stats' else 2
        if self.native:
            pack = False                    # the library packs and unpacks the statistics itself, on the engine's stream
            collective = lambda: root.allreduce(which)                                                                  # noqa: E731
        else:
            t = self.tensors()[first // 2]
            pack = which == 'stats' and not self._host
            collective = lambda: self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group)                   # noqa: E731
        if pack:
            root.stats_pack()
        if ev:
            ev[first].record()
        collective()
        if ev:
            ev[first + 1].record()
        if pack:
            root.stats_unpack()
        self.n_collectives += 1

    def __call__(self, which, fan_back=True):
        """Reduce the 'stats' or the 'grads' buffers into the root.  The statistics then go back to every other local engine, dropped ones
        included: each of them runs the replicated global step (local_MapReduce.py:318-320)."""
        root = self.root
        for e in self.contributing[1:]:
            root.combine(e, which, 'add')           # statistics_reducer on the device(s)
        if self.dropped:
            root.scale_buffer(which, 0.0)
        if self.dist is not None:
            self._collective(which)
        if self.fraction is not None and self.fraction != 1.0:
            root.scale_buffer(which, 1.0 / self.fraction)
        if fan_back and which == 'stats':
            for e in self.engines:
                if e is not root:
                    e.combine(root, 'stats', 'copy')


def _each(engines, fn):
    for e in engines:
        fn(e)


def evaluate(engines, reduce=None, want_embedding_grads=False, for_each=_each):
    """One bound+gradient evaluation -> (what the root's finish() returns, the jitter mask the evaluation ended with: 0, or the matrices that
    needed the reference's 1e-7 jitter -- found by finish() here or, after an evaluation that needed it, already inside the root's
    global_step(), which leaves it in ``_jitter_used``).  ``reduce``: a BufferReduce, or None for one engine on its own.  ``for_each``
    applies a function to every engine (Driver: one thread per shard).  One host synchronisation, in finish()."""
    root = engines[0] if reduce is None else reduce.root
    for_each(engines, lambda e: e.phase1())
    if reduce is not None:
        reduce('stats')
    mask = 0

    def second(e):
        e.global_step(sync=False, jitter=mask)      # replicated M x M algebra
        e.phase2(want_embedding_grads)
    while True:                 # the retry mask only grows (bit 0 Kmm, bit 1 Kmm + beta Psi2): at most two repeats
        for_each(engines, second)
        if reduce is not None:
            reduce('grads')
        try:
            return root.finish(), mask | getattr(root, '_jitter_used', 0)
        except JitterRetry as r:
            # a failed factorisation (partial_terms.py:452-456: first without the 1e-7 jitter, then with).  Every engine, on every rank, holds
            # the same reduced statistics and runs the same global step: all repeat it together; only the gradient sums are reduced again
            mask = r.mask


def refresh_statistics(engines, reduce, all_engines=False):
    """Bring the root engine's global step up to date without an evaluation (predict, infer): phase 1, the reduce, the root's global step.
    ``all_engines``: the reduced statistics go back to every engine and each runs the global step (scoring the resident rows of every shard)."""
    for e in engines:
        e.phase1()
    reduce('stats', fan_back=all_engines)
    for e in (engines if all_engines else [reduce.root]):
        e.global_step(sync=True)
