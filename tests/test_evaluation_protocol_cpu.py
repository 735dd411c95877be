"""The evaluation protocol of gparml_amd/evaluation.py on CPU: the four host surfaces (ShardEngine.evaluate, Driver's fast mode, ResidentModel,
DistributedEvaluator) driven with a recording stand-in engine, a fake torch.distributed and fake timing events.  Every case compares the whole
trace -- (engine id, method, arguments), the collectives and the event records, in order -- with a literal one.  The literal traces were
recorded by running these same case functions against the commit BEFORE the four surfaces became callers of evaluation.py (each then spelled
the loop and the reduce out itself), not against the code under test: what is asserted is that nothing moved."""
import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)

from gparml_amd._lib import JitterRetry
from gparml_amd.engine import ShardEngine

LOG = []
M, Q, D = 2, 1, 1


class Rec(object):
    """Stand-in with the methods of ShardEngine the evaluators use; every call is logged as (engine id, method, arguments...)."""
    regime_A_hint = False
    _count = [0]

    def __init__(self, N_s=1, D=D, M=M, Q=Q, device=0):
        self.id = Rec._count[0]
        Rec._count[0] += 1
        self.N_s, self.D, self.M, self.Q, self.device = N_s, D, M, Q, device
        self.script = []            # finish() raises JitterRetry with these masks, one per call, before it succeeds

    def _log(self, *what):
        LOG.append((self.id,) + what)

    def set_timing(self, level):
        self._log('set_timing', level)

    def upload_shard(self, Y, X_mu, X_S, xs_is_raw=False):
        self._log('upload_shard', xs_is_raw)

    def set_globals(self, Z, sf2, alpha, beta, N_global=None, step_size=0.0):
        self._log('set_globals', N_global, step_size)

    def phase1(self):
        self._log('phase1')

    def combine(self, src, which='stats', op='add'):
        self._log('combine', src.id, which, op)

    def scale_buffer(self, which, factor):
        self._log('scale_buffer', which, factor)

    def stats_packed_buffer(self):
        self._log('stats_packed_buffer')
        return 1000 + self.id, 5

    def grads_buffer(self):
        self._log('grads_buffer')
        return 2000 + self.id, 3

    def stats_pack(self):
        self._log('stats_pack')

    def stats_unpack(self):
        self._log('stats_unpack')

    def allreduce(self, which='stats'):
        self._log('allreduce', which)

    def global_step(self, sync=True, jitter=0):
        self._log('global_step', sync, jitter)
        self._jitter_used = int(jitter)

    def phase2(self, want_embedding_grads=False):
        self._log('phase2', bool(want_embedding_grads))

    def finish(self):
        self._log('finish')
        if self.script:
            raise JitterRetry(self.script.pop(0), 'scripted')
        return dict(F=1.5, grad_Z=np.ones((self.M, self.Q)), grad_sf2=2.0, grad_alpha=np.ones(self.Q), grad_beta=3.0)

    def scalars(self):
        self._log('scalars')
        return dict(sum_YYT=0.0, sum_exp_K_ii=0.0, KL=0.0)

    def download(self, name):
        self._log('download', name)
        return np.zeros(1)

    def predict(self, X_mu, X_S=None, include_noise=False):
        self._log('predict', include_noise)
        return None, None

    def close(self):
        pass


class RecHost(Rec):
    """... with numpy buffers for torch.distributed, as the oracle-backed stand-in of tests/test_dist_gloo.py has them."""

    def host_buffers(self):
        self._log('host_buffers')
        return np.zeros(5), np.zeros(3)


class RecShard(Rec, ShardEngine):
    """ShardEngine.evaluate itself, on the recording methods (no library is loaded)."""


class FakeDist(object):
    """torch.distributed for one scripted rank; the collectives are logged with the length of their tensor (5 statistics, 3 gradient sums)."""
    class ReduceOp(object):
        SUM, MAX, MIN = 'SUM', 'MAX', 'MIN'

    def __init__(self, rank=0, world=2):
        self.rank, self.world = rank, world

    def is_available(self):
        return True

    def is_initialized(self):
        return True

    def get_rank(self, group=None):
        return self.rank

    def get_world_size(self, group=None):
        return self.world

    def get_backend(self, group=None):
        return 'gloo'

    def all_reduce(self, t, op=None, group=None):
        LOG.append(('dist', 'all_reduce', len(t), op))


class FakeEvent(object):
    def __init__(self, i):
        self.i = i

    def record(self):
        LOG.append(('event', self.i))


def _fresh():
    del LOG[:]
    Rec._count[0] = 0


def _fake_dist(monkeypatch, rank=0, native=False):
    """Put a FakeDist where ``import torch.distributed`` finds it; ``native``: dist.init_native_comm agrees to the library's own communicator."""
    import torch
    from gparml_amd import dist as gdist
    monkeypatch.setattr(torch, 'distributed', FakeDist(rank))
    monkeypatch.setattr(gdist, 'device_tensor', lambda ptr, n, device: np.zeros(n))
    monkeypatch.setattr(gdist, 'init_native_comm', lambda engine, dist, group=None: native)


# ---- ShardEngine.evaluate: one engine, no reduce ------------------------------------------------------------------------------------------
def shard_trace(script, want=False):
    _fresh()
    eng = RecShard()
    eng.script = list(script)
    out = eng.evaluate(want)
    assert out['F'] == 1.5
    return list(LOG), eng


ONE_PASS = [(0, 'phase1'), (0, 'global_step', False, 0), (0, 'phase2', False), (0, 'finish')]


def test_shard_engine_no_retry():
    log, eng = shard_trace([])
    assert log == ONE_PASS and eng.last_jitter == 0
    log, eng = shard_trace([], want=True)
    assert log == [(0, 'phase1'), (0, 'global_step', False, 0), (0, 'phase2', True), (0, 'finish'), (0, 'download', 'GRAD_X_MU'),
                   (0, 'download', 'GRAD_X_S')]


def test_shard_engine_one_and_two_retries():
    log, eng = shard_trace([2])
    assert log == ONE_PASS + [(0, 'global_step', False, 2), (0, 'phase2', False), (0, 'finish')] and eng.last_jitter == 2
    log, eng = shard_trace([1, 3])
    assert log == ONE_PASS + [(0, 'global_step', False, 1), (0, 'phase2', False), (0, 'finish'),
                              (0, 'global_step', False, 3), (0, 'phase2', False), (0, 'finish')] and eng.last_jitter == 3


# ---- Driver._evaluate_fast: three shards in one process, node drop-out --------------------------------------------------------------------
class FakeMapReduce(object):
    def __init__(self, engines, kept=None, frac=None):
        self.engines, self.kept, self.frac = engines, kept, frac

    def _input_files(self, options):
        return ['shard%d' % e.id for e in self.engines]

    def _prepare_shards(self, options, files, gs):
        return self.engines

    def _draw_drop_out(self, n_nodes, fraction):
        return self.kept, self.frac

    def _for_each(self, items, fn):          # in order: the threads of gpu_MapReduce._for_each would interleave the log
        return [fn(x) for x in items]

    def save(self, path, value):
        pass


def driver_trace(kept=None, frac=None, root_script=()):
    from gparml_amd.driver import Driver
    _fresh()
    engines = [Rec() for _ in range(3)]
    engines[0].script = list(root_script)
    o = {'M': M, 'Q': Q, 'D': D, 'fixed_embeddings': True, 'statistics': 'unused', 'embeddings': 'unused', 'i': 0,
         'drop_out_fraction': 0.5 if kept is not None else 0}
    drv = Driver(o, FakeMapReduce(engines, kept, frac))
    F, grad = drv._evaluate_fast({'beta': np.array([[1.0]])})
    assert F == 1.5 and len(drv.time_acc['time_acc_statistics_map_reduce']) == 1
    return list(LOG), drv


DRIVER_TAIL = [(0, 'scalars'), (0, 'download', 'PSI2_SUM'), (0, 'download', 'PSI1TY'), (0, 'download', 'DF_DKMM'), (0, 'download', 'DF_DPSI1TY'),
               (0, 'download', 'DF_DPSI2')]
SECOND_PASS_3 = lambda mask: [(0, 'global_step', False, mask), (0, 'phase2', False), (1, 'global_step', False, mask), (1, 'phase2', False),   # noqa: E731
                              (2, 'global_step', False, mask), (2, 'phase2', False)]


def test_driver_fast_no_drop_out():
    log, drv = driver_trace()
    assert log == ([(0, 'phase1'), (1, 'phase1'), (2, 'phase1'), (0, 'combine', 1, 'stats', 'add'), (0, 'combine', 2, 'stats', 'add'),
                    (1, 'combine', 0, 'stats', 'copy'), (2, 'combine', 0, 'stats', 'copy')] + SECOND_PASS_3(0)
                   + [(0, 'combine', 1, 'grads', 'add'), (0, 'combine', 2, 'grads', 'add'), (0, 'finish')] + DRIVER_TAIL)
    assert drv.last_jitter == 0


def test_driver_fast_drop_out_keeps_shards_0_and_2():
    """The dropped shard is not added, and still gets the reduced statistics: it runs the global step and phase 2 for its own embeddings."""
    log, drv = driver_trace(kept=[0, 2], frac=2.0 / 3.0)
    assert log == ([(0, 'phase1'), (1, 'phase1'), (2, 'phase1'), (0, 'combine', 2, 'stats', 'add'), (0, 'scale_buffer', 'stats', 1.5),
                    (1, 'combine', 0, 'stats', 'copy'), (2, 'combine', 0, 'stats', 'copy')] + SECOND_PASS_3(0)
                   + [(0, 'combine', 2, 'grads', 'add'), (0, 'scale_buffer', 'grads', 1.5), (0, 'finish')] + DRIVER_TAIL)


def test_driver_fast_one_retry_with_drop_out():
    """The gradient sums are reduced and rescaled on both passes, the statistics once."""
    log, drv = driver_trace(kept=[0, 2], frac=2.0 / 3.0, root_script=[2])
    assert log == ([(0, 'phase1'), (1, 'phase1'), (2, 'phase1'), (0, 'combine', 2, 'stats', 'add'), (0, 'scale_buffer', 'stats', 1.5),
                    (1, 'combine', 0, 'stats', 'copy'), (2, 'combine', 0, 'stats', 'copy')] + SECOND_PASS_3(0)
                   + [(0, 'combine', 2, 'grads', 'add'), (0, 'scale_buffer', 'grads', 1.5), (0, 'finish')] + SECOND_PASS_3(2)
                   + [(0, 'combine', 2, 'grads', 'add'), (0, 'scale_buffer', 'grads', 1.5), (0, 'finish')] + DRIVER_TAIL)
    assert drv.last_jitter == 2


# ---- ResidentModel: two engines in this process, with and without a process group ---------------------------------------------------------
def resident_model(group=None):
    from gparml_amd.resident import ResidentModel
    _fresh()
    z = lambda n: np.zeros((n, 1))         # noqa: E731
    model = ResidentModel([(z(3), z(3), z(3)), (z(2), z(2), z(2))], M, Q, D, fixed_embeddings=True, dist_group=group, N_global=5, engine_class=Rec)
    assert LOG == [(0, 'set_timing', 0), (0, 'upload_shard', False), (1, 'set_timing', 0), (1, 'upload_shard', False)]
    del LOG[:]
    return model


X = np.zeros(M * Q + 1 + Q + 1)


def resident_trace(group=None, root_script=()):
    model = resident_model(group)
    model.engines[0].script = list(root_script)
    f, g = model.likelihood_and_gradient(X, 0)
    assert f == -1.5 and g.shape == X.shape
    return list(LOG), model


def test_resident_model_two_engines_alone():
    log, model = resident_trace()
    # the parent set the globals and ran phase 1 engine by engine; all globals first, then every phase 1, is the one interleaving that moved
    assert log == [(0, 'set_globals', 5, 0), (1, 'set_globals', 5, 0), (0, 'phase1'), (1, 'phase1'), (0, 'combine', 1, 'stats', 'add'),
                   (1, 'combine', 0, 'stats', 'copy'), (0, 'global_step', False, 0), (0, 'phase2', False), (1, 'global_step', False, 0),
                   (1, 'phase2', False), (0, 'combine', 1, 'grads', 'add'), (0, 'finish')]
    assert model.last_jitter == 0 and model.n_collectives == 0 and model.version == 1
    log, model = resident_trace(root_script=[2])
    assert log[-6:] == [(0, 'global_step', False, 2), (0, 'phase2', False), (1, 'global_step', False, 2), (1, 'phase2', False),
                        (0, 'combine', 1, 'grads', 'add'), (0, 'finish')] and len(log) == 18 and log[11] == (0, 'finish')
    assert model.last_jitter == 2


def test_resident_model_torch_collectives(monkeypatch):
    """Across processes through torch.distributed: the views are made once, at the first collective; pack and unpack around the statistics."""
    _fake_dist(monkeypatch)
    log, model = resident_trace(group='group')
    assert log == [(0, 'set_globals', 5, 0), (1, 'set_globals', 5, 0), (0, 'phase1'), (1, 'phase1'), (0, 'combine', 1, 'stats', 'add'),
                   (0, 'stats_packed_buffer'), (0, 'grads_buffer'), (0, 'stats_pack'), ('dist', 'all_reduce', 5, 'SUM'), (0, 'stats_unpack'),
                   (1, 'combine', 0, 'stats', 'copy'), (0, 'global_step', False, 0), (0, 'phase2', False), (1, 'global_step', False, 0),
                   (1, 'phase2', False), (0, 'combine', 1, 'grads', 'add'), ('dist', 'all_reduce', 3, 'SUM'), (0, 'finish')]
    assert model.n_collectives == 2
    del LOG[:]
    model.likelihood_and_gradient(X, 1)
    assert (0, 'stats_packed_buffer') not in LOG and len(LOG) == 16 and model.n_collectives == 4


def test_resident_model_native_collectives(monkeypatch):
    _fake_dist(monkeypatch, native=True)
    log, model = resident_trace(group='group', root_script=[2])
    assert log == [(0, 'set_globals', 5, 0), (1, 'set_globals', 5, 0), (0, 'phase1'), (1, 'phase1'), (0, 'combine', 1, 'stats', 'add'),
                   (0, 'allreduce', 'stats'), (1, 'combine', 0, 'stats', 'copy'),
                   (0, 'global_step', False, 0), (0, 'phase2', False), (1, 'global_step', False, 0), (1, 'phase2', False),
                   (0, 'combine', 1, 'grads', 'add'), (0, 'allreduce', 'grads'), (0, 'finish'),
                   (0, 'global_step', False, 2), (0, 'phase2', False), (1, 'global_step', False, 2), (1, 'phase2', False),
                   (0, 'combine', 1, 'grads', 'add'), (0, 'allreduce', 'grads'), (0, 'finish')]
    assert model.n_collectives == 3 and model.last_jitter == 2


def test_resident_model_predict_refreshes_the_statistics_when_they_are_stale():
    model = resident_model()
    refresh = [(0, 'set_globals', 5, 0.0), (1, 'set_globals', 5, 0.0), (0, 'phase1'), (1, 'phase1'), (0, 'combine', 1, 'stats', 'add'),
               (0, 'global_step', True, 0)]
    model.predict(X, np.zeros((1, Q)))
    assert LOG == refresh + [(0, 'predict', False)]
    del LOG[:]
    model.predict(X, np.zeros((1, Q)), include_noise=True)           # same vector, same version: the statistics stand
    assert LOG == [(0, 'predict', True)]
    del LOG[:]
    model.version += 1                                              # an optimiser moved the resident embeddings
    model.predict(X, np.zeros((1, Q)))
    assert LOG == refresh + [(0, 'predict', False)]
    del LOG[:]
    model.likelihood_and_gradient(X, 0)                             # an evaluation at X leaves the root's statistics current
    del LOG[:]
    model.predict(X, np.zeros((1, Q)))
    assert LOG == [(0, 'predict', False)]


# ---- DistributedEvaluator: one engine per rank, world 2 -----------------------------------------------------------------------------------
def dist_trace(monkeypatch, rank=0, kept_mask=None, timed=False, native=False, script=(), engine=RecHost):
    from gparml_amd.dist import DistributedEvaluator
    _fake_dist(monkeypatch, rank, native)
    _fresh()
    eng = engine()
    eng.script = list(script)
    ev = DistributedEvaluator(eng)
    assert ev.world == 2 and ev.rank == rank and ev.native == native
    if timed:
        ev.time_collectives = True
        ev._cev = [FakeEvent(i) for i in range(4)]
    out = ev.evaluate(False, kept_mask=kept_mask)
    assert out['F'] == 1.5
    return list(LOG), ev


def test_distributed_evaluator_kept_rank(monkeypatch):
    log, ev = dist_trace(monkeypatch)
    assert log == [(0, 'host_buffers'), (0, 'phase1'), ('dist', 'all_reduce', 5, 'SUM'), (0, 'global_step', False, 0), (0, 'phase2', False),
                   ('dist', 'all_reduce', 3, 'SUM'), (0, 'finish')]
    assert ev.last_jitter == 0
    log, ev = dist_trace(monkeypatch, kept_mask=[True, False], script=[2])       # the other rank is dropped: kept fraction 1/2
    assert log == [(0, 'host_buffers'), (0, 'phase1'), ('dist', 'all_reduce', 5, 'SUM'), (0, 'scale_buffer', 'stats', 2.0),
                   (0, 'global_step', False, 0), (0, 'phase2', False), ('dist', 'all_reduce', 3, 'SUM'), (0, 'scale_buffer', 'grads', 2.0), (0, 'finish'),
                   (0, 'global_step', False, 2), (0, 'phase2', False), ('dist', 'all_reduce', 3, 'SUM'), (0, 'scale_buffer', 'grads', 2.0), (0, 'finish')]
    assert ev.last_jitter == 2


def test_distributed_evaluator_dropped_rank(monkeypatch):
    log, ev = dist_trace(monkeypatch, rank=1, kept_mask=[True, False])
    assert log == [(0, 'host_buffers'), (0, 'phase1'), (0, 'scale_buffer', 'stats', 0.0), ('dist', 'all_reduce', 5, 'SUM'),
                   (0, 'scale_buffer', 'stats', 2.0), (0, 'global_step', False, 0), (0, 'phase2', False), (0, 'scale_buffer', 'grads', 0.0),
                   ('dist', 'all_reduce', 3, 'SUM'), (0, 'scale_buffer', 'grads', 2.0), (0, 'finish')]


def test_distributed_evaluator_event_positions(monkeypatch):
    """torch path on the device buffers: event 0 behind the pack, event 1 in front of the unpack; native path: the events around allreduce."""
    log, ev = dist_trace(monkeypatch, timed=True, engine=Rec)
    assert log == [(0, 'stats_packed_buffer'), (0, 'grads_buffer'), (0, 'phase1'), (0, 'stats_pack'), ('event', 0), ('dist', 'all_reduce', 5, 'SUM'),
                   ('event', 1), (0, 'stats_unpack'), (0, 'global_step', False, 0), (0, 'phase2', False), ('event', 2),
                   ('dist', 'all_reduce', 3, 'SUM'), ('event', 3), (0, 'finish')]
    log, ev = dist_trace(monkeypatch, timed=True, native=True, engine=Rec)
    assert log == [(0, 'phase1'), ('event', 0), (0, 'allreduce', 'stats'), ('event', 1), (0, 'global_step', False, 0), (0, 'phase2', False),
                   ('event', 2), (0, 'allreduce', 'grads'), ('event', 3), (0, 'finish')]
    log, ev = dist_trace(monkeypatch, rank=1, kept_mask=[True, False], timed=True, engine=RecHost)
    assert log == [(0, 'host_buffers'), (0, 'phase1'), (0, 'scale_buffer', 'stats', 0.0), ('event', 0), ('dist', 'all_reduce', 5, 'SUM'), ('event', 1),
                   (0, 'scale_buffer', 'stats', 2.0), (0, 'global_step', False, 0), (0, 'phase2', False), (0, 'scale_buffer', 'grads', 0.0),
                   ('event', 2), ('dist', 'all_reduce', 3, 'SUM'), ('event', 3), (0, 'scale_buffer', 'grads', 2.0), (0, 'finish')]


def test_one_engine_without_a_reduce_calls_nothing_but_the_engine():
    from gparml_amd.evaluation import evaluate
    _fresh()
    eng = Rec()
    eng.script = [1]
    out, mask = evaluate([eng], None, True)
    assert mask == 1 and LOG == [(0, 'phase1'), (0, 'global_step', False, 0), (0, 'phase2', True), (0, 'finish'), (0, 'global_step', False, 1),
                                 (0, 'phase2', True), (0, 'finish')]
