"""Which globals the device holds is ShardEngine's knowledge (ShardEngine.globals_key), not partial_terms': the real ShardEngine and the real
partial_terms on a scripted library that logs every gp_* call and returns GP_OK -- no GPU.  partial_terms pushes each distinct set of globals once,
and again after anything that moves the engine away from them; ShardEngine.set_globals itself never skips."""
import ctypes

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)

M, Q, N, D = 3, 2, 4, 2


class ScriptedLib(object):
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('gp_'):
            raise AttributeError(name)

        def call(*args):
            self.calls.append(name)
            if name == 'gp_create':
                ctypes.cast(args[0], ctypes.POINTER(ctypes.c_void_p))[0] = 1
            return 0
        return call

    def pushes(self):
        return self.calls.count('gp_set_globals')


@pytest.fixture
def lib(monkeypatch):
    from gparml_amd import _lib
    L = ScriptedLib()
    monkeypatch.setattr(_lib, 'load', lambda: L)
    return L


def _terms():
    from gparml_amd.partial_terms import partial_terms
    r = np.random.RandomState(0)
    pt = partial_terms(r.randn(M, Q), 1.0, np.ones(Q), 2.0, M, Q, N, D, update_global_statistics=False)
    return pt, (r.randn(N, D), r.randn(N, Q), np.zeros((N, Q)))


def test_the_predict_sequence_pushes_once(lib):
    """set_data -> get_local_statistics -> set_local_statistics -> logmarglik -> grad_X_mu: a second gp_set_globals in between would declare the
    Psi1 of set_data stale."""
    pt, data = _terms()
    pt.set_data(*data)
    st = pt.get_local_statistics()
    pt.set_local_statistics(st['sum_YYT'], st['sum_exp_K_mi_K_im'], st['exp_K_miY'], st['sum_exp_K_ii'], st['KL'])
    pt.logmarglik()
    pt.grad_X_mu()
    assert lib.pushes() == 1 and lib.calls.count('gp_phase2') == 1
    pt.beta = 3.0                      # a new value is pushed
    pt.logmarglik()
    assert lib.pushes() == 2


@pytest.mark.parametrize('what', ['upload_shard', 'upload_embeddings', 'set_direction', 'cg_update', 'close'])
def test_the_engine_forgets_its_globals_when_it_moves_away_from_them(lib, what):
    pt, data = _terms()
    pt.set_data(*data)
    eng = pt._engine()
    assert lib.pushes() == 1 and eng.globals_key is not None
    pt._push_globals()
    assert lib.pushes() == 1           # the engine holds them
    {'upload_shard': lambda: eng.upload_shard(*data), 'upload_embeddings': lambda: eng.upload_embeddings(data[1], data[2]),
     'set_direction': lambda: eng.set_direction(None), 'cg_update': lambda: eng.cg_update(3), 'close': eng.close}[what]()
    assert eng.globals_key is None
    if what == 'close':
        pt._eng = None                 # partial_terms makes itself a new engine
    pt.update_global_statistics()      # needs the globals: pushed again
    assert lib.pushes() == 2


def test_set_globals_of_the_engine_never_skips(lib):
    from gparml_amd.engine import ShardEngine
    eng = ShardEngine(N, D, M, Q)
    Z, alpha = np.zeros((M, Q)), np.ones(Q)
    for _ in range(3):
        eng.set_globals(Z, 1.0, alpha, 2.0)
    assert lib.pushes() == 3 and eng.globals_key == ShardEngine.make_globals_key(Z, 1.0, alpha, 2.0, N)
    Z[0, 0] = 1.0                      # the key is a copy: a caller that changes Z in place is seen
    assert eng.globals_key != ShardEngine.make_globals_key(Z, 1.0, alpha, 2.0, N)
