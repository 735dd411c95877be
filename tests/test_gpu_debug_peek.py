"""gp_debug_peek's name table (csrc/debug.hip): every plain buffer by name with the element count the entry documents, and the state refusals in the
order the entry resolves names.  The counts are restated here from N_s, D, M, Q and the padded sizes (gp_create, GsState::alloc, P2State::alloc),
so a row that is dropped, renamed or given another buffer's size fails by name.  What the buffers hold is the business of the tests that read
them (test_gpu_fixed_elementwise.py, test_gpu_psi2_elementwise.py, test_gpu_resident_vectors.py, ...).

One context at (N_s, D, M, Q) = (7, 2, 4, 3) -- N below one tile, M below one block, odd Q -- with free embeddings, after one full evaluation with
embedding gradients; no inference, selection or L-BFGS call has been made on it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_S, D, M, Q = 7, 2, 4, 3
TILE = 128
SC_COUNT = 8                                   # csrc/gp_common.h
GS_TOTAL = 16 + 8 + 8 * 64                     # scalars | failure flags | dots_kernel's partials


def _pad(n, m=TILE):
    return (n + m - 1) // m * m


NP, MP, DP = _pad(N_S), _pad(M), _pad(D)
LDK = MP + DP
CXP = CZP = _pad(2 * Q + 1, 4)
P2_SLICES = max(1, min(8 * max(1, 64 // (MP // TILE)), NP // TILE))
# the plain buffers: name -> doubles
PLAIN = {
    'Linv': 2 * MP * MP, 'Inv': 2 * MP * MP, 'E': MP * DP, 'PsiE': MP * DP, 'T1': MP * MP, 'T2': MP * MP, 'dFdK': MP * MP, 'Bbar': MP * MP,
    'Abar': MP * DP, 'Bm': LDK * MP, 'gK': M * Q + Q, 'gs': GS_TOTAL,
    'stats': MP * MP + MP * DP + SC_COUNT, 'Kaug': NP * LDK, 'Kmm': 2 * MP * MP, 'KmmKeep': MP * MP, 'Z': MP * Q, 'Zaug': MP * CZP, 'mu': NP * Q,
    'S': NP * Q, 'Xa': NP * CXP, 'grads': M * Q + Q, 'Rpart': (2 * (P2_SLICES + 8) + 512 // (MP // TILE)) * MP * CXP,
    'dir': 2 * N_S * Q,
}
# the rows with a precondition this context meets: the resident CG vectors and the base embeddings as stored
RESIDENT = {'cg_g_new': 2 * N_S * Q, 'cg_g_old': 2 * N_S * Q, 'cg_g_latest': 2 * N_S * Q, 'Xmu': N_S * Q, 'Xs': N_S * Q}


def _peek(e, name, count):
    """(status, message) of a request for ``count`` doubles; the buffer is one double longer, and that one must not be written."""
    from gparml_amd import _lib
    buf = np.full(count + 1, -7.0)
    rc = e.lib.gp_debug_peek(e.h, name.encode(), buf.ctypes.data_as(_lib._dp), count)
    assert buf[count] == -7.0, name
    return rc, e.lib.gp_last_error(e.h).decode()


@pytest.fixture(scope='module')
def engine():
    from gparml_amd.engine import ShardEngine
    rng = np.random.RandomState(0)
    e = ShardEngine(N_S, D, M, Q, device=0)
    X = rng.standard_normal((N_S, Q))
    Y = np.stack([np.sin(X.sum(1)), np.cos(X[:, 0])], 1) + 0.1 * rng.standard_normal((N_S, D))
    e.upload_shard(Y, X, 0.3 * rng.standard_normal((N_S, Q)), xs_is_raw=True)
    e.set_globals(rng.standard_normal((M, Q)), 1.3, 0.5 + rng.uniform(size=Q), 2.0, N_global=N_S)
    e.phase1(); e.global_step(); e.phase2(True); e.finish()
    yield e
    e.close()


@pytest.mark.parametrize('name', sorted(PLAIN) + sorted(RESIDENT))
def test_every_buffer_takes_its_documented_count_and_refuses_one_double_fewer(name, engine):
    from gparml_amd._lib import GP_ERR_BAD_ARG, GP_OK
    count = PLAIN[name] if name in PLAIN else RESIDENT[name]
    rc, msg = _peek(engine, name, count)
    assert rc == GP_OK, (name, rc, msg)
    rc, msg = _peek(engine, name, count - 1)
    assert rc == GP_ERR_BAD_ARG and msg == 'gp_debug_peek: %d doubles needed' % count, (name, rc, msg)


def test_state_refusals_in_the_order_names_are_resolved(engine):
    from gparml_amd._lib import GP_ERR_BAD_ARG, GP_ERR_STATE, GP_OK
    from gparml_amd.engine import ShardEngine
    e = engine
    # 'infer_LEA' is a name of its own in front of the 'infer_' prefix: a lookup of the plan (none yet: nothing to copy), not the optimiser's state
    assert _peek(e, 'infer_LEA', 4)[0] == GP_OK
    assert _peek(e, 'infer_x', 4) == (GP_ERR_STATE, "gp_debug_peek: 'infer_x' before gp_infer_latent has built the optimiser's state")
    assert _peek(e, 'infer_nothing', 4) == (GP_ERR_BAD_ARG, "gp_debug_peek: unknown buffer 'infer_nothing'")
    assert _peek(e, 'select_L', 4) == (GP_ERR_STATE, "gp_debug_peek: 'select_L' outside gp_select_begin .. gp_select_end")
    assert _peek(e, 'select_d', 4) == (GP_ERR_STATE, "gp_debug_peek: 'select_d' outside gp_select_begin .. gp_select_end")
    assert _peek(e, 'lbfgs_g', 4) == (GP_ERR_STATE, "gp_debug_peek: 'lbfgs_g' outside gp_lbfgs_begin .. gp_lbfgs_end, or not a vector that holds anything")
    assert _peek(e, 'no_such_buffer', 4) == (GP_ERR_BAD_ARG, "gp_debug_peek: unknown buffer 'no_such_buffer'")
    # a second context: no data, then fixed embeddings
    rng = np.random.RandomState(1)
    f = ShardEngine(N_S, D, M, Q, device=0)
    try:
        assert _peek(f, 'Xmu', N_S * Q) == (GP_ERR_STATE, "gp_debug_peek: 'Xmu' before gp_upload_shard")
        f.upload_shard(rng.standard_normal((N_S, D)), rng.standard_normal((N_S, Q)), np.full((N_S, Q), 0.5), xs_is_raw=False)
        assert _peek(f, 'cg_g_new', 2 * N_S * Q) == (GP_ERR_STATE, "gp_debug_peek: 'cg_g_new' exists only with shard data and free embeddings (raw variances)")
        assert _peek(f, 'Xmu', N_S * Q)[0] == GP_OK
    finally:
        f.close()
