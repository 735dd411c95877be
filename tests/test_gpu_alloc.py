"""Device memory of contexts that are created, used and destroyed many times (the optimisers, the fuzz tests, long-lived C consumers): every
buffer has one owner (csrc/devbuf.h), so destroying a context frees all of it, and an allocation that fails part way through gp_create or through
a lazily allocated group leaves nothing behind.  The failures are injected with gp_debug_set_option("alloc_fail_after", k): the k-th
allocation after the call fails with GP_ERR_HIP.  A lazily allocated group is published whole or not at all, so a context whose allocation was made
to fail stays usable: the same call on it, with nothing armed, gives what it gives on a fresh context, bit for bit.  Each step runs in a child process
of its own."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

PRELUDE = r'''
import ctypes, sys, time
import numpy as np
sys.path.insert(0, %(root)r)
from gparml_amd import _lib
from gparml_amd.engine import ShardEngine
from oracle import factorised as Fz
lib = _lib.load()
SLACK = 64 << 20
probe = ShardEngine(128, 1, 1, 1)          # stays open: its memory_info() reads the device's free memory
def free_now(base=None):
    """Free device memory; with ``base``: once it is back within SLACK of it, or after 5 s (the runtime returns freed memory to the device
    asynchronously: a reading right after hipFree can be a gigabyte short, 0.2 s later it is not -- a leak never comes back)."""
    if base is None:
        time.sleep(0.5)                      # a baseline: let frees still in flight land first
    t0 = time.time()
    while True:
        free = probe.memory_info()[0]
        if base is None or abs(free - base) <= SLACK or time.time() - t0 > 5.0:
            return free
        time.sleep(0.05)
def engine(N, D, M, Q, regime, seed=1):
    d = Fz.synthetic_shard(N, D, M, Q, regime=regime, seed=seed, zseed=2, alpha_value=0.3)
    e = ShardEngine(N, D, M, Q)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    return e, d
'''

ROUNDS = PRELUDE + r'''
# (N, D, M, Q, regime, int8 phase 1): p1v2 (fixed embeddings), int8 phase 1, and regime B on the column, psi2_sym, tile-pair and generic kernels
SHAPES = [(20000, 10, 200, 10, 'A', False), (65536, 10, 512, 5, 'A', True), (3000, 5, 40, 10, 'B', False), (3000, 5, 512, 10, 'B', False),
          (3000, 5, 200, 20, 'B', False), (300, 2, 12, 70, 'B', False)]
base = None
for rnd in range(4):
    for (N, D, M, Q, regime, i8) in SHAPES:
        assert lib.gp_debug_set_option(b'p1_i8', 1 if i8 else 0) == 0
        e, d = engine(N, D, M, Q, regime, seed=rnd)
        for _ in range(3):
            out = e.evaluate(regime == 'B')
        assert np.isfinite(out['F'])
        if i8:
            assert e.i8_status()['checks'] >= 1, e.i8_status()       # the int8 path (and its guard buffers) ran
        e.predict(d['X_mu'][:50])                                    # certain inputs
        e.predict(d['X_mu'][:50], np.full((50, Q), 0.1))             # uncertain inputs
        e.stats_pack()
        e2, _ = engine(N, D, M, Q, regime, seed=rnd + 7)
        e2.phase1()
        assert lib.gp_debug_force_staging(1) == 0
        try:
            e.combine(e2, 'stats')                                   # the staging buffer of the cross-device path
        finally:
            lib.gp_debug_force_staging(0)
        e2.close()
        e.close()
    lib.gp_debug_set_option(b'p1_i8', 0)
    free = free_now(base)
    if base is None:
        base = free
    print('round %d free %.1f MB (drift %.1f MB)' % (rnd, free / 2**20, (free - base) / 2**20), flush=True)
    assert abs(free - base) <= SLACK, ('device memory drifts', rnd, (free - base) / 2**20)
print('ROUNDS_OK', flush=True)
'''

CREATE = PRELUDE + r'''
# Kaug alone is 2e5 x 640 x 8 B = 1 GB: a leak of it cannot hide in the slack
N, D, M, Q = 200000, 100, 512, 10
base = free_now()
k = 1
while True:
    assert lib.gp_debug_set_option(b'alloc_fail_after', k) == 0
    h = ctypes.c_void_p()
    rc = lib.gp_create(ctypes.byref(h), 0, N, D, M, Q)
    lib.gp_debug_set_option(b'alloc_fail_after', 0)
    if rc == 0:
        lib.gp_destroy(h)
        break
    assert rc == _lib.GP_ERR_HIP, (k, rc)
    assert b'injected' in lib.gp_last_error(None), (k, lib.gp_last_error(None))
    assert not h.value
    free = free_now(base)
    assert abs(free - base) <= SLACK, ('gp_create leaks after the failed allocation', k, (free - base) / 2**20)
    k += 1
assert k > 20, k
assert abs(free_now(base) - base) <= SLACK
print('CREATE_OK', k - 1, 'failures', flush=True)
'''

LAZY = PRELUDE + r'''
def armed(make, call, what):
    """For k = 1, 2, ...: a fresh context from make(), the k-th allocation of call(e) made to fail; then, with nothing armed, call(e) again on the
    same context must return what call returns on a fresh context, bit for bit; then the context is destroyed.  Until call succeeds at once."""
    e = make()
    ref = call(e)
    e.close()
    base = free_now()
    k = 1
    while True:
        e = make()
        assert lib.gp_debug_set_option(b'alloc_fail_after', k) == 0
        try:
            out = call(e)
            ok = True
        except _lib.GparmlHipError as err:
            ok = False
            assert 'injected' in str(err), (what, k, str(err))
        finally:
            lib.gp_debug_set_option(b'alloc_fail_after', 0)
        if not ok:
            out = call(e)
        assert len(out) == len(ref)
        for i, (a, b) in enumerate(zip(ref, out)):
            assert np.array_equal(a, b), (what, 'differs from a fresh context after the failed allocation', k, i)
        e.close()
        free = free_now(base)
        assert abs(free - base) <= SLACK, (what, 'leaks after the failed allocation', k, (free - base) / 2**20)
        if ok:
            break
        k += 1
    print(what, k - 1, 'failures', flush=True)
    return k - 1

# the first phase 1 of a regime-B context: its tables and buffers (LE alone is 1e5 x 512 x 8 B = 410 MB) and the partial buffer's growth
def make_b():
    return engine(100000, 5, 512, 10, 'B')[0]
def phase1_stats(e):
    """phase 1, then the packed statistics: Psi2 | C | scalars"""
    e.phase1()
    return e.download('PSI2_SUM'), e.download('PSI1TY'), e.download('SCALARS')
assert armed(make_b, phase1_stats, 'phase1_regime_B') >= 10

# the first prediction at uncertain inputs, after one evaluation: both groups of chunk buffers (16384-point chunks: the product buffer alone is 100 MB)
X = np.random.RandomState(3).randn(40, 5)
assert lib.gp_debug_set_option(b'predict_rows', 16384) == 0
def make_p():
    e, d = engine(20000, 10, 512, 5, 'A')
    e.evaluate(False)
    return e
try:
    assert armed(make_p, lambda e: e.predict(X, np.full(X.shape, 0.2)), 'predict_uncertain') >= 10
finally:
    lib.gp_debug_set_option(b'predict_rows', 0)

# the first latent inference on a trained regime-A context: its three groups (model tables, chunk buffers, optimiser state; 16384-row chunks: V and
# LEA are 67 MB each)
Yi, Xi, Si = np.random.RandomState(4).randn(40, 10), np.random.RandomState(5).randn(40, 5), np.full((40, 5), 0.2)
assert lib.gp_debug_set_option(b'infer_rows', 16384) == 0
try:
    assert armed(make_p, lambda e: e.infer_latent(Yi, Xi, Si, max_iters=2), 'infer_latent') >= 20
finally:
    lib.gp_debug_set_option(b'infer_rows', 0)
print('LAZY_OK', flush=True)
'''


def _run(tmp_path, name, script, token):
    path = tmp_path / (name + '.py')
    path.write_text(script.replace('%(root)r', repr(ROOT)))
    r = subprocess.run([sys.executable, str(path)], capture_output=True, text=True, timeout=900, cwd=ROOT, env=dict(os.environ))
    assert r.returncode == 0 and token in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    print(r.stdout[-1500:])


def test_contexts_of_every_lazy_family_do_not_leak(tmp_path):
    _run(tmp_path, 'alloc_rounds', ROUNDS, 'ROUNDS_OK')


def test_failed_create_leaves_nothing_behind(tmp_path):
    _run(tmp_path, 'alloc_create', CREATE, 'CREATE_OK')


def test_failed_lazy_allocation_leaves_nothing_behind(tmp_path):
    _run(tmp_path, 'alloc_lazy', LAZY, 'LAZY_OK')
