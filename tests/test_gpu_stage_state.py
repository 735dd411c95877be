"""An evaluation's result is a function of the shape and the inputs, not of what the context ran before (csrc/gp_common.h: every stage owns its
state; csrc/devbuf.h, gp::Workspace: the one borrowed workspace, whose capacity is a function of the shape alone).  The stages whose decomposition
follows the room in the workspace -- the global step's split-k factors, the int8 phase 1's slice count -- read that capacity, so a regime-B
evaluation in between, whose pair kernel reserves a larger workspace (M = 1024: 2080 partial tiles against a capacity of 1188), must not change
the summation order of the fixed-embedding evaluations around it.  One context: fixed embeddings, then embeddings with variances and embedding
gradients, then the first embeddings again -- the third result must equal the first bit for bit, the second a fresh context's.  Runs in a child
process like its neighbours (tests/test_gpu_poison.py)."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, %(root)r)
from gparml_amd.engine import ShardEngine
from oracle import factorised as Fz
# (N, D, M, Q): the split-k gate and the largest pair tables of the small paths; the big-tile products and the int8 global step
SHAPES = [(3000, 5, 512, 10), (2048, 3, 1024, 4)]
DOWN = ('PSI2_SUM', 'PSI1TY', 'SCALARS')
def evaluate(eng, d, emb):
    eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    out = eng.evaluate(emb)
    out['jitter'] = eng.last_jitter
    for k in DOWN:
        out[k] = eng.download(k)
    return out
def same(a, b, keys, what):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k, 'differs')
for (N, D, M, Q) in SHAPES:
    d = Fz.synthetic_shard(N, D, M, Q, regime='A', seed=21, zseed=22, alpha_value=0.3)
    b = Fz.synthetic_shard(N, D, M, Q, regime='B', seed=23, zseed=22, alpha_value=0.3)
    eng = ShardEngine(N, D, M, Q)
    eng.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    first = evaluate(eng, d, False)
    eng.upload_embeddings(b['X_mu'], b['X_S'])
    second = evaluate(eng, d, True)
    eng.upload_embeddings(d['X_mu'], d['X_S'])
    third = evaluate(eng, d, False)
    eng.close()
    fresh_eng = ShardEngine(N, D, M, Q)
    fresh_eng.upload_shard(d['Y'], b['X_mu'], b['X_S'])
    fresh = evaluate(fresh_eng, d, True)
    fresh_eng.close()
    keys = ('F', 'grad_Z', 'grad_alpha', 'grad_beta', 'grad_sf2', 'jitter') + DOWN
    assert np.isfinite(first['F']) and np.isfinite(second['F'])
    same(third, first, keys, ((N, D, M, Q), 'third evaluation against the first'))
    same(second, fresh, keys + ('grad_X_mu', 'grad_X_S'), ((N, D, M, Q), 'second evaluation against a fresh context'))
    print('HISTORY_OK', N, D, M, Q, flush=True)
'''


def test_an_evaluation_does_not_depend_on_what_the_context_ran_before(tmp_path):
    script = tmp_path / 'stage_state_child.py'
    script.write_text(CHILD % {'root': ROOT})
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ))
    assert r.returncode == 0 and r.stdout.count('HISTORY_OK') == 2, r.stdout[-1500:] + r.stderr[-3000:]
