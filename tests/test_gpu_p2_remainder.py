"""Fixed-embedding phase 2 with the ragged last round of row tiles cut along k (gparml_amd/csrc/p2_rem.hip: p2_rem_kernel, p2_rem_fix_kernel).

run_phase2 deals ntiles = ceil(N / 128) row tiles to S = min(8 * max(1, 64 / MT), ntiles) slices, MT = ceil(M / 128).  With ntiles = q S + r, 0 < r < S,
the main launch runs q rounds and the last r row tiles go to the remainder path; r = 0 leaves the whole-tile plan alone.  The shapes sit at the path's
edges (S, r, what the shape covers):
  M = 512, D = 100, Q = 10   S = 128, ntiles = 2 * 128 + 1   N = 32896 exactly: 39 splits of one k chunk each (splits = chunks), 8 row groups
  M = 512, D = 100, Q = 10   S = 128, ntiles = 2 * 128 + 5   N = 33357: padded rows inside the last remainder tile, 25 splits of one or two chunks,
                                                             D = 100: four padded Y columns in the last chunk, three groups of four feature columns
  M = 128, D = 10,  Q = 3    S = 512, ntiles = 512 + 3       one m tile, one group of feature columns, 170 workgroups per tile product but 9 chunks: 9 splits
  M = 256, D = 100, Q = 1    S = 256, ntiles = 256 + 2       one group of feature columns ([mu | 1 | 0 0])
  M = 256, D = 100, Q = 7    S = 256, ntiles = 256 + 3       two groups, N not a multiple of 128
Every case: bound and gradients against the CPU oracle at the tolerances of test_gpu_parity's fixed-embedding cases; the path switched on against the
same context with it switched off, same norm; two evaluations bit for bit; one evaluation in the poison mode (gp_debug_set_option('poison_alloc', 1),
the switch GPARML_POISON=1 sets at load time: every buffer an evaluation must write before it reads holds NaN bytes) with the same bits.

The inverse squared length scales keep K_mm well conditioned, so that the oracle itself is good to the tolerances: 128 random inducing points in three
dimensions at alpha = 0.5 give cond(K_mm) = 5e9 (at 5: 1e3), and 256 random points on a line are singular at any scale -- the Q = 1 case puts them on a
grid of spacing 0.0196 with alpha = 3600 (neighbours correlate at 0.5, cond(K_mm) = 18)."""
import functools

import numpy as np
import pytest

from conftest import assert_close

pytestmark = pytest.mark.gpu

F_RTOL = 1e-6      # tests/test_gpu_parity.py
G_RTOL = 1e-5
KEYS = ('grad_Z', 'grad_alpha', 'grad_sf2', 'grad_beta')

#        N                 D    M    Q   alpha  r
CASES = [(257 * 128,       100, 512, 10, 0.3,   1),
         (260 * 128 + 77,  100, 512, 10, 0.3,   5),
         (515 * 128,       10,  128, 3,  5.0,   3),
         (258 * 128,       100, 256, 1,  3600., 2),
         (258 * 128 + 50,  100, 256, 7,  0.3,   3)]


def _lib():
    from gparml_amd import _lib as L
    return L.load()


def _evaluate(eng, d, on):
    assert _lib().gp_debug_set_option(b'p2_rem', 1 if on else 0) == 0
    try:
        eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
        eng.phase1()
        eng.global_step()
        eng.phase2(False)
        return eng.finish()
    finally:
        _lib().gp_debug_set_option(b'p2_rem', 1)


def _engine(d, N, D, M, Q):
    from gparml_amd.engine import ShardEngine
    eng = ShardEngine(N, D, M, Q)
    eng.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    return eng


@functools.lru_cache(maxsize=None)
def _runs(N, D, M, Q, alpha):
    """One shape: the oracle once, one context evaluated on / on / off, and a second context created and evaluated in the poison mode."""
    from oracle import factorised as Fz
    d = Fz.synthetic_shard(N, D, M, Q, regime='A', seed=21, zseed=22, alpha_value=alpha)
    if Q == 1:
        d['Z'] = np.linspace(-2.5, 2.5, M).reshape(M, 1)
    ref = Fz.evaluate(d['Z'], d['sf2'], d['alpha'], d['beta'], d['Y'], d['X_mu'], d['X_S'], want_embeddings=False)
    eng = _engine(d, N, D, M, Q)
    on, on2, off = _evaluate(eng, d, True), _evaluate(eng, d, True), _evaluate(eng, d, False)
    eng.close()
    assert _lib().gp_debug_set_option(b'poison_alloc', 1) == 0
    try:
        eng = _engine(d, N, D, M, Q)
        poisoned = _evaluate(eng, d, True)
        eng.close()
    finally:
        _lib().gp_debug_set_option(b'poison_alloc', 0)
    return dict(ref=ref, on=on, on2=on2, off=off, poisoned=poisoned)


def _same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ('F',) + KEYS)


@pytest.mark.parametrize('N,D,M,Q,alpha,r', CASES)
def test_remainder_path_against_oracle(N, D, M, Q, alpha, r):
    mt = -(-M // 128)
    assert (-(-N // 128)) % (8 * max(1, 64 // mt)) == r          # the case is the one the table above says
    R = _runs(N, D, M, Q, alpha)
    for k in ('F',) + KEYS:
        ref = np.asarray(R['ref'][k], dtype=float)
        print('%s: rel err on %.3e, off %.3e' % (k, np.max(np.abs(np.asarray(R['on'][k]) - ref)) / np.max(np.abs(ref)),
                                                 np.max(np.abs(np.asarray(R['off'][k]) - ref)) / np.max(np.abs(ref))))
    assert_close(R['on']['F'], R['ref']['F'], F_RTOL, what='F')
    for k in KEYS:
        assert_close(R['on'][k], R['ref'][k], G_RTOL, what=k)


@pytest.mark.parametrize('N,D,M,Q,alpha,r', CASES)
def test_remainder_path_against_whole_tile_plan(N, D, M, Q, alpha, r):
    R = _runs(N, D, M, Q, alpha)
    assert_close(R['on']['F'], R['off']['F'], F_RTOL, what='F on / off')
    for k in KEYS:
        assert_close(R['on'][k], R['off'][k], G_RTOL, what=k + ' on / off')
    # the two plans add the row tiles in different orders: equal bits in every element of grad_Z would mean the path was not taken
    assert not np.array_equal(R['on']['grad_Z'], R['off']['grad_Z'])


@pytest.mark.parametrize('N,D,M,Q,alpha,r', CASES)
def test_remainder_path_is_reproducible(N, D, M, Q, alpha, r):
    R = _runs(N, D, M, Q, alpha)
    assert _same_bits(R['on'], R['on2'])


@pytest.mark.parametrize('N,D,M,Q,alpha,r', CASES)
def test_remainder_path_reads_nothing_it_did_not_write(N, D, M, Q, alpha, r):
    R = _runs(N, D, M, Q, alpha)
    assert np.all(np.isfinite(R['poisoned']['grad_Z'])) and _same_bits(R['on'], R['poisoned'])


@pytest.mark.parametrize('N,D,M,Q,alpha', [(256 * 128, 10, 512, 10, 0.3), (1000, 6, 200, 5, 0.5)])
def test_no_remainder_leaves_the_plan_alone(N, D, M, Q, alpha):
    """ntiles = q S: the option changes nothing, bit for bit."""
    from oracle import factorised as Fz
    d = Fz.synthetic_shard(N, D, M, Q, regime='A', seed=21, zseed=22, alpha_value=alpha)
    eng = _engine(d, N, D, M, Q)
    on, off = _evaluate(eng, d, True), _evaluate(eng, d, False)
    eng.close()
    assert _same_bits(on, off)
