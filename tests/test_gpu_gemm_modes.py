"""The FP64 GEMM core (csrc/gemm.hip, gemm32.h) in every mode the library launches it, through gp_debug_gemm_modes, against tests/gemm_ref.py
(run with -m gpu).  Inputs are integer-valued, so the exact answer is float64 `@` in any summation order and the device has to give it bit for
bit: a dropped k-chunk, a swapped stride, a tile that is not mirrored or a write outside the result's windows cannot hide in a tolerance.  Every
parent buffer is NaN outside the operand windows and a sentinel outside the result's.  One rounding case per layout uses real inputs and a
derived bound."""
import zlib

import numpy as np
import pytest

import gemm_ref as G

pytestmark = pytest.mark.gpu

GP_OK = 0
CASES = G.all_exact_cases()


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7fffffff


def _run(case, bufs):
    rc, out = G.run_case(case, bufs)
    if rc != GP_OK:
        from gparml_amd import _lib
        _lib.raise_for(rc, _lib.load(), None, 'gp_debug_gemm_modes')
    return out


@pytest.mark.parametrize('name', sorted(n for n in CASES if not n.startswith(('xtx-', 'trtri-'))))
def test_exact(name):
    """the grid (four layouts x 32- and 128-tile kernel x tri x alpha/beta, windows with ld = cols + 128), split-k with beta != 0, the panel solve and
    the trailing update of the blocked Cholesky at Mp = 640 (batch 2; A == B and C windows of one matrix), the predict / infer shape n = 2 Mp"""
    case = CASES[name]
    bufs = G.make_buffers(case, _seed(name))
    G.check_exact(case, bufs, _run(case, bufs))


@pytest.mark.parametrize('K', G.XTX_SIZES)
def test_xtx_same_bits_in_every_mode(K):
    """A^-1 = X^T X, batch 2 with distinct matrices: lower tiles from their first non-zero k, mirrored, with 1, 2, 4 and 8 k-splits on the 128-tile kernel
    and on the 32-tile kernel -- each exact, hence all the same bits; and the same bits as the plain full product of the same operands on either kernel
    (the claim made at GemmP)."""
    first = G.xtx_case(K, 1, 1)
    bufs = G.make_buffers(first, _seed('xtx-%d' % K))
    outs = {}
    for splits, big in G.XTX_RUNS:
        case = CASES['xtx-%d-s%d-big%d' % (K, splits, big)]
        outs[(splits, big)] = _run(case, bufs)
        G.check_exact(case, bufs, outs[(splits, big)])
    for big in (0, 1):
        case = CASES['xtx-plain-%d-big%d' % (K, big)]
        outs[('plain', big)] = _run(case, bufs)
        G.check_exact(case, bufs, outs[('plain', big)])
    ref = outs[(1, 1)]
    for key, out in outs.items():
        assert np.array_equal(G.bits(out), G.bits(ref)), 'X^T X at %d: run %s differs in bits from the unsplit mirrored run' % (K, key)


@pytest.mark.parametrize('level', G.trtri_levels(), ids=lambda lv: 'h%d-p%d-np%d-rows%d' % lv)
def test_trtri_level(level):
    """the two launches of one level of the inverse factor by halves at Mp = 640 (five panels): h = 1 with two pairs, h = 2 with one, h = 4 with the pair that is
    cut off by the end of the matrix.  Inner batch = the pairs (stride 2 b (ld + 1)), outer = the two matrices; the second launch reads the first one's
    packed work panel."""
    p, q = G.trtri_cases(*level)
    pb = G.make_buffers(p, _seed('trtri-T-%d' % level[0]))
    T = _run(p, pb)
    G.check_exact(p, pb, T)
    qb = G.make_buffers(q, _seed('trtri-X21-%d' % level[0]), given={'Twork': T})
    # what the second launch reads of the work panel is what the first one wrote: integers within the bound its exactness rests on
    for i, o in G.entries(q):
        assert np.max(np.abs(T[G.window_index(q, 'B', i, o)])) <= q['bmax']
    G.check_exact(q, qb, _run(q, qb))


_LONG = {}


def _rounding(la, lb):
    if (la, lb) not in _LONG:
        case = G.rounding_case(la, lb, 0)
        bufs = G.make_buffers(case, _seed('rounding-%s%s' % (la, lb)), exact=False)
        _LONG[(la, lb)] = (bufs, G.gemm_modes_ref(case, bufs, dtype=np.longdouble), G.rounding_bound(case, bufs))
    return _LONG[(la, lb)]


@pytest.mark.parametrize('big', [0, 1])
@pytest.mark.parametrize('la,lb', G.LAYOUTS)
def test_rounding(la, lb, big):
    """real inputs, 256 x 256 x 272 (two chunks of the 32-tile kernel and a partial one), against an 80-bit product: elementwise within
    (K + 2) 2^-53 (|alpha| |A||B| + |beta| |C0|) -- derived (gemm_ref.rounding_bound), not measured"""
    bufs, (ref, must, may), bound = _rounding(la, lb)
    case = G.rounding_case(la, lb, big)
    out = _run(case, bufs)
    C0 = bufs['PC']
    assert must.sum() == 256 * 256 and not may.any()
    assert np.array_equal(G.bits(out)[~must], G.bits(C0)[~must])
    err = np.abs(out.astype(np.longdouble) - ref)[must].astype(np.float64)
    worst = np.max(err / bound[must])
    print('rounding %s%s big %d: worst error at %.3f of the bound' % (la, lb, big, worst))
    assert np.isfinite(out[must]).all() and worst <= 1.0


@pytest.mark.parametrize('name', sorted(G.refusal_cases()))
def test_hook_refusals(name):
    """everything that would reach launch_gemm's own refusals (GP_ERR_STATE), drop a k tail or leave a parent buffer is refused with GP_ERR_BAD_ARG, and gp_last_error says why"""
    from gparml_amd import _lib
    case, word = G.refusal_cases()[name]
    bufs = {p: np.full(length, 7.0) for p, length in case['parents'].items()}
    rc, out = G.run_case(case, bufs)
    assert rc == _lib.GP_ERR_BAD_ARG
    msg = _lib.load().gp_last_error(None).decode()
    assert 'gp_debug_gemm_modes' in msg and word in msg, msg
    assert (out == 7.0).all()
