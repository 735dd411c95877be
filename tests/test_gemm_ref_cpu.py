"""tests/gemm_ref.py checked without a device: the reference is plain `@` on the trivial mode, every case of the table is exact in float64 and
keeps its windows inside their parents and apart, the checker itself notices each kind of error it is there for, and gp_debug_gemm_modes refuses
what it must before it touches a device."""
import numpy as np
import pytest

import gemm_ref as G

CASES = G.all_exact_cases()


def _view(buf, off, rows, cols, ld):
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(rows, cols), strides=(8 * ld, 8))


def test_reference_is_plain_matmul_on_the_trivial_mode():
    rs = np.random.RandomState(0)
    m, n, K = 256, 128, 48
    A, B, C0 = rs.randn(m, K), rs.randn(K, n), rs.randn(m, n)
    for la, lb in G.LAYOUTS:
        case = G.finish(dict(la=la, lb=lb, m=m, n=n, K=K, alpha=1.5, beta=-0.5,
                             A=G.win('PA', 0, K if la == 'K' else m), B=G.win('PB', 0, K if lb == 'K' else n), C=G.win('PC', 0, n)))
        bufs = {name: np.zeros(length) for name, length in case['parents'].items()}
        bufs['PA'][:m * K] = (A if la == 'K' else A.T).ravel()
        bufs['PB'][:n * K] = (B.T if lb == 'K' else B).ravel()
        bufs['PC'][:m * n] = C0.ravel()
        ref, must, may = G.gemm_modes_ref(case, bufs)
        assert np.array_equal(ref[:m * n].reshape(m, n), 1.5 * (A @ B) + -0.5 * C0)
        assert must[:m * n].all() and not must[m * n:].any() and not may.any()
        assert np.array_equal(ref[m * n:], bufs['PC'][m * n:])


def test_batches_strides_and_triangles_as_statements_about_elements():
    """two inner x two outer entries with all four strides distinct, tri = 1: entry (i, o) is the product of ITS windows, on the lower triangle"""
    case = G.finish(dict(la='K', lb='F', m=128, n=128, K=16, inner=2, outer=2, tri=1,
                         A=G.win('PA', 4, 20, s=128 * 20, o=3 * 128 * 20), B=G.win('PB', 2, 140, s=16 * 140, o=40 * 140), C=G.win('PC', 6, 130, s=130 * 130, o=300 * 130)))
    bufs = G.make_buffers(case, 1)
    ref, must, may = G.gemm_modes_ref(case, bufs)
    for i in range(2):
        for o in range(2):
            a = _view(bufs['PA'], 4 + i * 128 * 20 + o * 3 * 128 * 20, 128, 16, 20)
            b = _view(bufs['PB'], 2 + i * 16 * 140 + o * 40 * 140, 16, 128, 140)
            c = _view(ref, 6 + i * 130 * 130 + o * 300 * 130, 128, 128, 130)
            assert np.array_equal(c, a @ b)
    assert must.sum() == 4 * 128 * 129 // 2 and may.sum() == 4 * 128 * 127 // 2
    assert not np.isnan(ref[must | may]).any() and (ref[~(must | may)] == G.SENTINEL).all()


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_case_is_exact_in_float64_and_keeps_its_windows_apart(name):
    case = CASES[name]
    assert case['K'] * 16 < 2 ** 53 and case['K'] <= 2048
    assert G.exactness_bound(case) < 2 ** 53
    assert case['m'] % 128 == 0 and case['n'] % 128 == 0 and case['K'] % 16 == 0
    # every window inside its parent; no C window shares an element with another window of its parent (marked element by element)
    written = np.zeros(case['parents'][case['C']['parent']], dtype=np.int8)
    for i, o in G.entries(case):
        for which in 'ABC':
            idx = G.window_index(case, which, i, o)
            assert idx.min() >= 0 and idx.max() < case['parents'][case[which]['parent']]
        written[G.window_index(case, 'C', i, o)] += 1
    assert written.max() == 1
    for i, o in G.entries(case):
        for which in 'AB':
            if case[which]['parent'] == case['C']['parent']:
                assert not written[G.window_index(case, which, i, o)].any()


def test_the_checker_notices_what_it_is_there_for():
    """check_exact on a simulated device: passes on the reference's own answer (with the skipped triangle left alone, or computed), fails on one wrong
    element, a write outside the windows, an unmirrored tile"""
    case = G.windowed('K', 'F', 256, 256, 32, tri=1, alpha=-1.0, beta=1.0, batch=2)
    bufs = G.make_buffers(case, 2)
    ref, must, may = G.gemm_modes_ref(case, bufs)
    G.check_exact(case, bufs, ref)
    lazy = np.where(may, bufs['PC'], ref)
    G.check_exact(case, bufs, lazy)
    for idx, val in ((np.flatnonzero(must)[77], 0.5), (np.flatnonzero(may)[5], 1e9), (np.flatnonzero(~(must | may))[-1], 0.0)):
        wrong = lazy.copy()
        wrong[idx] = val
        with pytest.raises(AssertionError):
            G.check_exact(case, bufs, wrong)
    x = G.xtx_case(384, 1, 1)
    xb = G.make_buffers(x, 3)
    xref, xmust, _ = G.gemm_modes_ref(x, xb)
    assert xmust.sum() == 2 * 384 * 384
    G.check_exact(x, xb, xref)
    unmirrored = xref.copy()
    up = G.window_index(x, 'C', 1, 0)[:128, 256:]
    unmirrored[up] = xb['PC'][up]
    with pytest.raises(AssertionError):
        G.check_exact(x, xb, unmirrored)
    # the zero a klow operand promises is there
    Xw = xb['X'][G.window_index(x, 'A', 0, 0)]
    assert not np.triu(Xw, 1).any() and np.tril(Xw).any()


def test_sign_of_zero_is_the_only_thing_bit_equality_forgives():
    a = np.array([0.0, -0.0, 1.0, np.nan])
    assert G.same_value_bits(a, np.array([-0.0, 0.0, 1.0, np.nan])).all()
    assert not G.same_value_bits(a, np.array([0.0, 0.0, np.nextafter(1.0, 2.0), np.nan]))[2]


@pytest.mark.parametrize('name', sorted(G.refusal_cases()))
def test_hook_refuses_without_touching_a_device(name):
    from gparml_amd import _lib
    case, word = G.refusal_cases()[name]
    bufs = {p: np.zeros(length) for p, length in case['parents'].items()}
    rc, _ = G.run_case(case, bufs)
    assert rc == _lib.GP_ERR_BAD_ARG
    msg = _lib.load().gp_last_error(None).decode()
    assert 'gp_debug_gemm_modes' in msg and word in msg, msg
