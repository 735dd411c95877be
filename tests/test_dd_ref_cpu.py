"""tests/dd_ref.py checked without a device: the three exact methods agree, numpy emulations of the device arithmetic (ddacc_block, the four-quarter
row residual, the ten-digit int8 model) meet the derived bounds on every case of the table, every cancellation case separates the kernels from the
float64 product they replace, the checker notices each fault it is there for, and gp_debug_dd_product refuses what it must before it touches a device."""
import numpy as np
import pytest

import dd_ref as D

CASES = D.all_cases()
BOUND_CASES = sorted(n for n, c in CASES.items() if c['check'] == 'bound')


def _plain(case):
    a, B = D.operand(case)
    out = a @ B if not case['product'] else case['Csub'] - a @ B
    if case['form'] == D.ROW_RESIDUAL:
        out[case['M']:] = 0.0
    return out


def test_the_three_exact_methods_agree():
    """slices and Python integers (exact_product) against Fraction and against fsum over error-free products, sum and residual, with a wide dynamic range"""
    rs = np.random.RandomState(5)
    A, B = D.cancellation(rs, 8, 8, 64, a_range_bits=30)
    for Csub in (None, (A @ B) * (1 + 1e-12 * rs.randn(8, 8))):
        hi, lo = D.exact_product(A, B, Csub)
        fr = D.exact_fraction(A, B, Csub)
        fs = D.exact_fsum(A, B, Csub)
        for i in range(8):
            for j in range(8):
                assert float(fr[i, j]) == hi[i, j] == fs[i, j]
                assert float(fr[i, j] - D.Fraction(float(hi[i, j]))) == lo[i, j]


def test_rounded_operand_is_one_fma_and_one_add():
    """a case where the FMA and the two-rounding expression differ, and the diagonal's jitter"""
    beta, psi, keep = 1.7, np.array([[1.0 + 2.0 ** -30]]), np.array([[-1.7]])
    a = D.rounded_operand(keep, psi, beta, 0.0, 1)[0, 0]
    assert a == float(D.Fraction(beta) * D.Fraction(float(psi[0, 0])) + D.Fraction(-1.7)) and a != beta * psi[0, 0] + keep[0, 0]
    assert D.rounded_operand(keep, psi, beta, 1e-7, 1)[0, 0] == a + 1e-7


@pytest.mark.parametrize('name', BOUND_CASES)
def test_emulation_meets_the_bound(name):
    case = CASES[name]
    worst = D.check(case, D.emulate(case), 'emulation')
    print('%s: emulation at %.4f of the bound' % (name, worst))


@pytest.mark.parametrize('name', sorted(n for n, c in CASES.items() if c['check'] == 'bits' and c['K'] <= 512))
def test_emulation_is_exact_on_integers(name):
    D.check(CASES[name], D.emulate(CASES[name]), 'emulation')


@pytest.mark.parametrize('name', sorted(n for n, c in CASES.items() if c['cls'] == 'cancellation'))
def test_float64_product_violates_the_bound_on_most_elements(name):
    """the condition every cancellation case must meet: otherwise it does not separate the kernel from the float64 product it replaces"""
    share = D.share_outside(CASES[name], _plain(CASES[name]))
    assert share > 0.5, '%s: float64 `@` is outside the bound at only %.3f of the elements' % (name, share)


@pytest.mark.parametrize('da,db', [(1, 1), (1, 10), (10, 1), (5, 6), (4, 7), (6, 6), (10, 10), (2, 10)])
def test_probe_emulation(da, db):
    case = D.probe_case(da, db)
    assert case['check'] == ('bits' if da + db <= 11 else 'bound')
    D.check(case, D.emulate(case), 'emulation')


def _fails(case, out):
    with pytest.raises(AssertionError):
        D.check(case, out, 'faulty emulation')


def test_the_checker_notices_what_it_is_there_for():
    gemm, res, row = CASES['dd-gemm-128'], CASES['dd-residual-256x128'], CASES['row-M130-Dp128-jit0']
    for case in (gemm, res, row):
        _fails(case, D.emulate(case, 'lo'))                       # lo never added
        _fails(case, D.emulate(case, 'pe'))                       # the products' low parts never added
    _fails(res, D.emulate(res, 'sub'))                            # Csub - (hi + lo): hi + lo rounds away what the residual is made of
    _fails(row, D.emulate(row, 'sub'))
    i8 = CASES['i8-64x64x64-sum']
    _fails(i8, D.emulate(i8, 'weight'))                           # one order's weight off by 128
    probe = D.probe_case(5, 6)                                    # order 11, the last one kept
    D.check(probe, D.emulate(probe))
    _fails(probe, D.emulate(probe, 'order'))                      # ... dropped
    _fails(D.probe_case(3, 5), D.emulate(D.probe_case(3, 5), 'weight'))     # order 8 (index 6 counted from 0)
    # one wrong element, a NaN, a non-zero padding row
    for case in (gemm, row):
        good = D.emulate(case)
        for val in (np.nan, good[0, 3] * (1 + 2.0 ** -20)):
            bad = good.copy(); bad[0, 3] = val
            _fails(case, bad)
    bad = D.emulate(row); bad[200, 5] = 1e-300
    _fails(row, bad)
    integer = CASES['dd-gemm-512-integer']
    bad = D.emulate(integer); bad[511, 511] += 1.0
    _fails(integer, bad)


@pytest.mark.parametrize('name', sorted(D.refusal_cases()))
def test_hook_refuses_without_touching_a_device(name):
    from gparml_amd import _lib
    product, form, dims, ops, word = D.refusal_cases()[name]
    rc, ran, out = D.run_hook(product, form, dims, rows=0, cols=4, **ops)
    assert rc == _lib.GP_ERR_BAD_ARG, (rc, _lib.load().gp_last_error(None).decode())
    msg = _lib.load().gp_last_error(None).decode()
    assert 'gp_debug_dd_product' in msg and word in msg, msg
    assert not out.any()
