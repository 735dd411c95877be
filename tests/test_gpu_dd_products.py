"""The global step's two extended-precision products in each of their four device forms -- ddacc_gemm_kernel, ddacc_residual_kernel,
solve_residual_kernel and the int8 digit product (csrc/gsi8.hip) -- through gp_debug_dd_product, against tests/dd_ref.py (run with -m gpu).  Every
element of every result is held to the exact value: within the form's derived bound on cancellation and scale-edge inputs, bit for bit on the
digit-order probes and on integer inputs.  The hook's device buffers start as NaN bytes; the two sentinel rows behind the result must come back so."""
import numpy as np
import pytest

import dd_ref as D

pytestmark = pytest.mark.gpu

GP_OK = 0
CASES = D.all_cases()


def _run(case, form=None):
    rc, ran, out, sentinel = D.run_case(case, form)
    if rc != GP_OK:
        from gparml_amd import _lib
        _lib.raise_for(rc, _lib.load(), None, 'gp_debug_dd_product')
    assert (sentinel.view(np.uint64) == D.SENTINEL_BITS).all(), '%s: the rows behind the result were written' % case['name']
    return ran, out


@pytest.mark.parametrize('name', sorted(CASES))
def test_case(name):
    """the table: dd-gemm at 128 and 256, dd-residual at 256 x 512 and forced at 256 x 128, row-residual at M in {1, 3, 5, 127, 128, 130} x Dp in {128, 384} x
    jitA in {0, 1e-7}, int8 at four shapes in both forms, its scale edges, its int32 accumulators at K = 2048, and the production shape of each
    double-double form on integers"""
    case = CASES[name]
    ran, out = _run(case)
    assert ran == case['form']
    worst = D.check(case, out)
    print('%s (%s): worst error at %.4f of the bound' % (name, D.FORM_NAMES[ran], worst))


@pytest.mark.parametrize('da', range(1, 11))
def test_digit_order_probes(da):
    """one digit position per operand, every (da, db): order da + db <= 11 is kept and the product is exact, bit for bit; beyond, within the int8 bound"""
    for db in range(1, 11):
        case = D.probe_case(da, db)
        ran, out = _run(case)
        assert ran == D.I8
        D.check(case, out)


# (Mp, Dp) -> the forms the step chooses for G and for the residual; None: the step does not run these products there (the fused one-panel tail)
STEP_FORMS = {(128, 128): None, (128, 256): (D.DD_GEMM, D.ROW_RESIDUAL), (256, 128): (D.DD_GEMM, D.ROW_RESIDUAL), (256, 512): (D.DD_GEMM, D.DD_RESIDUAL),
              (1024, 128): (D.I8, D.I8)}


def _step_case(product, Mp, Dp):
    """integer-exact operands for form 0 at (Mp, Dp): A symmetric, and Keep + 1.0 * Psi2 = A for the row form (M = Mp: no padding rows)"""
    name = 'step-%s-%dx%d' % ('residual' if product else 'G', Mp, Dp)
    case = D.integer_case(name, 0, product, Mp, Dp if product else Mp, Mp, symmetric=True)
    rs = np.random.RandomState(D._seed(name) ^ 1)
    psi = rs.randint(-8, 9, size=(Mp, Mp)).astype(np.float64)
    psi = np.triu(psi) + np.triu(psi, 1).T
    case.update(M=Mp, Mp=Mp, Dp=Dp, Psi2=psi, Keep=case['A'] - psi, beta=1.0, jitA=0.0)
    return case


@pytest.mark.parametrize('shape', sorted(STEP_FORMS))
def test_the_steps_choice(shape):
    from gparml_amd import _lib
    Mp, Dp = shape
    for product in (0, 1):
        case = _step_case(product, Mp, Dp)
        if STEP_FORMS[shape] is None:
            rc, ran, out, _ = D.run_case(case, 0)
            assert rc == _lib.GP_ERR_BAD_ARG and 'tail' in _lib.load().gp_last_error(None).decode()
            continue
        ran, out = _run(case, 0)
        assert ran == STEP_FORMS[shape][product], '%s: the step chose %s' % (case['name'], D.FORM_NAMES.get(ran, ran))
        D.check(case, out)


@pytest.fixture
def gs_i8_off():
    from gparml_amd import _lib
    lib = _lib.load()
    assert lib.gp_debug_set_option(b'gs_i8', 0) == 0
    yield
    assert lib.gp_debug_set_option(b'gs_i8', 1) == 0


def _both_ways(case, expect_off, request):
    ran, out = _run(case, 0)
    assert ran == D.I8
    D.check(case, out)
    request.getfixturevalue('gs_i8_off')
    ran0, out0 = _run(case, 0)
    assert ran0 == expect_off, 'with gs_i8 off the step chose %s' % D.FORM_NAMES.get(ran0, ran0)
    D.check(case, out0)
    assert np.array_equal(out.view(np.uint64), out0.view(np.uint64))


def test_production_G_int8_and_dd_gemm_same_bits(request):
    """G at Mp = 1024 (1024 x 1024 x 1024, integer-exact): the step takes the int8 product; with gs_i8 off, dd-gemm; both exact, so the same bits"""
    _both_ways(_step_case(0, 1024, 128), D.DD_GEMM, request)


@pytest.mark.parametrize('Dp,off', [(128, D.ROW_RESIDUAL), (512, D.DD_RESIDUAL)])
def test_production_residual_int8_and_double_double_same_bits(Dp, off, request):
    """the residual at Mp = 1024: int8; with gs_i8 off the step's rule (Dp >= 512) gives the row form at Dp = 128 and dd-residual at Dp = 512"""
    _both_ways(_step_case(1, 1024, Dp), off, request)


@pytest.mark.parametrize('name', sorted(D.refusal_cases()))
def test_hook_refusals(name):
    from gparml_amd import _lib
    product, form, dims, ops, word = D.refusal_cases()[name]
    rc, ran, out = D.run_hook(product, form, dims, rows=0, cols=4, **ops)
    assert rc == _lib.GP_ERR_BAD_ARG
    msg = _lib.load().gp_last_error(None).decode()
    assert 'gp_debug_dd_product' in msg and word in msg, msg
    assert not out.any()
