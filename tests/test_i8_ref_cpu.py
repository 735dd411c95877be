"""tests/i8_ref.py checked without a device: the exact value is the right quantity (the truncation model of p1i8.hip's header against a long-double
K^T [K | Y]), the emulated conversion meets the bound the GPU test applies, every fault of the table is either rejected by that bound or by the exact
probe, the restated plan gives the slice counts written here as literals, and the integer sums do not depend on the slicing.

The fault table (test_each_fault_is_caught; factors = worst error / bound at N = 4096, M = 150, D = 130, printed by the test):
  caught by the bound, all eight:  order7 (the order-7 products dropped) 6e6, order8 (order 8 included) 1e5, floor 3e7, kstep (32 rows missing from
                        one tile) 2e13, slice2 (one slice twice) 3e13, diag (the diagonal from the digits) 3e3, cshift (a column block of C one tile off)
                        9e18, yscale2 (yscale doubled) 6e3.  The last one was expected to hide below a worst-case bound; it does not, because the bound is
                        17 u of the value while a doubled scale moves every digit by one bit and with it WHICH products are dropped: the exact value of
                        the kept products changes by the size of the truncation, 2^-44 of the scales, not by a rounding.
  The exact probe (i8_ref.probe_inputs) sees five of them bit for bit, yscale2 among them (41-bit odd integers in Y lose their last bit:
                        test_the_exact_probe_catches_a_doubled_yscale), and not order8, diag and floor, which change nothing when Psi1 has one digit and
                        every operand is exactly six digits long (floor digits stand for the same number)."""
import numpy as np
import pytest

import compat_ref as R
import i8_ref as I8

pytestmark = pytest.mark.skipif(not R.available(), reason='numpy long double has no 64-bit significand here')

N, M, D, Q = 4096, 150, 130, 3
_CACHE = {}


def _inputs():
    if 'in' not in _CACHE:
        from oracle import literal as L
        rs = np.random.RandomState(21)
        X = rs.randn(N, Q)
        Z = X[rs.permutation(N)[:M]] + 0.05 * rs.randn(M, Q)
        sf2, alpha = 1.7, np.full(Q, 0.8)
        Psi1 = L.psi1(Z, sf2, alpha, X, np.zeros((N, Q)))
        Y = (np.sin(X @ rs.randn(Q, D)) + 0.1 * rs.randn(N, D)) * np.linspace(0.01, 30.0, D)[None, :]
        Y[:, 3] = 0.0                                               # a zero column: yscale 1, digits zero
        Y[:, 4] = np.clip(Y[:, 4], -0.9, 0.9); Y[17, 4] = 1.0      # maximum exactly a power of two
        Y[:, 5] = -np.abs(Y[:, 5]); Y[19, 5] = -4.0                 # ... and negative
        Psi1.setflags(write=False); Y.setflags(write=False)
        _CACHE['in'] = (Psi1, Y, sf2)
    return _CACHE['in']


def _ref(fault=None):
    if fault not in _CACHE:
        _CACHE[fault] = I8.reference(*_inputs(), fault=fault)
    return _CACHE[fault]


def test_yscale_rule():
    """p1i8.hip:244-246: the unique power of two with 2 max < scale <= 4 max; 1 for a zero column; the sign of the extreme does not matter"""
    Y = np.array([[0.0, 1.0, -4.0, 3.0, -7.3, 2.0 ** 41 - 1, 2.0 ** 40, 0.75e-300, 1e300],
                  [0.0, 0.5, 1.0, -2.9, 7.2, 5.0, -3.0, -1e-300, -0.9e300]])
    s = I8.yscale(Y)
    assert list(s[:7]) == [1.0, 4.0, 16.0, 8.0, 16.0, 2.0 ** 42, 2.0 ** 42]
    m = np.max(np.abs(Y), axis=0)[1:]
    assert np.all(2 * m < s[1:]) and np.all(s[1:] <= 4 * m) and np.all(np.frexp(s[1:])[0] == 0.5)
    assert np.all(np.abs(Y / s) <= 0.5)


def test_digits_reach_plus_and_minus_64_and_represent_the_value():
    t = np.array([0.5, -0.5, 0.5 - 2.0 ** -43, 63.5 / 128, -63.5 / 128, 0.0, 2.0 ** -43, 2.0 ** -44, 1.0 / 3.0])
    d = I8.digits(t)
    assert d[0][0] == 64 and d[0][1] == -64 and all(x[0] == 0 and x[1] == 0 for x in d[1:])
    assert d[0][3] == 64 and d[1][3] == -64           # 63.5 rounds to even, the remainder -1/2 gives -64 in the next digit
    assert all(x[6] == 0 and x[7] == 0 for x in d)    # 2^-43 128^6 = 1/2 rounds to even: zero
    back = sum(np.asarray(x, dtype=I8.LD) * I8.LD(128.0) ** -(j + 1) for j, x in enumerate(d))
    assert np.all(np.abs(back - t) <= 2.0 ** -43)
    with pytest.raises(AssertionError):
        I8.digits(np.array([0.51]))


def test_exact_value_is_the_truncated_product():
    """the reference's exact value against long-double K^T [K | Y], inside the truncation model (i8_ref.truncation_bound) and not trivially so"""
    Psi1, Y, sf2 = _inputs()
    ref = _ref()
    K, E = np.asarray(Psi1, dtype=I8.LD), np.asarray(np.concatenate([Psi1, Y], axis=1), dtype=I8.LD)
    full = K.T @ E
    tol = I8.truncation_bound(Psi1, Y, sf2, ref['yscale'])
    got = np.concatenate([ref['Psi2'], ref['C']], axis=1)
    off = np.concatenate([~np.eye(M, dtype=bool), np.ones((M, D), dtype=bool)], axis=1)
    r = np.where(off, np.asarray(np.abs(got - full) / tol, dtype=np.float64), 0.0)
    print('exact int8 value against the long-double product: worst %.3f of the truncation model' % r.max())
    assert r.max() <= 1.0
    assert r.max() > 1e-3                                            # the model is not vacuous: the truncation is there and of that size
    dg = np.asarray(np.diag(ref['Psi2']) - np.diag(full), dtype=np.float64)
    assert np.all(np.abs(dg) <= (N + 18) * 2.0 ** -64 * np.diag(full).astype(np.float64))
    assert not ref['C'][:, 3].any() and ref['yscale'][3] == 1.0 and ref['yscale'][4] == 4.0 and ref['yscale'][5] == 16.0


def test_emulated_conversion_meets_the_bound():
    ref = _ref()
    bad = I8.hold('emulation', ref['emu2'], ref['emuC'], ref)
    assert not bad, bad
    assert np.array_equal(ref['emu2'], ref['emu2'].T)


CAUGHT_BY_THE_BOUND = I8.FAULTS


def _worst(fault):
    clean, f = _ref(), _ref(fault)
    return max(float(I8.ratios(f['emu2'], clean['Psi2'], clean['tol2']).max()), float(I8.ratios(f['emuC'], clean['C'], clean['tolC']).max()))


@pytest.mark.parametrize('fault', I8.FAULTS)
def test_each_fault_is_caught(fault):
    worst = _worst(fault)
    print('fault %-8s worst error / bound %.3g' % (fault, worst))
    assert fault in CAUGHT_BY_THE_BOUND and worst > 10.0, 'the bound does not reject %s with a margin' % fault


def _probe(n=4096, m=150):
    from oracle import literal as L
    d = I8.probe_inputs(n, m)
    Psi1 = L.psi1(d['Z'], d['sf2'], d['alpha'], d['X_mu'], d['X_S'])
    return d, Psi1


def test_the_exact_probe_is_exact_in_the_emulation():
    """the reference and the emulated device conversion of the probe are the integer sums, bit for bit, at the size the GPU test uses"""
    d, Psi1 = _probe(65536, 512)
    on = Psi1[np.arange(d['N']), d['cls']]
    mask = np.ones_like(Psi1, dtype=bool); mask[np.arange(d['N']), d['cls']] = False
    assert np.all(on == d['sf2']) and Psi1[mask].max() * 0.5 / d['sf2'] < 2.0 ** -43
    ref = I8.reference(Psi1, d['Y'], d['sf2'])
    P2, C = I8.probe_expected(d)
    for name, a, b in (('Psi2', ref['emu2'], P2), ('C', ref['emuC'], C), ('exact Psi2', np.asarray(ref['Psi2'], dtype=np.float64), P2),
                       ('exact C', np.asarray(ref['C'], dtype=np.float64), C)):
        assert np.array_equal(a, b), name
    assert np.array_equal(np.asarray(ref['C'], dtype=np.float64).astype(I8.LD), ref['C'])           # nothing below float64 in the exact value
    assert list(ref['yscale']) == [2.0 ** 42, 2.0 ** 42, 2.0 ** 42, 1.0, 2.0 ** -258, 2.0 ** 342, 8.0, 2.0 ** 21]
    assert np.array_equal(np.diag(ref['I'][0][:, :512]), 4096.0 * np.bincount(d['cls'], minlength=512))   # the digit +64 is what is summed


@pytest.mark.parametrize('fault', I8.FAULTS)
def test_the_exact_probe_against_each_fault(fault):
    """which faults the probe sees bit for bit (small size, same construction): all but 'order8' (nothing of order 8 exists: one digit per Psi1 entry
    times at most six), 'diag' (the digit diagonal of a one-digit Psi1 is exact) and 'floor' (operands of exactly 42 bits: floor digits stand for the same
    number) -- all three rejected by the bound above"""
    d, Psi1 = _probe()
    ref = I8.reference(Psi1, d['Y'], d['sf2'], fault=fault)
    P2, C = I8.probe_expected(d)
    seen = not (np.array_equal(ref['emu2'], P2) and np.array_equal(ref['emuC'], C))
    print('fault %-8s seen by the exact probe: %s' % (fault, seen))
    assert seen == (fault not in ('order8', 'diag', 'floor'))


def test_the_exact_probe_catches_a_doubled_yscale():
    d, Psi1 = _probe()
    ref = I8.reference(Psi1, d['Y'], d['sf2'], fault='yscale2')
    C = I8.probe_expected(d)[1]
    wrong = (ref['emuC'] != C).any(axis=0)
    assert wrong[0] and wrong[2] and wrong[4] and wrong[5] and not wrong[3]      # the 41-bit columns lose their last bit


# the shapes of tests/test_gpu_p1_i8_exact.py: (N, D, M) -> (tiles, slices, shared slices, roundings Psi2 / C / diagonal)
PLANS = {(65536, 100, 512): (14, 72, 0, 18, 17, 194), (66003, 130, 600): (25, 40, 0, 14, 13, 195), (65536, 8, 512): (14, 72, 0, 18, 17, 194),
         (65536, 3, 385): (14, 72, 0, 18, 17, 194), (1000000, 100, 512): (14, 72, 0, 18, 17, 759)}


@pytest.mark.parametrize('shape', sorted(PLANS))
def test_restated_plan_at_the_gpu_shapes(shape):
    n, dd, m = shape
    pl = I8.plan(n, dd, m)
    assert (pl['T'], pl['S'], pl['n_shared']) + I8.roundings(pl['S']) + (I8.diag_roundings(n),) == PLANS[shape]
    b = pl['bounds']
    assert b[0][0] == 0 and b[-1][1] == pl['ksteps'] == I8.pad(n) // 32 and all(x[1] == y[0] for x, y in zip(b, b[1:]))
    assert all(0 < 32 * (k1 - k0) <= I8.I8_MAX_ROWS for k0, k1 in b)
    if shape[0] != 1000000:
        assert len({k1 - k0 for k0, k1 in b}) > 1                  # ragged: the k-steps do not divide by the slices, both roundings of k0, k1 occur


def test_shared_slices_are_placed_at_no_shape():
    """p1i8_prepare's "shared slices" branch (p1i8.hip:336-340) needs T <= 32 tiles, the cost search to end at s8 = 32 / T, and 8 (32 mod T) >= T CUs left
    over.  T = mt (mt + 1) / 2 + mt dt with mt >= 4: the search runs over nine consecutive values, and for T = 14 (the one T that leaves enough CUs) the
    value 9 or a later one always wins over 2.  So no shape the path applies to has shared slices, and the chain length is ceil(8 s8 / 8) = s8."""
    for mt in range(4, 17):
        for dt in range(1, 9):
            for n in (65536, 66003, 131072, 655360, 655361, 1000000, 1310721, 4000000, 8000000):
                try:
                    pl = I8.plan(n, 128 * dt, 128 * mt)
                except AssertionError:
                    continue
                assert pl['n_shared'] == 0, (n, dt, mt, pl['S'])


def test_integer_sums_do_not_depend_on_the_slicing():
    Psi1, Y, sf2 = _inputs()
    ref = _ref()
    K = I8.pad(N) // 32
    for cuts in ([0, K], [0, 1, 2, K], [0, 7, 50, 51, 100, K]):
        other = I8.reference(Psi1, Y, sf2, bounds=list(zip(cuts[:-1], cuts[1:])))
        assert np.array_equal(other['I'], ref['I'])
        assert np.array_equal(other['Psi2'], ref['Psi2']) and np.array_equal(other['C'], ref['C'])
