"""The reference of the greedy conditional-variance selection (tests/select_ref.py) checked on the CPU: the condition that keeps the device's pivot
comparison honest, the reference's own identities, the monotone trace, and the reference against a dense pivoted Cholesky of K_nn."""
import numpy as np
import pytest

import select_ref as R

LD = np.longdouble


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_every_step_has_a_clear_pivot_and_the_mirror_is_far_inside_the_gap(name):
    """At every step run after step 0: gap >= 1e-6, or the two best rows are identical (the lowest index then wins by the rule); and -- what the
    figure 1e-6 stands for -- the float64 mirror's d is within gap / 100 of the long-double d over the unselected rows."""
    X, sf2, alpha, K = R.make_case(name)
    ref, mir, err = R.reference(name)
    kp = len(ref['pivots'])
    assert np.array_equal(mir['pivots'], ref['pivots'])
    for j in range(1, kp):
        free = np.ones(X.shape[0], dtype=bool)
        free[ref['pivots'][:j]] = False
        dd = float(np.max(np.abs(mir['d_steps'][j].astype(LD) - ref['d_steps'][j])[free]) / LD(sf2))
        if ref['same'][j]:
            assert ref['gap'][j] == 0.0, (name, j)
            best = np.nonzero(free & (mir['d_steps'][j] == mir['d_steps'][j][ref['pivots'][j]]))[0]
            assert best.size >= 2 and best[0] == ref['pivots'][j], (name, j, 'identical rows: the lowest index is the pivot')
        else:
            assert ref['gap'][j] >= R.MIN_GAP, (name, j, ref['gap'][j])
            assert dd < ref['gap'][j] / 100, (name, j, dd, ref['gap'][j])
    print('%s: K\' = %d, mirror error %.3e' % (name, kp, err))
    assert np.isfinite(err)


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_reference_identities_and_trace(name):
    X, sf2, alpha, K = R.make_case(name)
    ref = R.reference(name)[0]
    e1, e2 = R.identities(X, sf2, alpha, ref['pivots'], ref['L'], ref['d'])
    assert e1 <= 1e-15 and e2 <= 1e-15, (name, e1, e2)
    tr = ref['trace']
    assert np.all(tr[1:] <= tr[:-1]) and np.all(tr >= 0) and (tr.size == 0 or tr[0] <= X.shape[0] * LD(sf2))
    assert ref['pivots'][0] == 0 and len(set(ref['pivots'].tolist())) == len(ref['pivots'])


def test_duplicates_stop_at_the_number_of_distinct_rows():
    name = 'dup_n40_Q3_K20'
    X, sf2, alpha, K = R.make_case(name)
    ref = R.reference(name)[0]
    assert len(np.unique(X, axis=0)) == R.DUP_DISTINCT < K
    assert len(ref['pivots']) == R.DUP_DISTINCT and len(np.unique(X[ref['pivots']], axis=0)) == R.DUP_DISTINCT


def test_reference_equals_a_dense_pivoted_cholesky():
    """n = 127: K_nn formed whole in long double and factorised by the textbook outer-product form with diagonal pivoting (the Schur complement
    is updated entry by entry): the same pivots, the same columns, and a trace equal to the trace of the Schur complement."""
    name = 'n127_Q70_K33'
    X, sf2, alpha, K = R.make_case(name)
    ref = R.reference(name)[0]
    Xl, al = X.astype(LD), alpha.astype(LD)
    n = X.shape[0]
    S = np.stack([R.kernel_column(Xl, Xl[i], sf2, al, LD) for i in range(n)])
    S = (S + S.T) / 2
    chosen = np.zeros(n, dtype=bool)
    for j in range(K):
        diag = np.where(chosen, -np.inf, np.diag(S))
        p = int(np.argmax(diag))
        assert p == ref['pivots'][j], j
        col = S[:, p] / np.sqrt(S[p, p])
        assert np.max(np.abs(col - ref['L'][:, j])) <= 1e-15 * np.sqrt(sf2), j
        S = S - np.outer(col, col)
        chosen[p] = True
        assert abs(np.maximum(np.diag(S)[~chosen], 0).sum() - ref['trace'][j]) <= 1e-15 * n * sf2, j
