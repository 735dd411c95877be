"""tests/cg_ref.py, the host image of the resident SCG / GD vectors, against the reference's own files (no GPU).

The recorded runs of parallel_GPLVM.main (tests/golden/pipe_gplvm_2shards.npz, pipe_config1_1shard.npz: SCG; gdpipe_gplvm_2shards.npz: GD) hold, for
every call of the objective and every shard, the .embedding, .variance, .grad_d and .grad_latest files before (in_) and after (out_) the call.  Between
two consecutive calls the optimiser ran its helpers on those files, so the pair (call k out_, call k + 1 in_) is a recorded input and output of
set_grads, update_X and update_d.  The image must reproduce them to rounding: 2 ulp per element, the reference doing the same two roundings in
NumPy.  Step and gamma are not taken from anywhere but the arrays: each is recovered as the float64 scalar that reproduces the recorded output (the
ratio at the largest elements, then the neighbouring floats), and the recovered step must be the step_size the next evaluation was called with."""
import os

import numpy as np
import pytest

import cg_ref as R
from pipeline_util import GOLDEN_DIR

ULP = 2.0


def recover(target, d, other, sign, hint=None):
    """The float64 a with target = a d + sign other to 2 ulp per element: (a, worst ulps).  Candidates: the median of the elementwise ratios at the
    64 largest |d|, its 64 neighbours on either side, and ``hint``."""
    target, d, other = np.ravel(target), np.ravel(d), np.ravel(other)
    top = np.argsort(-np.abs(d))[:64]
    a0 = float(np.median((target[top] - sign * other[top]) / d[top]))
    cands = ([float(hint)] if hint is not None else []) + [a0]      # several floats may reproduce the arrays equally well: the hint wins a tie
    lo = hi = a0
    for _ in range(64):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        cands += [float(lo), float(hi)]
    best = min(cands, key=lambda a: float(np.max(R.ulps(R.two_roundings(a, d, other, sign), target))))
    return best, float(np.max(R.ulps(R.two_roundings(best, d, other, sign), target)))


def load(name):
    z = np.load(os.path.join(GOLDEN_DIR, name))
    return {k: z[k] for k in z.files}


def files(g, k, side, s):
    get = lambda n: g.get('call%d_%s_shard%d_%s' % (k, side, s, n))      # noqa: E731
    return get('embedding'), get('variance'), get('grad_d'), get('grad_latest')


def assert_ulp(got, want, what):
    worst = float(np.max(R.ulps(got, want)))
    assert worst <= ULP, (what, worst)
    return worst


@pytest.mark.parametrize('name,gd', [('pipe_gplvm_2shards.npz', False), ('pipe_config1_1shard.npz', False), ('gdpipe_gplvm_2shards.npz', True)])
def test_image_reproduces_the_reference_files_between_consecutive_calls(name, gd):
    g = load(name)
    n_calls, n_shards = int(g['n_calls']), int(g['n_shards'])
    seen = dict(set_grads=0, update=0, unchanged=0)
    for s in range(n_shards):
        # call 0 -> 1: set_grads on the first evaluation's grad_latest
        mu, S, _, latest = files(g, 0, 'out', s)
        im = R.Image(mu, S, latest=latest)
        (im.gd_set_grads if gd else im.set_grads)()
        for k in range(1, n_calls):
            mu_in, S_in, d_in, latest_in = files(g, k, 'in', s)
            mu_prev, S_prev, d_prev, latest_prev = files(g, k - 1, 'out', s)
            step_prev = float(g['call%d_step' % (k - 1)])
            assert np.array_equal(latest_in, latest_prev)                   # nothing between two calls writes grad_latest
            if k == 1:
                assert np.array_equal(d_in.ravel(), im.d) and np.array_equal(im.new, latest_prev.ravel())
                seen['set_grads'] += 1
            elif np.array_equal(mu_in, mu_prev):
                # a probe or a rejected step: nothing moved
                assert np.array_equal(S_in, S_prev) and np.array_equal(d_in, d_prev)
                seen['unchanged'] += 1
            else:
                # an accepted step: update_X(step), grad_new = grad_latest, update_d(gamma), in the order each optimiser runs them
                im = R.Image(mu_prev, S_prev, d=d_prev, new=im.new, old=im.old, latest=latest_prev)
                step, w = recover(np.stack([mu_in, S_in]), d_prev, np.stack([mu_prev, S_prev]), 1.0, hint=step_prev)
                assert w <= ULP and step == step_prev, (k, s, step, step_prev, w)        # the step of the evaluation that was accepted
                if gd:
                    im.gd_update_grad_now()
                    im.gd_update_X(step)
                    gamma, w = recover(-d_in, d_prev, im.new, 1.0, hint=0.0)             # d = -(grad_now + gamma d)
                    assert w <= ULP, (k, s, gamma, w)
                    im.gd_update_d(gamma)
                else:
                    im.update_X(step)
                    im.update_grad_old()
                    im.update_grad_new()
                    gamma, w = recover(d_in, d_prev, im.new, -1.0)                       # d = gamma d - grad_new
                    assert w <= ULP and np.isfinite(gamma), (k, s, gamma, w)
                    im.update_d(gamma)
                wx = assert_ulp(im.X_mu, mu_in, (name, k, s, 'embedding'))
                ws = assert_ulp(im.X_S, S_in, (name, k, s, 'variance'))
                wd = assert_ulp(im.d, d_in.ravel(), (name, k, s, 'grad_d'))
                print('%s call %d shard %d: step %.17g gamma %.17g; worst ulps X_mu %.2g X_S %.2g d %.2g' % (name, k, s, step, gamma, wx, ws, wd))
                seen['update'] += 1
            # within the call only grad_latest is written
            mu_out, S_out, d_out, latest_out = files(g, k, 'out', s)
            assert np.array_equal(mu_out, mu_in) and np.array_equal(S_out, S_in) and np.array_equal(d_out, d_in)
            im.latest = latest_out.ravel().copy()
    assert seen['set_grads'] == n_shards and seen['update'] >= 2 * n_shards and seen['unchanged'] >= n_shards, seen


def test_apply_numbers_the_assignments_as_gp_cg_update_does():
    rng = np.random.RandomState(0)
    v = lambda: rng.standard_normal(14)      # noqa: E731
    base = R.Image(rng.standard_normal((7, 1)), rng.standard_normal((7, 1)), v(), v(), v(), v())
    want = {0: dict(d=-base.new), 1: dict(d=0.3 * base.d - base.new), 2: dict(X=base.X + 0.3 * base.d), 3: dict(old=base.new), 4: dict(new=base.latest),
            5: dict(new=base.latest, old=base.latest, d=-base.latest)}
    for which, changed in want.items():
        im = base.copy()
        im.apply(which, 0.3)
        for key, arr in im.arrays().items():
            assert np.array_equal(arr, changed.get(key, base.arrays()[key])), (which, key)
    # the GD forms: d = -(g + gamma d) is update_d(-gamma) bit for bit (rounding to nearest is symmetric), which is how ResidentGD calls the library
    a, b = base.copy(), base.copy()
    a.gd_update_d(0.3); b.update_d(-0.3)
    assert np.array_equal(a.d, b.d)


def test_candidates_and_reductions_of_the_image():
    rng = np.random.RandomState(1)
    d, g = rng.standard_normal(300), rng.standard_normal(300)
    f, t = R.fused(-0.7371, d, g, -1.0), R.two_roundings(-0.7371, d, g, -1.0)
    assert np.all(np.abs(f - t) <= 2 * R.U * (np.abs(0.7371 * d) + np.abs(g))) and np.any(f != t)      # both within the bound, and not the same thing
    assert np.array_equal(R.fused(0.25, d, g), R.two_roundings(0.25, d, g))  # a power of two: the product is exact
    # chain: one block of one element; a full second block; the cap
    assert (R.chain(2), R.chain(258), R.chain(262144), R.chain(262152)) == (1 + 8 + 0, 1 + 8 + 1, 1 + 8 + 1023, 2 + 8 + 1023)
    idx = R.sample_indices(2097184, 1048592)
    assert len(idx) >= 4096 and {0, 2097183, 1048591, 1048592, 255, 256, 2097151, 2097152} <= set(idx.tolist())
    im = R.Image(d[:150], g[:150], d, g, g + 0.5, g * 1.5)
    vals, mags = im.dots()
    np.testing.assert_allclose(vals.astype(np.float64), [g.dot(d), d.dot(d), d.dot(0.5 * g), g.dot(g), g.dot(g + 0.5)], rtol=1e-13)
    assert np.all(mags >= np.abs(vals.astype(np.float64)) * (1 - 1e-15)) and im.max_d() == np.max(np.abs(d))
    assert float(np.max(np.abs(R.softplus_ld([-20.0, 0.0, 30.0]).astype(np.float64) - np.array([2.061153620314381e-09, np.log(2.0), 30.000000000000092]))
                        / np.array([2e-9, 1.0, 30.0]))) < 1e-15
