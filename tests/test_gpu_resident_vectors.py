"""The resident SCG / GD vector kernels (csrc/api.hip: cg_update_kernel, cg_dots_kernel + cg_reduce, cg_abs_kernel, gp_cg_max_d, grad_latest_kernel) and the
trial point of prep_elem_kernel (csrc/psi.hip), each against a host reference of its own (tests/cg_ref.py).

Engines as in test_gpu_lbfgs.Mirror: D = 2, M = 4, raw variances, real tiny evaluations.  Every input is known exactly on the host through
gp_debug_peek ('cg_g_new', 'cg_g_old', 'cg_g_latest', 'dir', 'Xmu', 'Xs') and gp_set_direction, so
  * the pure assignments are held to BIT equality, and every array an assignment does not name must not move;
  * the two multiply-add forms (d = a d - g_new, X += a d) must give, element by element, the correctly rounded value (fractions.Fraction, on the
    sample of cg_ref.sample_indices) or NumPy's two-rounding value, and |err| <= 2u (|a d| + |other|) over the whole array;
  * the resident grad_latest equals the downloaded one bit for bit and both are within 8u |ref| of -[grad_X_mu, grad_X_S sigma(raw + step d_S)];
  * the trial point: the means by the two-candidate rule, the variances within u (4 + 4 |S|) of the longdouble log1p(exp(raw + step d_S));
  * the reductions are within gamma_(L+2) sum |term| of the longdouble sum, L = cg_ref.chain(2 N Q), the maxima bit-equal.
The inducing points of these engines are placed symmetrically (z, -z, z', -z'), so the origin the library centres the means at (gp_ctx::shift) is
exactly zero and X_MU_TRIAL is the kernel's own multiply-add; one case with another origin holds the centred array to fl(candidate - origin).
Measured on an MI355X: see DESIGN.md section 9.3.1."""
import numpy as np
import pytest

import cg_ref as R
from fixed_ref import origin

pytestmark = pytest.mark.gpu

U, LD = R.U, np.longdouble
# (N_s, Q): the smallest vectors | odd N Q: the mu / S split of update_X on an odd index | 2 N Q = 258: a ragged block behind a full one |
# 262152 > 1024 x 256: the reductions' block cap, 8 threads take a second trip | 2097184 > 8192 x 256: blocks_for's cap in cg_update_kernel |
# N Q = 2097168 > 8192 x 256: grad_latest_kernel's cap (prep_elem_kernel caps its grid at 16384 blocks: TRIAL_EXTRA crosses that one)
SHAPES = [(1, 1), (7, 3), (43, 3), (10923, 12), (65537, 16), (131073, 16)]
VECTOR_SHAPES = SHAPES[:5]
TRIAL_EXTRA = (262145, 16)              # Np Q > 16384 x 256
A_VALUES = (-0.7371, 2.0 ** -30, 0.25, 0.37, 0.0)
ids = lambda s: 'N%d_Q%d' % s          # noqa: E731


class Shard(object):
    """One engine (D = 2, M = 4, raw variances) and what the host knows of it."""

    def __init__(self, N_s, Q, seed=0, raw=None, centred=True):
        from gparml_amd.engine import ShardEngine
        rng = np.random.RandomState(seed)
        self.N_s, self.Q, self.nq, self.n2, self.rng = N_s, Q, N_s * Q, 2 * N_s * Q, rng
        self.eng = ShardEngine(N_s, 2, 4, Q, device=0)
        X = rng.standard_normal((N_s, Q))
        Y = np.stack([np.sin(X.sum(1)), np.cos(X[:, 0])], 1) + 0.1 * rng.standard_normal((N_s, 2))
        self.eng.upload_shard(Y, X, 0.3 * rng.standard_normal((N_s, Q)) if raw is None else raw, xs_is_raw=True)
        z = rng.standard_normal((2, Q))
        Z = np.stack([z[0], -z[0], z[1], -z[1]]) if centred else rng.standard_normal((4, Q)) + 0.75
        self.origin = origin(Z)
        assert not centred or not np.any(self.origin)
        self.globals = (Z, 1.3, 0.5 + rng.uniform(size=Q), 2.0)

    def evaluate(self, step=0.0, phase1_only=False):
        e = self.eng
        e.set_globals(*self.globals, N_global=self.N_s, step_size=step)
        e.phase1()
        if not phase1_only:
            e.global_step(); e.phase2(True); e.finish()

    def set_direction(self, scale=0.05):
        self.dir = scale * self.rng.standard_normal(self.n2)
        self.eng.set_direction(self.dir.reshape(2, self.N_s, self.Q))

    def state(self):
        p = self.eng.cg_peek
        return dict(d=p('dir').ravel(), new=p('cg_g_new').ravel(), old=p('cg_g_old').ravel(), latest=p('cg_g_latest').ravel(),
                    X=np.concatenate([p('Xmu').ravel(), p('Xs').ravel()]))

    def image(self, st=None):
        st = st or self.state()
        return R.Image(st['X'][:self.nq].reshape(self.N_s, self.Q), st['X'][self.nq:].reshape(self.N_s, self.Q), st['d'], st['new'], st['old'], st['latest'])

    def close(self):
        self.eng.close()


@pytest.fixture(scope='module')
def shards():
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = Shard(*shape)
        return made[shape]
    yield get
    for h in made.values():
        h.close()


def check_muladd(got, a, d, other, sign, idx):
    """``got`` = a d + sign other: each sampled element is the fused or the two-rounding value; the whole array is within 2u (|a d| + |other|).
    Returns (elements equal to the fused value alone, to the two-rounding value alone, sampled elements at which the two differ)."""
    two = R.two_roundings(a, d, other, sign)
    one = R.fused(a, d[idx], other[idx], sign)
    g = got[idx]
    ok = (g == one) | (g == two[idx])
    assert np.all(ok), (a, idx[~ok][:5], g[~ok][:5], one[~ok][:5], two[idx][~ok][:5])
    exact = LD(a) * d.astype(LD) + LD(sign) * other.astype(LD)
    err = np.abs(got.astype(LD) - exact)
    bound = 2 * U * (np.abs(a * d) + np.abs(other))
    assert np.all(err <= bound), (a, float(np.max(err - bound)))
    differ = one != two[idx]
    return int(np.sum(differ & (g == one))), int(np.sum(differ & (g == two[idx]))), int(np.sum(differ))


# ---- a. the assignments ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', VECTOR_SHAPES, ids=ids)
def test_assignments_bit_for_bit_and_multiply_adds_by_the_two_candidate_rule(shape, shards):
    h = shards(shape)
    e = h.eng
    idx = R.sample_indices(h.n2, h.nq)
    tally = {1: np.zeros(3, dtype=np.int64), 2: np.zeros(3, dtype=np.int64)}
    h.evaluate(0.0)
    before = [h.state()]

    def run(which, a=0.0):
        im = h.image(before[0])
        im.apply(which, a)
        e.cg_update(which, a)
        after = h.state()
        for key, want in im.arrays().items():
            if (which, key) == (1, 'd'):
                tally[1] += check_muladd(after['d'], a, before[0]['d'], before[0]['new'], -1.0, idx)
            elif (which, key) == (2, 'X'):
                tally[2] += check_muladd(after['X'], a, before[0]['d'], before[0]['X'], 1.0, idx)
            else:
                assert np.array_equal(after[key], want), (which, a, key)
        before[0] = after

    run(5)                                  # g_new = g_old = g_latest, d = -g_latest
    assert np.array_equal(before[0]['d'], -before[0]['latest']) and np.any(before[0]['latest'])
    h.set_direction()
    h.evaluate(0.37)                        # a new g_latest: from here the four vectors all differ
    before[0] = h.state()
    assert np.array_equal(before[0]['d'], h.dir) and not np.array_equal(before[0]['latest'], before[0]['new'])
    run(3)                                  # g_old = g_new: they are equal already, and g_latest is another vector
    run(4)                                  # g_new = g_latest; g_old keeps the first gradient
    for a in A_VALUES:
        run(1, a)                           # d = a d - g_new
    h.evaluate(0.05 / np.max(np.abs(before[0]['d'])))
    before[0] = h.state()                   # a third g_latest: d, g_new, g_old and g_latest are four different vectors for the two copies below
    assert len({before[0][k].tobytes() for k in ('d', 'new', 'old', 'latest')}) == 4 or h.n2 < 16
    run(3)                                  # g_old = g_new
    run(0)                                  # d = -g_new
    h.set_direction()
    before[0] = h.state()
    for a in A_VALUES:
        run(2, a)                           # X_mu += a d[:NQ], X_S += a d[NQ:]
    for which, name in ((1, 'd = a d - g_new'), (2, 'X += a d')):
        t = tally[which]
        print('%s %s: of %d sampled elements whose candidates differ, %d are the fused value and %d the two-rounding value' % (shape, name, t[2], t[0], t[1]))
        assert t[1] == t[2] and (t[2] > 0 or h.n2 < 64)            # mul_then_add: the product is rounded first, as in the reference


# ---- b. the resident grad_latest ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_resident_grad_latest_is_the_downloaded_one_and_both_are_the_transformed_gradient(shape, shards):
    h = shards(shape)
    e = h.eng
    worst = 0.0
    for step in (0.0, 0.37):
        if step:
            h.set_direction()
        else:
            e.set_direction(None)
        h.evaluate(step)
        res, dl = e.cg_peek('cg_g_latest'), e.download('GRAD_LATEST')
        assert np.array_equal(res, dl), step
        gmu, gS, raw = e.download('GRAD_X_MU'), e.download('GRAD_X_S'), e.cg_peek('Xs')
        x = raw.astype(LD) + (LD(step) * h.dir.reshape(2, h.N_s, h.Q)[1].astype(LD) if step else 0)
        ref = -(gS.astype(LD) * R.sigma_ld(x))
        assert np.array_equal(res[0], -gmu)
        err = np.abs(res[1].astype(LD) - ref)
        ratio = float(np.max(np.where(ref != 0, err / (U * np.abs(ref) + (ref == 0)), err)))
        worst = max(worst, ratio)
        print('%s step %g: grad_latest variance half at %.3g u |ref| (bound 8)' % (shape, step, ratio))
        assert np.all(err <= 8 * U * np.abs(ref)), (step, ratio)
    assert worst > 0 or h.n2 < 16


# ---- c. the trial point (phase 1 only) ---------------------------------------------------------------------------------------------------
def trial_case(N_s, Q, centred=True):
    rng = np.random.RandomState(11)
    raw = rng.normal(-1.0, 1.0, size=(N_s, Q))
    if N_s >= 2:
        raw[N_s // 3], raw[N_s - 1] = -20.0, 30.0
    return Shard(N_s, Q, seed=2, raw=raw, centred=centred)


def check_trial(h, step, with_dir, idx, refs):
    e = h.eng
    h.evaluate(step, phase1_only=True)
    X_mu, raw = e.cg_peek('Xmu').ravel(), e.cg_peek('Xs').ravel()
    d = h.dir if with_dir else np.zeros(h.n2)
    a = step if with_dir else 0.0                       # without a direction the step must be ignored
    mu, S = e.download('X_MU_TRIAL').ravel(), e.download('X_S_TRIAL').ravel()
    tally = check_muladd(mu, a, d[:h.nq], X_mu, 1.0, idx)
    if a not in refs:                                   # three distinct points: raw, raw + 0.37 d_S, raw - 2^-20 d_S
        refs[a] = R.softplus_ld(raw.astype(LD) + LD(a) * d[h.nq:].astype(LD))
    ref = refs[a]
    err = np.abs(S.astype(LD) - ref)
    bound = U * (4 + 4 * np.abs(ref))
    ratio = float(np.max(err / bound))
    assert ratio <= 1.0, (step, with_dir, ratio)
    return tally, ratio


@pytest.mark.parametrize('shape', SHAPES + [TRIAL_EXTRA], ids=ids)
def test_trial_point_is_x_plus_step_d_and_softplus_of_it(shape):
    h = trial_case(*shape)
    idx = R.sample_indices(h.nq, h.nq, grid_cap=16384)
    h.set_direction()
    worst, tally, refs = 0.0, np.zeros(3, dtype=np.int64), {}
    for with_dir in (True, False):
        if not with_dir:
            h.eng.set_direction(None)
        for step in (0.0, 0.37, -2.0 ** -20):
            t, r = check_trial(h, step, with_dir, idx, refs)
            tally += t
            worst = max(worst, r)
    print('%s: X_S_TRIAL at %.3g of u (4 + 4 |S|); means: %d fused, %d two-rounding of %d that differ' % (shape, worst, tally[0], tally[1], tally[2]))
    assert tally[1] == tally[2]                 # mul_then_add: the product is rounded first, as in the reference
    h.close()


def test_trial_means_under_a_nonzero_origin_are_the_candidates_minus_the_origin():
    """With inducing points off centre the resident trial means are stored centred: fl(candidate - origin), and the download adds the origin back."""
    h = trial_case(43, 3, centred=False)
    e, o = h.eng, np.tile(h.origin, 43)
    assert np.all(h.origin != 0)
    h.set_direction()
    h.evaluate(0.37, phase1_only=True)
    X_mu = e.cg_peek('Xmu').ravel()
    got = e.peek('mu', 128 * 3)[:h.nq]                                       # [Np][Q], Np = 128
    one = R.fused(0.37, h.dir[:h.nq], X_mu) - o
    two = R.two_roundings(0.37, h.dir[:h.nq], X_mu) - o
    assert np.all((got == one) | (got == two))
    assert np.array_equal(e.download('X_MU_TRIAL').ravel(), got + o)
    h.close()


# ---- d. the reductions -------------------------------------------------------------------------------------------------------------------------
def check_reductions(h):
    """gp_cg_dots, gp_cg_abs and gp_cg_max_d on the engine's vectors as they are: (out6, abs2, worst error / bound)."""
    e, im = h.eng, h.image()
    out, ab = e.cg_dots(), e.cg_abs()
    vals, mags = im.dots()
    bound = im.bound(mags)
    err = np.abs(out[:5].astype(LD) - vals).astype(np.float64)
    assert np.all(err <= bound), (err, bound)
    sv, sm = im.abs_sum()
    aerr, abound = abs(float(LD(ab[0]) - sv)), float(im.bound(sm))
    assert aerr <= abound, (aerr, abound)
    assert out[5] == im.max_d() and ab[1] == im.max_new()
    for alpha in (-0.37, 2.5, 0.0):
        assert e.cg_max_d(alpha) == abs(alpha) * im.max_d()
    assert np.array_equal(out, e.cg_dots()) and np.array_equal(ab, e.cg_abs())          # repeated calls: the same bits
    ratios = [er / b for er, b in zip(list(err) + [aerr], list(bound) + [abound]) if b > 0]
    return out, ab, max(ratios) if ratios else 0.0


def distinct_vectors(h):
    """set_grads, then an update_d and a new evaluation along it: d, g_new, g_old and g_latest all differ."""
    e = h.eng
    e.set_direction(None)
    h.evaluate(0.0)
    e.cg_update(5)
    h.set_direction()
    h.evaluate(0.37)
    e.cg_update(4)
    e.cg_update(1, 0.3)
    h.evaluate(0.05 / e.cg_dots()[5])


@pytest.mark.parametrize('shape', VECTOR_SHAPES, ids=ids)
def test_reductions_hold_the_chain_bound_and_maxima_are_exact(shape, shards):
    h = shards(shape)
    e = h.eng
    e.set_direction(None)
    h.evaluate(0.0)
    e.cg_update(5)
    out, ab, w1 = check_reductions(h)
    # g_new = g_old = g_latest, d = -g_latest: theta is a sum of exact zeros, mu and kappa are the same sums with opposite signs
    assert out[2] == 0.0 and out[0] == -out[1] and out[1] == out[3] == out[4] and out[1] > 0 and ab[0] > 0
    distinct_vectors(h)
    out, ab, w2 = check_reductions(h)
    assert len(set(out[:5].tolist())) == 5 and out[2] != 0.0
    print('%s: reductions at %.3g (after set_grads) and %.3g (all vectors distinct) of gamma_%d sum|term|' % (shape, w1, w2, R.chain(h.n2) + 2))


def test_a_dropped_element_or_second_trip_lands_outside_the_reductions_bound(shards):
    """The bound is tight enough to see one missing term: shown once on the REFERENCE (the last element, then the 8 elements of the second
    grid-stride trip, left out of it)."""
    h = shards(SHAPES[3])
    assert h.n2 - R.reduce_blocks(h.n2) * 256 == 8
    distinct_vectors(h)
    im, out, ab = h.image(), h.eng.cg_dots(), h.eng.cg_abs()
    got = [LD(v) for v in out[:5]] + [LD(ab[0])]
    for drop in (1, 8):
        keep = slice(0, h.n2 - drop)
        vals, mags = im.dots()
        part, _ = im.dots(keep)
        refs, parts, bounds = list(vals) + [im.abs_sum()[0]], list(part) + [im.abs_sum(keep)[0]], list(im.bound(mags)) + [float(im.bound(im.abs_sum()[1]))]
        for name, g, full, cut, b in zip(R.DOT_NAMES + ('sum_abs',), got, refs, parts, bounds):
            assert abs(float(g - full)) <= b, (name, drop)
            assert abs(float(g - cut)) > b, (name, drop, float(g - cut), b)


# ---- e. the helper sequence on a two-shard model ---------------------------------------------------------------------------------------------
MODEL = dict(cuts=[0, 431, 1000], D=4, M=8, Q=3, seed=3)


def _gplvm(seed, N, D, M, Q):
    rng = np.random.RandomState(seed)
    X = rng.standard_normal((N, Q))
    Y = np.stack([np.sin(X[:, 0]), np.cos(X[:, 1]), X[:, 0] * X[:, 2], np.sin(X.sum(1))], 1)[:, :D] + 0.1 * rng.standard_normal((N, D))
    X_mu = X + 0.3 * rng.standard_normal((N, Q))
    X_S = 0.2 * rng.standard_normal((N, Q)) - 1.0
    x0 = np.concatenate([X_mu[rng.choice(N, M, replace=False)].ravel(), [1.0], np.ones(Q), [2.0]])
    return Y, X_mu, X_S, x0


def _model(p=MODEL):
    from gparml_amd.resident import ResidentModel
    Y, X_mu, X_S, x0 = _gplvm(p['seed'], p['cuts'][-1], p['D'], p['M'], p['Q'])
    cuts = p['cuts']
    return ResidentModel([(Y[a:b], X_mu[a:b], X_S[a:b]) for a, b in zip(cuts[:-1], cuts[1:])], p['M'], p['Q'], p['D']), X_mu, X_S, x0


def _images(model, latest_from_download=False):
    out = []
    for e in model.engines:
        p = e.cg_peek
        latest = e.download('GRAD_LATEST') if latest_from_download else p('cg_g_latest')
        out.append(R.Image(p('Xmu'), p('Xs'), p('dir'), p('cg_g_new'), p('cg_g_old'), latest))
    return out


def check_getters(cg, gd, imgs, what):
    """Every getter of ResidentCG and ResidentGD against the images' sums over the shards; the bound is (d)'s, added over the shards."""
    vals, bound, sabs, babs = np.zeros(5, dtype=LD), np.zeros(5), LD(0), 0.0
    for im in imgs:
        v, m = im.dots()
        vals, bound = vals + v, bound + im.bound(m)
        s, m = im.abs_sum()
        sabs, babs = sabs + s, babs + float(im.bound(m))
    got = [cg.embeddings_get_grads_mu(), cg.embeddings_get_grads_kappa(), cg.embeddings_get_grads_theta(), cg.embeddings_get_grads_current_grad(),
           cg.embeddings_get_grads_gamma()]
    for name, g, v, b in zip(R.DOT_NAMES, got, vals, bound):
        assert abs(float(LD(g) - v)) <= b, (what, name, g, float(v), b)
    maxd, maxn = max(im.max_d() for im in imgs), max(im.max_new() for im in imgs)
    for alpha in (-0.37, 1.5):
        assert cg.embeddings_get_grads_max_d(None, alpha) == abs(alpha) * maxd, (what, alpha)
    assert abs(float(LD(gd.embeddings_get_grads_current_grad()) - sabs)) <= babs, what
    assert gd.embeddings_get_grads_max_gradnow() == maxn, what
    return np.array(got)


def test_helper_sequence_on_two_shards_follows_the_image_call_by_call():
    from gparml_amd.resident import ResidentCG, ResidentGD
    model, _, _, x0 = _model()
    cg, gd = ResidentCG(model), ResidentGD(model)
    seen = []

    def evaluate(step, what):
        model.likelihood_and_gradient(x0, 0, step)
        imgs = _images(model, latest_from_download=True)
        for im, e in zip(imgs, model.engines):
            assert np.array_equal(im.latest, e.cg_peek('cg_g_latest').ravel()), what
        seen.append(check_getters(cg, gd, imgs, what))

    def mutate(ops, name, image_method, *args):
        imgs = _images(model)                                    # re-seeded from the device: nothing compounds
        before = [im.copy() for im in imgs]
        getattr(ops, name)(None, *args)
        for im, b, e in zip(imgs, before, model.engines):
            getattr(im, image_method)(*args)
            now = _images_one(e)
            for key, want in im.arrays().items():
                if np.array_equal(now[key], want):
                    continue
                # a multiply-add that is not the image's two roundings would still have to be within (a)'s bound, and is then taken as it is
                assert image_method in ('update_d', 'update_X', 'gd_update_d', 'gd_update_X') and key in ('d', 'X'), (name, key)
                other = b.X if key == 'X' else b.new
                assert np.all(np.abs(now[key] - want) <= 2 * U * (np.abs(args[0] * b.d) + np.abs(other))), (name, key)
                setattr(im, key, now[key])
        seen.append(check_getters(cg, gd, imgs, name))

    def _images_one(e):
        p = e.cg_peek
        return dict(d=p('dir').ravel(), new=p('cg_g_new').ravel(), old=p('cg_g_old').ravel(), latest=p('cg_g_latest').ravel(),
                    X=np.concatenate([p('Xmu').ravel(), p('Xs').ravel()]))

    def probe_and_step(shrink=1.0):
        mu, kappa = cg.embeddings_get_grads_mu(), cg.embeddings_get_grads_kappa()
        sigma = 1e-4 / np.sqrt(kappa)
        evaluate(sigma, 'probe')
        theta = cg.embeddings_get_grads_theta() / sigma
        delta = theta + kappa if theta + kappa > 0 else kappa
        alpha = shrink * -mu / delta
        evaluate(alpha, 'trial')
        return mu, alpha

    model.likelihood_and_gradient(x0, 0, 0)
    mutate(cg, 'embeddings_set_grads', 'set_grads')
    assert seen[-1][2] == 0.0 and seen[-1][0] == -seen[-1][1]
    # an accepted step
    mu, alpha = probe_and_step()
    assert seen[-2][2] != 0.0                                    # theta moved with the probe's grad_latest: the cache did not keep the zero
    mutate(cg, 'embeddings_set_grads_update_X', 'update_X', alpha)
    mutate(cg, 'embeddings_set_grads_update_grad_old', 'update_grad_old')
    mutate(cg, 'embeddings_set_grads_update_grad_new', 'update_grad_new')
    Gamma = (cg.embeddings_get_grads_gamma() - cg.embeddings_get_grads_current_grad()) / mu
    mutate(cg, 'embeddings_set_grads_update_d', 'update_d', Gamma)
    # a rejected step: two trials from the same point, nothing is updated in between
    mu, alpha = probe_and_step(shrink=40.0)
    evaluate(alpha / 4.0, 'second trial')
    # a restart
    mutate(cg, 'embeddings_set_grads_reset_d', 'reset_d')
    assert seen[-1][0] == -seen[-1][3]                           # d = -g_new: mu = -|g_new|^2, the same sums with opposite signs
    # the GD helpers on the same vectors
    mutate(gd, 'embeddings_set_grads', 'set_grads')              # the library's set_grads also writes g_old, which GD never reads
    evaluate(0.01, 'gd trial')
    mutate(gd, 'embeddings_set_grads_update_grad_now', 'gd_update_grad_now')
    mutate(gd, 'embeddings_set_grads_update_X', 'gd_update_X', 0.01)
    mutate(gd, 'embeddings_set_grads_update_d', 'gd_update_d', 0.1)
    model.close()


# ---- f. the trajectory ---------------------------------------------------------------------------------------------------------------------------
class Recorder(object):
    """Passes every helper call through to ``ops`` and keeps the names of the mutating ones."""

    def __init__(self, ops):
        self._ops, self.log = ops, []

    def __getattr__(self, name):
        fn = getattr(self._ops, name)
        if name.startswith('embeddings_set'):
            def logged(*args):
                self.log.append(name)
                return fn(*args)
            return logged
        return fn


def _run(optimiser, ops_class):
    """Six iterations on the two-shard model.  ``ops_class`` None: the resident vectors; otherwise the vectors live on the host in ``ops_class`` as
    [mu, raw S] per shard and the model only evaluates.  Returns (calls [(x, f, step)], the mutating helper calls, the final [mu, raw S])."""
    from gparml_amd.gd import GD
    from gparml_amd.resident import ResidentCG, ResidentGD
    from gparml_amd.scg_adapted import SCG_adapted
    model, X_mu, X_S, x0 = _model()
    cuts, calls = MODEL['cuts'], []
    if ops_class is None:
        ops = Recorder((ResidentGD if optimiser == 'gd' else ResidentCG)(model))

        def f_and_g(x, iteration, step_size=0):
            f, g = model.likelihood_and_gradient(x, iteration, step_size)
            calls.append((np.array(x), f, float(step_size)))
            return f, g
    else:
        inner = ops_class(np.concatenate([np.stack([X_mu[a:b], X_S[a:b]]).ravel() for a, b in zip(cuts[:-1], cuts[1:])]))
        inner.gd = optimiser == 'gd'
        ops = Recorder(inner)

        def f_and_g(x, iteration, step_size=0):
            Xt = inner.X + (step_size * inner.d if inner.d is not None and step_size != 0 else 0.0)       # local_MapReduce.py:205-211
            at = 0
            for e in model.engines:
                loc = Xt[at:at + 2 * e.N_s * e.Q].reshape(2, e.N_s, e.Q)
                e.set_direction(None)
                e.upload_embeddings(loc[0], loc[1], xs_is_raw=True)
                at += loc.size
            model.version += 1
            f, g = model.likelihood_and_gradient(x, iteration, 0)
            inner.latest = np.concatenate([e.download('GRAD_LATEST').ravel() for e in model.engines])
            calls.append((np.array(x), f, float(step_size)))
            return f, g
    if optimiser == 'gd':
        GD(f_and_g, x0.copy(), ops, fixed_embeddings=False, maxiters=6, ftol=0, gtol=0)
    else:
        SCG_adapted(f_and_g, x0.copy(), ops, fixed_embeddings=False, maxiters=6, xtol=0, ftol=0, gtol=0)
    if ops_class is None:
        final = np.concatenate([np.stack([e.cg_peek('Xmu'), e.cg_peek('Xs')]).ravel() for e in model.engines])
    else:
        final = inner.X.copy()
    model.close()
    return calls, ops.log, final


def _gap(a, b):
    """The largest relative difference of two runs, per call, over x, f and the step, and of the final embeddings."""
    (ca, la, fa), (cb, lb, fb) = a, b
    assert len(ca) == len(cb) and la == lb, (len(ca), len(cb))
    rel = lambda p, q: float(np.max(np.abs(np.asarray(p) - np.asarray(q))) / max(np.max(np.abs(q)), 1e-300))      # noqa: E731
    per_call = [max(rel(xa, xb), rel(f1, f2), rel(s1, s2) if s2 else abs(s1)) for (xa, f1, s1), (xb, f2, s2) in zip(ca, cb)]
    return per_call + [rel(fa, fb)]


@pytest.fixture(scope='module')
def runs():
    made = {}

    def get(optimiser, ops_class):
        if (optimiser, ops_class) not in made:
            made[optimiser, ops_class] = _run(optimiser, ops_class)
        return made[optimiser, ops_class]
    return get


def yardstick(runs):
    """The largest gap between two runs of the HOST reference that differ only in the summation order of its reductions (numpy.dot against
    math.fsum): SCG's; GD's trajectory does not pass through a reduction, so its own is exactly zero and SCG's, over the same model and the same
    number of iterations, serves both."""
    gaps = _gap(runs('scg', R.FsumOps), runs('scg', R.NumpyOps))
    gd = max(_gap(runs('gd', R.FsumOps), runs('gd', R.NumpyOps)))
    print('host reference, numpy.dot against math.fsum: SCG gap %.3g (per call: %s), GD gap %.3g' % (max(gaps), ' '.join('%.1e' % v for v in gaps), gd))
    assert 0 < max(gaps) < 1e-9 and gd == 0.0
    return max(gaps)


def follow(runs, host_class, yard):
    worst = {}
    for opt in ('scg', 'gd'):
        res, ref = runs(opt, None), runs(opt, host_class)
        gaps = _gap(res, ref)                                   # asserts the same number of calls and the same helper sequence
        worst[opt] = max(gaps)
        print('%s: %d evaluations, %d accepted steps; resident against %s per call: %s' %
              (opt, len(res[0]), res[1].count('embeddings_set_grads_update_X'), host_class.__name__, ' '.join('%.1e' % v for v in gaps)))
        if opt == 'gd':
            assert [c[2] for c in res[0]] == [c[2] for c in ref[0]]             # halved and doubled from 0.01: exactly the same
        assert res[1].count('embeddings_set_grads_update_X') >= 3
    print('resident against %s, worst: SCG %.3g, GD %.3g; allowed %.3g' % (host_class.__name__, worst['scg'], worst['gd'], 10 * yard))
    return worst


def test_resident_scg_and_gd_follow_the_host_run_of_the_same_optimiser(runs):
    """SCG and GD, 6 iterations each on the two-shard model (431 + 569 rows, Q = 3, M = 8, D = 4): the resident vectors against cg_ref.NumpyOps
    holding [mu, raw S] on the host with the model only evaluating.  Same number of evaluations, same helper calls in the same order (so the same
    accepted / rejected pattern), the same steps, and per call x, f and the step within 10 x ``yardstick``, which must itself stay below 1e-9.

    GD passes through no reduction and the library rounds every multiply-add as NumPy does (varpoint.h, mul_then_add), so the resident GD run is
    IDENTICAL to the host's; SCG differs by the summation order of its five sums alone, which is what the yardstick varies.  Measured on an
    MI355X: see DESIGN.md section 9.3.1."""
    yard = yardstick(runs)
    worst = follow(runs, R.NumpyOps, yard)
    assert worst['scg'] <= 10 * yard and worst['gd'] <= 10 * yard


# ---- the state rule and the peeks' own errors ------------------------------------------------------------------------------------------------
def test_peeks_refuse_what_a_context_does_not_hold():
    from gparml_amd import _lib
    from gparml_amd._lib import GP_ERR_STATE
    from gparml_amd.engine import ShardEngine
    rng = np.random.RandomState(0)
    e = ShardEngine(7, 2, 4, 3, device=0)
    buf = np.zeros(42)

    def rc(name):
        return e.lib.gp_debug_peek(e.h, name.encode(), buf.ctypes.data_as(_lib._dp), buf.size), e.lib.gp_last_error(e.h).decode()
    for name in ('cg_g_new', 'cg_g_old', 'cg_g_latest', 'Xmu', 'Xs'):                 # no data
        code, msg = rc(name)
        assert code == GP_ERR_STATE and name in msg, (name, code, msg)
    e.upload_shard(rng.standard_normal((7, 2)), rng.standard_normal((7, 3)), np.full((7, 3), 0.5), xs_is_raw=False)
    for name in ('cg_g_new', 'cg_g_old', 'cg_g_latest'):                              # fixed embeddings: no CG vectors
        code, msg = rc(name)
        assert code == GP_ERR_STATE and 'free embeddings' in msg, (name, code, msg)
    assert np.array_equal(e.cg_peek('Xs'), np.full((7, 3), 0.5))                      # as stored
    raw = rng.standard_normal((7, 3))
    e.upload_embeddings(rng.standard_normal((7, 3)), raw, xs_is_raw=True)
    assert np.array_equal(e.cg_peek('Xs'), raw) and e.cg_peek('cg_g_new').shape == (2, 7, 3)
    e.close()
