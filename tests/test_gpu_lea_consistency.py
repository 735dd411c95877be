"""One exponent on every path: LEA[n][m] = 1/2 ln c2_n - 1/2 sum_q w (mu - z)^2 - 1/2 sum_q v2 z^2 of the factorised psi2 as the shard's tables hold it
(b_le_kernel on its registers, lea_rows_kernel beyond the compiled widths), as gp_predict forms it for uncertain inputs and as gp_infer_objective
forms it, for the same points: identical bits.  The arithmetic has one definition (csrc/varpoint.h); the buffers come through gp_debug_peek."""
import numpy as np
import pytest

import infer_ref as I
from test_gpu_predictive import _engine, _model

pytestmark = pytest.mark.gpu

N, D, M = 300, 3, 130            # N off the 128-row granule (padding rows exist), M over two 128-column tiles with a ragged second one
NP, MP = 384, 256
K_PAD_LOG = -1.0e5               # csrc/fexp.h


def _shard(Q, seed):
    d = _model(N, D, M, Q, 'B', seed=seed)
    d['X_S'] = np.random.RandomState(seed + 3).uniform(0.05, 0.55, size=(N, Q))
    return d, _engine(d, N, D, M, Q)


def _one_chunk(fn):
    """fn() with the prediction and inference chunks sized to hold the shard's 300 points at once (384 rows)."""
    from gparml_amd import _lib
    lib = _lib.load()
    lib.gp_debug_set_option(b'predict_rows', NP)
    lib.gp_debug_set_option(b'infer_rows', NP)
    try:
        return fn()
    finally:
        lib.gp_debug_set_option(b'predict_rows', 0)
        lib.gp_debug_set_option(b'infer_rows', 0)


def _pred_and_infer_lea(e, d, xs, raw):
    def run():
        e.predict(d['X_mu'], xs, xs_is_raw=raw)
        pred = e.peek('pred_LEA', NP * MP).reshape(NP, MP)
        e.infer_objective(d['Y'], d['X_mu'], xs, xs_is_raw=raw)
        return pred, e.peek('infer_LEA', NP * MP).reshape(NP, MP)
    return _one_chunk(run)


# the shard's kernel: b_le_kernel with two columns per lane (latent tables 4 and 24 wide), with one (52 wide), and lea_rows_kernel (Q >= 64)
@pytest.mark.parametrize('Q', [3, 17, 40, 70])
def test_shard_predict_and_infer_hold_the_same_lea(Q):
    d, e = _shard(Q, seed=40 + Q)
    shard = e.peek('LEA', NP * MP).reshape(NP, MP)
    pred, inf = _pred_and_infer_lea(e, d, d['X_S'], False)
    e.close()
    live = shard[:N, :M]
    assert np.all(np.isfinite(live)) and np.all(live > K_PAD_LOG) and np.all(live <= np.log(d['sf2']))
    assert np.array_equal(pred[:N, :M], live), 'gp_predict: %d of %d entries differ from the shard' % (np.sum(pred[:N, :M] != live), live.size)
    assert np.array_equal(inf[:N, :M], live), 'gp_infer_objective: %d of %d entries differ from the shard' % (np.sum(inf[:N, :M] != live), live.size)
    assert np.all(pred[N:, :] == K_PAD_LOG) and np.all(pred[:, M:] == K_PAD_LOG)


def test_raw_variances_give_predict_and_infer_the_same_lea():
    """The same points with their variances in softplus-inverse space: predict and infer hold identical bits, and both agree with LEA formed on the
    host in long double from softplus(raw) and the device's own centred mu and Z (LEA alone depends on the origin).
    Bound.  With u = 2^-53: exp and log return S = log(1 + e^x) with an absolute error of about 3 u (1 + e^x in [1.05, 1.8]), so S >= 0.05 carries up
    to 60 u relative; w = alpha / (2 alpha S + 1) no more; v2 = (alpha - w) / 2 = alpha S w amplifies w's error by w / (alpha - w) = 1 / (2 alpha S).
    The few roundings of the sums themselves (Q = 3) fit beside that, so every term of LEA = ln sf2 - 1/4 sum ln d2 - 1/2 s - 1/2 t is within
    64 u (1 + 1 / (2 alpha S)) of its size, and |LEA_dev - LEA_host| <= 64 u max_q (1 + 1 / (2 alpha_q S_nq)) (|ln sf2| + 1/4 sum ln d2 + s/2 + t/2).
    A softplus that is off in its ninth digit misses it tenfold (asserted)."""
    Q = 3
    d, e = _shard(Q, seed=7)
    raw = I.softplus_inv(d['X_S'])
    pred, inf = _pred_and_infer_lea(e, d, raw, True)
    mu = e.peek('mu', NP * Q).reshape(NP, Q)[:N].astype(np.longdouble)          # the shard's points, centred as predict centres them
    Z = e.peek('Z', MP * Q).reshape(MP, Q)[:M].astype(np.longdouble)
    e.close()
    assert np.all(np.isfinite(pred[:N, :M])) and np.all(pred[:N, :M] > K_PAD_LOG)
    assert np.array_equal(pred[:N, :M], inf[:N, :M])

    def host(S):
        a = d['alpha'].astype(np.longdouble)
        d2 = 2 * a * S + 1
        w = a / d2
        lg = 0.25 * np.sum(np.log(d2), axis=1)[:, None]
        s = 0.5 * np.sum(w[:, None, :] * (mu[:, None, :] - Z[None, :, :]) ** 2, axis=2)
        t = 0.5 * np.sum(0.5 * (a - w)[:, None, :] * Z[None, :, :] ** 2, axis=2)
        l0 = np.log(np.longdouble(d['sf2']))
        amp = np.max(1 + 1 / (2 * a * S), axis=1)[:, None]
        return l0 - lg - s - t, 64 * 2.0 ** -53 * amp * (abs(l0) + lg + s + t)
    S = np.log1p(np.exp(raw.astype(np.longdouble)))
    ref, bound = host(S)
    err = np.abs(pred[:N, :M] - ref)
    print('[lea raw] worst |dev - host| / bound = %.3g (largest error %.3g, bound there %.3g)' % (np.max(err / bound), np.max(err), bound.flat[np.argmax(err)]))
    assert np.all(err <= bound)
    off, _ = host(S * (1 + np.longdouble(1e-9)))
    assert np.max(np.abs(pred[:N, :M] - off) / bound) > 10
