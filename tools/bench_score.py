#!/usr/bin/env python3
"""Time gp_predict_score (held-out scoring on the device) and print one JSON line.

Model: M 512, Q 10, D 100, free embeddings, N = 1e6 resident rows.  Cases: host rows n = 1e5 and the resident rows N = 1e6, each with
deterministic and with uncertain inputs.  Next to each, on the same rows in the same process: ShardEngine.predict plus the same score
formed in numpy from its output (what a user had to do before).  Times are wall milliseconds of one synchronous call (host copies included),
best of --reps after one warm-up; ``numpy_ms`` is the host part of the second route alone.  Traffic model: host rows send Y
(8 n D bytes) up instead of taking the mean, and for uncertain inputs the variance, down; resident rows take 8 (3 n + 5 D) bytes down in all
where predict sends 8 n Q (x2) up and takes 8 n D (x2) down."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    fn()
    best = float('inf')
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return best * 1e3


def numpy_score(Y, mean, var):
    """row_logp, row_sse, row_chi2 and the (D, 5) column sums from predict's output: the formulas of gp_predict_score, fully observed."""
    e = Y - mean
    e2 = e * e
    q = e2 / var
    logp = -0.5 * (np.log(2.0 * np.pi * var) + q)
    cols = np.stack([np.full(Y.shape[1], float(Y.shape[0])), e.sum(axis=0), e2.sum(axis=0), q.sum(axis=0), logp.sum(axis=0)], axis=1)
    return logp.sum(axis=1), e2.sum(axis=1), q.sum(axis=1), cols


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--N', type=int, default=1000000)
    ap.add_argument('--n', type=int, default=100000)
    args = ap.parse_args()
    from oracle import factorised as Fz
    from gparml_amd.engine import ShardEngine
    M, Q, D, N, n = 512, 10, 100, args.N, args.n
    d = Fz.synthetic_shard(N, D, M, Q, regime='B', seed=2, zseed=3)
    e = ShardEngine(N, D, M, Q)
    e.set_timing(0)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    e.phase1()
    e.global_step(sync=True)
    out = {'M': M, 'Q': Q, 'D': D, 'N_resident': N, 'n_host': n, 'reps': args.reps}
    rs = np.random.RandomState(0)
    Xh, Sh = rs.randn(n, Q), rs.uniform(0.05, 0.5, size=(n, Q))
    Yh = e.predict(Xh)[0] + rs.randn(n, D) / np.sqrt(d['beta'])
    Xr, Sr, Yr = e.download('X_MU'), np.ascontiguousarray(d['X_S'], dtype=np.float64), np.ascontiguousarray(d['Y'], dtype=np.float64)
    keep = {}

    def route_numpy(X, S, Y, key):
        t = time.perf_counter()
        m, v = e.predict(X, S, include_noise=True)
        t1 = time.perf_counter()
        keep[key] = numpy_score(Y, m, v)
        keep[key + '_numpy_ms'] = (time.perf_counter() - t1) * 1e3
        keep[key + '_predict_ms'] = (t1 - t) * 1e3

    for name, X, S, Y, resident in (('host_det', Xh, None, Yh, False), ('host_unc', Xh, Sh, Yh, False), ('resident_det', Xr, None, Yr, True),
                                    ('resident_unc', Xr, Sr, Yr, True)):
        rows = X.shape[0]
        if resident:
            fused = lambda: keep.__setitem__(name + '_dev', e.score(None, use_resident_S=S is not None))      # noqa: E731
        else:
            fused = lambda: keep.__setitem__(name + '_dev', e.score(Y, X, S))                                  # noqa: E731
        ms = timed(fused, args.reps)
        ms_np = timed(lambda: route_numpy(X, S, Y, name), args.reps)
        dev, ref = keep[name + '_dev'], keep[name]
        scale = np.maximum(np.abs(ref[0]), 1.0)
        out[name] = {'rows': rows, 'score_ms': ms, 'predict_plus_numpy_ms': ms_np, 'of_which_predict_ms': keep[name + '_predict_ms'],
                     'of_which_numpy_ms': keep[name + '_numpy_ms'], 'speedup': ms_np / ms,
                     'bytes_up_score': 0 if resident else 8 * rows * (D + Q * (2 if S is not None else 1)),
                     'bytes_down_score': 8 * (3 * rows + 5 * D),
                     'bytes_up_predict': 8 * rows * Q * (2 if S is not None else 1),
                     'bytes_down_predict': 8 * rows * (D + (D if S is not None else 1)),
                     'max_rel_diff_row_logp': float(np.max(np.abs(dev['row_logp'] - ref[0]) / scale)),
                     'nlpd_pooled': float(dev['pooled']['nlpd']), 'rmse_pooled': float(dev['pooled']['rmse'])}
    e.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
