#!/usr/bin/env python3
"""Time gp_condition_set / gp_condition_predict (the posterior conditioned on extra observed rows) and print one JSON line.

Model: M 512, Q 10, D 100, fixed embeddings, N = 1e6 resident rows (the headline regression workload).  In one process: gp_condition_set at
m = 1, 128 and 1024; gp_condition_predict at n = 1e5 under each; gp_predict on the same rows; and the path this replaces -- a second engine's
upload of the shard with the m rows appended, phase 1, global step and gp_predict.  Times are wall milliseconds of synchronous calls, best of
--reps after one warm-up.  Beside the two ratios (condition_predict / gp_predict; refit path / (set + predict)) the work model: set =
2 m Mp (Dp + 2 Mp) + 2 m^2 Mp + m^3 / 3 + 2 m^2 (Mp + Dp) flop, predict adds 2 n mp (Mp + Dp) to gp_predict's 2 n M (D + 2 M); ``model_ms`` is
gp_predict's time plus the added flop at gp_predict's own measured rate, ``over_model`` the measured time over it (> 1: a finding, to be broken
down by kernel with a profiler)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--N', type=int, default=1000000)
    ap.add_argument('--n', type=int, default=100000)
    args = ap.parse_args()
    from oracle import factorised as Fz
    from gparml_amd.engine import ShardEngine
    M, Q, D, N, n = 512, 10, 100, args.N, args.n
    Mp, Dp = 512, 128
    d = Fz.synthetic_shard(N, D, M, Q, regime='A', seed=2, zseed=3)
    e = ShardEngine(N, D, M, Q)
    e.set_timing(0)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    e.phase1()
    e.global_step(sync=True)
    rs = np.random.RandomState(5)
    X = rs.randn(n, Q)
    out = {'M': M, 'Q': Q, 'D': D, 'N_resident': N, 'n': n, 'reps': args.reps}
    predict_ms = timed(lambda: e.predict(X), args.reps)
    predict_flop = 2.0 * n * M * (D + 2 * M)
    out['predict_ms'] = predict_ms
    out['predict_gflops'] = predict_flop / predict_ms * 1e-6
    sets = {}
    for m in (1, 128, 1024):
        mp = (m + 127) // 128 * 128
        Xc = 0.5 * rs.randn(m, Q)
        Yc = np.sin(Xc.dot(rs.randn(Q, D))) + 0.3 * rs.randn(m, D)
        sets[m] = (Xc, Yc)
        set_ms = timed(lambda: e.condition(Xc, Yc), args.reps)
        cp_ms = timed(lambda: e.condition_predict(X, want_reduction=True), args.reps)
        added = 2.0 * n * mp * (Mp + Dp)
        model_ms = predict_ms * (1.0 + added / predict_flop)
        out['m_%d' % m] = {'set_ms': set_ms, 'condition_predict_ms': cp_ms, 'ratio_to_predict': cp_ms / predict_ms,
                           'set_flop': 2.0 * m * Mp * (Dp + 2 * Mp) + 2.0 * m * m * Mp + m ** 3 / 3.0 + 2.0 * m * m * (Mp + Dp),
                           'predict_added_flop': added, 'model_ms': model_ms, 'over_model': cp_ms / model_ms}
    e.condition_clear()
    e.close()
    # the path this replaces, at m = 128: the shard with the rows appended on a fresh engine
    m = 128
    Xc, Yc = sets[m]
    Y2, X2, S2 = np.vstack((d['Y'], Yc)), np.vstack((d['X_mu'], Xc)), np.zeros((N + m, Q))
    e2 = ShardEngine(N + m, D, M, Q)
    e2.set_timing(0)
    e2.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])

    def refit():
        e2.upload_shard(Y2, X2, S2)
        e2.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
        e2.phase1()
        e2.global_step(sync=True)
        e2.predict(X)
    refit_ms = timed(refit, args.reps)
    e2.close()
    out['refit_path_ms'] = refit_ms
    out['refit_over_set_plus_predict'] = refit_ms / (out['m_128']['set_ms'] + out['m_128']['condition_predict_ms'])
    print(json.dumps(out))


if __name__ == '__main__':
    main()
