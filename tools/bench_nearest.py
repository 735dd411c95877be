#!/usr/bin/env python3
"""Time the start of latent inference (gp_nearest_rows, gparml_amd.init.nearest_start) and print one JSON line.

N = 1e6 resident training rows, D = 100, n = 1e4 new rows, normal data (the per-GPU shard of the benchmark; predict.py:44-66 searches it with a
k-d tree per shard on the host):
  resident_all_ms / resident_cols10_ms   wall milliseconds of one synchronous ShardEngine.nearest_rows call over all D columns / over a subset
                                         of 10 scattered columns (the upload of the new rows included), best of --reps after one warm-up
  terms_per_s_all / terms_per_s_cols10   the implied distance terms (n N columns; a subtraction and an fma each) per second
  frac_peak_all                          2 n N D FP64 VALU lane-slots over the time, against 74 TF / 2 per second
  start_resident_ms                      a whole init.nearest_start on the engine (search, gather of the means, cut-off)
  host_kdtree_n / host_kdtree_s / host_kdtree_s_per_row
                                         Predictor.nearest_training_embeddings (cKDTree, leaf size 100, cut-off 6) on this host over the same
                                         training rows for the first --host-n new rows (building the tree included, as the reference pays it per call)
  host_kdtree_s_extrapolated_n           (time per new row) x n: EXTRAPOLATED to the device's n, not measured
  index_differing_from_host              new rows among the first --host-n whose device start differs from the host's
No gate: the exit status is 0 whenever the run completes."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TF = 74.0


def timed(fn, reps):
    fn()
    best = float('inf')
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--N', type=int, default=1000000)
    ap.add_argument('--D', type=int, default=100)
    ap.add_argument('--Q', type=int, default=10)
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--host-n', type=int, default=20, help='new rows of the host k-d tree timing (0: skip it)')
    args = ap.parse_args()
    from gparml_amd import init
    from gparml_amd.engine import ShardEngine
    from gparml_amd.predict import Predictor
    N, D, Q, n = args.N, args.D, args.Q, args.n
    rs = np.random.RandomState(0)
    Yt, Xt = rs.randn(N, D), rs.randn(N, Q)
    Ys = Yt[rs.choice(N, n, replace=n > N)] + 0.3 * rs.randn(n, D)          # new rows near training rows: most lie within the cut-off
    cols = sorted(set(np.linspace(0, D - 1, 10).astype(int).tolist()))
    out = {'N': N, 'D': D, 'Q': Q, 'n': n, 'cols10': cols}
    eng = ShardEngine(N, D, 1, Q)
    eng.upload_shard(Yt, Xt, np.zeros((N, Q)))
    for key, c in (('all', None), ('cols10', cols)):
        t = timed(lambda: eng.nearest_rows(Ys, cols=c), args.reps)
        terms = float(n) * N * (D if c is None else len(c))
        out['resident_%s_ms' % key], out['terms_%s' % key], out['terms_per_s_%s' % key] = t * 1e3, terms, terms / t
    out['frac_peak_all'] = 2.0 * out['terms_all'] / (out['resident_all_ms'] * 1e-3) / (PEAK_TF * 1e12 / 2.0)
    out['start_resident_ms'] = timed(lambda: init.nearest_start([eng], Ys), 1) * 1e3
    X_dev, dist, _, _ = init.nearest_start([eng], Ys)
    out['new_rows_within_cutoff'] = int(np.sum(dist < 6.0))
    eng.close()
    if args.host_n > 0:
        hn = min(args.host_n, n)
        t = time.perf_counter()
        X_host = Predictor.nearest_training_embeddings(Ys[:hn], [(Yt, Xt)], Q)
        out['host_kdtree_n'], out['host_kdtree_s'] = hn, time.perf_counter() - t
        out['host_kdtree_s_per_row'] = out['host_kdtree_s'] / hn
        out['host_kdtree_s_extrapolated_n'] = out['host_kdtree_s_per_row'] * n
        out['index_differing_from_host'] = int(np.sum(np.any(X_host != X_dev[:hn], axis=1)))
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
