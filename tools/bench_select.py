#!/usr/bin/env python3
"""Time the greedy conditional-variance selection of the inducing points (gp_select_begin + gp_select_run, csrc/select.hip) and print one JSON line.

N = 1e6 rows, Q = 10, K = 512, normal data, alpha_q = 1 / Q, sf2 = 1 (the per-GPU shard of the benchmark):
  select_resident_s / select_host_rows_s   wall seconds of ShardEngine.select_begin + select_run(K) + select_end over the resident X_mu / over host
                                           rows (the 80 MB upload included), best of --reps after one warm-up
  selected, trace_first, trace_last        K' and the Nystrom trace residual after the first and the last step
  model_bytes, implied_GBps                the byte model 4 n K^2 (the streaming reads of the factor: step j reads 8 n j bytes) and what the resident
                                           time makes of it
  kmeans_s, kmeans_passes                  init.kmeans on the same resident rows from K random rows to scipy's threshold, in the same run
No time is a pass/fail threshold: the exit status is 0 whenever both ran."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--N', type=int, default=1000000)
    ap.add_argument('--Q', type=int, default=10)
    ap.add_argument('--K', type=int, default=512)
    ap.add_argument('--no-kmeans', action='store_true')
    args = ap.parse_args()
    from gparml_amd import init
    from gparml_amd.engine import ShardEngine
    N, Q, K = args.N, args.Q, args.K
    rs = np.random.RandomState(0)
    X = rs.randn(N, Q)
    alpha = np.full(Q, 1.0 / Q)
    eng = ShardEngine(N, 1, 1, Q)
    eng.upload_shard(np.zeros((N, 1)), X, np.zeros((N, Q)))
    last = {}

    def run(rows):
        eng.select_begin(K, 1.0, alpha, X=rows)
        try:
            last['rows'], last['trace'] = eng.select_run(K)
        finally:
            eng.select_end()

    def timed(fn):
        fn()
        best = float('inf')
        for _ in range(max(1, args.reps)):
            t = time.perf_counter()
            fn()
            best = min(best, time.perf_counter() - t)
        return best

    out = {'N': N, 'Q': Q, 'K': K}
    out['select_resident_s'] = timed(lambda: run(None))
    out['selected'], out['trace_first'], out['trace_last'] = int(len(last['rows'])), float(last['trace'][0]), float(last['trace'][-1])
    out['select_host_rows_s'] = timed(lambda: run(X))
    out['model_bytes'] = 4.0 * N * K * K
    out['implied_GBps'] = out['model_bytes'] / out['select_resident_s'] / 1e9
    if not args.no_kmeans:
        C = X[rs.choice(N, K, replace=False)].copy()
        t = time.perf_counter()
        centres, dist, passes = init.kmeans([eng], K, seeds=C)
        out['kmeans_s'], out['kmeans_passes'], out['kmeans_centres'] = time.perf_counter() - t, int(passes), int(centres.shape[0])
    eng.close()
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
