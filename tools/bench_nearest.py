#!/usr/bin/env python3
"""Time the start of latent inference (gp_nearest_rows, gp_nearest_rows_masked, gparml_amd.init.nearest_start) and print one JSON line.

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
  masked_all_ms / masked_pair_unmasked_ms  the masked search (ShardEngine.nearest_rows(observed=), gp_nearest_rows_masked) with every column
                                         observed, and the unmasked search timed in alternation with it; best of --reps each
  masked_over_unmasked_all               their ratio; masked_all_identical: the two returned the same bits
  masked_hide10_ms / terms_per_s_masked_hide10
                                         the masked search with ten random columns hidden per row (NaN there): n N (D - 10) terms
  masked_hide10_start_host_rows_s        Predictor.infer's ragged device start on those rows: one masked init.nearest_start with the training
                                         rows passed as host rows (their upload included)
  masked_perpattern_n / masked_perpattern_device_s / masked_perpattern_device_s_per_row
                                         the per-pattern device start that it replaces, on the first --pattern-n of those rows: every row has a
                                         pattern of its own, so one init.nearest_start(cols=) with host rows per row
  masked_perpattern_device_s_extrapolated_n   (time per row) x n: EXTRAPOLATED to n, not measured
  masked_start_differing_from_perpattern new rows among the first --pattern-n whose masked start differs from the per-pattern one
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


def timed_pair(fa, fb, reps):
    """best of ``reps`` of each, the two alternating after a warm-up of both"""
    fa()
    fb()
    best = [float('inf'), float('inf')]
    for _ in range(reps):
        for k, fn in enumerate((fa, fb)):
            t = time.perf_counter()
            fn()
            best[k] = min(best[k], time.perf_counter() - t)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--N', type=int, default=1000000)
    ap.add_argument('--D', type=int, default=100)
    ap.add_argument('--Q', type=int, default=10)
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--host-n', type=int, default=20, help='new rows of the host k-d tree timing (0: skip it)')
    ap.add_argument('--pattern-n', type=int, default=200, help='new rows of the per-pattern device start timing (0: skip it)')
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
    # the masked search: all columns observed against the unmasked call, then ten random columns hidden per row
    ones = np.ones((n, D), dtype=bool)
    tm, tu = timed_pair(lambda: eng.nearest_rows(Ys, observed=ones), lambda: eng.nearest_rows(Ys), args.reps)
    out['masked_all_ms'], out['masked_pair_unmasked_ms'], out['masked_over_unmasked_all'] = tm * 1e3, tu * 1e3, tm / tu
    out['masked_all_identical'] = bool(all(np.array_equal(a, b) for a, b in zip(eng.nearest_rows(Ys, observed=ones), eng.nearest_rows(Ys))))
    hide = min(10, D - 1)
    obs = np.ones((n, D), dtype=bool)
    for i in range(n):
        obs[i, rs.choice(D, hide, replace=False)] = False
    Yh = np.where(obs, Ys, np.nan)
    t = timed(lambda: eng.nearest_rows(Yh, observed=obs), args.reps)
    out['masked_hide10_ms'], out['terms_per_s_masked_hide10'] = t * 1e3, float(n) * N * (D - hide) / t
    t = time.perf_counter()
    X_masked = Predictor._nearest_on_device(eng, Yh, [(Yt, Xt)], observed=obs)
    out['masked_hide10_start_host_rows_s'] = time.perf_counter() - t
    if args.pattern_n > 0:
        pn = min(args.pattern_n, n)
        t = time.perf_counter()
        X_pat = np.concatenate([Predictor._nearest_on_device(eng, Yh[i:i + 1], [(Yt, Xt)], np.flatnonzero(obs[i])) for i in range(pn)])
        out['masked_perpattern_n'], out['masked_perpattern_device_s'] = pn, time.perf_counter() - t
        out['masked_perpattern_device_s_per_row'] = out['masked_perpattern_device_s'] / pn
        out['masked_perpattern_device_s_extrapolated_n'] = out['masked_perpattern_device_s_per_row'] * n
        out['masked_start_differing_from_perpattern'] = int(np.sum(np.any(X_pat != X_masked[:pn], axis=1)))
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
