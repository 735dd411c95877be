#!/usr/bin/env python3
"""Time the initialisation of the inducing points (gp_kmeans_accumulate, gparml_amd.init.kmeans) and print one JSON line.

N = 1e6 rows, Q = 10, K = 512, normal data (the per-GPU shard of the benchmark; parallel_GPLVM.py:179-186 runs scipy.cluster.vq.kmeans there):
  pass_resident_ms / pass_host_rows_ms   wall milliseconds of one synchronous ShardEngine.kmeans_accumulate call on the resident X_mu / on host rows
                                         (the 80 MB upload included), best of --reps after one warm-up
  kmeans_passes / kmeans_s               a whole init.kmeans run on the resident rows from K random rows, to scipy's threshold 1e-5
  scipy_vq_pass_s                        one scipy.cluster.vq.vq pass over the same rows and centres on this host: what a pass cost before
  scipy_kmeans_1e5_iter1_s               scipy.cluster.vq.kmeans(X[:100000], 512, iter=1) on this host (the reference runs iter=20 of these)
The gate (exit status 1 when it fails): one resident device pass takes less time than one scipy vq pass.
Work model: N K Q distance terms, a subtraction and an fma each, 2 N K Q FP64 VALU lane-slots against 74 TF / 2 per second."""
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
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--N', type=int, default=1000000)
    ap.add_argument('--Q', type=int, default=10)
    ap.add_argument('--K', type=int, default=512)
    ap.add_argument('--no-host', action='store_true', help='skip the two scipy timings (and the gate)')
    args = ap.parse_args()
    import scipy.cluster.vq as cl
    from gparml_amd import init
    from gparml_amd.engine import ShardEngine
    N, Q, K = args.N, args.Q, args.K
    rs = np.random.RandomState(0)
    X = rs.randn(N, Q)
    C = X[rs.choice(N, K, replace=False)].copy()
    eng = ShardEngine(N, 1, 1, Q)
    eng.upload_shard(np.zeros((N, 1)), X, np.zeros((N, Q)))
    out = {'N': N, 'Q': Q, 'K': K}
    out['pass_resident_ms'] = timed(lambda: eng.kmeans_accumulate(C), args.reps) * 1e3
    out['pass_host_rows_ms'] = timed(lambda: eng.kmeans_accumulate(C, X=X), args.reps) * 1e3
    lanes = 2.0 * N * K * Q
    out['valu_lane_slots'] = lanes
    out['frac_peak'] = lanes / (out['pass_resident_ms'] * 1e-3) / (PEAK_TF * 1e12 / 2.0)
    t = time.perf_counter()
    centres, dist, passes = init.kmeans([eng], K, seeds=C)
    out['kmeans_s'], out['kmeans_passes'], out['kmeans_centres'], out['kmeans_mean_distance'] = time.perf_counter() - t, passes, int(centres.shape[0]), dist
    labels = eng.kmeans_accumulate(C, want_labels=True)[3]
    eng.close()
    ok = True
    if not args.no_host:
        t = time.perf_counter()
        code, _ = cl.vq(X, C)
        out['scipy_vq_pass_s'] = time.perf_counter() - t
        out['labels_differing_from_scipy'] = int(np.sum(code != labels))       # scipy's expanded form may break near-ties the other way
        np.random.seed(0)
        t = time.perf_counter()
        cl.kmeans(X[:100000], K, iter=1)
        out['scipy_kmeans_1e5_iter1_s'] = time.perf_counter() - t
        ok = out['pass_resident_ms'] * 1e-3 < out['scipy_vq_pass_s']
        out['gate_device_pass_faster_than_scipy_vq'] = bool(ok)
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
