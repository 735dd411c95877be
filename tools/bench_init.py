#!/usr/bin/env python3
"""Time the initialisation of the inducing points (gp_kmeans_accumulate, gparml_amd.init.kmeans) and print one JSON line.

N = 1e6 rows, Q = 10, K = 512, normal data (the per-GPU shard of the benchmark; parallel_GPLVM.py:179-186 runs scipy.cluster.vq.kmeans there):
  pass_resident_ms / pass_host_rows_ms   wall milliseconds of one synchronous ShardEngine.kmeans_accumulate call on the resident X_mu / on host rows
                                         (the 80 MB upload included), best of --reps after one warm-up
  kmeans_passes / kmeans_s               a whole init.kmeans run on the resident rows from K random rows, to scipy's threshold 1e-5
  scipy_vq_pass_s                        one scipy.cluster.vq.vq pass over the same rows and centres on this host: what a pass cost before
  scipy_kmeans_1e5_iter1_s               scipy.cluster.vq.kmeans(X[:100000], 512, iter=1) on this host (the reference runs iter=20 of these)
The gate (exit status 1 when it fails): one resident device pass takes less time than one scipy vq pass.
Work model: N K Q distance terms, a subtraction and an fma each, 2 N K Q FP64 VALU lane-slots against 74 TF / 2 per second.

The PCA that initialises the embeddings (gp_scatter_accumulate / gp_project_rows, gparml_amd.init.pca), additional keys under 'pca': per D of
--pca-D (default 100 and 1000) at --pca-N rows (default 1e6), a dict with
  scatter_resident_ms / scatter_host_rows_ms       one synchronous ShardEngine.scatter_accumulate call (sums + Gram matrix), best of --reps
  sum_resident_ms                                  the sum-only pass
  project_resident_ms_Q<q> / project_host_rows_ms_Q<q>   one ShardEngine.project_rows call for every q of --pca-Q (default 10 and 50)
  scatter_frac_peak                                N D (D + 1) flop of the triangle over the resident time, against 74 TF
  host_scatter_s / host_project_s_Q<q>             the arithmetic of gpu_MapReduce._streaming_pca over the same rows on this host, in blocks of
                                                   1e5 rows (shift, column sums, Yc^T Yc; (Y - mean) V / std), parsing excluded
  gate_device_scatter_faster_than_host             the second gate: the resident scatter pass against host_scatter_s"""
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
    ap.add_argument('--no-host', action='store_true', help='skip the host timings (and the gates)')
    ap.add_argument('--no-kmeans', action='store_true', help='skip the k-means figures')
    ap.add_argument('--no-pca', action='store_true', help='skip the PCA figures')
    ap.add_argument('--pca-N', type=int, default=1000000)
    ap.add_argument('--pca-D', type=str, default='100,1000')
    ap.add_argument('--pca-Q', type=str, default='10,50')
    args = ap.parse_args()
    out, ok = {}, True
    if not args.no_kmeans:
        ok = bench_kmeans(args, out)
    if not args.no_pca:
        out['pca'] = {}
        for D in [int(d) for d in args.pca_D.split(',')]:
            ok = bench_pca(args, D, out['pca']) and ok
    print(json.dumps(out))
    return 0 if ok else 1


def bench_pca(args, D, out):
    from gparml_amd.engine import ShardEngine
    N, Qs = args.pca_N, [int(q) for q in args.pca_Q.split(',')]
    rs = np.random.RandomState(1)
    B = min(N, 100000)
    block = rs.randn(B, 8).dot(rs.randn(8, D)) + 0.1 * rs.randn(B, D)
    Y = np.empty((N, D))
    for k, i in enumerate(range(0, N, B)):          # ten blocks of one draw, scaled and shifted apart: cheap to make, full rank
        Y[i:i + B] = block[:min(B, N - i)] * (1.0 + 0.01 * k) + 100.0 + k
    o = out['D%d' % D] = {'N': N, 'D': D}
    eng = ShardEngine(N, D, 1, 1)
    eng.upload_shard(Y, np.zeros((N, 1)), np.zeros((N, 1)))
    centre = eng.scatter_accumulate(np.zeros(D), want_gram=False)[0] / N
    o['sum_resident_ms'] = timed(lambda: eng.scatter_accumulate(centre, want_gram=False), args.reps) * 1e3
    o['scatter_resident_ms'] = timed(lambda: eng.scatter_accumulate(centre), args.reps) * 1e3
    o['scatter_host_rows_ms'] = timed(lambda: eng.scatter_accumulate(centre, Y=Y), max(1, args.reps // 2)) * 1e3
    o['scatter_flop'] = float(N) * D * (D + 1)
    o['scatter_frac_peak'] = o['scatter_flop'] / (o['scatter_resident_ms'] * 1e-3) / (PEAK_TF * 1e12)
    from gparml_amd import init
    ssum, gram = eng.scatter_accumulate(centre)
    for Q in Qs:
        mean, V, std = init.pca_axes(N, centre, ssum, gram, Q)
        P = V / std
        o['project_resident_ms_Q%d' % Q] = timed(lambda: eng.project_rows(mean, P), args.reps) * 1e3
        o['project_host_rows_ms_Q%d' % Q] = timed(lambda: eng.project_rows(mean, P, Y=Y), max(1, args.reps // 2)) * 1e3
        o['project_flop_Q%d' % Q] = 2.0 * N * D * Q
    X = eng.project_rows(mean, P)
    eng.close()
    ok = True
    if not args.no_host:
        t = time.perf_counter()
        shift, hs, hg = Y[:B].mean(axis=0), np.zeros(D), np.zeros((D, D))
        for i in range(0, N, B):
            Yc = Y[i:i + B] - shift
            hs += Yc.sum(axis=0)
            hg += Yc.T.dot(Yc)
        o['host_scatter_s'] = time.perf_counter() - t
        for Q in Qs:
            hm, hV, hstd = init.pca_axes(N, shift, hs, hg, Q)
            t = time.perf_counter()
            Xh = np.concatenate([(Y[i:i + B] - hm).dot(hV) / hstd for i in range(0, N, B)])
            o['host_project_s_Q%d' % Q] = time.perf_counter() - t
        o['max_abs_diff_from_host_embedding'] = float(np.max(np.abs(X - Xh)))
        ok = o['scatter_resident_ms'] * 1e-3 < o['host_scatter_s']
        o['gate_device_scatter_faster_than_host'] = bool(ok)
    print('[bench_init] pca D=%d done' % D, file=sys.stderr, flush=True)
    return ok


def bench_kmeans(args, out):
    import scipy.cluster.vq as cl
    from gparml_amd import init
    from gparml_amd.engine import ShardEngine
    N, Q, K = args.N, args.Q, args.K
    rs = np.random.RandomState(0)
    X = rs.randn(N, Q)
    C = X[rs.choice(N, K, replace=False)].copy()
    eng = ShardEngine(N, 1, 1, Q)
    eng.upload_shard(np.zeros((N, 1)), X, np.zeros((N, Q)))
    out.update({'N': N, 'Q': Q, 'K': K})
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
    return ok


if __name__ == '__main__':
    sys.exit(main())
