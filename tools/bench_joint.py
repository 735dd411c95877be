#!/usr/bin/env python3
"""Time gp_predict_joint and gp_predict_sample (joint posterior covariance and coherent draws) and print one JSON line.

Model: configs[2]'s shape (M 512, Q 10, D 100), tools/bench_predict.py's generator.  gp_predict_joint at n = 4096 and 16384, gp_predict_sample at
n = 4096 and 8192 with 16 draws.  Times are wall milliseconds of one synchronous ShardEngine call (host copies of inputs and outputs included: the
n x n matrix is 2 GB at n = 16384), best of --reps after one warm-up.  pred_cov_kernel's own time is not measured here: take it from a separate
    rocprofv3 --kernel-trace --stats -- python tools/bench_joint.py --reps 1
run (the kernel's rows of the stats table).  Work model, np = n rounded up to 128, Mp = M rounded up to 128:
  covariance   (np/128)(np/128 + 1)/2 tiles x 2 . 128^2 . 2 Mp MFMA flop + n^2/2 . (2 Q + 17) FP64 VALU lane-slots for k(x_i, x_j)
  draws        the same covariance + np^3 / 3 (Cholesky) + 2 np^2 . draws . D (Lc eps) flop
fraction of peak against 74 TF (FP64 4x4x4 MFMA / VALU FMA rate, mma_f64.h), MFMA and VALU work counted on the one pipe they share.  The fraction of
the covariance's model is of the WHOLE call (products of R, the kernel, the copy of the matrix to the host), so it is a lower bound of the kernel's.
--host: the same quantities with numpy on this host from the downloaded statistics (tests/joint_ref.py), at n = 4096 only."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

PEAK_TF = 74.0
N_DRAWS = 16


def model(M, Q, D, N=4000):
    from oracle import factorised as Fz
    from gparml_amd.engine import ShardEngine
    d = Fz.synthetic_shard(N, D, M, Q, regime='A', seed=2, zseed=3)
    e = ShardEngine(N, D, M, Q)
    e.set_timing(0)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    e.phase1()
    e.global_step(sync=True)
    return e, d


def timed(fn, reps):
    fn()
    best = float('inf')
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return best * 1e3


def cov_work(n, M, Q):
    up = lambda x: -(-x // 128) * 128
    nt = up(n) // 128
    return nt * (nt + 1) / 2 * 2.0 * 128 * 128 * 2 * up(M), n * n / 2.0 * (2 * Q + 17)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--host', action='store_true', help='also time the numpy reference on this host (n = 4096)')
    args = ap.parse_args()
    rs = np.random.RandomState(0)
    out = {'peak_tf': PEAK_TF, 'peak': 'FP64 v_mfma_f64_4x4x4_4b_f64 = FP64 VALU FMA rate (mma_f64.h)', 'kernel_ms': 'not measured (rocprofv3 --kernel-trace --stats)'}
    M, Q, D = 512, 10, 100
    e, d = model(M, Q, D)
    frac = lambda mfma, valu, ms: (mfma / 2.0 + valu) * 2.0 / (ms * 1e-3) / (PEAK_TF * 1e12)      # FMA-equivalents on the shared FP64 pipe
    for n in (4096, 16384):
        X = rs.randn(n, Q)
        ms = timed(lambda: e.predict_joint(X), args.reps)
        mfma, valu = cov_work(n, M, Q)
        out['joint_n%d' % n] = {'ms': ms, 'mfma_flop': mfma, 'valu_lane_slots': valu, 'frac_peak_whole_call': frac(mfma, valu, ms)}
    for n in (4096, 8192):
        X = rs.randn(n, Q)
        eps = rs.randn(N_DRAWS, n, D)
        ms = timed(lambda: e.predict_sample(X, N_DRAWS, include_noise=True, eps=eps), args.reps)
        mfma, valu = cov_work(n, M, Q)
        up = -(-n // 128) * 128
        mfma += up ** 3 / 3.0 + 2.0 * up * up * N_DRAWS * D
        out['sample_n%d_draws%d' % (n, N_DRAWS)] = {'ms': ms, 'mfma_flop': mfma, 'valu_lane_slots': valu, 'frac_peak_whole_call': frac(mfma, valu, ms)}
    if args.host:
        import joint_ref as J
        n = 4096
        X = rs.randn(n, Q)
        Psi2, C = e.download('PSI2_SUM'), e.download('PSI1TY')
        t = time.perf_counter()
        mean, cov = J.joint(d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2, C, X, include_noise=True)
        t_cov = time.perf_counter() - t
        eps = rs.randn(N_DRAWS, n, D)
        t = time.perf_counter()
        Lc = np.linalg.cholesky(cov + 1e-8 * d['sf2'] * np.eye(n))
        draws = mean[None] + Lc @ eps
        t_draw = time.perf_counter() - t
        out['host_numpy_n%d' % n] = {'joint_ms': t_cov * 1e3, 'sample_ms': (t_cov + t_draw) * 1e3, 'threads': os.environ.get('OMP_NUM_THREADS', 'default')}
        del draws
    e.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
