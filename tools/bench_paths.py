#!/usr/bin/env python3
"""Time gp_paths_eval (pathwise posterior function draws) and print one JSON line.

Model: configs[2]'s shape (M 512, Q 10, D 100), tools/bench_joint.py's generator.  16 draws on F = 1024 frequency pairs, evaluated at n = 8192 and
n = 65536; in the same run gp_predict_sample at n = 8192 with 16 draws, the n^3 path the draws replace.  Times are wall milliseconds of one
synchronous ShardEngine call (host copies of inputs and outputs included: the draws are 839 MB at n = 65536), best of --reps after one warm-up;
gp_paths_set is timed once.  The kernels' own times are not measured here: take them from a separate
    rocprofv3 --kernel-trace --stats -- python tools/bench_paths.py --reps 1
run.  Work model, Mp = M rounded up to 128: the chunk product is 2 n S D (2F + 2 Mp) flop, next to it n F sincos and the
front of gp_predict (Psi1*, 2 n Mp (Dp + 2 Mp) flop); fraction of peak of the chunk product alone against 74 TF (FP64 4x4x4 MFMA, mma_f64.h), of
the WHOLE call, so a lower bound of the kernel's."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

PEAK_TF = 74.0
N_DRAWS, N_FEATURES = 16, 1024


def main():
    from bench_joint import model, timed
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--sizes', type=int, nargs='*', default=[8192, 65536])
    args = ap.parse_args()
    rs = np.random.RandomState(0)
    M, Q, D = 512, 10, 100
    Mp = -(-M // 128) * 128
    out = {'peak_tf': PEAK_TF, 'peak': 'FP64 v_mfma_f64_4x4x4_4b_f64 (mma_f64.h)', 'kernel_ms': 'not measured (rocprofv3 --kernel-trace --stats)',
           'M': M, 'Q': Q, 'D': D, 'n_draws': N_DRAWS, 'F': N_FEATURES}
    e, d = model(M, Q, D)
    omega = rs.randn(N_FEATURES, Q) * np.sqrt(d['alpha'])
    w, eps_u = rs.randn(N_DRAWS, 2 * N_FEATURES, D), rs.randn(N_DRAWS, M, D)
    t = time.perf_counter()
    e.paths_set(omega, w, eps_u, centre=d['Z'].mean(axis=0))
    out['paths_set_ms'] = (time.perf_counter() - t) * 1e3
    for n in args.sizes:
        X = rs.randn(n, Q)
        ms = timed(lambda: e.paths_eval(X), args.reps)
        flop = 2.0 * n * N_DRAWS * D * (2 * N_FEATURES + 2 * Mp)
        out['paths_n%d' % n] = {'ms': ms, 'model_flop': flop, 'frac_peak_whole_call': flop / (ms * 1e-3) / (PEAK_TF * 1e12),
                                'out_bytes': 8.0 * N_DRAWS * n * D}
    e.paths_clear()
    n = 8192
    X = rs.randn(n, Q)
    eps = rs.randn(N_DRAWS, n, D)
    out['sample_n%d_draws%d' % (n, N_DRAWS)] = {'ms': timed(lambda: e.predict_sample(X, N_DRAWS, eps=eps), args.reps)}
    e.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
