#!/usr/bin/env python3
"""Time gp_paths_grad (derivatives of the pathwise posterior draws) and print one JSON line.

Model: configs[2]'s shape (M 512, Q 10, D 100), tools/bench_joint.py's generator.  16 draws on F = 1024 frequency pairs, at n = 1024 and n = 8192,
each measured twice: all outputs (jac, metric, grad, mean_jac: jac alone is n S D Q doubles, 1 GB at n = 8192, and its copy to pageable host
memory dominates that call) and metric + grad only (the contraction-only call: the one that shows the kernels).  Next to them, in the same run on
the same points, the 2 Q gp_paths_eval calls that central differences of the draws cost.  Times are wall milliseconds of one synchronous
ShardEngine call (host copies of inputs and outputs included), best of --reps after one warm-up.  The kernels' own times are not measured here:
take them from a separate
    rocprofv3 --kernel-trace --stats -- python tools/bench_paths_grad.py --reps 1
run.  Work model, Mp = M rounded up to 128: the chunk product is 2 n Q S D (2F + 2 Mp) flop, the projections
2 n Q Mp (Dp + 2 Mp), next to them n F sincos; fraction of peak of the two against 74 TF (FP64 4x4x4 MFMA, mma_f64.h), of the WHOLE call, so a
lower bound of the kernels'.  No time is a pass/fail threshold."""
import argparse
import json
import os
import sys

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
    ap.add_argument('--sizes', type=int, nargs='*', default=[1024, 8192])
    args = ap.parse_args()
    rs = np.random.RandomState(0)
    M, Q, D = 512, 10, 100
    Mp, Dp = -(-M // 128) * 128, -(-D // 128) * 128
    out = {'peak_tf': PEAK_TF, 'peak': 'FP64 v_mfma_f64_4x4x4_4b_f64 (mma_f64.h)', 'kernel_ms': 'not measured (rocprofv3 --kernel-trace --stats)',
           'M': M, 'Q': Q, 'D': D, 'n_draws': N_DRAWS, 'F': N_FEATURES}
    e, d = model(M, Q, D)
    omega = rs.randn(N_FEATURES, Q) * np.sqrt(d['alpha'])
    w, eps_u = rs.randn(N_DRAWS, 2 * N_FEATURES, D), rs.randn(N_DRAWS, M, D)
    e.paths_set(omega, w, eps_u, centre=d['Z'].mean(axis=0))
    wv = rs.randn(D)
    h = 1e-5
    for n in args.sizes:
        X = rs.randn(n, Q)
        flop = 2.0 * n * Q * N_DRAWS * D * (2 * N_FEATURES + 2 * Mp) + 2.0 * n * Q * Mp * (Dp + 2 * Mp)
        row = {'model_flop': flop, 'model_sincos': float(n * N_FEATURES), 'jac_bytes': 8.0 * N_DRAWS * n * D * Q}
        for name, kw in (('all_outputs', dict(weights=wv, jac=True, metric=True, want_mean=True)), ('metric_grad', dict(weights=wv, jac=False, metric=True))):
            ms = timed(lambda: e.paths_grad(X, **kw), args.reps)
            row[name] = {'ms': ms, 'frac_peak_whole_call': flop / (ms * 1e-3) / (PEAK_TF * 1e12)}

        def differences():
            for q in range(Q):
                step = np.zeros(Q)
                step[q] = h
                e.paths_eval(X + step)
                e.paths_eval(X - step)
        row['finite_differences_2Q_paths_eval'] = {'ms': timed(differences, args.reps), 'calls': 2 * Q}
        row['metric_grad_speedup_over_finite_differences'] = row['finite_differences_2Q_paths_eval']['ms'] / row['metric_grad']['ms']
        out['n%d' % n] = row
    e.paths_clear()
    e.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
