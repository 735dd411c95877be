#!/usr/bin/env python3
"""Time gp_predict_grad (Jacobian, variance derivative, expected metric tensor and its log-determinant at new inputs) and print one JSON line.

Model: configs[2]'s shape (M 512, Q 10, D 100), tools/bench_joint.py's generator.  Three calls: n = 1e4 with all outputs, n = 1e5 with all outputs,
n = 1e5 with metric and logdet only.  Times are wall milliseconds of one synchronous ShardEngine call (host copies of inputs and outputs included:
jac is 800 MB at n = 1e5), best of --reps after one warm-up.  The kernels' own times are not measured here: take them from a separate
    rocprofv3 --kernel-trace --stats -- python tools/bench_grad.py --reps 1
run.  Work model, Mp / Dp = M / D rounded up to 128:
  2 n Q Mp (Dp + 2 Mp) MFMA flop (the two products) + n Q (Q + 1) / 2 (Dp + 2 Mp) FMA slots (the per-point Gram)
fraction of peak against 74 TF (FP64 4x4x4 MFMA / VALU FMA rate, mma_f64.h), of the WHOLE call.  The first points of the large call are also
evaluated alone: `alone_bits_equal` says whether they carry the same bits (the large call's products run on the 128 x 128-tile GEMM kernel, a
single point's on the 32 x 32-tile one).  host_numpy: tests/grad_ref.py's float64 form at n = 1e3 with numpy on this host."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from bench_joint import PEAK_TF, model, timed     # noqa: E402


def work(n, M, Q, D):
    up = lambda x: -(-x // 128) * 128
    w = up(D) + 2 * up(M)
    return 2.0 * n * Q * up(M) * w, n * Q * (Q + 1) / 2.0 * w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=2)
    args = ap.parse_args()
    rs = np.random.RandomState(0)
    out = {'peak_tf': PEAK_TF, 'kernel_ms': 'not measured (rocprofv3 --kernel-trace --stats)'}
    M, Q, D = 512, 10, 100
    e, d = model(M, Q, D)
    frac = lambda mfma, fma, ms: (mfma + 2.0 * fma) / (ms * 1e-3) / (PEAK_TF * 1e12)
    X = rs.randn(100000, Q)
    all_out = dict(jac=True, dvar=True, metric=True, logdet=True)
    for name, n, which in (('all_n10000', 10000, all_out), ('all_n100000', 100000, all_out),
                           ('metric_logdet_n100000', 100000, dict(jac=False, dvar=False, metric=True, logdet=True))):
        ms = timed(lambda: e.predict_grad(X[:n], **which), args.reps)
        mfma, fma = work(n, M, Q, D)
        out[name] = {'ms': ms, 'mfma_flop': mfma, 'fma_slots': fma, 'frac_peak_whole_call': frac(mfma, fma, ms)}
    big = e.predict_grad(X[:20000])
    out['alone_bits_equal'] = bool(all(np.array_equal(e.predict_grad(X[i:i + 1])[k][0], big[k][i]) for i in (0, 1, 19999) for k in big))
    import grad_ref as G
    Psi2, C = e.download('PSI2_SUM'), e.download('PSI1TY')
    t = time.perf_counter()
    ref = G.grad(d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2, C, X[:1000])
    out['host_numpy_n1000'] = {'ms': (time.perf_counter() - t) * 1e3, 'threads': os.environ.get('OMP_NUM_THREADS', 'default')}
    out['max_rel_diff_to_host_numpy'] = {k: float(np.max(np.abs(big[k][:1000] - ref[k])) / np.max(np.abs(ref[k]))) for k in ref}
    e.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
