#!/usr/bin/env python3
"""Time gp_curve_energy (expected energy of discrete curves under the posterior of f, and its gradient) and print one JSON line.

Model: configs[2]'s shape (M 512, Q 10, D 100), tools/bench_joint.py's generator.  1000 curves of T = 64 points (random walks of 0.1 length scales per
step): the energy alone, and the energy with its gradient.  Times are wall milliseconds of one synchronous ShardEngine call (host copies of inputs and
outputs included), best of --reps after one warm-up.  The kernels' own times are not measured here: take them from a separate
    rocprofv3 --kernel-trace --stats -- python tools/bench_curve.py --reps 1
run.  Work model, S = n_curves (T - 1), Mp / Dp = M / D rounded up to 128:
  2 S Mp (Dp + 2 Mp) MFMA flop for the energy (the two forward products), twice that with the gradient (the three back-products)
fraction of peak against 74 TF (FP64 4x4x4 MFMA rate, mma_f64.h), of the WHOLE call.  `alone_bits_equal`: the first, second and last curve of the
batch, evaluated alone, carry the batch's bits.  host_numpy: tests/curve_ref.py's float64 form on 16 of the curves with numpy on this host.
geodesic: one Predictor-style solve (gparml_amd.predict.minimise_curves on this engine) of 100 pairs of end points two length scales apart, T = 32,
at most --iterations L-BFGS-B iterations, with its count of function evaluations (one device call each)."""
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


def work(n_curves, T, M, D, grad):
    up = lambda x: -(-x // 128) * 128
    return (2.0 if grad else 1.0) * 2.0 * n_curves * (T - 1) * up(M) * (up(D) + 2 * up(M))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--iterations', type=int, default=50)
    args = ap.parse_args()
    from gparml_amd.predict import minimise_curves, straight_curves
    rs = np.random.RandomState(0)
    out = {'peak_tf': PEAK_TF, 'kernel_ms': 'not measured (rocprofv3 --kernel-trace --stats)'}
    M, Q, D = 512, 10, 100
    e, d = model(M, Q, D)
    ls = 1.0 / np.sqrt(d['alpha'])
    n, T = 1000, 64
    X = rs.randn(n, 1, Q) + np.cumsum(0.1 * rs.randn(n, T, Q) * ls, axis=1)
    for name, grad in (('energy_n1000_T64', False), ('energy_grad_n1000_T64', True)):
        ms = timed(lambda: e.curve_energy(X, want_segments=False, want_grad=grad), args.reps)
        flop = work(n, T, M, D, grad)
        out[name] = {'ms': ms, 'mfma_flop': flop, 'frac_peak_whole_call': flop / (ms * 1e-3) / (PEAK_TF * 1e12)}
    big = e.curve_energy(X, want_segments=True)
    out['alone_bits_equal'] = bool(all(np.array_equal(e.curve_energy(X[i:i + 1], want_segments=True)[k][0], big[k][i]) for i in (0, 1, n - 1) for k in big))
    import curve_ref as CR
    Psi2, C = e.download('PSI2_SUM'), e.download('PSI1TY')
    t = time.perf_counter()
    ref = CR.curve(d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2, C, X[:16])
    out['host_numpy_n16_T64'] = {'ms': (time.perf_counter() - t) * 1e3, 'threads': os.environ.get('OMP_NUM_THREADS', 'default')}
    out['max_rel_diff_to_host_numpy'] = {k: float(np.max(np.abs(big[k][:16] - ref[k])) / np.max(np.abs(ref[k]))) for k in ref}
    x0 = rs.randn(100, Q)
    u = rs.randn(100, Q)
    x1 = x0 + 2.0 * ls * u / np.sqrt(np.sum(u * u, axis=1))[:, None]
    start = straight_curves(x0, x1, 32)

    def f(Y):
        r = e.curve_energy(Y)
        return r['energy'], r['grad']
    t = time.perf_counter()
    curves, info = minimise_curves(f, start, iterations=args.iterations)
    ms = (time.perf_counter() - t) * 1e3
    end = e.curve_energy(curves, want_grad=False)['energy']
    out['geodesic_100_pairs_T32'] = {'ms': ms, 'evaluations': info['evaluations'], 'ms_per_evaluation': ms / max(1, info['evaluations']),
                                     'energy_over_straight_line_mean': float(np.mean(end / info['energy0'])), 'message': info['message']}
    e.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
