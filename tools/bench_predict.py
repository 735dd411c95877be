#!/usr/bin/env python3
"""Time gp_predict (posterior predictive mean and variance) and print one JSON line.

deterministic: n = 1e5 and 1e6 points at configs[2]'s model (M 512, Q 10, D 100); uncertain: n = 1e4 at configs[2]'s model and n = 1e3 at
configs[4]'s (M 1024, Q 50, D 1000).  Times are wall milliseconds of one synchronous ShardEngine.predict call (host copies of inputs and outputs
included), best of --reps after one warm-up.  Work models:
  deterministic   2 n M (D + 2 M) MFMA flop  (Psi1* [beta E | Lk^-T | La^-T])
  uncertain       2 n M^2 (D + 1) MFMA flop (psi2* W and the trace; the kernel issues 2 n M^2 D_p, D_p = D rounded up to 128, reported as
                  *_issued) + n M^2 (Q + 17) FP64 VALU lane-slots (exponent and exp)
fraction of peak against 74 TF (FP64 4x4x4 MFMA / VALU FMA rate, mma_f64.h); the uncertain one counts MFMA and VALU work on the one pipe they share."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TF = 74.0


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
    return e


def timed(fn, reps):
    fn()
    best = float('inf')
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    rs = np.random.RandomState(0)
    out = {'peak_tf': PEAK_TF, 'peak': 'FP64 v_mfma_f64_4x4x4_4b_f64 = FP64 VALU FMA rate (mma_f64.h)'}
    M, Q, D = 512, 10, 100
    e = model(M, Q, D)
    for n in (100000, 1000000):
        X = rs.randn(n, Q)
        ms = timed(lambda: e.predict(X), args.reps)
        fl = 2.0 * n * M * (D + 2 * M)
        out['det_n%d' % n] = {'ms': ms, 'flop': fl, 'tflops': fl / ms * 1e-9, 'frac_peak': fl / ms * 1e-9 / PEAK_TF}
    runs = [(e, M, Q, D, 10000)]
    e4 = model(1024, 50, 1000, N=3000)
    runs.append((e4, 1024, 50, 1000, 1000))
    for eng, M, Q, D, n in runs:
        X, S = rs.randn(n, Q), rs.uniform(0.05, 0.5, size=(n, Q))
        ms = timed(lambda: eng.predict(X, S), args.reps)
        Dp = -(-D // 128) * 128
        fl = 2.0 * n * M * M * (D + 1)          # useful work: psi2 W and the trace (the issue's model)
        fl_issued = 2.0 * n * M * M * Dp        # what the kernel issues: the column tiles are 128 wide
        valu = float(n) * M * M * (Q + 17)
        frac = lambda f: (f / 2.0 + valu) * 2.0 / (ms * 1e-3) / (PEAK_TF * 1e12)    # FMA-equivalents on the shared FP64 pipe
        out['unc_M%d_Q%d_D%d_n%d' % (M, Q, D, n)] = {'ms': ms, 'mfma_flop': fl, 'mfma_flop_issued': fl_issued, 'valu_lane_slots': valu,
                                                     'frac_peak': frac(fl), 'frac_peak_issued': frac(fl_issued)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
