#!/usr/bin/env python3
"""Time gp_infer_objective and gp_infer_latent (latent inference for new rows) and print one JSON line.

n = 1e4 new rows at configs[2]'s model (M 512, Q 10, D 100), all columns observed.  Times are wall milliseconds of one synchronous call (host
copies included), best of --reps after one warm-up: one objective evaluation with gradients, and one gp_infer_latent call of --iters iterations
(gtol 0: every row runs them all; an iteration is up to two evaluations).  Work model: n M^2 (Q + 17) / 2 FP64 VALU
lane-slots per evaluation, the exponent and exp of half the pairs, as for pred_psi2w_kernel; the fraction is against the 74 TF VALU FMA rate
(37e12 lane-slots per second)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

PEAK_TF = 74.0


def main():
    from bench_predict import model, timed
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--iters', type=int, default=20)
    args = ap.parse_args()
    M, Q, D, n = 512, 10, 100, args.n
    e = model(M, Q, D)
    rs = np.random.RandomState(0)
    X, S = rs.randn(n, Q), rs.uniform(0.05, 0.5, size=(n, Q))
    Y = rs.randn(n, D)
    slots = float(n) * M * M * (Q + 17) / 2.0
    frac = lambda ms, evals: evals * slots * 2.0 / (ms * 1e-3) / (PEAK_TF * 1e12)
    ms_obj = timed(lambda: e.infer_objective(Y, X, S), args.reps)
    res = []
    ms_lat = timed(lambda: res.append(e.infer_latent(Y, X, S, max_iters=args.iters, gtol=0.0)), args.reps)
    it = res[-1][3]
    out = {'peak_tf': PEAK_TF, 'n': n, 'M': M, 'Q': Q, 'D': D, 'valu_lane_slots_per_evaluation': slots,
           'objective': {'ms': ms_obj, 'frac_peak': frac(ms_obj, 1)},
           'latent': {'ms': ms_lat, 'max_iters': args.iters, 'mean_iters': float(it.mean()), 'ms_per_iteration': ms_lat / args.iters,
                      'frac_peak_at_two_evaluations_per_iteration': frac(ms_lat, 2 * args.iters + 1)}}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
