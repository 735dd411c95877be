#!/usr/bin/env python3
"""Time gp_infer_objective and gp_infer_latent (latent inference for new rows) and print one JSON line.

n = 1e4 new rows at configs[2]'s model (M 512, Q 10, D 100), all columns observed.  Times are wall milliseconds of one synchronous call (host
copies included), best of --reps after one warm-up: one objective evaluation with gradients, and one gp_infer_latent call of --iters iterations
(gtol 0: every row runs them all; an iteration is up to two evaluations).  Work model: n M^2 (Q + 17) / 2 FP64 VALU
lane-slots per evaluation, the exponent and exp of half the pairs, as for pred_psi2w_kernel; the fraction is against the 74 TF VALU FMA rate
(37e12 lane-slots per second).

The ragged keys time gp_infer_objective_rows / gp_infer_latent_rows on the same rows with ten random columns hidden per row by a seeded generator
(practically every row has a pattern of its own): ``ragged_objective_ms``, ``ragged_latent_ms`` (the same iterations, no early stop),
``ragged_patterns_per_chunk`` (the chunking rule of csrc/infer.hip: min(P_cap, rows per chunk, distinct patterns)), ``ragged_shared_pattern_latent_ms``
(the same rows all given ONE pattern through the new entry: the overhead of the ragged form, next to ``latent``), ``grouped_latent_ms_per_row``
(Predictor.infer(ragged=False), one device call per pattern, on the first --grouped-rows of those rows from the same starts with the same iterations,
per row) and ``gate_ragged_faster_than_grouped`` (ragged_latent_ms / n < grouped_latent_ms_per_row, same run)."""
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
    ap.add_argument('--grouped-rows', type=int, default=200)
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
    # ---- rows with holes in random places
    hide = np.random.RandomState(7)
    obs = np.ones((n, D), dtype=bool)
    for i in range(n):
        obs[i, hide.choice(D, 10, replace=False)] = False
    distinct = len({o.tobytes() for o in obs})
    assert distinct >= 0.99 * n, 'only %d distinct patterns in %d rows' % (distinct, n)
    Yn = np.where(obs, Y, np.nan)
    Mp = -(-M // 128) * 128
    rows_per_chunk = max(128, min(16384, (64 << 20) // (8 * (2 * Mp + -(-D // 128) * 128)) // 128 * 128))
    out['ragged_distinct_patterns'] = distinct
    out['ragged_patterns_per_chunk'] = min(max(1, (2 << 30) // (Mp * Mp * 8)), rows_per_chunk, distinct)
    out['ragged_objective_ms'] = timed(lambda: e.infer_objective_rows(Yn, X, S, observed=obs), args.reps)
    out['ragged_latent_ms'] = timed(lambda: e.infer_latent_rows(Yn, X, S, observed=obs, max_iters=args.iters, gtol=0.0), args.reps)
    one = np.repeat(obs[:1], n, axis=0)
    out['ragged_shared_pattern_latent_ms'] = timed(lambda: e.infer_latent_rows(Y, X, S, observed=one, max_iters=args.iters, gtol=0.0), args.reps)
    # the grouped path on a sample of those rows: the trained model's statistics go through a Predictor, as a user's would
    from oracle import factorised as Fz
    from gparml_amd.predict import Predictor
    d = Fz.synthetic_shard(4000, D, M, Q, regime='A', seed=2, zseed=3)               # bench_predict.model's generator: its Z, sf2, alpha, beta
    sc = e.scalars()
    acc = dict(sum_YYT=sc['sum_YYT'], sum_exp_K_mi_K_im=e.download('PSI2_SUM'), sum_exp_K_miY=e.download('PSI1TY'), sum_exp_K_ii=sc['sum_exp_K_ii'],
               sum_KL=sc['KL'])
    pred = Predictor(dict(Z=d['Z'], sf2=d['sf2'], alpha=d['alpha'], beta=d['beta']), acc, 4000, D)
    g = min(args.grouped_rows, n)
    ms_grouped = timed(lambda: pred.infer(Yn[:g], X_mu0=X[:g], X_S0=S[:g], iterations=args.iters, gtol=0.0), 1)
    out['grouped_rows'] = g
    out['grouped_latent_ms_per_row'] = ms_grouped / g
    out['ragged_latent_ms_per_row'] = out['ragged_latent_ms'] / n
    out['grouped_over_ragged'] = out['grouped_latent_ms_per_row'] / out['ragged_latent_ms_per_row']
    out['gate_ragged_faster_than_grouped'] = bool(out['ragged_latent_ms_per_row'] < out['grouped_latent_ms_per_row'])
    print(json.dumps(out))


if __name__ == '__main__':
    main()
