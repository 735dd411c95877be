#!/usr/bin/env python3
"""Time gp_loo_score (exact leave-one-out / leave-block-out scoring of the resident rows) and print one JSON line.

Model: M 512, Q 10, D 100, fixed embeddings, N = 1e6 resident rows (the headline regression workload).  In one process on one engine:
gp_loo_score at block = 1, 8 and 128; gp_predict_score on the same resident rows (the comparison that counts: ``ratio_to_score``); and one global
step, whose time multiplied by N is the brute-force figure of one refit per row (the refits' own phase 1 not even counted).  Times are wall
milliseconds of one synchronous call, best of --reps after one warm-up."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--N', type=int, default=1000000)
    args = ap.parse_args()
    from oracle import factorised as Fz
    from gparml_amd.engine import ShardEngine
    M, Q, D, N = 512, 10, 100, args.N
    d = Fz.synthetic_shard(N, D, M, Q, regime='A', seed=2, zseed=3)
    e = ShardEngine(N, D, M, Q)
    e.set_timing(0)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    e.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    e.phase1()
    step_ms = timed(lambda: e.global_step(sync=True), args.reps)
    out = {'M': M, 'Q': Q, 'D': D, 'N_resident': N, 'reps': args.reps}
    keep = {}
    score_ms = timed(lambda: keep.__setitem__('score', e.score(None)), args.reps)
    out['predict_score_ms'] = score_ms
    out['global_step_ms'] = step_ms
    out['refit_per_row_s'] = step_ms * 1e-3 * N
    for block in (1, 8, 128):
        ms = timed(lambda: keep.__setitem__(block, e.loo(block=block)), args.reps)
        r = keep[block]
        out['loo_block_%d' % block] = {'ms': ms, 'ratio_to_score': ms / score_ms, 'nlpd_pooled': float(r['pooled']['nlpd']),
                                       'rmse_pooled': float(r['pooled']['rmse']), 'max_lev': float(np.max(r['lev']))}
    out['nlpd_pooled_training_score'] = float(keep['score']['pooled']['nlpd'])
    e.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
