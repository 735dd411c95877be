#!/usr/bin/env python3
"""Time one SVI iteration (gp_svi_*) and print one JSON line.

Model: M 512, Q 10, D 100, fixed embeddings, batches of |B| = 1e4 of N = 1e6 rows.  In one process: the whole iteration on a batch-sized context
(set_globals, phase 1, scale, gp_svi_natural_step, gp_svi_step, phase 2, scale, finish: ``svi_iteration_ms``), gp_svi_natural_step + gp_svi_step
alone as training runs them, on statistics that changed since the last step, so that K_mm, its factorisation and the whitening products are
recomputed every time (``svi_steps_ms``; the change is a scale_stats(1.0), one elementwise launch over the statistics that is inside the
figure), the same two steps on unchanged statistics, where that front is kept (``svi_steps_front_kept_ms``), gp_global_step on the
same context (``global_step_ms``) and one full-data collapsed evaluation at N = 1e6 (``full_evaluation_ms``).  Times are wall milliseconds of
synchronous sequences, best of --reps after one warm-up.  ``steps_over_global`` = svi_steps_ms / global_step_ms, like for like: both build and
factorise K_mm; above 3 it is a finding to be broken down by kernel with a profiler."""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--N', type=int, default=1000000)
    ap.add_argument('--batch', type=int, default=10000)
    args = ap.parse_args()
    from oracle import factorised as Fz
    from gparml_amd.engine import ShardEngine
    M, Q, D, N, B = 512, 10, 100, args.N, args.batch
    d = Fz.synthetic_shard(N, D, M, Q, regime='A', seed=2, zseed=3)
    g = (d['Z'], d['sf2'], d['alpha'], d['beta'])
    b = ShardEngine(B, D, M, Q)
    b.set_timing(0)
    b.upload_shard(d['Y'][:B], d['X_mu'][:B], d['X_S'][:B])
    b.svi_begin()
    scale = float(N) / B

    def iteration():
        b.set_globals(*g, N_global=N)
        b.phase1()
        b.scale_stats(scale)
        b.svi_natural_step(0.5)
        b.svi_step(sync=False)
        b.phase2(False)
        b.scale_buffer('grads', scale)
        b.finish()

    def steps():
        b.scale_stats(1.0)              # the statistics changed: the front is computed again, as in every training iteration
        b.svi_natural_step(0.5)
        b.svi_step(sync=True)

    def steps_front_kept():
        b.svi_natural_step(0.5)
        b.svi_step(sync=True)

    def collapsed_step():
        b.global_step(sync=True)
    out = {'M': M, 'Q': Q, 'D': D, 'N': N, 'batch': B, 'reps': args.reps}
    out['svi_iteration_ms'] = timed(iteration, args.reps)
    b.set_globals(*g, N_global=N)
    b.phase1()
    b.scale_stats(scale)
    out['svi_steps_ms'] = timed(steps, args.reps)
    out['svi_steps_front_kept_ms'] = timed(steps_front_kept, args.reps)
    out['global_step_ms'] = timed(collapsed_step, args.reps)
    out['steps_over_global'] = out['svi_steps_ms'] / out['global_step_ms']
    b.svi_end()
    b.close()
    e = ShardEngine(N, D, M, Q)
    e.set_timing(0)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])

    def full():
        e.set_globals(*g)
        e.phase1()
        e.global_step(sync=False)
        e.phase2(False)
        e.finish()
    out['full_evaluation_ms'] = timed(full, args.reps)
    e.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
