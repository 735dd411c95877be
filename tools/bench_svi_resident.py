#!/usr/bin/env python3
"""Time minibatch training from the resident shard (gp_gather_shard, gparml_amd.svi.ResidentSVI) and print one JSON line.

Model: M 512, Q 10, D 100, batches of |B| = 1e4 of N = 1e6 resident rows.  In one process, wall milliseconds of synchronous calls, best of --reps
after one warm-up:

  gather_ms                 gp_gather_shard of one batch (unsorted rows) -- the whole call: index upload, the two kernels, sum_YYT and its read-back
  gather_call_share_of_hbm  the bytes the rows themselves need, 8 n (2 Dp + 4 Q), over gather_ms, as a share of the 8 TB/s HBM peak: a whole-call
                            rate, not a kernel's share of peak (the call also writes and reads the dense copy for sum_YYT and waits for the host)
  upload_ms                 gp_upload_shard of the same rows from host arrays that are already contiguous (the fancy indexing is not timed) ...
  host_rows_ms              ... and that indexing, Y[idx], X[idx], which SVI.step pays as well
  resident_iteration_ms     one ResidentSVI.step(learn=True) with fixed embeddings
  host_iteration_ms         one SVI.step(learn=True) on the same data and options, its upload included: the comparison that counts
  free_iteration_ms         one ResidentSVI.step(learn=True) with free embeddings (local step and scatter included)

A missing GPU is an error, not a fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12      # bytes / s


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
    ap.add_argument('--M', type=int, default=512)
    args = ap.parse_args()
    from oracle import factorised as Fz
    from gparml_amd.engine import ShardEngine
    from gparml_amd.svi import SVI, ResidentSVI
    M, Q, D, N, B = args.M, 10, 100, args.N, args.batch
    d = Fz.synthetic_shard(N, D, M, Q, regime='A', seed=2, zseed=3)
    opts = dict(Z=d['Z'], sf2=d['sf2'], alpha=d['alpha'], beta=d['beta'], batch=B, seed=1)
    out = {'M': M, 'Q': Q, 'D': D, 'N': N, 'batch': B, 'reps': args.reps}
    full = ShardEngine(N, D, M, Q)
    full.set_timing(0)
    full.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    b = ShardEngine(B, D, M, Q)
    b.set_timing(0)
    idx = np.random.RandomState(4).permutation(N)[:B]
    Dp = (D + 127) // 128 * 128
    out['gather_bytes'] = 8 * B * (2 * Dp + 4 * Q)
    out['gather_ms'] = timed(lambda: b.gather_from(full, idx), args.reps)
    out['gather_call_share_of_hbm'] = out['gather_bytes'] / (out['gather_ms'] * 1e-3) / HBM_PEAK
    rows = {}

    def host_rows():
        rows['Y'], rows['X'], rows['S'] = d['Y'][idx], d['X_mu'][idx], d['X_S'][idx]
    out['host_rows_ms'] = timed(host_rows, args.reps)
    out['upload_ms'] = timed(lambda: b.upload_shard(rows['Y'], rows['X'], rows['S']), args.reps)
    b.close()
    # the two drivers, alternating, so that both see the same machine
    res = ResidentSVI(full, opts)
    host = SVI(lambda n: ShardEngine(n, D, M, Q), d['Y'], d['X_mu'], opts)
    for e in (res.eng, host.eng):
        e.set_timing(0)
    best = {'resident_iteration_ms': float('inf'), 'host_iteration_ms': float('inf')}
    for r in range(args.reps + 1):
        for key, drv in (('resident_iteration_ms', res), ('host_iteration_ms', host)):
            t = time.perf_counter()
            drv.step(0.5, learn=True)
            if r:
                best[key] = min(best[key], (time.perf_counter() - t) * 1e3)
    out.update(best)
    out['resident_over_host'] = out['resident_iteration_ms'] / out['host_iteration_ms']
    res.close()
    host.close()
    # free embeddings: the same shard with variances of 0.5, stored raw
    full.upload_embeddings(d['X_mu'], np.full((N, Q), np.log(np.expm1(0.5))), xs_is_raw=True)
    free = ResidentSVI(full, dict(opts, lr_x=1e-3))
    free.eng.set_timing(0)
    out['free_iteration_ms'] = timed(lambda: free.step(0.5, learn=True), args.reps)
    free.close()
    full.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
