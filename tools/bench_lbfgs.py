#!/usr/bin/env python3
"""Time the resident L-BFGS history (gp_lbfgs_*, csrc/lbfgs.hip) and print one JSON line.

Per m in (10, 32), at N = 1e6 rows, Q = 10 (2e7 doubles, 160 MB a vector), every slot filled:
  dots_wall_s, direction_wall_s    wall seconds of one gp_lbfgs_dots(slot) / one gp_lbfgs_direction(dense coefficients) with the stream drained, best of
                                   --reps after a warm-up (the library records no device events around these calls: device time is not reported)
  dots_bytes, direction_bytes      the byte model: (2m + 1 + 3 ceil((2m + 1) / 16)) vectors read / (2m + 1) read and one written
  dots_hbm_fraction, ...           bytes / seconds over --hbm-GBps (default 8000, the MI355X's nominal rate)
  numpy_dots_s, numpy_direction_s  the same algebra in numpy on this host (--numpy-N rows, scaled to N)
On a mid-size GPLVM (N = 2e4, D = 20, M = 64, Q = 5, fixed seed): evaluations and seconds LBFGS, SCG_adapted and GD take to reach the bound SCG has after
50 iterations.  No figure is a pass/fail threshold: the exit status is 0 whenever everything ran."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Reached(Exception):
    pass


def passes(args, out):
    import torch
    from gparml_amd.engine import ShardEngine
    N, Q = args.N, args.Q
    rs = np.random.RandomState(0)
    eng = ShardEngine(N, 1, 4, Q)
    eng.upload_shard(rs.randn(N, 1), rs.randn(N, Q), np.zeros((N, Q)), xs_is_raw=True)
    eng.set_globals(rs.randn(4, Q), 1.0, np.ones(Q), 1.0, N_global=N)
    eng.phase1(); eng.global_step(); eng.phase2(True); eng.finish()
    eng.set_direction(rs.randn(2, N, Q))

    def timed(fn):
        fn(); torch.cuda.synchronize()
        best = float('inf')
        for _ in range(max(1, args.reps)):
            t = time.perf_counter()
            fn(); torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t)
        return best

    vec = 16.0 * N * Q
    for m in (10, 32):
        W = 2 * m + 1
        eng.lbfgs_begin(m)
        eng.lbfgs_grad()
        for k in range(m):
            eng.lbfgs_push(k, 0.5)
        coef = rs.randn(W)
        r = {'dots_wall_s': timed(lambda: eng.lbfgs_dots(0)), 'direction_wall_s': timed(lambda: eng.lbfgs_direction(coef)),
             'dots_bytes': vec * (W + 3 * ((W + 15) // 16)), 'direction_bytes': vec * (W + 1), 'history_bytes': vec * W}
        for k in ('dots', 'direction'):
            r[k + '_hbm_fraction'] = r[k + '_bytes'] / r[k + '_wall_s'] / (args.hbm_GBps * 1e9)
        eng.lbfgs_end()
        n = args.numpy_N
        B = rs.randn(W, 2 * n * Q)
        t = time.perf_counter(); B[[0, m, 2 * m]] @ B.T; r['numpy_dots_s'] = (time.perf_counter() - t) * N / n
        t = time.perf_counter(); coef @ B; r['numpy_direction_s'] = (time.perf_counter() - t) * N / n
        out['m%d' % m] = r
    eng.close()


def optimisers(args, out):
    from gparml_amd.gd import GD
    from gparml_amd.lbfgs import LBFGS
    from gparml_amd.resident import ResidentCG, ResidentGD, ResidentLBFGS, ResidentModel
    from gparml_amd.scg_adapted import SCG_adapted
    N, D, M, Q = args.gplvm
    rs = np.random.RandomState(1)
    X = rs.randn(N, Q)
    Y = np.tanh(X @ rs.randn(Q, D)) + 0.1 * rs.randn(N, D)
    X_mu, X_S = X + 0.3 * rs.randn(N, Q), np.full((N, Q), -1.0)
    x0 = np.concatenate([X_mu[rs.choice(N, M, replace=False)].ravel(), [1.0], np.ones(Q), [2.0]])

    def run(opt, ops_class, target, **kw):
        model = ResidentModel([(Y, X_mu, X_S)], M, Q, D)
        count, t0 = [0], time.perf_counter()

        def f(x, it, step=0):
            v, g = model.likelihood_and_gradient(x, it, step)
            count[0] += 1
            if target is not None and v <= target:
                raise Reached()
            return v, g
        flog, status = None, 'reached'
        try:
            _, flog, _, status = opt(f, x0.copy(), ops_class(model), xtol=0, ftol=0, gtol=0, max_f_eval=args.max_evals, **kw)
            reached = target is None
        except Reached:
            reached = True
        s = time.perf_counter() - t0
        model.close()
        return {'evaluations': count[0], 'seconds': s, 'reached': reached, 'status': status}, flog

    scg, flog = run(SCG_adapted, ResidentCG, None, maxiters=50)
    target = float(flog[-1])
    out['gplvm'] = {'N': N, 'D': D, 'M': M, 'Q': Q, 'target_after_50_scg_iterations': target, 'scg': scg,
                    'lbfgs': run(LBFGS, ResidentLBFGS, target, maxiters=args.max_evals, m=10)[0],
                    'gd': run(GD, ResidentGD, target, maxiters=args.max_evals)[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--N', type=int, default=1000000)
    ap.add_argument('--Q', type=int, default=10)
    ap.add_argument('--numpy-N', type=int, default=100000)
    ap.add_argument('--hbm-GBps', type=float, default=8000.0)
    ap.add_argument('--gplvm', type=int, nargs=4, default=[20000, 20, 64, 5], metavar=('N', 'D', 'M', 'Q'))
    ap.add_argument('--max-evals', type=int, default=400)
    ap.add_argument('--skip', choices=['passes', 'optimisers'], default=None)
    args = ap.parse_args()
    out = {'N': args.N, 'Q': args.Q}
    if args.skip != 'passes':
        passes(args, out)
    if args.skip != 'optimisers':
        optimisers(args, out)
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
