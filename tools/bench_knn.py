#!/usr/bin/env python3
"""Time the neighbour search in latent space (gp_knn_rows, ShardEngine.knn_rows) and print one JSON line.

Normal data, Q = 10, k = 10 (--Q, --k); per N of --N (default 1e5 and 1e6) a dict under 'N<N>' with
  all_pairs_s              wall seconds of one synchronous all-pairs search on the resident rows, every row without itself (bit 0): N^2 Q terms,
                           best of --reps after one warm-up
  all_pairs_weighted_s     the same in a weighted metric (one more multiplication per term)
  terms_per_s              N^2 Q over all_pairs_s
  host_queries_s           --n (default 1e4) host queries against the resident rows (their upload included)
  ckdtree_build_s          scipy.spatial.cKDTree over the same rows on this host
  ckdtree_query_s          its query (k + 1 neighbours, the first being the row itself) for --tree-queries (default 2000) of the rows, and
  ckdtree_all_pairs_s      that time scaled to all N rows
  lists_differ             of the tree's queries, the neighbour lists (row indices) that differ from the device's
  device_faster            all_pairs_s < ckdtree_build_s + ckdtree_all_pairs_s: the figure that counts, same run, same box
Work model: n n_train Q terms, a subtraction and an fma each (and a multiplication with weights): 2 n n_train Q FP64 VALU lane-slots, plus a
comparison per pair; the insertion into a list is rare (k / rows seen)."""
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
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--N', type=str, default='100000,1000000')
    ap.add_argument('--Q', type=int, default=10)
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--tree-queries', type=int, default=2000)
    ap.add_argument('--no-host', action='store_true', help='skip the host tree')
    args = ap.parse_args()
    from gparml_amd.engine import ShardEngine
    Q, k = args.Q, args.k
    out = {'Q': Q, 'k': k}
    for N in [int(float(v)) for v in args.N.split(',')]:
        rs = np.random.RandomState(N % 1000 + Q)
        X = rs.randn(N, Q)
        Xq = rs.randn(args.n, Q)
        w = 0.5 + rs.rand(Q)
        eng = ShardEngine(N, 1, 2, Q)
        eng.upload_shard(np.zeros((N, 1)), X, np.zeros((N, Q)))
        r = {}
        try:
            r['all_pairs_s'] = timed(lambda: eng.knn_rows(None, k, skip_self=True), args.reps)
            r['all_pairs_weighted_s'] = timed(lambda: eng.knn_rows(None, k, weight=w, skip_self=True), args.reps)
            r['terms_per_s'] = float(N) * N * Q / r['all_pairs_s']
            r['host_queries_s'] = timed(lambda: eng.knn_rows(Xq, k), args.reps)
            rows = eng.knn_rows(None, k, skip_self=True)[1]
        finally:
            eng.close()
        if not args.no_host:
            from scipy.spatial import cKDTree
            t = time.perf_counter()
            tree = cKDTree(X)
            r['ckdtree_build_s'] = time.perf_counter() - t
            sel = rs.choice(N, size=min(args.tree_queries, N), replace=False)
            t = time.perf_counter()
            idx = tree.query(X[sel], k=k + 1)[1]
            r['ckdtree_query_s'] = time.perf_counter() - t
            r['ckdtree_queries'] = int(len(sel))
            r['ckdtree_all_pairs_s'] = r['ckdtree_query_s'] * N / len(sel)
            # the tree returns the row itself first (distance zero); the device left it out
            r['lists_differ'] = int(np.any(idx[:, 1:] != rows[sel], axis=1).sum())
            r['device_faster'] = bool(r['all_pairs_s'] < r['ckdtree_build_s'] + r['ckdtree_all_pairs_s'])
        out['N%d' % N] = r
    print(json.dumps(out))


if __name__ == '__main__':
    main()
