#!/usr/bin/env python3
"""Every entry point at new inputs, once, with all outputs written to one .npz -- to compare two builds of the library bit for bit.

    GPARML_LIB=$PWD/gparml_amd/lib_parent.so.bin python3 tools/dump_new_inputs.py --out /tmp/parent.npz
    python3 tools/dump_new_inputs.py --out /tmp/intree.npz
    python3 tools/dump_new_inputs.py --compare /tmp/parent.npz /tmp/intree.npz

Shapes where the shared chunk pipeline can go wrong rather than the workload's: N = 300, M = 40 (Mp = 128), chunks of predict_rows = 128 points and
n = 130 of them (a full chunk and a ragged one).  Models (Q, D): (3, 5), (20, 5), (70, 5) for the 16-wide, 64-wide and run-time latent paths and
(3, 130) for two column tiles of the uncertain-input variance; each trained for three evaluations from one fixed seed.  Per model: gp_predict
(deterministic, actual and raw X_S; mean only, var only, both; with and without the noise), gp_predict_score (host rows with and without a mask,
the resident rows with and without their variances), gp_predict_joint and gp_predict_sample (3 draws), gp_predict_grad (all outputs; logdet only
at Q <= 64, the entry's own limit), gp_paths_set / gp_paths_eval (F = 8, 2 draws, n = 130 and n = 1), gp_curve_energy (5 curves of T = 7, two
curves per chunk, all outputs).  One fixed-embedding model, (3, 5), for the scoring passes gp_predict_score and gp_loo_score share: gp_loo_score at
block 1, 5, 64 and 128 (with and without a mask, flags 0 and 1), gp_predict_score on the resident rows (with and without a mask), each at the
default chunk and at chunks of 128 rows, and gp_predict at deterministic inputs.  --compare takes the arrays as bytes: NaN positions and signs of zero count."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, M, n = 300, 40, 130
MODELS = ((3, 5), (20, 5), (70, 5), (3, 130))


def trained_engine(Q, D, regime='B'):
    from oracle import factorised as Fz
    from gparml_amd.engine import ShardEngine
    d = Fz.synthetic_shard(N, D, M, Q, regime=regime, seed=11, zseed=12, alpha_value=0.5)
    e = ShardEngine(N, D, M, Q)
    e.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    Z, alpha = d['Z'].copy(), np.asarray(d['alpha'], dtype=np.float64).reshape(-1).copy()
    for _ in range(3):          # a few steps along the gradient: the model the predictions see is not the synthetic starting point
        e.set_globals(Z, d['sf2'], alpha, d['beta'])
        e.phase1()
        e.global_step(sync=True)
        e.phase2(False)
        g = e.finish()
        Z = Z + 1e-4 * g['grad_Z'] / max(1.0, np.abs(g['grad_Z']).max())
    e.set_globals(Z, d['sf2'], alpha, d['beta'])
    e.phase1()
    e.global_step(sync=True)
    return e, d


def predict_raw(e, X, S, raw, noise, want_mean, want_var):
    """gp_predict itself: ShardEngine.predict always asks for both outputs."""
    from gparml_amd import _lib
    dp = lambda a: a.ctypes.data_as(_lib._dp) if a is not None else None          # noqa: E731
    mean = np.full((X.shape[0], e.D), -7.0) if want_mean else None
    var = np.full((X.shape[0], 1 if S is None else e.D), -7.0) if want_var else None
    e._ck(e.lib.gp_predict(e.h, X.shape[0], dp(X), dp(S), raw, noise, dp(mean), dp(var)), 'gp_predict')
    return mean, var


def dump_model(Q, D, out):
    e, d = trained_engine(Q, D)
    tag = 'Q%d_D%d/' % (Q, D)
    rs = np.random.RandomState(100 * Q + D)
    X = np.ascontiguousarray(rs.randn(n, Q))
    S = np.ascontiguousarray(rs.uniform(0.05, 0.5, size=(n, Q)))
    Sraw = np.ascontiguousarray(np.log(np.expm1(S)))
    for kind, s, raw in (('det', None, 0), ('unc', S, 0), ('raw', Sraw, 1)):
        for noise in (0, 1):
            for which, (wm, wv) in (('mean', (True, False)), ('var', (False, True)), ('both', (True, True))):
                mean, var = predict_raw(e, X, s, raw, noise, wm, wv)
                key = tag + 'predict/%s/noise%d/%s/' % (kind, noise, which)
                if wm:
                    out[key + 'mean'] = mean
                if wv:
                    out[key + 'var'] = var
    Y = np.ascontiguousarray(rs.randn(n, D))
    mask = rs.uniform(size=(n, D)) < 0.7
    mask[:, 0] = True
    cases = (('host', dict(Y=Y, X_mu=X)), ('host_unc', dict(Y=Y, X_mu=X, X_S=S)), ('host_mask', dict(Y=Y, X_mu=X, observed=mask)),
             ('host_unc_mask', dict(Y=Y, X_mu=X, X_S=S, observed=mask)), ('resident', dict(Y=None)), ('resident_S', dict(Y=None, use_resident_S=True)))
    for name, kw in cases:
        r = e.score(**kw)
        for k in ('row_logp', 'row_sse', 'row_chi2', 'cols'):
            out[tag + 'score/%s/%s' % (name, k)] = r[k]
    out[tag + 'joint/mean'], out[tag + 'joint/cov'] = e.predict_joint(X, include_noise=True)
    eps = rs.randn(3, n, D)
    out[tag + 'sample/draws'], out[tag + 'sample/mean'] = e.predict_sample(X, 3, include_noise=True, eps=eps)
    for k, v in e.predict_grad(X, logdet=Q <= 64).items():
        out[tag + 'grad/' + k] = v
    F = 8
    e.paths_set(rs.randn(F, Q) * np.sqrt(0.5), rs.randn(2, 2 * F, D), rs.randn(2, M, D), centre=rs.randn(Q))
    out[tag + 'paths/n130'], out[tag + 'paths/n130_mean'] = e.paths_eval(X, want_mean=True)
    out[tag + 'paths/n1'], out[tag + 'paths/n1_mean'] = e.paths_eval(X[7:8], want_mean=True)
    e.paths_clear()
    curves = np.cumsum(0.1 * rs.randn(5, 7, Q), axis=1)
    for k, v in e.curve_energy(curves, want_energy=True, want_segments=True, want_grad=True).items():
        out[tag + 'curve/' + k] = v
    e.close()


def dump_fixed(lib, out):
    """The fixed-embedding model (Q, D) = (3, 5) and the scoring passes gp_predict_score and gp_loo_score share (csrc/score_pass.h), at the default
    chunk and at chunks of 128 rows: 300 rows are three segments with a ragged last one; block 5 makes chunks of 125 rows, block-aligned but not
    segment-aligned, so rows wait in the window for the next chunk's."""
    Q, D = 3, 5
    e, d = trained_engine(Q, D, regime='A')
    tag = 'fixed_Q%d_D%d/' % (Q, D)
    rs = np.random.RandomState(100 * Q + D + 1)
    X = np.ascontiguousarray(rs.randn(n, Q))
    for noise in (0, 1):
        out[tag + 'predict/det/noise%d/mean' % noise], out[tag + 'predict/det/noise%d/var' % noise] = predict_raw(e, X, None, 0, noise, True, True)
    mask = rs.uniform(size=(N, D)) < 0.7
    mask[:, 0] = True
    mask[129] = False
    for rows in (0, 128):
        assert lib.gp_debug_set_option(b'predict_rows', rows) == 0
        for mname, obs in (('full', None), ('mask', mask)):
            r = e.score(None, observed=obs)
            for k in ('row_logp', 'row_sse', 'row_chi2', 'cols'):
                out[tag + 'score/resident_%s/chunk%d/%s' % (mname, rows, k)] = r[k]
            for block in (1, 5, 64, 128):
                for noise in (0, 1):
                    try:
                        r = e.loo(block=block, observed=obs, include_noise=bool(noise))
                    except (FloatingPointError, np.linalg.LinAlgError) as err:      # the outputs are compared all the same, NaN rows included
                        r = err.result
                    for k in ('row_logp', 'row_sse', 'row_chi2', 'lev', 'var_loo', 'cols'):
                        out[tag + 'loo/block%d/%s/flags%d/chunk%d/%s' % (block, mname, noise, rows, k)] = r[k]
    e.close()


def compare(a, b):
    A, B = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(B.files), 'different arrays: %s' % sorted(set(A.files) ^ set(B.files))
    bad = [k for k in A.files if A[k].shape != B[k].shape or A[k].dtype != B[k].dtype or A[k].tobytes() != B[k].tobytes()]
    for k in bad:
        print('DIFFERS', k, A[k].shape, B[k].shape)
    print('%d arrays compared, %d differ, %d bytes in all' % (len(A.files), len(bad), sum(A[k].nbytes for k in A.files)))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--compare', nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    from gparml_amd import _lib
    lib = _lib.load()
    assert lib.gp_debug_set_option(b'predict_rows', 128) == 0 and lib.gp_debug_set_option(b'curve_curves', 2) == 0
    out = {}
    for Q, D in MODELS:
        dump_model(Q, D, out)
        print('model Q = %d, D = %d: %d arrays so far' % (Q, D, len(out)), flush=True)
    dump_fixed(lib, out)
    print('fixed-embedding model: %d arrays so far' % len(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez(args.out, **out)
    print('wrote %d arrays to %s (library: %s)' % (len(out), args.out, _lib.LIB_PATH))


if __name__ == '__main__':
    main()
