#!/usr/bin/env python3
"""Benchmark of the hot path: bound+gradient evaluations per second.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Workload at N=1: BASELINE.json configs[2]  (1 shard, N=1e6, D=100, M=512, Q=10, ARD-RBF, fixed embeddings = regime A),
the configuration the metric is quoted on.  With N>1 every rank holds its own shard of the same size (configs[3],
weak scaling) and the two per-evaluation reductions are RCCL all-reduces.  A step = one evaluation = phase 1 +
all-reduce + global step + phase 2 + all-reduce + gradient read-back, inputs resident in HBM.

A plain run sets up, warms up, times K steps and prints the JSON line.  ``--dump-outputs DIR`` also writes what the last timed step
computed as DIR/<name>.npy.  ``--full`` adds what takes runs of its own, all after the timed region: the parity against the
extended-precision truth, the global step's extended-precision cost, the int8 variant, the "extra" shapes and the CPU baseline.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FP64_PEAK_TFLOPS = 78.6   # MI355X datasheet FP64 (vector = matrix); ubench ceiling 74 (profiles/r01_ubench_f64_mfma4x4x4.txt)


def usable_cpus():
    """The CPUs this process may keep busy: its affinity mask, capped by OMP_NUM_THREADS where the environment sets it.  Not
    os.cpu_count(): on a shared host that counts every core, and OpenBLAS segfaults when several concurrent callers each ask it for
    more threads than the process has CPUs."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        n = min(n, int(os.environ.get('OMP_NUM_THREADS', '')))
    except ValueError:
        pass
    return max(1, n)


def synthetic(N, D, M, Q, seed, regime='A', z_seed=None):
    """SURVEY.md 8(d) synthetic shard; generated with numpy on the host, outside the timed region.  ``z_seed`` (None = the benchmark's
    own inducing points) draws another set of inducing points: the parity fixtures cover several (tests/golden/make_hp_truth_large.py)."""
    rs = np.random.RandomState(seed)
    X = rs.randn(N, Q)
    W = np.random.RandomState(1234).randn(Q, D)          # same map on every rank
    Y = np.sin(X.dot(W)) + 0.1 * rs.randn(N, D)
    X_mu = X + 0.05 * rs.randn(N, Q)
    X_S = np.zeros((N, Q)) if regime == 'A' else rs.uniform(0.05, 0.55, size=(N, Q))
    rz = np.random.RandomState(1 if z_seed is None else 2 * z_seed + 1)
    Z = np.random.RandomState(0 if z_seed is None else 2 * z_seed).randn(4 * M, Q)[rz.permutation(4 * M)[:M]] + 0.05 * rz.randn(M, Q)   # same Z on every rank
    return dict(Y=Y, X_mu=X_mu, X_S=X_S, Z=Z, sf2=1.0, alpha=np.full(Q, 0.1), beta=10.0)


def synthetic_threaded(N, D, M, Q, seed, regime='B'):
    """The same generator in row chunks on the host's threads, one random stream per chunk: BASELINE configs[4]'s per-GPU shard
    (N=1e6, D=1000: 8 GB of Y) in a few seconds instead of a minute."""
    from multiprocessing.pool import ThreadPool
    Wmap = np.random.RandomState(1234).randn(Q, D)
    Y, X_mu, X_S = np.empty((N, D)), np.empty((N, Q)), np.zeros((N, Q))
    step = 50000

    def chunk(i):
        rs = np.random.RandomState(seed * 1000 + i)
        a, b = i * step, min(N, (i + 1) * step)
        X = rs.randn(b - a, Q)
        Y[a:b] = np.sin(X.dot(Wmap))
        Y[a:b] += 0.1 * rs.randn(b - a, D)
        X_mu[a:b] = X + 0.05 * rs.randn(b - a, Q)
        if regime == 'B':
            X_S[a:b] = rs.uniform(0.05, 0.55, size=(b - a, Q))

    with ThreadPool(min(32, usable_cpus())) as pool:
        pool.map(chunk, range((N + step - 1) // step))
    rs = np.random.RandomState(seed + 1)
    Z = X_mu[rs.permutation(N)[:M]] + 0.3 * rs.randn(M, Q)
    return dict(Y=Y, X_mu=X_mu, X_S=X_S, Z=Z, sf2=1.0, alpha=np.full(Q, min(0.1, 1.0 / Q)), beta=10.0)


TRUTH_BLOCKS = ('grad_Z', 'grad_alpha', 'grad_sf2', 'grad_beta')


def input_checksums(d):
    """The checksums tests/golden/make_hp_truth_large.py stores with its extended-precision truth (same formulas)."""
    w = np.cos(np.arange(d['Y'].shape[0], dtype=np.float64))
    return np.array([d['Y'].sum(), np.abs(d['Y']).sum(), w.dot(d['Y']).sum(), d['X_mu'].sum(), w.dot(d['X_mu']).sum(),
                     d['Z'].sum(), np.abs(d['Z']).sum()])


def truth_errors(d, out, N, D, M, Q, seed):
    """Errors of this run's bound and gradients against the committed long-double truth of the SAME workload
    (tests/golden/hp_truth_large_N<N>.npz, oracle/hp_truth.c), relative to each block's largest magnitude; None when there is no
    truth for this shape / seed or the regenerated inputs do not reproduce its checksums."""
    f = os.path.join(ROOT, 'tests', 'golden', 'hp_truth_large_N%d.npz' % N)
    if not os.path.exists(f):
        return None
    z = np.load(f)
    if (int(z['N']), int(z['D']), int(z['M']), int(z['Q']), int(z['seed'])) != (N, D, M, Q, seed):
        return None
    cs = input_checksums(d)
    if not np.allclose(cs, z['input_checksums'], rtol=1e-11, atol=1e-9):      # sin() may differ in the last bit between hosts
        return None
    res = {'cond_A': float(z['cond_A']), 'cond_Kmm': float(z['cond_Kmm']),
           'F_err_vs_truth': abs(out['F'] - float(z['truth_F'])) / abs(float(z['truth_F']))}
    for k in TRUTH_BLOCKS:
        t = np.asarray(z['truth_' + k])
        res['%s_err_vs_truth' % k] = float(np.max(np.abs(np.asarray(out[k]) - t)) / np.max(np.abs(t)))
        res['%s_err_float64_lu' % k] = float(z['err_lu_' + k])
        res['%s_err_float64_cholesky' % k] = float(z['err_chol_' + k])
    res['error_norm'] = ('per block: max |x - truth| / max |truth| (the block\'s max-norm, tests/conftest.py assert_close) -- NOT elementwise relative error; '
                         'this is how the 1e-5 gradient contract of BASELINE.json is read everywhere in tests/ and here')
    x, y = res['grad_Z_err_vs_truth'], res['grad_Z_err_float64_lu']
    res['reading'] = ('grad_Z of this run is within %.1e of the 80-bit truth; the reference\'s own float64 arrangement (LU inv / slogdet, partial_terms.py:449-450) is %.1e '
                      'from the same truth at this conditioning (cond(Kmm + beta Psi2) = %.1e), so device-vs-reference is bounded by %.1e and exceeds the 1e-5 '
                      'contract only because of the reference\'s %.1e: the device is the accurate side (small goldens match the reference directly at 1e-5)'
                      % (x, y, res['cond_A'], x + y, y))
    res['truth'] = 'tests/golden/hp_truth_large_N%d.npz (80-bit long double, own uncertainty %.1e on grad_Z)' % (N, float(z['truth_uncertainty'][1]))
    return res


def extended_precision_cost(eng, d, N, D, M, Q, seed):
    """Global-step device time and grad_Z's distance from the extended-precision truth for three settings of the global step: float64 only,
    + one double-double refinement step of E (round 3), + K_mm^-1 Psi2 accumulated in double-double (round 4, the default)."""
    from gparml_amd import _lib
    lib = _lib.load()
    res = {}
    try:
        for name, dd, ref in (('float64', 0, 0), ('refine_E', 0, 1), ('refine_E+dd_KiPsi2 (default)', 1, 1)):
            lib.gp_debug_set_option(b'dd_kipsi2', dd)
            lib.gp_debug_set_option(b'refine_E', ref)
            eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'], N_global=N)
            g = []
            for _ in range(4):
                out = eng.evaluate(False)
                g.append(eng.timings()['global_ms'])
            te = truth_errors(d, out, N, D, M, Q, seed)
            res[name] = {'global_ms': round(min(g[1:]), 4), 'grad_Z_err_vs_truth': None if te is None else te['grad_Z_err_vs_truth']}
    finally:
        lib.gp_debug_set_option(b'dd_kipsi2', 1)
        lib.gp_debug_set_option(b'refine_E', 1)
    res['cost_ms'] = round(res['refine_E+dd_KiPsi2 (default)']['global_ms'] - res['float64']['global_ms'], 4)
    return res


INT8_PEAK_TOPS = 4880.0    # v_mfma_i32_32x32x32_i8, sustained for 190 ms on this part (tools/ubench/i8_ubench.hip, profiles/r05_int8_phase2.txt)


def int8_variants(eng, d, N, D, M, Q, seed, steps=10):
    """The same workload on the opt-in int8 paths, timed OUTSIDE the headline region and priced against the int8 matrix core's own peak (the headline
    stays on the float64 matrix core): phase 1 (csrc/p1i8.hip: six signed 7-bit digits per operand, 21 exact digit products, Psi2's diagonal from float64
    sums of squares, guarded at run time -- gp_i8_status).  (A phase 2 on the int8 matrix core was built in round 5 -- parity-green, not faster:
    profiles/r05_int8_phase2.txt -- and removed in round 6.)  Device ms per evaluation next to the float64 default of the same run and the distance of each variant's
    gradients from the extended-precision truth."""
    from gparml_amd import _lib
    lib = _lib.load()
    res = {}
    try:
        for name, p1 in (('float64 (default: p1v2_kernel, p2_fast8_kernel)', 0), ('int8 phase 1 (p1i8_kernel)', 1)):
            lib.gp_debug_set_option(b'p1_i8', p1)
            eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'], N_global=N)
            tot = {}
            for i in range(steps + 3):            # the first int8 evaluation is the guard's check (both phase-1 paths): not in the average
                out = eng.evaluate(False)
                if i >= 3:
                    for k, v in eng.timings().items():
                        tot[k] = tot.get(k, 0.0) + v / steps
            te = truth_errors(d, out, N, D, M, Q, seed)
            r = {'ms_per_eval_device': round(tot['total_ms'], 4), 'psi1_ms': round(tot['psi1_ms'], 4), 'p1_kernel_ms': round(tot['p1_kernel_ms'], 4),
                 'p2_kernel_ms': round(tot['p2_kernel_ms'], 4), 'global_ms': round(tot['global_ms'], 4),
                 'grad_Z_err_vs_truth': None if te is None else te['grad_Z_err_vs_truth'], 'F_err_vs_truth': None if te is None else te['F_err_vs_truth']}
            if p1:
                # 21 digit products of (N M^2 / 2 + N M D) multiply-adds each on the int8 matrix core
                ops = 2.0 * 21.0 * (0.5 * N * M * M + float(N) * M * D)
                ach = ops / (tot['p1_kernel_ms'] * 1e-3) / 1e12
                r['roofline'] = {'bound': 'mfma', 'kernel': 'gp::p1i8_kernel', 'achieved': ach, 'peak': INT8_PEAK_TOPS, 'unit': 'TOP/s (int8)', 'frac': ach / INT8_PEAK_TOPS}
                r['guard'] = eng.i8_status()
            res[name] = r
    finally:
        lib.gp_debug_set_option(b'p1_i8', 0)
    return res


def regime_b_extra(name, N, D, M, Q, device, steps=2, threaded=False):
    """One free-embedding (Bayesian GPLVM, regime B) evaluation shape, timed OUTSIDE the headline region: ms per evaluation (HIP
    events on the engine's stream), SURVEY.md 8(d)'s W_B = N M^2 (4Q + 10) and its fraction of the FP64 peak, the dominant kernels."""
    from gparml_amd.engine import ShardEngine
    if threaded:
        d = synthetic_threaded(N, D, M, Q, seed=7, regime='B')
    else:
        d = synthetic(N, D, M, Q, seed=7, regime='B')
        d['alpha'] = np.full(Q, min(0.1, 1.0 / Q))
    eng = ShardEngine(N, D, M, Q, device=device)
    free0, total = eng.memory_info()
    eng.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'])
    eng.evaluate(True)
    tot = {}
    for _ in range(steps):
        out = eng.evaluate(True)
        for k, v in eng.timings().items():
            tot[k] = tot.get(k, 0.0) + v / steps
    free1, _ = eng.memory_info()
    eng.close()
    W_B = float(N) * M * M * (4.0 * Q + 10.0)
    return {'workload': name, 'N': N, 'D': D, 'M': M, 'Q': Q, 'ms': tot['total_ms'], 'W_B_flop': W_B,
            'device_memory_GB': {'regime_B_buffers_after_create': round((free0 - free1) / 2.0 ** 30, 2), 'device_total': round(total / 2.0 ** 30, 1)},
            'achieved_tflops': W_B / (tot['total_ms'] * 1e-3) / 1e12, 'frac': W_B / (tot['total_ms'] * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
            'ms_per_1e6_points': tot['total_ms'] * 1e6 / N,
            'kernel_ms': {'psi2_phase1 (Psi2 pair kernel)': round(tot['p1_kernel_ms'], 3), 'psi2_phase2 (T_n = Bbar o psi2_n kernel)': round(tot['p2_kernel_ms'], 3),
                          'generate': round(tot['generate_ms'], 3), 'phase1': round(tot['phase1_ms'], 3), 'global': round(tot['global_ms'], 3),
                          'phase2': round(tot['phase2_ms'], 3)},
            'F': out['F']}


def config1_extra(device, steps=50):
    """BASELINE configs[1] (N=1e5, D=10, M=128, Q=10, fixed embeddings): a latency-bound evaluation (~35 launches, 7e9 flop).  Every step
    sets new global parameters, as an optimiser does; wall time per evaluation against the device time of its kernels = the share the host
    spends enqueueing."""
    from gparml_amd.engine import ShardEngine
    N, D, M, Q = 100000, 10, 128, 10
    d = synthetic(N, D, M, Q, seed=11)
    rs = np.random.RandomState(12)
    Zs = [d['Z'] + 1e-3 * rs.randn(M, Q) for _ in range(steps)]
    eng = ShardEngine(N, D, M, Q, device=device)
    eng.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    # wall clock: what an optimiser pays per evaluation -- no timing events on the stream (gp_set_timing(0): each of the thirteen events of an
    # evaluation is a signal packet the stream idles on for 4-7 us, 15 % of an evaluation at this size)
    eng.set_timing(0)
    # steady state: an evaluation is 0.3 ms, and for tens of milliseconds after the device has idled (the seconds of host-only work in front of this
    # function) every submission is slow -- five warm-up evaluations and fifty timed ones read 0.37 ms in a fresh process and 0.6 ... 2.4 ms here
    # (tests/devtools/dev_c1_wall.py: the same after a 3 s sleep).  So: half a second of evaluations first, then five blocks of `steps`; the median block.
    t0 = time.time()
    while time.time() - t0 < 0.5:
        for i in range(steps):
            eng.set_globals(Zs[i], d['sf2'], d['alpha'], d['beta'])
            out = eng.evaluate(False)
    blocks = []
    for b in range(5):
        t0 = time.time()
        for i in range(steps):
            eng.set_globals(Zs[i], d['sf2'], d['alpha'], d['beta'])
            out = eng.evaluate(False)
        blocks.append((time.time() - t0) / steps * 1e3)
    wall = sorted(blocks)[2]
    # device time of one evaluation from its first to its last kernel: two events only (level 1), read outside the wall-clock loop
    eng.set_timing(1)
    dev = 0.0
    for i in range(10):
        eng.set_globals(Zs[i], d['sf2'], d['alpha'], d['beta'])
        out = eng.evaluate(False)
        dev += eng.timings()['total_ms'] / 10
    # per-kernel events (level 2, the default): the breakdown; their own idle time is in these numbers
    eng.set_timing(2)
    tm = {}
    for i in range(10):
        eng.set_globals(Zs[i], d['sf2'], d['alpha'], d['beta'])
        out = eng.evaluate(False)
        for k, v in eng.timings().items():
            tm[k] = tm.get(k, 0.0) + v / 10
    eng.close()
    W = float(N) * M * (3.0 * M + 4.0 * D + 12.0 * Q)
    return {'workload': 'BASELINE configs[1]: N=1e5, D=10, M=128, Q=10, fixed embeddings, new global parameters every step', 'N': N, 'D': D, 'M': M, 'Q': Q,
            'ms_per_eval_wall': wall, 'ms_per_eval_wall_blocks': [round(x, 4) for x in blocks], 'evals_per_s': 1e3 / wall, 'device_ms': dev, 'host_enqueue_share': max(0.0, 1.0 - dev / wall),
            'global_ms': tm['global_ms'], 'device_ms_by_stage_with_per_kernel_events': {k: round(v, 4) for k, v in tm.items()}, 'eval_flops_survey_8d': W, 'frac': W / (wall * 1e-3) / 1e12 / FP64_PEAK_TFLOPS, 'F': out['F']}


def cpu_baseline(D, M, Q, N_full, budget_rows):
    """The oracle's CPU evaluation (kind "port": numpy/OpenBLAS restatement of the same path, oracle/factorised.py) on a bounded sample of
    the same workload, scaled linearly in N.  ``value`` is the BLAS-bound arrangement (evaluate_blas: K_nm kept between the phases, work
    buffers reused, 32768-row chunks) with its row chunks spread over a thread pool -- the element-wise numpy work (exp, products, row sums
    over 32768 x 512 arrays) is single-threaded per call, so one caller leaves most of a many-core host idle; W workers x T BLAS threads
    with W * T = the CPUs this process may use (usable_cpus) -- in steady state (the best of the calls after the first, which pays the
    page faults of the work buffers).  ``cores`` = the logical CPUs the configuration keeps busy; ``single_caller`` is the round-2 configuration (one caller,
    all BLAS threads); ``two_phase_port`` is the kernel-spec form (evaluate: K_nm regenerated in phase 2, 8192-row chunks)."""
    from oracle import factorised as Fz
    ncpu = usable_cpus()
    try:
        from threadpoolctl import threadpool_limits
    except Exception:
        threadpool_limits = None
    d = synthetic(budget_rows, D, M, Q, seed=99)
    W = float(budget_rows) * M * (3.0 * M + 4.0 * D + 12.0 * Q)            # SURVEY.md 8(d) flop count of the sample
    args = (d['Z'], d['sf2'], d['alpha'], d['beta'], d['Y'], d['X_mu'])
    nch = max(1, (budget_rows + 32767) // 32768)

    def timed(workers, blas_threads, reps):
        work, best, first = {}, None, None
        for r in range(reps + 1):
            t = time.time()
            if threadpool_limits is not None and blas_threads:
                with threadpool_limits(limits=blas_threads):
                    Fz.evaluate_blas(*args, work=work, workers=workers)
            else:
                Fz.evaluate_blas(*args, work=work, workers=workers)
            dt = time.time() - t
            if r == 0:
                first = dt
            else:
                best = dt if best is None else min(best, dt)
        return best, first

    dt1, first1 = timed(1, None, 1)                                         # one caller, all BLAS threads
    trials = {}
    for workers in sorted({w for w in (2, 4, 8, 16) if w <= min(nch, ncpu)}):
        trials[workers] = timed(workers, max(1, ncpu // workers), 1)[0]
    bw = min(trials, key=trials.get) if trials else 1
    dt = min(trials[bw], dt1) if trials else dt1
    if not trials or dt1 <= trials[bw]:
        bw = 1
    n2 = min(budget_rows, 100000)                                           # the two-phase form on a smaller slice (it is ~4x slower)
    t = time.time()
    Fz.evaluate(d['Z'], d['sf2'], d['alpha'], d['beta'], d['Y'][:n2], d['X_mu'][:n2], d['X_S'][:n2], want_embeddings=False, chunk=8192)
    dt2 = (time.time() - t) * budget_rows / float(n2)
    scale = float(N_full) / budget_rows
    return {'value': 1.0 / (dt * scale), 'unit': 'evals/s', 'cores': int(ncpu), 'kind': 'port', 'gflops': W / dt / 1e9,
            'workers': int(bw), 'blas_threads_per_worker': int(max(1, ncpu // bw)),
            'workers_tried_s': {str(k): round(v, 3) for k, v in trials.items()},
            'single_caller': {'value': 1.0 / (dt1 * scale), 'gflops': W / dt1 / 1e9, 'first_call_evals_per_s': 1.0 / (first1 * scale)},
            'two_phase_port': {'value': 1.0 / (dt2 * scale), 'gflops': W / dt2 / 1e9},
            'sample': 'oracle/factorised.py evaluate_blas() on %d of %d rows (D=%d M=%d Q=%d): %.2f s steady state with %d chunk workers x %d BLAS '
                      'threads (one caller with all BLAS threads: %.2f s), evaluate() %.1f s; scaled linearly in N'
                      % (budget_rows, N_full, D, M, Q, dt, bw, max(1, ncpu // bw), dt1, dt2)}


DUMP_MAX_ELEMENTS = 1 << 21      # per array (16 MB of float64): the dump stays well under 64 MB in all


def dump_outputs(dirname, out, eng, emb):
    """What the last timed step computed, as DIR/<name>.npy in float64: the bound and the global gradients the evaluation returns and, with
    free embeddings, the embedding gradients it left on the device.  An array of more than DUMP_MAX_ELEMENTS is written as a fixed,
    seeded sample of its rows (the same rows for the same shape), so that two builds can be compared output for output."""
    os.makedirs(dirname, exist_ok=True)
    arrays = {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}
    if emb:
        arrays['grad_X_mu'] = eng.download('GRAD_X_MU')
        arrays['grad_X_S'] = eng.download('GRAD_X_S')
    for name, v in sorted(arrays.items()):
        if v.size > DUMP_MAX_ELEMENTS:
            n = v.shape[0]
            v = v[np.sort(np.random.RandomState(0).choice(n, DUMP_MAX_ELEMENTS // (v.size // n), replace=False))]
        np.save(os.path.join(dirname, name + '.npy'), v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--N', type=int, default=1000000)
    ap.add_argument('--D', type=int, default=100)
    ap.add_argument('--M', type=int, default=512)
    ap.add_argument('--Q', type=int, default=10)
    ap.add_argument('--regime', choices=['A', 'B'], default='A',
                    help='A (default, the metric\'s configuration): X_S = 0, fixed embeddings; B: Bayesian GPLVM, X_S > 0, embedding gradients')
    ap.add_argument('--dump-outputs', metavar='DIR', help='write what the last timed step computed to DIR/<name>.npy (float64)')
    ap.add_argument('--full', action='store_true',
                    help='after the headline: parity against the extended-precision truth, the extended-precision cost, the int8 variant, '
                         'the "extra" shapes and the CPU baseline (all outside the timed region)')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baseline')
    ap.add_argument('--no-extra', action='store_true', help='with --full: skip the int8 variant and the shapes reported under "extra"')
    ap.add_argument('--cpu-rows', type=int, default=400000)
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error('--steps must be at least 1 and --warmup at least 0')

    world = int(os.environ.get('WORLD_SIZE', '1'))
    if a.gpus != world:
        if world == 1 and a.gpus > 1:
            # plain `python bench.py --gpus N`: start the N ranks as a fresh torchrun child (nothing has touched the GPU yet)
            import socket
            import subprocess
            sk = socket.socket(); sk.bind(('127.0.0.1', 0)); port = sk.getsockname()[1]; sk.close()
            cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(a.gpus), '--master-addr', '127.0.0.1',
                   '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
            raise SystemExit(subprocess.call(cmd))
        raise SystemExit('bench.py: --gpus %d but WORLD_SIZE=%d; launch as\n  python -m torch.distributed.run --nnodes=1 --nproc-per-node %d '
                         '--master-addr 127.0.0.1 --master-port P bench.py --gpus %d ...' % (a.gpus, world, a.gpus, a.gpus))
    import torch
    import torch.distributed as dist
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs a GPU: the hot path has no CPU fallback')
    # test hooks (tests/test_gpu_bench_ranks.py): several ranks on ONE device over gloo exercise the N>1 code path on a 1-GPU box
    if os.environ.get('GPARML_BENCH_ONE_DEVICE'):
        local_rank = 0
    torch.cuda.set_device(local_rank)
    own_group = False
    if world > 1 and not dist.is_initialized():        # (tests/test_gpu_bench_ranks.py calls main() inside a process that already has its group)
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group(os.environ.get('GPARML_BENCH_BACKEND', 'nccl'), rank=rank, world_size=world)
        own_group = True
    dev = torch.device('cuda', local_rank)

    from gparml_amd.engine import ShardEngine
    from gparml_amd.dist import DistributedEvaluator

    d = synthetic(a.N, a.D, a.M, a.Q, seed=100 + rank, regime=a.regime)
    emb = a.regime == 'B'
    eng = ShardEngine(a.N, a.D, a.M, a.Q, device=local_rank)
    eng.upload_shard(d['Y'], d['X_mu'], d['X_S'])
    eng.set_globals(d['Z'], d['sf2'], d['alpha'], d['beta'], N_global=a.N * world)
    ev = DistributedEvaluator(eng, device=dev)
    # collective on every rank (before the timed region): one 1.0 per rank through the library's communicator
    probe_sum = eng.comm_info(probe=True)['probe_sum'] if (world > 1 and ev.native) else None

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # what a real optimiser pays: NEW global parameters for every evaluation (gp_set_globals: pinned staging + async copy + the Zaug kernel,
    # no host synchronisation).  A fixed seeded sequence of perturbed (Z, sf2, alpha, beta); the LAST timed step is the unperturbed point, whose
    # result is compared with the extended-precision truth below.
    rp = np.random.RandomState(4242)
    n_ev = a.warmup + a.steps
    pert = [(d['Z'] + 1e-3 * rp.randn(a.M, a.Q), d['sf2'] * (1 + 1e-3 * rp.randn()), d['alpha'] * (1 + 1e-3 * rp.randn(a.Q)),
             d['beta'] * (1 + 1e-3 * rp.randn())) for _ in range(n_ev - 1)] + [(d['Z'], d['sf2'], d['alpha'], d['beta'])]

    def set_point(i):
        eng.set_globals(pert[i][0], pert[i][1], pert[i][2], pert[i][3], N_global=a.N * world)

    for i in range(a.warmup):
        set_point(i)
        out = ev.evaluate(emb)
    barrier()
    t0 = time.time()
    kern = {'psi1_ms': 0.0, 'p1_kernel_ms': 0.0, 'p2_kernel_ms': 0.0, 'global_ms': 0.0, 'total_ms': 0.0}
    ev.time_collectives = world > 1   # events around the two all-reduces (read back after the evaluation's own synchronisation)
    coll = {'allreduce_stats_ms': 0.0, 'allreduce_grads_ms': 0.0}
    F_seen = set()
    for i in range(a.steps):
        set_point(a.warmup + i)
        out = ev.evaluate(emb)
        F_seen.add(out['F'])
        tm = eng.timings()            # HIP events on the engine's stream around each kernel of this evaluation
        for k in kern:
            kern[k] += tm[k]
        for k, v in ev.collective_ms().items():
            coll[k] += v
    barrier()
    dt = time.time() - t0
    rank_ms = [dt / a.steps * 1e3]
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device=dev)
        allt = [torch.zeros_like(tt) for _ in range(world)]
        dist.all_gather(allt, tt)                                 # every rank's own time: a straggler shows in the N > 1 line
        rank_ms = [float(t.item()) / a.steps * 1e3 for t in allt]
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    for k in kern:
        kern[k] /= a.steps
    for k in coll:
        coll[k] /= a.steps
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, out, eng, emb)

    if rank == 0:
        N, D, M, Q = a.N, a.D, a.M, a.Q
        # algorithmic FLOPs (FMA = 2) of the dominant kernel, the fast phase-2 kernel: K.(2 Bbar) 2NM^2 + Y.Abar^T 2NMD + the
        # n-contraction W^T [mu, 1]: 2NM(Q+1)   (the mu^2 term of grad_alpha only needs row sums)
        flops_p2 = 2.0 * N * M * (M + D) + 2.0 * N * M * (Q + 1)
        # the kernel run_phase2 (csrc/psi.hip) dispatches for this Q with fixed embeddings: Q + 1 feature columns in groups of four
        nrb = (Q + 1 + 3) // 4
        p2_kernel = 'gp::p2_fast8_kernel<%d>' % nrb if nrb <= 3 else 'gp::p2_gen8_kernel<false>'
        ach = flops_p2 / (kern['p2_kernel_ms'] * 1e-3) / 1e12
        # HBM bytes per launch of that kernel from the PMC passes of the SAME command (tools/r02_prof.sh -> profiles/traffic.json,
        # FETCH_SIZE x2 + WRITE_SIZE as MI355X_MICROARCH.md prescribes); quoted only while it describes the kernel that ran here
        traffic, traffic_src = None, None
        tf = os.path.join(ROOT, 'profiles', 'traffic.json')
        if os.path.exists(tf):
            try:
                tj = json.load(open(tf))
                if tj.get('kernel') == p2_kernel and (tj.get('N'), tj.get('D'), tj.get('M'), tj.get('Q')) == (N, D, M, Q):
                    traffic = tj.get('p2_kernel_hbm_bytes_per_launch')
                    traffic_src = {'file': 'profiles/traffic.json', 'commit': tj.get('commit'), 'date': tj.get('date')}
            except Exception:
                traffic = None
        W_eval = float(N) * M * (3.0 * M + 4.0 * D + 12.0 * Q)      # SURVEY.md 8(d) regime-A figure for a whole evaluation
        res = {
            'metric': 'variational bound+grad evals/sec', 'value': world * a.steps / dt, 'unit': 'evals/s (one eval = one %d-point shard)' % N,
            'n_gpus': world, 'steps': a.steps, 'warmup': a.warmup, 'ms_per_step': dt / a.steps * 1e3,
            'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f64', 'data': 'synthetic',
            'config': {'workload': '%s%d shard(s) x N=%d, D=%d, M=%d, Q=%d, ARD-RBF sparse GP (fixed embeddings)'
                                   % ('BASELINE configs[%d]: ' % (2 if world == 1 else 3) if (N, D, M, Q) == (1000000, 100, 512, 10) else '', world, N, D, M, Q),
                       'N_per_gpu': N, 'D': D, 'M': M, 'Q': Q, 'regime': 'A', 'parallelism': 'dp%d' % world,
                       'points_per_sec': world * N * a.steps / dt, 'F': out['F'],
                       'timed_loop': 'gp_set_globals with new (Z, sf2, alpha, beta) before every evaluation (seeded 1e-3 perturbations; the last step is the '
                                     'unperturbed point); %d distinct bound values in %d steps' % (len(F_seen), a.steps),
                       'device_ms': {k: round(v, 4) for k, v in kern.items()},
                       'eval_flops_survey_8d': W_eval, 'eval_fraction_of_fp64_peak': W_eval / (kern['total_ms'] * 1e-3) / 1e12 / FP64_PEAK_TFLOPS},
            'roofline': {'bound': 'mfma', 'kernel': p2_kernel, 'achieved': ach, 'peak': FP64_PEAK_TFLOPS, 'unit': 'TFLOP/s',
                         'frac': ach / FP64_PEAK_TFLOPS, 'traffic': traffic, 'traffic_source': traffic_src},
        }
        if a.regime == 'B':
            # not the metric's configuration: the free-embedding (Bayesian GPLVM) variant of the same size.  The pair kernels
            # run on the FP64 pipe that VALU and MFMA share, so the whole evaluation is priced against the same peak with
            # SURVEY.md 8(d)'s regime-B figure W_B = N M^2 (4Q + 10)
            W_B = float(N) * M * M * (4.0 * Q + 10.0)
            achB = W_B / (kern['total_ms'] * 1e-3) / 1e12
            res['config']['workload'] = 'N=%d, D=%d, M=%d, Q=%d, ARD-RBF Bayesian GPLVM (free embeddings, X_S > 0), %d shard(s)' % (N, D, M, Q, world)
            res['config']['regime'] = 'B'
            res['config']['eval_flops_survey_8d'] = W_B
            res['config']['eval_fraction_of_fp64_peak'] = achB / FP64_PEAK_TFLOPS
            res['roofline'] = {'bound': 'mfma', 'kernel': 'whole evaluation (psi2 pair kernels, FP64 VALU/MFMA pipe)', 'achieved': achB,
                               'peak': FP64_PEAK_TFLOPS, 'unit': 'TFLOP/s', 'frac': achB / FP64_PEAK_TFLOPS, 'traffic': None}
        if world > 1:
            # what the N > 1 line needs to attribute a scaling loss: the two collectives and the replicated global step, per evaluation
            res['config']['allreduce_ms'] = {k: round(v, 4) for k, v in coll.items()}
            res['config']['allreduce_ms']['total'] = round(sum(coll.values()), 4)
            res['config']['global_ms'] = round(kern['global_ms'], 4)
            # did RCCL see N ranks?  the library's own answer (gp_comm_info: ranks as given to ncclCommInitRank and a one-double probe all-reduce
            # that must sum to N), which backend carried the two all-reduces, and their payloads
            from gparml_amd import dist as gdist
            info = eng.comm_info(probe=False)
            res['config']['collective_backend'] = 'rccl-native' if ev.native else ('torch-nccl' if dist.get_backend() == 'nccl' else dist.get_backend())
            res['config']['comm_ranks'] = info['ranks']
            res['config']['comm_probe_sum'] = probe_sum
            res['config']['allreduce_payload_bytes'] = {'stats': info['stats_bytes'], 'grads': info['grads_bytes']}
            if gdist.native_comm_reason:
                res['config']['native_comm_fallback_reason'] = gdist.native_comm_reason
            res['config']['ms_per_step_by_rank'] = {'min': round(min(rank_ms), 4), 'max': round(max(rank_ms), 4), 'all': [round(v, 4) for v in rank_ms]}
        res['config']['global_step'] = ('float64 blocked Cholesky + inverses; Kmm^-1 Psi2 accumulated in double-double; E = (Kmm + beta Psi2)^-1 Psi1^T Y '
                                        'refined once with a double-double residual (GPARML_DD_KIPSI2 / GPARML_REFINE_E = 0 switch them off)')
        if a.full and a.regime == 'A' and world == 1:
            # the price of the two extended-precision pieces: the global step timed (HIP events) with and without them, after the timed region,
            # with grad_Z's distance from the truth for each setting
            res['config']['extended_precision_cost'] = extended_precision_cost(eng, d, N, D, M, Q, 100 + rank)
            if not a.no_extra and (N, D, M, Q) == (1000000, 100, 512, 10):
                res['config']['int8_variant'] = int8_variants(eng, d, N, D, M, Q, 100 + rank)
        if a.full and a.regime == 'A':
            # parity of THIS run's last evaluation against the extended-precision truth of the same workload (rank 0's shard alone:
            # only meaningful for one shard), and the conditioning it was obtained at
            te = truth_errors(d, out, N, D, M, Q, 100 + rank) if world == 1 else None
            if te is not None:
                res['config'].update({'cond_A': te['cond_A'], 'cond_Kmm': te['cond_Kmm'], 'grad_Z_err_vs_truth': te['grad_Z_err_vs_truth'],
                                      'F_err_vs_truth': te['F_err_vs_truth'], 'parity_vs_truth': te})
        if a.full and not a.no_extra and world == 1 and a.regime == 'A' and (N, D, M, Q) == (1000000, 100, 512, 10):
            # regime B (free embeddings) is not the metric's configuration; two shapes, each a slice of a BASELINE config, measured after
            # the timed region so that the driver's own run carries them
            eng.close()
            res['extra'] = [config1_extra(local_rank),
                            regime_b_extra('BASELINE configs[2] shape with free embeddings (Bayesian GPLVM), 1e5-point slice', 100000, 100, 512, 10, local_rank),
                            regime_b_extra('the same with a 12-dimensional latent space (r06: psi2_sym_kernel<12>; round 5: 56.3 ms)', 100000, 100, 512, 12, local_rank),
                            regime_b_extra('BASELINE configs[4] per-GPU shape (D=1000, M=1024, Q=50, free embeddings), 2e4-point slice', 20000, 1000, 1024, 50,
                                           local_rank),
                            regime_b_extra('BASELINE configs[4] at its FULL per-GPU size: N=1e6, D=1000, M=1024, Q=50, free embeddings', 1000000, 1000, 1024, 50,
                                           local_rank, steps=1, threaded=True)]
        if a.full and not a.no_cpu_baseline and world == 1 and a.regime == 'A':     # rank 0 at N=1 only
            # last: its BLAS worker threads keep spinning for a while and slow the host side of whatever is timed after them (configs[1]'s
            # wall clock per evaluation read 1.15 ms behind the CPU baseline, 0.37 ms in a fresh process)
            res['cpu_baseline'] = cpu_baseline(D, M, Q, N, min(a.cpu_rows, N))
        print(json.dumps(res))
    if own_group:
        dist.destroy_process_group()
    eng.close()


if __name__ == '__main__':
    main()
