"""Host orchestration of one evaluation: Python-3 restatement of ``parallel_GPLVM.likelihood_and_gradient``
(parallel_GPLVM.py:222-279) and its helpers ``calculate_global_statistics`` (:302-334), ``calculate_global_derivatives``
(:336-369), ``flatten/rebuild_global_statistics`` (:286-299), ``clean`` (:373-404), against a MapReduce backend module
with the ``local_MapReduce`` function set (``gparml_amd.gpu_MapReduce``).

Two modes produce the same numbers and the same files:
  * ``fast=False`` (compat): exactly the reference's call sequence -- cache, statistics_MR (12 statistics incl. the four
    derivative 3-tensors), partial_terms.grad_Z/grad_alpha/grad_sf2/grad_beta on the master, embeddings_MR.
  * ``fast=True``: the two-phase device protocol: phase 1 on every shard, device-side reduce of the
    packed statistics, replicated global step, phase 2 with the Z/alpha gradients contracted on the device, device-side
    reduce of the packed gradient sums.  The 3-tensors are never formed.

The optimiser keeps its contract: ``f, g = likelihood_and_gradient(x, iteration, step_size)`` returns ``(-F, -grad)`` in
the softplus-inverse parametrisation, flat order Z (row-major), sf2, alpha, beta (parallel_GPLVM.py:139-141, 203-212).
"""
import os
import time

import numpy

from .evaluation import BufferReduce, evaluate


def _f(x):
    return float(numpy.asarray(x).reshape(-1)[0])


LIM_VAL = -numpy.log(numpy.finfo(float).eps)          # supporting_functions.py:125


def transform(b, x):
    if b == (0, None):                                # supporting_functions.py:127-132
        assert -LIM_VAL < x < LIM_VAL
        return numpy.log(1 + numpy.exp(x))
    return x


def transform_back(b, x):
    if b == (0, None):                                # supporting_functions.py:135-140
        assert numpy.finfo(float).eps < x < LIM_VAL
        return numpy.log(-1 + numpy.exp(x))
    return x


def transform_grad(b, x):
    if b == (0, None):                                # supporting_functions.py:143-148
        assert -LIM_VAL < x < LIM_VAL
        return 1 / (numpy.exp(-x) + 1)
    return 1


def positive_mask(bounds):
    """Boolean mask of the (0, None)-bounded entries of a flat parameter vector."""
    return numpy.array([b == (0, None) for b in bounds], dtype=bool)


def transform_vec(mask, x):
    """``[transform(b, x_i)]`` over a whole flat vector at once (supporting_functions.py:127-132): softplus on the positive entries,
    identity elsewhere, the same range assertion.  The per-element Python loop costs ~50 k calls per evaluation at M*Q = 51 200."""
    x = numpy.asarray(x, dtype=float)
    out = x.copy()
    xp = x[mask]
    assert numpy.all((-LIM_VAL < xp) & (xp < LIM_VAL))
    out[mask] = numpy.log(1 + numpy.exp(xp))
    return out


def transform_grad_vec(mask, x):
    """``[transform_grad(b, x_i)]`` as a vector (supporting_functions.py:143-148)."""
    x = numpy.asarray(x, dtype=float)
    out = numpy.ones_like(x)
    xp = x[mask]
    assert numpy.all((-LIM_VAL < xp) & (xp < LIM_VAL))
    out[mask] = 1 / (numpy.exp(-xp) + 1)
    return out


def split_flat(flat, M, Q):
    """(Z (M, Q), sf2, alpha (Q,), beta) of a flat parameter vector: order Z (row-major), sf2, alpha, beta (parallel_GPLVM.py:139-141)."""
    flat = numpy.asarray(flat, dtype=float)
    n = M * Q
    return flat[:n].reshape(M, Q), flat[n], flat[n + 1:n + 1 + Q], flat[n + 1 + Q]


def _device_kmeans(map_reduce, options, names, engine_class=None):
    """options['init_Z'] == 'device': k-means over the embeddings of ALL shards (gparml_amd.init.kmeans), the assignment passes on the GPUs the
    shards are spread over -- one temporary engine per device, the embeddings passed as host rows.  The seeds are drawn from numpy's global
    stream."""
    from . import init
    if engine_class is None:
        from .engine import ShardEngine as engine_class
    devices = map_reduce._devices(options) if hasattr(map_reduce, '_devices') else [int(options.get('device', 0))]
    engines, parts = {}, []
    try:
        for i, name in enumerate(names):
            dev = devices[i % len(devices)]                                              # where the shard will live (gpu_MapReduce._device_of)
            if dev not in engines:
                engines[dev] = engine_class(1, 1, 1, options['Q'], device=dev)           # K is free of the context's M
            parts.append(init.HostRows(engines[dev], map_reduce.load(options['embeddings'] + '/' + name + '.embedding.npy')))
        return init.kmeans(parts, options['M'], restarts=options.get('init_Z_restarts', 1))[0]
    finally:
        for e in engines.values():
            e.close()


def _device_greedy(map_reduce, options, names, sf2, alpha, engine_class=None):
    """options['init_Z'] == 'greedy': greedy conditional-variance selection (gparml_amd.init.greedy_select) of M rows among the embeddings of
    ALL shards under the initial kernel (sf2, alpha) -- one temporary engine and one part per device, holding the embeddings of the shards
    that will live there in the order of their names.  Raises LinAlgError when fewer than M rows can be told apart: nothing is invented."""
    from . import init
    if engine_class is None:
        from .engine import ShardEngine as engine_class
    devices = map_reduce._devices(options) if hasattr(map_reduce, '_devices') else [int(options.get('device', 0))]
    rows = {}
    for i, name in enumerate(names):
        rows.setdefault(devices[i % len(devices)], []).append(map_reduce.load(options['embeddings'] + '/' + name + '.embedding.npy'))
    engines = []
    try:
        parts = []
        for dev in sorted(rows):
            engines.append(engine_class(1, 1, 1, options['Q'], device=dev))
            parts.append(init.HostRows(engines[-1], numpy.concatenate(rows[dev])))
        Z, _, trace = init.greedy_select(parts, options['M'], sf2, alpha, tol=options.get('init_Z_tol', 1e-10))
    finally:
        for e in engines:
            e.close()
    if Z.shape[0] < options['M']:
        raise numpy.linalg.LinAlgError('greedy initialisation of Z: only K\' = %d of the M = %d inducing points could be selected: the conditional '
                                       'variance of every remaining row is within tol of zero (last trace residual %.3e)'
                                       % (Z.shape[0], options['M'], trace[-1] if len(trace) else float('nan')))
    return Z


def init_statistics(map_reduce, options, engine_class=None):
    """parallel_GPLVM.init_statistics (:134-214): the names the backends pass around, the initial global statistics -- inducing points
    Z by k-means over the first shards' embeddings (scipy.cluster.vq.kmeans, topped up with the first embeddings when k-means returns
    fewer than M centres) plus 0.05 * randn, sf2 = alpha = beta = 1 (:179-194), or the ``*_f.npy`` files of a previous run with
    ``options['load']`` (:195-200) -- and the optimisation bounds.  Returns (options, global_statistics).  One-off host work, unless
    ``options['init_Z'] == 'device'``: the k-means then runs on the GPUs over the embeddings of all shards (_device_kmeans; hours of host
    time at N = 1e6, M = 512 otherwise), with the same top-up and noise.  ``options['init_Z'] == 'greedy'``: the greedy
    conditional-variance selection instead (_device_greedy): Z is M data rows chosen under the initial kernel, LinAlgError
    when the data has fewer than M rows the kernel tells apart.  ``engine_class`` (tests only) replaces ShardEngine there."""
    M, Q = options['M'], options['Q']
    Driver(options, map_reduce)          # fills the *_names entries and the flat bounds exactly as the evaluations expect them
    if not options.get('load'):
        names = sorted(os.listdir(options['input'] + '/'))
        idx = 0
        embeddings = map_reduce.load(options['embeddings'] + '/' + names[idx] + '.embedding.npy')
        while embeddings.shape[0] < M:                                                  # :172-176
            idx += 1
            embeddings = numpy.concatenate((embeddings, map_reduce.load(options['embeddings'] + '/' + names[idx] + '.embedding.npy')))
        if embeddings.shape[1] != Q:
            raise Exception('Given Q does not equal existing embedding data dimensions!')
        if options.get('init_Z') == 'greedy':
            # kernel-aware placement under the initial sf2 = alpha = 1 below: M data rows, no top-up and no noise (every point stays a data row)
            Z = _device_greedy(map_reduce, options, names, 1.0, numpy.ones(Q), engine_class)
            gs = {'Z': Z, 'sf2': numpy.array([[1.0]]), 'alpha': numpy.ones((1, Q)), 'beta': numpy.array([[1.0]])}
            return options, gs
        if options.get('init_Z') == 'device':
            Z = _device_kmeans(map_reduce, options, names, engine_class)
        else:
            import scipy.cluster.vq as cl
            Z = cl.kmeans(embeddings, M)[0]                                             # :180-181
        missing = M - Z.shape[0]
        if missing > 0:
            Z = numpy.concatenate((Z, embeddings[:missing]))                            # :183-185
        Z = Z + numpy.random.randn(M, Q) * 0.05                                         # :187
        gs = {'Z': Z, 'sf2': numpy.array([[1.0]]), 'alpha': numpy.ones((1, Q)), 'beta': numpy.array([[1.0]])}
    else:
        gs = {key: map_reduce.load(options['statistics'] + '/global_statistics_' + key + '_f.npy')
              for key in options['global_statistics_names']}
    return options, gs


def initial_flat_vector(options, global_statistics):
    """The optimiser's starting point (parallel_GPLVM.py:98-100): flat order Z, sf2, alpha, beta with the positive entries mapped
    through transform_back (softplus inverse)."""
    flat = numpy.concatenate([numpy.asarray(global_statistics[k], dtype=float).flatten() for k in ('Z', 'sf2', 'alpha', 'beta')])
    return numpy.array([transform_back(b, v) for b, v in zip(options['flat_global_statistics_bounds'], flat)])


class Driver(object):
    def __init__(self, options, map_reduce=None, fast=True):
        if map_reduce is None:
            from . import gpu_MapReduce as map_reduce
        self.map_reduce = map_reduce
        self.options = options
        self.fast = fast
        self.time_acc = {'time_acc_statistics_map_reduce': [], 'time_acc_statistics_mapper': [], 'time_acc_statistics_reducer': [],
                         'time_acc_calculate_global_statistics': [], 'time_acc_embeddings_MR': [], 'time_acc_embeddings_MR_mapper': []}
        o = options
        # parallel_GPLVM.init_statistics (:139-157, 203-212)
        o['global_statistics_names'] = {'Z': (o['M'], o['Q']), 'sf2': (1, 1), 'alpha': (1, o['Q']), 'beta': (1, 1)}
        o['accumulated_statistics_names'] = ['sum_YYT', 'sum_exp_K_mi_K_im', 'sum_exp_K_miY', 'sum_exp_K_ii', 'sum_KL',
                                             'sum_d_exp_K_miY_d_Z', 'sum_d_exp_K_mi_K_im_d_Z', 'sum_d_exp_K_miY_d_alpha',
                                             'sum_d_exp_K_mi_K_im_d_alpha', 'sum_d_exp_K_ii_d_sf2', 'sum_d_exp_K_miY_d_sf2',
                                             'sum_d_exp_K_mi_K_im_d_sf2']
        o['partial_derivatives_names'] = ['F', 'dF_dsum_exp_K_ii', 'dF_dKmm', 'dF_dsum_exp_K_miY', 'dF_dsum_exp_K_mi_K_im']
        o['cache_names'] = ['Kmm', 'Kmm_inv']
        o['flat_global_statistics_bounds'] = ([(None, None)] * (o['M'] * o['Q']) + [(0, None)] + [(0, None)] * o['Q'] + [(0, None)])
        self._pos = positive_mask(o['flat_global_statistics_bounds'])
        o.setdefault('keep', True)
        o.setdefault('fixed_beta', False)
        o.setdefault('drop_out_fraction', 0)

    # ---- parallel_GPLVM.py:286-299
    def flatten_global_statistics(self, gs):
        return numpy.concatenate([numpy.asarray(gs[k], dtype=float).flatten() for k in ('Z', 'sf2', 'alpha', 'beta')])

    def rebuild_global_statistics(self, flat):
        Z, sf2, alpha, beta = split_flat(flat, self.options['M'], self.options['Q'])
        return {'Z': Z, 'sf2': sf2.reshape(1, 1), 'alpha': alpha.reshape(1, -1), 'beta': beta.reshape(1, 1)}

    # ---- parallel_GPLVM.py:373-404
    def clean(self):
        o = self.options
        if not o['keep'] and o['i'] != 'f':
            for group, prefix in (('global_statistics_names', 'global_statistics_'), ('accumulated_statistics_names', 'accumulated_statistics_'),
                                  ('partial_derivatives_names', 'partial_derivatives_'), ('cache_names', 'cache_')):
                for key in o[group]:
                    for it in (-1, o['i'] - 1, o['i']):
                        self.map_reduce.remove(o['statistics'] + '/' + prefix + key + '_' + str(it) + '.npy')

    # ---- parallel_GPLVM.py:222-279
    def likelihood_and_gradient(self, flat_array, iteration, step_size=0):
        o, mr = self.options, self.map_reduce
        flat_t = transform_vec(self._pos, flat_array)
        gs = self.rebuild_global_statistics(flat_t)
        o['i'] = iteration
        o['step_size'] = step_size
        self.clean()
        for key in gs:
            mr.save(o['statistics'] + '/global_statistics_' + key + '_' + str(o['i']) + '.npy', gs[key])
        if self.fast:
            F, gradient = self._evaluate_fast(gs)
        else:
            F, gradient = self._evaluate_compat(gs)
        grad = self.flatten_global_statistics(gradient)
        grad = grad * transform_grad_vec(self._pos, flat_array)
        return -1 * F, -1 * grad

    # ---- the reference's sequence through the backend surface (parallel_GPLVM.py:243-265, 302-369)
    def _evaluate_compat(self, gs):
        o, mr = self.options, self.map_reduce
        t0 = time.time()
        mr.cache(o, gs)
        files, mt, rt = mr.statistics_MR(o)
        t1 = time.time()
        acc = {k: mr.load(f) for k, f in files}
        pt = mr.load_partial_terms(o, gs)
        mr.load_cache(o, pt)
        pt.set_local_statistics(acc['sum_YYT'], acc['sum_exp_K_mi_K_im'], acc['sum_exp_K_miY'], acc['sum_exp_K_ii'], acc['sum_KL'])
        pd = {'F': pt.logmarglik(), 'dF_dsum_exp_K_ii': pt.dF_dexp_K_ii(), 'dF_dsum_exp_K_miY': pt.dF_dexp_K_miY(),
              'dF_dsum_exp_K_mi_K_im': pt.dF_dexp_K_mi_K_im(), 'dF_dKmm': pt.dF_dKmm()}
        for key in pd:
            mr.save(o['statistics'] + '/partial_derivatives_' + key + '_' + str(o['i']) + '.npy', pd[key])
        grad_Z = pt.grad_Z(pd['dF_dKmm'], pt.dKmm_dZ(), pd['dF_dsum_exp_K_miY'], acc['sum_d_exp_K_miY_d_Z'],
                           pd['dF_dsum_exp_K_mi_K_im'], acc['sum_d_exp_K_mi_K_im_d_Z'])
        grad_alpha = pt.grad_alpha(pd['dF_dKmm'], pt.dKmm_dalpha(), pd['dF_dsum_exp_K_miY'], acc['sum_d_exp_K_miY_d_alpha'],
                                   pd['dF_dsum_exp_K_mi_K_im'], acc['sum_d_exp_K_mi_K_im_d_alpha'])
        grad_sf2 = pt.grad_sf2(pd['dF_dKmm'], pt.dKmm_dsf2(), pd['dF_dsum_exp_K_ii'], acc['sum_d_exp_K_ii_d_sf2'],
                               pd['dF_dsum_exp_K_miY'], acc['sum_d_exp_K_miY_d_sf2'], pd['dF_dsum_exp_K_mi_K_im'],
                               acc['sum_d_exp_K_mi_K_im_d_sf2'])
        gradient = {'Z': grad_Z, 'sf2': grad_sf2, 'alpha': grad_alpha,
                    'beta': numpy.zeros((1, 1)) if o['fixed_beta'] else pt.grad_beta()}
        t2 = time.time()
        self.time_acc['time_acc_statistics_map_reduce'].append(t1 - t0)
        self.time_acc['time_acc_statistics_mapper'].append(mt)
        self.time_acc['time_acc_statistics_reducer'].append(rt)
        self.time_acc['time_acc_calculate_global_statistics'].append(t2 - t1)
        if not o['fixed_embeddings']:
            t3 = time.time()
            et = mr.embeddings_MR(o)
            self.time_acc['time_acc_embeddings_MR'].append(time.time() - t3)
            self.time_acc['time_acc_embeddings_MR_mapper'].append(et)
        return pd['F'], gradient

    # ---- two-phase device protocol
    def _evaluate_fast(self, gs):
        o, mr = self.options, self.map_reduce
        t0 = time.time()
        files = mr._input_files(o)
        engines = mr._prepare_shards(o, files, gs)
        # node drop-out (local_MapReduce.py:119-129, 263-264): the same draw as statistics_MR; dropped shards contribute to neither
        # reduction and both reduced buffers are divided by kept/(kept+dropped)
        kept, frac = list(range(len(files))), None
        if o.get('drop_out_fraction', 0) > 0:
            kept, frac = mr._draw_drop_out(len(files), o['drop_out_fraction'])
        reduce = BufferReduce(engines, contributing=[engines[i] for i in kept], fraction=frac)
        root = reduce.root
        want_emb = not o['fixed_embeddings']
        starts = []

        def for_each(items, fn):                # one thread per shard
            starts.append(time.time())
            mr._for_each(items, fn)
        res, self.last_jitter = evaluate(engines, reduce, want_emb, for_each)
        t1 = starts[1]          # phase 1 and the statistics reduce end where the first pass of global step + phase 2 begins
        sc = root.scalars()
        # the artefacts other tools read (--load, predict.py): the five base sums and the partial derivatives
        it = str(o['i'])
        base = {'sum_YYT': sc['sum_YYT'], 'sum_exp_K_ii': sc['sum_exp_K_ii'], 'sum_KL': sc['KL'],
                'sum_exp_K_mi_K_im': root.download('PSI2_SUM'), 'sum_exp_K_miY': root.download('PSI1TY')}
        for key, val in base.items():
            mr.save(o['statistics'] + '/accumulated_statistics_' + key + '_' + it + '.npy', val)
        pd = {'F': res['F'], 'dF_dsum_exp_K_ii': -0.5 * _f(gs['beta']) * o['D'], 'dF_dKmm': root.download('DF_DKMM'),
              'dF_dsum_exp_K_miY': root.download('DF_DPSI1TY'), 'dF_dsum_exp_K_mi_K_im': root.download('DF_DPSI2')}
        for key, val in pd.items():
            mr.save(o['statistics'] + '/partial_derivatives_' + key + '_' + it + '.npy', val)
        if want_emb:
            for f, e in zip(files, engines):
                mr.save(o['embeddings'] + '/' + os.path.basename(f) + '.grad_latest.npy', e.download('GRAD_LATEST'))
        t2 = time.time()
        self.time_acc['time_acc_statistics_map_reduce'].append(t1 - t0)
        self.time_acc['time_acc_calculate_global_statistics'].append(t2 - t1)
        gradient = {'Z': res['grad_Z'], 'sf2': numpy.array([[res['grad_sf2']]]), 'alpha': res['grad_alpha'].reshape(1, -1),
                    'beta': numpy.zeros((1, 1)) if o['fixed_beta'] else numpy.array([[res['grad_beta']]])}
        return res['F'], gradient
