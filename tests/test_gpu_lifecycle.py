"""The context's lifecycle at the C ABI: which call is admitted after which (csrc/lifecycle.h, DESIGN.md section 4.1 "Lifecycle").

Two contexts at N = 5, D = 2, M = 3, Q = 2 -- free embeddings with raw variances (the CG vectors and GRAD_LATEST exist) and fixed embeddings.
Every row of EXPECTED is one situation: a new context after a prefix of the canonical sequence (upload_shard, set_globals, phase1, global_step,
phase2(1), finish), or a fully evaluated context after one MUTATOR.  From that situation every PROBE is called once (the context is evaluated
again in between: a probe changes the state too) and its status code recorded, one digit per probe in PROBES' order; behind a mutator row the
first digit is the mutator's own status.  The digits were recorded by observe() of this file on the library built from the commit BEFORE
the lifecycle moved into csrc/lifecycle.h (profiles/lifecycle_parent_table.txt), inconsistencies included: what is asserted is that nothing moved.

Whether the prep kernels' results are kept (fixed embeddings: they run once per upload / origin / mode, Lifecycle::prep_is_current) has no
status code to show: test_fixed_prep_is_never_stale
follows every mutator by a complete evaluation WITHOUT a new upload and compares it with a new context given the same final inputs."""
import ctypes

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)

pytestmark = pytest.mark.gpu

N, D, M, Q = 5, 2, 3, 2
KINDS = ('free', 'fixed')
PREFIXES = ('fresh', 'upload_shard', 'set_globals', 'phase1', 'global_step', 'phase2', 'finish')
_r = np.random.RandomState(7)
Y0, XMU0, XMU1, XS_RAW = _r.randn(N, D), _r.randn(N, Q), _r.randn(N, Q), _r.randn(N, Q)
Z0 = _r.randn(M, Q)
ALPHA, SF2, BETA = np.full(Q, 0.25), 1.3, 2.0
# far enough that gp_set_globals chooses a new origin: further from the old column mean than the spread of Z plus one length scale (choose_origin)
Z_FAR = Z0 + 6.0
assert np.all(6.0 > np.max(np.abs(Z0 - Z0.mean(0)), 0) + ALPHA ** -0.5)
DIR = _r.randn(2, N, Q)
PSI2, CMAT = np.eye(M) * 2.0, _r.randn(M, D)
XNEW, SNEW, YNEW = _r.randn(1, Q), np.full((1, Q), 0.5), _r.randn(1, D)

_dp = ctypes.POINTER(ctypes.c_double)
_p = lambda a: a.ctypes.data_as(_dp)          # noqa: E731  (every array above and below is C-contiguous float64)


class Ctx(object):
    """One gp_ctx of a kind, with the inputs it was last given (what a new context needs to arrive at the same place)."""

    def __init__(self, lib, kind):
        self.lib, self.kind, self.h = lib, kind, ctypes.c_void_p()
        assert lib.gp_create(ctypes.byref(self.h), 0, N, D, M, Q) == 0
        self.raw = 1 if kind == 'free' else 0
        self.XS = XS_RAW if kind == 'free' else np.zeros((N, Q))
        self.xmu, self.z = XMU0, Z0

    def close(self):
        self.lib.gp_destroy(self.h)

    # ---- the canonical sequence
    def upload_shard(self, xmu=XMU0):
        self.xmu = xmu
        return self.lib.gp_upload_shard(self.h, _p(Y0), _p(xmu), _p(self.XS), self.raw)

    def set_globals(self, z=Z0):
        self.z = z
        return self.lib.gp_set_globals(self.h, _p(z), SF2, _p(ALPHA), BETA, N, 0.0)

    def finish(self, grads=True):
        F, gs, gb = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        gZ, ga = np.empty((M, Q)), np.empty(Q)
        rc = self.lib.gp_finish(self.h, ctypes.byref(F), _p(gZ) if grads else None, ctypes.byref(gs), _p(ga) if grads else None, ctypes.byref(gb))
        return rc, dict(F=np.float64(F.value), grad_Z=gZ, grad_alpha=ga, grad_sf2=np.float64(gs.value), grad_beta=np.float64(gb.value))

    def steps(self, want):
        lib, h = self.lib, self.h
        return [('upload_shard', lambda: self.upload_shard(self.xmu)), ('set_globals', lambda: self.set_globals(self.z)), ('phase1', lambda: lib.gp_phase1(h)),
                ('global_step', lambda: lib.gp_global_step(h)), ('phase2', lambda: lib.gp_phase2(h, want)), ('finish', lambda: self.finish()[0])]

    def run(self, upto='finish', want=1, skip_upload=False):
        """The canonical sequence up to and including ``upto`` ('fresh': nothing), with the canonical inputs -- or, with ``skip_upload``, from
        gp_set_globals on with what the context was last given; every step must succeed."""
        if upto == 'fresh':
            return
        if not skip_upload:
            self.xmu, self.z = XMU0, Z0
        for name, fn in self.steps(want)[1 if skip_upload else 0:]:
            rc = fn()
            assert rc == 0, '%s failed in the canonical sequence: %d %s' % (name, rc, self.lib.gp_last_error(self.h))
            if name == upto:
                return

    def download(self, name):
        from gparml_amd import _lib
        n = {'GRAD_LATEST': 2 * N * Q, 'X_MU': N * Q, 'DKMM_DZ': M * Q * M, 'PSI2_POINTS': N * M * M}[name]
        return self.lib.gp_download(self.h, _lib.ARR[name], _p(np.empty(n)), n)


def _predict(c):
    return c.lib.gp_predict(c.h, 1, _p(XNEW), None, 0, 0, _p(np.empty((1, D))), _p(np.empty((1, 1))))


def _infer(c):
    return c.lib.gp_infer_objective(c.h, 1, _p(YNEW), None, 0, _p(XNEW), _p(SNEW), 0, _p(np.empty(1)), _p(np.empty((1, Q))), _p(np.empty((1, Q))))


PROBES = [
    ('phase1', lambda c: c.lib.gp_phase1(c.h)),
    ('stats_unpack', lambda c: c.lib.gp_stats_unpack(c.h)),
    ('scale_buffer(0)', lambda c: c.lib.gp_scale_buffer(c.h, 0, 1.0)),
    ('scale_buffer(1)', lambda c: c.lib.gp_scale_buffer(c.h, 1, 1.0)),
    ('global_step', lambda c: c.lib.gp_global_step(c.h)),
    ('global_status', lambda c: c.lib.gp_global_status(c.h, None)),
    ('phase2', lambda c: c.lib.gp_phase2(c.h, 1)),
    ('finish(grads)', lambda c: c.finish(True)[0]),
    ('finish(F only)', lambda c: c.finish(False)[0]),
    ('predict', _predict),
    ('infer_objective', _infer),
    ('download GRAD_LATEST', lambda c: c.download('GRAD_LATEST')),
    ('download X_MU', lambda c: c.download('X_MU')),
    ('download DKMM_DZ', lambda c: c.download('DKMM_DZ')),
    ('download PSI2_POINTS', lambda c: c.download('PSI2_POINTS')),
    ('cg_update(4)', lambda c: c.lib.gp_cg_update(c.h, 4, 0.0)),
]

# name -> f(context, second context of the same kind, fully evaluated) -> status
MUTATORS = [
    ('upload_shard', lambda c, s: c.upload_shard(XMU1)),
    ('upload_embeddings', lambda c, s: (setattr(c, 'xmu', XMU1), c.lib.gp_upload_embeddings(c.h, _p(XMU1), _p(c.XS), c.raw))[1]),
    ('set_direction(d)', lambda c, s: c.lib.gp_set_direction(c.h, _p(DIR))),
    ('set_direction(NULL)', lambda c, s: c.lib.gp_set_direction(c.h, None)),
    ('set_globals(same Z)', lambda c, s: c.set_globals(Z0)),
    ('set_globals(far Z)', lambda c, s: c.set_globals(Z_FAR)),
    ('phase1', lambda c, s: c.lib.gp_phase1(c.h)),
    ('set_local_statistics', lambda c, s: c.lib.gp_set_local_statistics(c.h, 3.0, _p(PSI2), _p(CMAT), 4.0, 0.5)),
    ('stats_pack', lambda c, s: c.lib.gp_stats_pack(c.h)),
    ('stats_unpack', lambda c, s: c.lib.gp_stats_unpack(c.h)),
    ('buffer_combine(add)', lambda c, s: c.lib.gp_buffer_combine(c.h, s.h, 0, 0)),
    ('buffer_combine(copy)', lambda c, s: c.lib.gp_buffer_combine(c.h, s.h, 0, 1)),
    ('scale_buffer(0)', lambda c, s: c.lib.gp_scale_buffer(c.h, 0, 1.0)),
    ('scale_buffer(0, f=0)', lambda c, s: c.lib.gp_scale_buffer(c.h, 0, 0.0)),
    ('scale_buffer(1)', lambda c, s: c.lib.gp_scale_buffer(c.h, 1, 1.0)),
    ('global_step', lambda c, s: c.lib.gp_global_step(c.h)),
    ('phase2(0)', lambda c, s: c.lib.gp_phase2(c.h, 0)),
    ('phase2(1)', lambda c, s: c.lib.gp_phase2(c.h, 1)),
] + [('cg_update(%d)' % w, lambda c, s, w=w: c.lib.gp_cg_update(c.h, w, 0.25)) for w in range(6)]

ROWS = ['after ' + p if p != 'fresh' else p for p in PREFIXES] + [m[0] for m in MUTATORS]

# status digits: 0 GP_OK, 1 BAD_ARG, 2 NOT_PD, 3 NON_FINITE, 4 HIP, 5 STATE, 6 UNSUPPORTED, 7 RETRY_JITTER
EXPECTED = {
    'free': {
        'fresh':                   '5555555555555555',
        'after upload_shard':      '5555555555550555',
        'after set_globals':       '0555555555550555',
        'after phase1':            '0505055555550505',
        'after global_step':       '0505000500050005',
        'after phase2':            '0500000000000000',
        'after finish':            '0500000000000000',
        'upload_shard':            '0|0555555555550550',
        'upload_embeddings':       '0|0555555555550550',
        'set_direction(d)':        '0|0555555555550550',
        'set_direction(NULL)':     '0|0500000000000000',
        'set_globals(same Z)':     '0|0555555555550550',
        'set_globals(far Z)':      '0|0555555555550550',
        'phase1':                  '0|0505055555550500',
        'set_local_statistics':    '0|0500000005500000',
        'stats_pack':              '0|0000000000000000',
        'stats_unpack':            '5|0500000005500000',
        'buffer_combine(add)':     '0|0500000005500000',
        'buffer_combine(copy)':    '0|0500000005500000',
        'scale_buffer(0)':         '0|0500000005500000',
        'scale_buffer(0, f=0)':    '0|0500000005500000',
        'scale_buffer(1)':         '0|0500000000000000',
        'global_step':             '0|0505000500050000',
        'phase2(0)':               '0|0500000000050000',
        'phase2(1)':               '0|0500000000000000',
        'cg_update(0)':            '0|0500000000000000',
        'cg_update(1)':            '0|0500000000000000',
        'cg_update(2)':            '0|0555555555550550',
        'cg_update(3)':            '0|0500000000000000',
        'cg_update(4)':            '0|0500000000000000',
        'cg_update(5)':            '0|0500000000000000',
    },
    'fixed': {
        'fresh':                   '5555555555555555',
        'after upload_shard':      '5555555555550555',
        'after set_globals':       '0555555555550555',
        'after phase1':            '0505055555550505',
        'after global_step':       '0505000500050005',
        'after phase2':            '0500000000030005',
        'after finish':            '0500000000030005',
        'upload_shard':            '0|0555555555550555',
        'upload_embeddings':       '0|0555555555550555',
        'set_direction(d)':        '0|0555555555550555',
        'set_direction(NULL)':     '0|0500000000030005',
        'set_globals(same Z)':     '0|0555555555550555',
        'set_globals(far Z)':      '0|0555555555550555',
        'phase1':                  '0|0505055555550505',
        'set_local_statistics':    '0|0500000005530005',
        'stats_pack':              '0|0000000000030005',
        'stats_unpack':            '5|0500000005530005',
        'buffer_combine(add)':     '0|0500000005530005',
        'buffer_combine(copy)':    '0|0500000005530005',
        'scale_buffer(0)':         '0|0500000005530005',
        'scale_buffer(0, f=0)':    '0|0500000005530005',
        'scale_buffer(1)':         '0|0500000000030005',
        'global_step':             '0|0505000500050005',
        'phase2(0)':               '0|0500000000050005',
        'phase2(1)':               '0|0500000000030005',
        'cg_update(0)':            '5|0500000000030005',
        'cg_update(1)':            '5|0500000000030005',
        'cg_update(2)':            '5|0500000000030005',
        'cg_update(3)':            '5|0500000000030005',
        'cg_update(4)':            '5|0500000000030005',
        'cg_update(5)':            '5|0500000000030005',
    },
}


def _lib():
    from gparml_amd import _lib as L
    return L.load()


def observe_row(lib, kind, row):
    """The digits of one row: every probe from the row's situation, on a context brought there anew for each."""
    out = ''
    if row in ROWS[:len(PREFIXES)]:
        for _, probe in PROBES:
            c = Ctx(lib, kind)                 # a new context per probe: nothing of an earlier probe is left
            c.run(row.replace('after ', ''))
            out += '%d' % probe(c)
            c.close()
        return out
    mutate = dict(MUTATORS)[row]
    c, src = Ctx(lib, kind), Ctx(lib, kind)
    src.run()
    for i, (_, probe) in enumerate(PROBES):
        c.run()                                # from gp_upload_shard on: the evaluation again, on the same context
        rc = mutate(c, src)
        out += ('%d|' % rc if i == 0 else '') + '%d' % probe(c)
        assert rc == int(out[0]), 'the mutator itself returned %d at first and %d now' % (int(out[0]), rc)
    c.close(); src.close()
    return out


def observe():
    """{kind: {row: digits}} of the loaded library, as EXPECTED spells it."""
    lib = _lib()
    return {kind: {row: observe_row(lib, kind, row) for row in ROWS} for kind in KINDS}


@pytest.mark.parametrize('row', ROWS)
@pytest.mark.parametrize('kind', KINDS)
def test_status_codes_are_the_parent_commits(kind, row):
    got, want = observe_row(_lib(), kind, row), EXPECTED[kind][row]
    names = [p[0] for p in PROBES]
    diff = ['%s: %s, recorded %s' % (n, g, w) for n, g, w in zip(names, got.split('|')[-1], want.split('|')[-1]) if g != w]
    print('[lifecycle] %-5s %-24s %s' % (kind, row, got))
    assert got == want, '%s context, %s: %s' % (kind, row, '; '.join(diff) or 'the mutator returned %s, recorded %s' % (got[0], want[0]))


def test_every_row_and_probe_is_recorded():
    assert sorted(EXPECTED) == sorted(KINDS)
    for kind in KINDS:
        assert sorted(EXPECTED[kind]) == sorted(ROWS)
        assert all(len(v.split('|')[-1]) == len(PROBES) for v in EXPECTED[kind].values())


@pytest.mark.parametrize('name', [m[0] for m in MUTATORS])
def test_fixed_prep_is_never_stale(name):
    """Fixed embeddings, phase2(ctx, 0): the prep kernels' outputs are kept from evaluation to evaluation.  After any mutator, an evaluation from
    gp_set_globals on (no upload) equals a new context's with the same final embeddings and Z -- bit for bit where both have the same origin
    of the centred coordinates, within tests/test_gpu_translation.py's bounds for a moved origin after the far-moved Z."""
    import shift_ref
    from test_gpu_translation import TOL
    lib = _lib()
    c, src = Ctx(lib, 'fixed'), Ctx(lib, 'fixed')
    src.run(want=0)
    c.run(want=0)
    dict(MUTATORS)[name](c, src)
    c.run(want=0, skip_upload=True)            # gp_set_globals again with the Z that was last set, then the rest
    rc, got = c.finish()
    new = Ctx(lib, 'fixed')
    assert new.upload_shard(c.xmu) == 0
    new.z = c.z
    new.run(want=0, skip_upload=True)
    rc2, want = new.finish()
    assert rc == 0 and rc2 == 0
    for k in ('F', 'grad_Z', 'grad_alpha', 'grad_sf2', 'grad_beta'):
        if name == 'set_globals(far Z)':
            err = shift_ref.rel_err(got[k], want[k])
            print('[lifecycle] %s %s rel. error %.3e (bound %.0e)' % (name, k, err, TOL[k]))
            assert err <= TOL[k], (name, k, err)
        else:
            assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (name, k, got[k], want[k])
    for x in (c, src, new):
        x.close()
