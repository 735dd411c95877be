"""The argument checks of the entry points at new rows (csrc/api.hip): status code and full message of every bad call, as the parent commit gave them.

api.hip writes each check once (inputs at new rows, the resident rows behind a NULL array, the observed entries of Y) and calls it from gp_predict,
gp_predict_score, the joint / grad / curve / paths entries, the four gp_infer_* entries, gp_kmeans_accumulate, the PCA passes, gp_select_begin and
the nearest-row search.  CASES is a table of bad calls on one tiny model (N = 64, M = 8, Q = 2, D = 3, one global step): n < 0, NULL where data is
required, a NaN in each input array, negative and zero variances, the resident rows before an upload and with the wrong n, a row with nothing
observed, a non-finite observed entry, and calls with two faults, which pin the order of the checks.  Every case fails in host code before anything
is launched.  What each returned on the library built from the commit BEFORE the checks were hoisted is profiles/entry_checks_parent_table.txt
(recorded by running this file as a script with GPARML_LIB set to that build); what is asserted is that nothing moved, byte for byte."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT

N, D, M, Q, n = 64, 3, 8, 2, 4
TABLE = os.path.join(ROOT, 'profiles', 'entry_checks_parent_table.txt')
NAN, INF = float('nan'), float('inf')

_r = np.random.RandomState(5)
Y0, XMU0, XS0, Z0 = _r.randn(N, D), _r.randn(N, Q), _r.uniform(0.1, 0.4, size=(N, Q)), _r.randn(M, Q)
ALPHA, SF2, BETA = np.full(Q, 0.5), 1.2, 3.0
PSI2, CMAT = np.eye(M) * 2.0, _r.randn(M, D)
X, S, Y = _r.randn(n, Q), _r.uniform(0.1, 0.4, size=(n, Q)), _r.randn(n, D)
OBS = np.ones((n, D), dtype=np.uint8)
EPS = _r.randn(2, n, D)
CENTRES = _r.randn(3, Q)
OUT = np.empty(4096)            # every output of every entry fits: a call that passed its checks after all would still write inside it
IOUT = np.empty(4096, dtype=np.int64)


def bad(a, *at):
    """a copy of ``a`` with flat element i set to v for every (i, v)"""
    b = np.array(a, dtype=np.float64, copy=True)
    for i, v in at:
        b.flat[i] = v
    return b


def hide(*rows):
    o = OBS.copy()
    o[list(rows)] = 0
    return o


def p(a):
    if a is None:
        return None
    if a.dtype == np.uint8:
        return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    if a.dtype == np.int32:
        return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    if a.dtype == np.int64:
        return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


o, io = p(OUT), p(IOUT)
COLS = np.array([0, 2], dtype=np.int32)
# (name, context, call): context 'model' has data and a global step, 'bare' a global step on injected statistics and no data
CASES = []


def case(name, ctx, fn):
    CASES.append((name, ctx, fn))


pr = lambda L, h, nn=n, x=X, s=None, raw=0, fl=0: L.gp_predict(h, nn, p(x), p(s), raw, fl, o, o)       # noqa: E731
case('predict n<0', 'model', lambda L, h: pr(L, h, nn=-1))
case('predict n<0 and flags', 'model', lambda L, h: pr(L, h, nn=-1, fl=8))
case('predict flags', 'model', lambda L, h: pr(L, h, fl=8))
case('predict X_mu NULL', 'model', lambda L, h: pr(L, h, x=None))
case('predict X_mu NaN', 'model', lambda L, h: pr(L, h, x=bad(X, (5, NAN))))
case('predict X_mu inf uncertain', 'model', lambda L, h: pr(L, h, x=bad(X, (0, INF)), s=S))
case('predict X_S NaN', 'model', lambda L, h: pr(L, h, s=bad(S, (7, NAN))))
case('predict X_S negative', 'model', lambda L, h: pr(L, h, s=bad(S, (2, -0.5))))
case('predict X_S inf raw', 'model', lambda L, h: pr(L, h, s=bad(S, (2, INF)), raw=1))
case('predict X_S negative before X_mu NaN', 'model', lambda L, h: pr(L, h, x=bad(X, (3, NAN)), s=bad(S, (1, -1.0))))
case('predict X_mu NaN before X_S negative', 'model', lambda L, h: pr(L, h, x=bad(X, (1, NAN)), s=bad(S, (3, -1.0))))
case('predict X_mu NaN and X_S negative in one element', 'model', lambda L, h: pr(L, h, x=bad(X, (3, NAN)), s=bad(S, (3, -1.0))))

sc = lambda L, h, nn=n, x=X, s=None, raw=0, y=Y, ob=None, fl=1: L.gp_predict_score(h, nn, p(x), p(s), raw, p(y), p(ob), fl, o, o, o, o)       # noqa: E731
YN = _r.randn(N, D)
case('score n<0', 'model', lambda L, h: sc(L, h, nn=-1))
case('score flags', 'model', lambda L, h: sc(L, h, fl=4))
case('score resident variances with host rows', 'model', lambda L, h: sc(L, h, fl=3))
case('score resident before upload', 'bare', lambda L, h: sc(L, h, nn=N, x=None, y=None))
case('score resident before upload and wrong n', 'bare', lambda L, h: sc(L, h, nn=5, x=None, y=None))
case('score resident wrong n', 'model', lambda L, h: sc(L, h, nn=5, x=None, y=None))
case('score resident n = 0', 'model', lambda L, h: sc(L, h, nn=0, x=None, y=None))
case('score resident with X_S', 'model', lambda L, h: sc(L, h, nn=N, x=None, s=XS0, y=None))
case('score resident Y NaN', 'model', lambda L, h: sc(L, h, nn=N, x=None, y=bad(YN, (10 * D + 2, NAN))))
case('score Y NULL', 'model', lambda L, h: sc(L, h, y=None))
case('score Y NULL and X_mu NaN', 'model', lambda L, h: sc(L, h, x=bad(X, (0, NAN)), y=None))
case('score X_mu NaN', 'model', lambda L, h: sc(L, h, x=bad(X, (5, NAN))))
case('score X_S NaN', 'model', lambda L, h: sc(L, h, s=bad(S, (5, NAN))))
case('score X_S negative', 'model', lambda L, h: sc(L, h, s=bad(S, (5, -1e-3))))
case('score X_S negative before X_mu NaN', 'model', lambda L, h: sc(L, h, x=bad(X, (6, NAN)), s=bad(S, (5, -1.0))))
case('score Y NaN', 'model', lambda L, h: sc(L, h, y=bad(Y, (2 * D + 1, NAN))))
case('score Y inf under a mask', 'model', lambda L, h: sc(L, h, y=bad(Y, (3 * D + 2, INF)), ob=OBS))
case('score Y NaN behind a hidden NaN', 'model', lambda L, h: sc(L, h, y=bad(Y, (0, NAN), (1 * D + 1, NAN)), ob=hide(0)))
case('score X_mu NaN and Y NaN', 'model', lambda L, h: sc(L, h, x=bad(X, (7, NAN)), y=bad(Y, (0, NAN))))

jo = lambda L, h, nn=n, x=X, fl=0: L.gp_predict_joint(h, nn, p(x), fl, o, o)       # noqa: E731
sa = lambda L, h, nn=n, x=X, fl=0, jit=1e-8, nd=2, e=EPS, out=o: L.gp_predict_sample(h, nn, p(x), fl, jit, nd, p(e), out, o)       # noqa: E731
gr = lambda L, h, nn=n, x=X, fl=0: L.gp_predict_grad(h, nn, p(x), fl, o, o, o, o)       # noqa: E731
cu = lambda L, h, nc=2, T=2, x=X, fl=0: L.gp_curve_energy(h, nc, T, p(x), fl, o, o, o)       # noqa: E731
case('joint n<0', 'model', lambda L, h: jo(L, h, nn=-1))
case('joint n<0 and flags', 'model', lambda L, h: jo(L, h, nn=-3, fl=2))
case('joint flags', 'model', lambda L, h: jo(L, h, fl=2))
case('joint X NULL', 'model', lambda L, h: jo(L, h, x=None))
case('joint X NaN', 'model', lambda L, h: jo(L, h, x=bad(X, (4, NAN))))
case('sample n<0', 'model', lambda L, h: sa(L, h, nn=-1))
case('sample jitter', 'model', lambda L, h: sa(L, h, jit=-1.0))
case('sample eps NULL', 'model', lambda L, h: sa(L, h, e=None))
case('sample X NULL', 'model', lambda L, h: sa(L, h, x=None))
case('sample X inf', 'model', lambda L, h: sa(L, h, x=bad(X, (7, -INF))))
case('sample eps NaN', 'model', lambda L, h: sa(L, h, e=bad(EPS, (n * D + 1, NAN))))
case('sample X NaN and eps NaN', 'model', lambda L, h: sa(L, h, x=bad(X, (0, NAN)), e=bad(EPS, (0, NAN))))
case('grad n<0', 'model', lambda L, h: gr(L, h, nn=-1))
case('grad flags', 'model', lambda L, h: gr(L, h, fl=1))
case('grad X NULL', 'model', lambda L, h: gr(L, h, x=None))
case('grad X NaN', 'model', lambda L, h: gr(L, h, x=bad(X, (1, NAN))))
case('curve n_curves<0', 'model', lambda L, h: cu(L, h, nc=-1))
case('curve T<2', 'model', lambda L, h: cu(L, h, T=1))
case('curve X NULL', 'model', lambda L, h: cu(L, h, x=None))
case('curve X NaN', 'model', lambda L, h: cu(L, h, x=bad(X, (6, NAN))))

pe = lambda L, h, nn=n, x=X, fl=0, out=o: L.gp_paths_eval(h, nn, p(x), fl, out, o)       # noqa: E731
case('paths_eval without draws', 'bare', lambda L, h: pe(L, h))
case('paths_eval n<0', 'model', lambda L, h: pe(L, h, nn=-1))
case('paths_eval flags', 'model', lambda L, h: pe(L, h, fl=1))
case('paths_eval X NULL', 'model', lambda L, h: pe(L, h, x=None))
case('paths_eval out NULL', 'model', lambda L, h: pe(L, h, out=None))
case('paths_eval X NaN', 'model', lambda L, h: pe(L, h, x=bad(X, (3, NAN))))
case('paths_set omega NaN', 'bare', lambda L, h: L.gp_paths_set(h, 1, 2, p(bad(_r.randn(2, Q), (1, NAN))), None, p(_r.randn(1, 4, D)), p(_r.randn(1, M, D))))

for who in ('gp_infer_objective', 'gp_infer_latent'):
    def io_(L, h, nn=n, y=Y, c=None, nc=0, x=X, s=S, raw=0, who=who):
        if who == 'gp_infer_objective':
            return L.gp_infer_objective(h, nn, p(y), p(c), nc, p(x), p(s), raw, o, o, o)
        return L.gp_infer_latent(h, nn, p(y), p(c), nc, p(np.array(x)) if x is not None else None, p(np.array(s)) if s is not None else None, raw, 3, 1e-6, o,
                                 p(np.empty(64, dtype=np.int32)))
    t = who[3:]
    case(t + ' n<0', 'model', lambda L, h, f=io_: f(L, h, nn=-1))
    case(t + ' n<0 and n_cols', 'model', lambda L, h, f=io_: f(L, h, nn=-1, nc=1))
    case(t + ' n_cols without cols', 'model', lambda L, h, f=io_: f(L, h, nc=1))
    case(t + ' n_cols > D', 'model', lambda L, h, f=io_: f(L, h, c=COLS, nc=4))
    case(t + ' cols not increasing', 'model', lambda L, h, f=io_: f(L, h, c=np.array([2, 0], dtype=np.int32), nc=2))
    case(t + ' Y NULL', 'model', lambda L, h, f=io_: f(L, h, y=None))
    case(t + ' X_S NULL', 'model', lambda L, h, f=io_: f(L, h, s=None))
    case(t + ' X_mu NaN', 'model', lambda L, h, f=io_: f(L, h, x=bad(X, (5, NAN))))
    case(t + ' X_S NaN', 'model', lambda L, h, f=io_: f(L, h, s=bad(S, (5, NAN))))
    case(t + ' X_S zero', 'model', lambda L, h, f=io_: f(L, h, s=bad(S, (4, 0.0))))
    case(t + ' X_S negative', 'model', lambda L, h, f=io_: f(L, h, s=bad(S, (4, -0.1))))
    case(t + ' raw X_S whose softplus is zero', 'model', lambda L, h, f=io_: f(L, h, s=bad(S, (4, -800.0)), raw=1))
    case(t + ' X_S zero before X_mu NaN', 'model', lambda L, h, f=io_: f(L, h, x=bad(X, (3, NAN)), s=bad(S, (1, 0.0))))
    case(t + ' X_mu NaN before X_S zero', 'model', lambda L, h, f=io_: f(L, h, x=bad(X, (1, NAN)), s=bad(S, (3, 0.0))))
    case(t + ' Y NaN', 'model', lambda L, h, f=io_: f(L, h, y=bad(Y, (1 * D + 1, NAN))))
    case(t + ' Y inf in a listed column', 'model', lambda L, h, f=io_: f(L, h, y=bad(Y, (1, NAN), (2 * D + 2, INF)), c=COLS, nc=2))
    case(t + ' X_mu NaN and Y NaN', 'model', lambda L, h, f=io_: f(L, h, x=bad(X, (7, NAN)), y=bad(Y, (0, NAN))))
case('infer_latent max_iters', 'model', lambda L, h: L.gp_infer_latent(h, n, p(Y), None, 0, p(X.copy()), p(S.copy()), 0, -1, 1e-6, o, p(np.empty(64, dtype=np.int32))))

for who in ('gp_infer_objective_rows', 'gp_infer_latent_rows'):
    def ir_(L, h, nn=n, y=Y, ob=OBS, x=X, s=S, raw=0, who=who):
        if who == 'gp_infer_objective_rows':
            return L.gp_infer_objective_rows(h, nn, p(y), p(ob), p(x), p(s), raw, o, o, o)
        return L.gp_infer_latent_rows(h, nn, p(y), p(ob), p(np.array(x)) if x is not None else None, p(np.array(s)) if s is not None else None, raw, 3, 1e-6, o,
                                      p(np.empty(64, dtype=np.int32)))
    t = who[3:]
    case(t + ' n<0', 'model', lambda L, h, f=ir_: f(L, h, nn=-1))
    case(t + ' observed NULL', 'model', lambda L, h, f=ir_: f(L, h, ob=None))
    case(t + ' X_mu NULL', 'model', lambda L, h, f=ir_: f(L, h, x=None))
    case(t + ' X_mu NaN', 'model', lambda L, h, f=ir_: f(L, h, x=bad(X, (2, NAN))))
    case(t + ' X_S zero', 'model', lambda L, h, f=ir_: f(L, h, s=bad(S, (2, 0.0))))
    case(t + ' X_S NaN raw', 'model', lambda L, h, f=ir_: f(L, h, s=bad(S, (2, NAN)), raw=1))
    case(t + ' row with nothing observed', 'model', lambda L, h, f=ir_: f(L, h, ob=hide(2)))
    case(t + ' Y NaN', 'model', lambda L, h, f=ir_: f(L, h, y=bad(Y, (1 * D + 2, NAN))))
    case(t + ' empty row 0 before Y NaN in row 1', 'model', lambda L, h, f=ir_: f(L, h, y=bad(Y, (1 * D, NAN)), ob=hide(0)))
    case(t + ' Y NaN in row 0 before empty row 2', 'model', lambda L, h, f=ir_: f(L, h, y=bad(Y, (1, NAN)), ob=hide(2)))
    case(t + ' X_S zero and empty row', 'model', lambda L, h, f=ir_: f(L, h, s=bad(S, (7, 0.0)), ob=hide(0)))

km = lambda L, h, nn=n, x=X, K=3, c=CENTRES: L.gp_kmeans_accumulate(h, nn, p(x), K, p(c), o, io, o, None)       # noqa: E731
case('kmeans n<0', 'model', lambda L, h: km(L, h, nn=-1))
case('kmeans K<1', 'model', lambda L, h: km(L, h, K=0))
case('kmeans centres NULL', 'model', lambda L, h: km(L, h, c=None))
case('kmeans resident before upload', 'bare', lambda L, h: km(L, h, nn=N, x=None))
case('kmeans resident before upload and centres NaN', 'bare', lambda L, h: km(L, h, nn=N, x=None, c=bad(CENTRES, (0, NAN))))
case('kmeans resident wrong n', 'model', lambda L, h: km(L, h, nn=N + 1, x=None))
case('kmeans centres NaN', 'model', lambda L, h: km(L, h, c=bad(CENTRES, (5, NAN))))
case('kmeans X NaN', 'model', lambda L, h: km(L, h, x=bad(X, (5, NAN))))
case('kmeans centres NaN and X NaN', 'model', lambda L, h: km(L, h, c=bad(CENTRES, (5, NAN)), x=bad(X, (0, NAN))))

CEN, PMAT = _r.randn(D), _r.randn(D, 2)
scat = lambda L, h, nn=n, y=Y, c=CEN: L.gp_scatter_accumulate(h, nn, p(y), p(c), o, o)       # noqa: E731
proj = lambda L, h, nn=n, y=Y, m=CEN, P=PMAT, out=o: L.gp_project_rows(h, nn, p(y), p(m), p(P), 2, out)       # noqa: E731
case('scatter n<0', 'model', lambda L, h: scat(L, h, nn=-1))
case('scatter centre NULL', 'model', lambda L, h: scat(L, h, c=None))
case('scatter resident before upload', 'bare', lambda L, h: scat(L, h, nn=N, y=None))
case('scatter resident wrong n', 'model', lambda L, h: scat(L, h, nn=2, y=None))
case('scatter Y NaN', 'model', lambda L, h: scat(L, h, y=bad(Y, (3, NAN))))
case('scatter centre NaN', 'model', lambda L, h: scat(L, h, c=bad(CEN, (1, NAN))))
case('scatter Y NaN and centre NaN', 'model', lambda L, h: scat(L, h, y=bad(Y, (3, NAN)), c=bad(CEN, (1, NAN))))
case('project n<0', 'model', lambda L, h: proj(L, h, nn=-1))
case('project resident before upload', 'bare', lambda L, h: proj(L, h, nn=N, y=None))
case('project resident wrong n', 'model', lambda L, h: proj(L, h, nn=2, y=None))
case('project Y inf', 'model', lambda L, h: proj(L, h, y=bad(Y, (3, INF))))
case('project P NaN', 'model', lambda L, h: proj(L, h, P=bad(PMAT, (1, NAN))))
case('project X NULL', 'model', lambda L, h: proj(L, h, out=None))

sel = lambda L, h, nn=n, x=X, K=2, a=ALPHA: L.gp_select_begin(h, nn, p(x), K, 1.0, p(a), 0.0)       # noqa: E731
case('select n<0', 'model', lambda L, h: sel(L, h, nn=-1))
case('select alpha NULL', 'model', lambda L, h: sel(L, h, a=None))
case('select resident before upload', 'bare', lambda L, h: sel(L, h, nn=N, x=None))
case('select resident wrong n', 'model', lambda L, h: sel(L, h, nn=N - 1, x=None))
case('select X NaN', 'model', lambda L, h: sel(L, h, x=bad(X, (2, NAN))))
case('select alpha negative and X NaN', 'model', lambda L, h: sel(L, h, x=bad(X, (2, NAN)), a=bad(ALPHA, (0, -1.0))))

YT = _r.randn(6, D)
nr = lambda L, h, nt=6, yt=YT, nn=n, y=Y, c=None, nc=0: L.gp_nearest_rows(h, nt, p(yt), nn, p(y), p(c), nc, o, io, None)       # noqa: E731
nm = lambda L, h, nt=6, yt=YT, nn=n, y=Y, ob=OBS: L.gp_nearest_rows_masked(h, nt, p(yt), nn, p(y), p(ob), o, io, None)       # noqa: E731
case('nearest n<0', 'model', lambda L, h: nr(L, h, nn=-1))
case('nearest resident before upload', 'bare', lambda L, h: nr(L, h, yt=None))
case('nearest n_train<0', 'model', lambda L, h: nr(L, h, nt=-1))
case('nearest Y_test NULL', 'model', lambda L, h: nr(L, h, y=None))
case('nearest Y_test NaN', 'model', lambda L, h: nr(L, h, y=bad(Y, (4, NAN))))
case('nearest Y_train NaN', 'model', lambda L, h: nr(L, h, yt=bad(YT, (4, NAN))))
case('nearest Y_test NaN and Y_train NaN', 'model', lambda L, h: nr(L, h, y=bad(Y, (4, NAN)), yt=bad(YT, (4, NAN))))
case('nearest_masked resident before upload', 'bare', lambda L, h: nm(L, h, yt=None))
case('nearest_masked observed NULL', 'model', lambda L, h: nm(L, h, ob=None))
case('nearest_masked row with nothing observed', 'model', lambda L, h: nm(L, h, ob=hide(1)))
case('nearest_masked Y_train inf', 'model', lambda L, h: nm(L, h, yt=bad(YT, (0, INF))))

NAMES = [c[0] for c in CASES]
assert len(set(NAMES)) == len(NAMES)


def contexts(lib):
    """'model': uploaded data, one global step, one set of path draws.  'bare': no data; a global step on injected statistics."""
    hm, hb = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.gp_create(ctypes.byref(hm), 0, N, D, M, Q) == 0 and lib.gp_create(ctypes.byref(hb), 0, N, D, M, Q) == 0
    assert lib.gp_upload_shard(hm, p(Y0), p(XMU0), p(XS0), 0) == 0
    for h in (hm, hb):
        assert lib.gp_set_globals(h, p(Z0), SF2, p(ALPHA), BETA, N, 0.0) == 0
    assert lib.gp_phase1(hm) == 0
    assert lib.gp_set_local_statistics(hb, 3.0, p(PSI2), p(CMAT), 4.0, 0.5) == 0
    for h in (hm, hb):
        assert lib.gp_global_step(h) == 0 and lib.gp_global_status(h, None) == 0, lib.gp_last_error(h)
    assert lib.gp_paths_set(hm, 1, 2, p(_r.randn(2, Q)), None, p(_r.randn(1, 4, D)), p(_r.randn(1, M, D))) == 0, lib.gp_last_error(hm)
    return {'model': hm, 'bare': hb}


def observe(lib, ctx, fn):
    rc = fn(lib, ctx)
    msg = lib.gp_last_error(ctx)
    return '%d\t%s' % (rc, msg.decode() if rc != 0 and msg else '')


def read_table():
    rows = {}
    for line in open(TABLE):
        if line.strip() and not line.startswith('#'):
            name, rest = line.rstrip('\n').split('\t', 1)
            rows[name] = rest
    return rows


@pytest.fixture(scope='module')
def world():
    from gparml_amd import _lib
    lib = _lib.load()
    ctx = contexts(lib)
    yield lib, ctx
    for h in ctx.values():
        lib.gp_destroy(h)


def test_every_case_is_recorded():
    assert sorted(read_table()) == sorted(NAMES)


@pytest.mark.gpu
@pytest.mark.parametrize('name,ctx,fn', CASES, ids=NAMES)
def test_status_and_message_are_the_parent_commits(world, name, ctx, fn):
    lib, handles = world
    got = observe(lib, handles[ctx], fn)
    print(name, '->', got)
    assert not got.startswith('0\t'), 'the call was admitted'
    assert got == read_table()[name]


@pytest.mark.gpu
def test_cg_max_d_needs_a_direction_as_dots_and_abs_do():
    """Not a row of the parent's table: the parent admitted gp_cg_max_d without a direction and reduced whatever the buffers held.  The three
    reductions now share one rule and one wording; with a direction all three run."""
    from gparml_amd import _lib
    lib = _lib.load()
    h, out, alone = ctypes.c_void_p(), np.zeros(6), ctypes.c_double(-1.0)
    assert lib.gp_create(ctypes.byref(h), 0, N, D, M, Q) == 0
    calls = {'gp_cg_dots': lambda: lib.gp_cg_dots(h, p(out)), 'gp_cg_abs': lambda: lib.gp_cg_abs(h, p(out)),
             'gp_cg_max_d': lambda: lib.gp_cg_max_d(h, 0.5, ctypes.byref(alone))}
    try:
        for who, fn in calls.items():                                                    # no data
            assert fn() == _lib.GP_ERR_STATE and lib.gp_last_error(h).decode() == who + ': no shard data'
        assert lib.gp_upload_shard(h, p(Y0), p(XMU0), p(np.log(np.expm1(XS0))), 1) == 0
        for who, fn in calls.items():                                                    # raw variances, no direction
            assert fn() == _lib.GP_ERR_STATE and lib.gp_last_error(h).decode().startswith(who + ': no ') and 'gp_cg_set_grads first' in lib.gp_last_error(h).decode()
        assert lib.gp_last_error(h).decode() == 'gp_cg_max_d: no search direction (gp_cg_set_grads first)' and alone.value == -1.0
        d = _r.randn(2, N, Q)
        assert lib.gp_set_direction(h, p(d)) == 0
        for fn in calls.values():
            assert fn() == 0
        assert alone.value == 0.5 * np.max(np.abs(d))
        assert lib.gp_set_direction(h, None) == 0                                        # dropped again
        assert calls['gp_cg_max_d']() == _lib.GP_ERR_STATE
    finally:
        lib.gp_destroy(h)


if __name__ == '__main__':          # record: GPARML_LIB=<the parent build> python3 tests/test_gpu_entry_checks.py > table
    from gparml_amd import _lib as _L
    _lib_ = _L.load()
    _ctx = contexts(_lib_)
    for _name, _c, _fn in CASES:
        print('%s\t%s' % (_name, observe(_lib_, _ctx[_c], _fn)))
