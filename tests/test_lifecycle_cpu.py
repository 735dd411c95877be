"""The rules of gparml_amd/csrc/lifecycle.h on the CPU: tests/lifecycle_table.cpp (the header alone, host compiler) walks the canonical evaluation,
raises every event from every point of it and prints every query's answer; the same walk is made here over SITES, the ten loose flags the
context had before the header existed and one row per place that assigned one (file:line of the commit before it) -- written down from those
entry points, not from the header.  The as-found disagreements (a NULL direction resets nothing, gp_buffer_combine leaves the packed copy
"current", ...) are rows like any other.  The program runs a second time built with -fsanitize=address,undefined."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, 'tests', 'lifecycle_table.cpp')
FLAGS = ('state', 'have_data', 'have_globals', 'have_dir', 'prep_fixa_valid', 'want_emb', 'spack_filled', 'pred_ok', 'gs_pending', 'have_glatest')
LIFT = 'max(state, 1)'
# the runtimes linked statically: the program then starts whatever the environment preloads
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan']

# event -> [(flag, value, where the commit before the header assigned it)]
SITES = {
    'data_uploaded': [('have_data', 1, 'api.hip:260 gp_upload_shard'), ('have_dir', 0, 'api.hip:261'), ('prep_fixa_valid', 0, 'api.hip:262')],
    'embeddings_changed': [('prep_fixa_valid', 0, 'api.hip:224 upload_embeddings, :945 gp_cg_update(2)'), ('state', 0, 'api.hip:228, :945'),
                           ('pred_ok', 0, 'api.hip:229, :945')],
    'direction_set(0)': [('have_dir', 0, 'api.hip:278 gp_set_direction(NULL): nothing else')],
    'direction_set(1)': [('have_dir', 1, 'api.hip:281 gp_set_direction(d)'), ('state', 0, 'api.hip:282'), ('pred_ok', 0, 'api.hip:283')],
    'direction_rewritten': [('have_dir', 1, 'api.hip:944 gp_cg_update(0, 1, 5): nothing else')],
    'origin_moved': [('prep_fixa_valid', 0, 'api.hip:317 choose_origin')],
    'globals_set': [('have_globals', 1, 'api.hip:359 gp_set_globals'), ('state', 0, 'api.hip:360'), ('pred_ok', 0, 'api.hip:361')],
    'prep_ran(0)': [('prep_fixa_valid', 0, 'psi.hip:550 run_prep_and_generate')],
    'prep_ran(1)': [('prep_fixa_valid', 1, 'psi.hip:550')],
    'phase1_ran': [('state', 1, 'api.hip:376 gp_phase1'), ('pred_ok', 0, 'api.hip:377'), ('spack_filled', 0, 'api.hip:378')],
    'stats_injected': [('spack_filled', 0, 'api.hip:695 gp_set_local_statistics'), ('pred_ok', 0, 'api.hip:696'), ('state', LIFT, 'api.hip:697')],
    'stats_combined': [('pred_ok', 0, 'api.hip:501 gp_buffer_combine(statistics)'), ('state', LIFT, 'api.hip:502: spack_filled is left alone')],
    'stats_scaled': [('spack_filled', 0, 'api.hip:513 gp_scale_buffer(statistics)'), ('pred_ok', 0, 'api.hip:513')],
    'stats_unpacked': [('pred_ok', 0, 'api.hip:441 stats_pack(unpack), in front of the spack_filled refusal')],
    'stats_packed': [('spack_filled', 1, 'api.hip:447 stats_pack(pack)')],
    'step_started': [('pred_ok', 0, 'api.hip:532 gp_global_step_jitter')],
    'step_enqueued': [('gs_pending', 1, 'linalg.hip:793, :879 run_global_step'), ('state', 2, 'api.hip:537'), ('pred_ok', 1, 'api.hip:538')],
    'step_read_back': [('gs_pending', 0, 'linalg.hip:702 check_global_from')],
    'phase2_mode(0)': [('want_emb', 0, 'api.hip:572 gp_phase2')],
    'phase2_mode(1)': [('want_emb', 1, 'api.hip:572')],
    'grad_latest_written': [('have_glatest', 1, 'api.hip:582 gp_phase2')],
    'phase2_ran': [('state', 3, 'api.hip:585 gp_phase2')],
}

# query -> the flag arithmetic that stood at its call sites
QUERIES = [
    ('has_data', lambda f: f['have_data']),                                        # api.hip:269, 567, 641, 781, 811, 930
    ('has_globals', lambda f: f['have_globals']),                                  # api.hip:682
    ('has_direction', lambda f: f['have_dir']),                                    # psi.hip:537, api.hip:581, 650, 970, 992
    ('embedding_mode', lambda f: f['want_emb']),                                   # api.hip:570, 577, psi.hip:1272, 1276, p1i8.hip:293
    ('can_phase1', lambda f: f['have_data'] and f['have_globals']),                # api.hip:367
    ('has_stats', lambda f: f['state'] >= 1),                                      # api.hip:436, 509, 528, comm.hip:133
    ('step_done', lambda f: f['state'] >= 2),                                      # api.hip:549, 556, 566, 617, 861, compat.hip:135
    ('phase2_done', lambda f: f['state'] >= 3),                                    # api.hip:510, 865, comm.hip:134
    ('psi1_available', lambda f: f['have_data'] and f['state'] >= 1),              # compat.hip:134
    ('step_outcome_pending', lambda f: f['gs_pending']),                           # linalg.hip:689, 700, api.hip:881
    ('model_current', lambda f: f['state'] >= 2 and f['have_globals'] and f['pred_ok']),     # api.hip:705, 732
    ('grad_latest_ready', lambda f: f['state'] >= 3 and f['want_emb']),            # api.hip:644
    ('has_grad_latest', lambda f: f['have_glatest']),                              # api.hip:939
    ('prep_is_current(0)', lambda f: 0),                                           # psi.hip:546: fixa && prep_fixa_valid
    ('prep_is_current(1)', lambda f: f['prep_fixa_valid']),
    ('packed_is_current', lambda f: f['spack_filled']),                            # api.hip:443
    ('phase1_timed', lambda f: f['state'] >= 1),                                   # api.hip:602, 603, 607, 608
    ('step_timed', lambda f: f['state'] >= 2),                                     # api.hip:604
    ('phase2_timed', lambda f: f['state'] >= 3),                                   # api.hip:598, 605, 609
]
# psi1_is_current has no flag behind it: it is the second meaning of `state` on its own (no entry point asks it yet).  True after a phase 1
# until the data, the embeddings, the direction or the globals change -- also where `state` stayed up (as found: direction_set(0), direction_rewritten)
PSI1_SET, PSI1_CLEARED = ('phase1_ran',), ('embeddings_changed', 'direction_set(0)', 'direction_set(1)', 'direction_rewritten', 'globals_set')

POINTS = [('new', []), ('gp_upload_shard', ['embeddings_changed', 'data_uploaded']), ('gp_set_globals', ['origin_moved', 'globals_set']),
          ('gp_phase1', ['prep_ran(1)', 'phase1_ran']), ('gp_stats_pack', ['stats_packed']), ('gp_global_step', ['step_started', 'step_enqueued']),
          ('gp_phase2', ['phase2_mode(1)', 'prep_ran(0)', 'grad_latest_written', 'phase2_ran']), ('gp_finish', ['step_read_back'])]


def _raise(f, event):
    f = dict(f)
    for flag, value, _ in SITES[event]:
        f[flag] = max(f['state'], 1) if value == LIFT else value
    if event in PSI1_SET or event in PSI1_CLEARED:
        f['psi1'] = int(event in PSI1_SET)
    return f


def _answers(f):
    return ''.join('1' if q(f) else '0' for _, q in QUERIES) + '%d' % f['psi1']


def expected_lines():
    at = dict({k: 0 for k in FLAGS}, psi1=0)
    lines = ['queries: ' + ' '.join([n for n, _ in QUERIES] + ['psi1_is_current'])]
    for point, events in POINTS:
        for e in events:
            at = _raise(at, e)
        lines.append('%s | - | %s' % (point, _answers(at)))
        lines += ['%s | %s | %s' % (point, e, _answers(_raise(at, e))) for e in SITES]
    return lines


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror'] + extra + [SRC, '-o', exe])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    return subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


@pytest.mark.parametrize('name,extra', [('plain', []), ('sanitized', SANITIZE)])
def test_lifecycle_rules_are_the_entry_points_of_before(tmp_path, name, extra):
    r = _build_and_run(tmp_path, 'lifecycle_table_' + name, extra)
    assert r.returncode == 0 and r.stderr == '', r.stderr
    got, want = r.stdout.splitlines(), expected_lines()
    assert len(want) == 1 + len(POINTS) * (1 + len(SITES))
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad and len(got) == len(want), 'first difference (program, expected): %s' % (bad[:1],)


def test_the_found_inconsistencies_are_in_the_table():
    """The rows a later behaviour change will have to turn over, spelled out: each holds today."""
    full = dict({k: 0 for k in FLAGS}, psi1=0)
    for _, events in POINTS:
        for e in events:
            full = _raise(full, e)
    q = dict(QUERIES)
    # a direction resets the evaluation; dropping it, or rewriting it on the device, does not
    assert not q['has_stats'](_raise(full, 'direction_set(1)'))
    assert q['phase2_done'](_raise(full, 'direction_set(0)')) and q['phase2_done'](_raise(full, 'direction_rewritten'))
    # new globals, then injected statistics and a step: phase 2 is admitted on the Psi1 from before the new globals
    f = _raise(_raise(_raise(_raise(full, 'globals_set'), 'stats_injected'), 'step_started'), 'step_enqueued')
    assert q['step_done'](f) and q['has_data'](f) and not f['psi1']
    # gp_buffer_combine leaves the packed copy of the statistics it replaced "current"; gp_set_local_statistics and gp_scale_buffer do not
    assert q['packed_is_current'](_raise(full, 'stats_combined'))
    assert not q['packed_is_current'](_raise(full, 'stats_injected')) and not q['packed_is_current'](_raise(full, 'stats_scaled'))
