"""psi1_kernel<QP, true, 0, false> (gparml_amd/csrc/psi1.hip): fixed variance with NON-temporal stores, the form the headline runs.  It is chosen
when [Psi1 | Y] is over 200 MB or by GPARML_PSI1_TEMPORAL=0, a switch read once per process, so the elementwise tests of test_gpu_compat_arrays.py
(small shards) only reach the temporal form.  Here the same inputs run in this process (temporal) and in one fresh child with the switch set; both
downloads are held to compat_ref's elementwise bound, and to each other bit for bit: the two forms differ in the store instruction alone.
N = 300, M = 513: WC = 4, Np = 384 = three workgroups of 8 groups along the rows (the whole fill / prefetch / commit cycle each, the last one with
the masked rows n >= N) at QP = 2, 10 and 32; M = 257, q = 2: WC = 2, where the second wave pair takes every other row of a group.
What this cannot see: that the child really took the non-temporal form.  The library has no query for the form it launched, so a switch that was
renamed in the library would leave two temporal runs that agree; tests/test_gpu_perf_guard.py's headline shape runs the form by size."""
import os
import subprocess
import sys

import numpy as np
import pytest

import compat_ref as R
from conftest import ROOT
from test_gpu_compat_arrays import engine_for, hold, reference

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.available(), reason='numpy long double has no 64-bit significand here')]

CASES = [(1, 513), (10, 513), (32, 513), (2, 257)]      # (q, M)

CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import compat_ref as R
from test_gpu_compat_arrays import engine_for
out = {}
for q, M in %(cases)r:
    eng = engine_for(R.psi1_case_inputs(q, 'A', M=M), step=False)
    out['q%%d_M%%d' %% (q, M)] = eng.download('PSI1')
    eng.close()
np.savez(%(out)r, **out)
print('PSI1_NT_OK', flush=True)
'''


def test_nontemporal_form_equals_temporal_form(tmp_path):
    out = str(tmp_path / 'psi1_nt.npz')
    script = tmp_path / 'psi1_nt_child.py'
    script.write_text(CHILD % {'root': ROOT, 'tests': os.path.join(ROOT, 'tests'), 'cases': CASES, 'out': out})
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, GPARML_PSI1_TEMPORAL='0'))
    assert r.returncode == 0 and 'PSI1_NT_OK' in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    nt = np.load(out)
    for q, M in CASES:
        d = R.psi1_case_inputs(q, 'A', M=M)
        ref = reference(d, names=('psi1',), tag='' if M == 513 else '_M%d' % M)     # M = 513: the entry test_gpu_compat_arrays.py caches
        eng = engine_for(d, step=False)
        t = eng.download('PSI1')
        eng.close()
        n = nt['q%d_M%d' % (q, M)]
        what = '%s M = %d' % (d['name'], M)
        hold(what + ' temporal', {'psi1': t}, ref, d['N'])
        hold(what + ' non-temporal', {'psi1': n}, ref, d['N'])
        assert np.array_equal(t, n), '%s: the two store forms differ in %d elements' % (what, int(np.sum(t != n)))
