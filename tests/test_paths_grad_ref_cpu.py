"""The derivatives of the pathwise draws without a device: the ABI surface, and the numpy reference (tests/paths_grad_ref.py) tied to code that
already exists -- finite differences of the draws themselves, grad_ref's mean Jacobian and metric, paths_ref.rff_defect -- rather than to the new
algebra."""
import ctypes
import os
import re

import numpy as np
import pytest

import grad_ref as G
import joint_ref as J
import paths_grad_ref as PG
import paths_ref as P
import predict_ref as R
from conftest import ROOT
from test_joint_cpu import _model

SHAPES = [(5, 1, 1), (16, 2, 3), (33, 5, 4)]
N_POINTS = 3
F, S = 8, 2

# Central differences of the long-double draws (unit roundoff u = 5.4e-20), as tests/test_grad_ref_cpu.py sets its bound: with the step h the
# truncation is h^2 / 6 times a third derivative and the rounding u / h times the function's scale.  The features add d^3 cos(theta) / d x_q^3 =
# omega_q^3 sin(theta), against a first derivative of size omega_q: a factor omega_q^2 <= 16 alpha_q (|omega_q| <= 4 sqrt(alpha_q) for every
# frequency drawn here, alpha_q of order 1), so about 1.7e-11 x 16 = 2.7e-10 and 5.4e-15 at h = 1e-5 (achieved: in the test's docstring).
H_LD = 1e-5
TOL_LD = 1e-8
# Mixed central difference of the float64 defect, [c(+,+) - c(+,-) - c(-,+) + c(-,-)] / (4 h^2): the rounding is 4 x 2.2e-16 x (a few units of sf2
# for the cancelling Gram products) / (4 h^2), the truncation h^2 / 6 times a fourth derivative, omega^2 (<= 16 alpha) times the second.  h = 2^-12
# puts them at 4e-9 x a few and 1e-8 x 16 alpha of the scale sf2 max(alpha, max omega^2).
H_COV = 2.0 ** -12
TOL_COV = 1e-6


def _setup(M, Q, D):
    N = max(300, M + 100)
    d = _model(N, D, M, Q, 'B' if Q > 1 else 'A', seed=M + Q + D)
    Psi2, C = R.statistics(d['Z'], d['sf2'], d['alpha'], d['Y'], d['X_mu'], d['X_S'])
    X = np.random.RandomState(11).randn(N_POINTS, Q)
    rs = np.random.RandomState(5)
    omega, w, eps_u = rs.randn(F, Q) * np.sqrt(d['alpha']), rs.randn(S, 2 * F, D), rs.randn(S, M, D)
    return d, (d['Z'], d['sf2'], d['alpha'], d['beta'], Psi2, C), X, omega, w, eps_u, d['Z'].mean(axis=0)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), np.finfo(float).tiny))


def test_header_declares_gp_paths_grad_and_the_library_exports_it():
    import __graft_entry__ as ge
    from gparml_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'gparml_hip.h')).read(), flags=re.S)
    m = re.search(r'int\s+gp_paths_grad\s*\(([^)]*)\)\s*;', src)
    assert m, 'gp_paths_grad is not declared in include/gparml_hip.h'
    assert len(m.group(1).split(',')) == 9
    assert re.search(r'#define\s+GP_PATHS_WEIGHTS_PER_ROW\s+1\b', src) and _lib.GP_PATHS_WEIGHTS_PER_ROW == 1
    assert 'gp_paths_grad' in _lib.SIGNATURES and len(_lib.SIGNATURES['gp_paths_grad'][1]) == 9
    ge.build()
    lib = ctypes.CDLL(os.path.join(ROOT, 'gparml_amd', 'libgparml_hip.so'))
    assert hasattr(lib, 'gp_paths_grad'), 'the library does not export gp_paths_grad'


def test_the_python_surface_is_there():
    from gparml_amd.engine import ShardEngine
    from gparml_amd.predict import PathDraws
    assert callable(ShardEngine.paths_grad)
    for name in ('jacobian', 'metric', 'value_and_grad', 'curve_energy'):
        assert callable(getattr(PathDraws, name)), name


@pytest.mark.parametrize('M,Q,D', SHAPES)
def test_jac_is_the_central_difference_of_the_draws(M, Q, D):
    """h = 1e-5 in long double.  Achieved (draw_jac_ld; float64 draw_jac against the same differences in brackets): (5,1,1) 4.3e-11 (4.7e-11);
    (16,2,3) 4.4e-11 (4.8e-11); (33,5,4) 1.4e-11 (1.4e-11), against 1e-8."""
    d, args, X, omega, w, eps_u, centre = _setup(M, Q, D)
    jac, _ = PG.draw_jac_ld(*args, X, omega, w, eps_u, centre)
    jac64, _ = PG.draw_jac(*args, X, omega, w, eps_u, centre)
    fd = np.zeros((S, N_POINTS, D, Q), dtype=R.LD)
    for q in range(Q):
        e = np.zeros(Q, dtype=R.LD)
        e[q] = R.LD(H_LD)
        fp = PG.draws_ld(*args, X.astype(R.LD) + e, omega, w, eps_u, centre)
        fm = PG.draws_ld(*args, X.astype(R.LD) - e, omega, w, eps_u, centre)
        fd[:, :, :, q] = (fp - fm) / (2 * R.LD(H_LD))
    errs = [_rel(jac, fd), _rel(jac64, fd)]
    print('jac %.3g (float64 form: %.3g), tol %.3g' % (errs[0], errs[1], TOL_LD))
    assert max(errs) <= TOL_LD, errs
    # the long-double draws are paths_ref.draws' functions
    ref, _ = P.draws(*args, X, omega, w, eps_u, centre)
    tol = J.cond_tol(d['Z'], d['sf2'], d['alpha'], d['beta'], args[4])
    assert _rel(ref, PG.draws_ld(*args, X, omega, w, eps_u, centre)) <= tol


@pytest.mark.parametrize('M,Q,D', SHAPES)
def test_zero_normals_give_grad_refs_mean_jacobian(M, Q, D):
    d, args, X, omega, w, eps_u, centre = _setup(M, Q, D)
    jac, jm = PG.draw_jac(*args, X, omega, 0.0 * w, 0.0 * eps_u, centre)
    ref = G.grad(*args, X)['jac']
    assert np.array_equal(jm, ref), 'jac_mean is not grad_ref.grad\'s jac'
    for s in range(S):
        assert np.array_equal(jac[s], ref), 'a draw of zero normals is not the mean'
    jl, jml = PG.draw_jac_ld(*args, X, omega, 0.0 * w, 0.0 * eps_u, centre)
    assert np.array_equal(jml, G.grad_ld(*args, X)['jac']) and np.array_equal(jl[0], jml)


@pytest.mark.parametrize('M,Q,D', SHAPES)
def test_draw_jac_is_the_mean_plus_the_linear_map(M, Q, D):
    """Term by term (G_s first) against the one map A = [dphi - a'^T Lk^-1 Phi_Z | b'^T]: two associations of the same sums, so they agree to
    float64 rounding at the model's conditioning (joint_ref.cond_tol), and both agree with the long-double form."""
    d, args, X, omega, w, eps_u, centre = _setup(M, Q, D)
    tol = J.cond_tol(d['Z'], d['sf2'], d['alpha'], d['beta'], args[4])
    jac, jm = PG.draw_jac(*args, X, omega, w, eps_u, centre)
    jm2, A = PG.linear_map_jac(*args, X, omega, centre)
    assert A.shape == (N_POINTS, Q, 2 * F + M) and np.array_equal(jm, jm2)
    via = jm[None] + np.transpose(np.einsum('nqk,skd->snqd', A, np.concatenate([w, eps_u], axis=1)), (0, 1, 3, 2))
    ref, _ = PG.draw_jac_ld(*args, X, omega, w, eps_u, centre)
    errs = [_rel(jac, via), _rel(jac, ref), _rel(via, ref)]
    print('term by term against the map %.3g, against long double %.3g, the map against long double %.3g (tol %.3g)' % (tuple(errs) + (tol,)))
    assert max(errs) <= tol, errs


@pytest.mark.parametrize('M,Q,D', SHAPES)
def test_expected_metric_differs_from_grad_refs_by_the_defects_mixed_derivative(M, Q, D):
    """E[J_s^T J_s] over (w, eps_u) is Jm^T Jm + D A A^T; grad_ref's metric is Jm^T Jm + D Cov(J) with the exact kernel.  A A^T - Cov(J) is the
    mixed second derivative at x = x' of paths_ref.rff_defect's P (K_F - K) P^T: section 16's identity, differentiated.  h = 2^-12 in float64,
    relative to sf2 max(alpha, max omega^2).  Achieved: (5,1,1) 1.1e-9; (16,2,3) 1.3e-9; (33,5,4) 2.1e-9, against 1e-6."""
    d, args, X, omega, w, eps_u, centre = _setup(M, Q, D)
    jm, A = PG.linear_map_jac(*args, X, omega, centre)
    g = G.grad(*args, X)
    expected = np.einsum('idq,idr->iqr', jm, jm) + D * np.einsum('iqk,irk->iqr', A, A)
    diff = (expected - g['metric']) / D                                    # A A^T - Cov(J)
    pts = np.concatenate([X[:, None, None, :] + s * H_COV * np.eye(Q)[None, :, None, :] for s in (1.0, -1.0)], axis=2)   # (n, Q, 2, Q): x +- h e_q
    c, _, _ = P.rff_defect(d['Z'], d['sf2'], d['alpha'], pts.reshape(-1, Q), omega, centre)
    c = c.reshape(N_POINTS, Q, 2, N_POINTS, Q, 2)
    fd = np.empty((N_POINTS, Q, Q))
    for i in range(N_POINTS):
        ci = c[i, :, :, i, :, :]                                           # [q][sign][r][sign]
        fd[i] = (ci[:, 0, :, 0] - ci[:, 0, :, 1] - ci[:, 1, :, 0] + ci[:, 1, :, 1]) / (4 * H_COV ** 2)
    scale = d['sf2'] * max(np.max(d['alpha']), np.max(omega ** 2))
    err = float(np.max(np.abs(diff - fd)) / scale)
    print('A A^T - Cov(J) against the defect\'s mixed difference: %.3g (tol %.3g; largest element %.3g of the scale)' % (
        err, TOL_COV, np.max(np.abs(fd)) / scale))
    assert err <= TOL_COV, err
