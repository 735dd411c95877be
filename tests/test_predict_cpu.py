"""gp_predict without a device: the ABI surface and the numpy reference the GPU tests compare against."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_gp_predict_and_lib_binds_it():
    src = open(os.path.join(ROOT, 'include', 'gparml_hip.h')).read()
    m = re.search(r'int\s+gp_predict\s*\(([^)]*)\)\s*;', src)
    assert m, 'gp_predict is not declared in include/gparml_hip.h'
    assert len(m.group(1).split(',')) == 8
    from gparml_amd import _lib
    assert 'gp_predict' in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['gp_predict'][1]) == 8


def test_python_surfaces_exist():
    from gparml_amd.engine import ShardEngine
    from gparml_amd.resident import ResidentModel
    from gparml_amd.predict import Predictor
    assert callable(ShardEngine.predict) and callable(ResidentModel.predict) and callable(Predictor.predict_outputs)


def test_reference_reproduces_the_exact_gp_in_the_limit():
    """Z = X_train, S = 0: Titsias' predictive equals the full GP posterior (the reference's algebra, checked without a device)."""
    import predict_ref as R
    rs = np.random.RandomState(3)
    X = np.stack(np.meshgrid(np.linspace(-3, 3, 8), np.linspace(-2, 2, 5)), -1).reshape(-1, 2)     # 40 separated points
    Y = np.sin(X.dot(rs.randn(2, 3))) + 0.1 * rs.randn(40, 3)
    sf2, alpha, beta = 1.3, np.array([0.8, 1.1]), 25.0
    Psi2, C = R.statistics(X, sf2, alpha, Y, X, np.zeros_like(X))
    Xs = rs.uniform(-3, 3, size=(7, 2))
    m, v = R.predict(X, sf2, alpha, beta, Psi2, C, Xs, include_noise=True)
    me, ve = R.exact_gp(X, Y, sf2, alpha, beta, Xs)
    assert np.max(np.abs(m - me)) <= 1e-7 * max(1.0, np.max(np.abs(me)))
    assert np.max(np.abs(v - ve)) <= 1e-7 * sf2


def test_reference_uncertain_form_reduces_to_the_deterministic_one():
    import predict_ref as R
    rs = np.random.RandomState(4)
    Z, X = rs.randn(9, 3), rs.randn(30, 3)
    Y = rs.randn(30, 2)
    sf2, alpha, beta = 0.9, np.array([0.5, 0.7, 0.3]), 8.0
    Psi2, C = R.statistics(Z, sf2, alpha, Y, X, np.zeros_like(X))
    Xs = rs.randn(5, 3)
    m0, v0 = R.predict(Z, sf2, alpha, beta, Psi2, C, Xs)
    m1, v1 = R.predict(Z, sf2, alpha, beta, Psi2, C, Xs, np.full_like(Xs, 1e-14))
    assert np.max(np.abs(m1 - m0)) <= 1e-10
    assert np.max(np.abs(v1 - v0)) <= 1e-9
