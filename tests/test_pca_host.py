"""The host part of the device PCA (gparml_amd.init.pca_axes, init.pca) against the SVD form of supporting_functions.PCA
(supporting_functions.py:102-121), with numpy-computed sums in place of the device passes.  No GPU.  The bound, 1e-9 relative per column, is the one
tests/test_init_against_reference.py asserts for this computation."""
import numpy as np
import pytest

from pca_util import NumpyEngine, assert_columns_close, svd_pca


def _data(seed=8, sizes=(57, 130, 21), D=40, offset=100.0):
    rs = np.random.RandomState(seed)
    W = rs.randn(7, D) * np.array([5, 4, 3, 2, 1.5, 0.3, 0.2])[:, None]
    return [rs.randn(n, 7).dot(W) + 0.05 * rs.randn(n, D) + offset for n in sizes]


def test_pca_axes_reproduces_the_svd_form():
    from gparml_amd import init
    Y = np.concatenate(_data())
    Q = 5
    shift = Y[:57].mean(axis=0)                  # a provisional centre that is not the mean
    Yc = Y - shift
    mean, V, std = init.pca_axes(Y.shape[0], shift, Yc.sum(axis=0), Yc.T.dot(Yc), Q)
    assert mean.shape == (40,) and V.shape == (40, Q) and std.shape == (Q,)
    np.testing.assert_allclose(mean, Y.mean(axis=0), rtol=1e-13)
    assert np.all(V[np.argmax(np.abs(V), axis=0), np.arange(Q)] > 0)              # the sign rule
    X = (Y - mean).dot(V) / std
    assert_columns_close(X, svd_pca(Y, Q), signed=True, what='pca_axes')
    ref = np.linalg.svd(Y - Y.mean(axis=0), full_matrices=False)[0][:, :Q]        # the reference's form with its free signs
    assert_columns_close(X, ref / ref.std(axis=0), signed=False, what='pca_axes, free signs')
    np.testing.assert_allclose(X.std(axis=0), 1.0, rtol=1e-12)


def test_pca_axes_raises_when_Q_exceeds_the_rank():
    from gparml_amd import init
    rs = np.random.RandomState(2)
    Y = rs.randn(50, 3).dot(rs.randn(3, 12)) + 7.0                               # rank 3 after centring
    shift = Y[0]
    Yc = Y - shift
    init.pca_axes(50, shift, Yc.sum(axis=0), Yc.T.dot(Yc), 3)
    with pytest.raises(np.linalg.LinAlgError):
        init.pca_axes(50, shift, Yc.sum(axis=0), Yc.T.dot(Yc), 4)


def test_pca_drives_the_passes_and_the_reduction():
    """init.pca over three parts: a sum-only pass with centre 0, a Gram pass centred on the global mean, a projection; with an ``allreduce`` that
    doubles (two ranks holding the same rows) the axes are those of the doubled data, which are the same."""
    from gparml_amd import init
    shards = _data()
    Y = np.concatenate(shards)
    parts = [NumpyEngine(s) for s in shards]
    mean, V, std, X = init.pca(parts, 5)
    assert all(p.calls == ['sum', 'gram', 'project'] for p in parts)
    assert [x.shape for x in X] == [(s.shape[0], 5) for s in shards]
    assert_columns_close(np.concatenate(X), svd_pca(Y, 5), what='init.pca')
    seen = []
    mean2, V2, std2, X2 = init.pca([NumpyEngine(s) for s in shards], 5, allreduce=lambda v: (seen.append(v.size), 2.0 * v)[1])
    assert seen == [41, 40 + 1600]
    np.testing.assert_allclose(mean2, mean, rtol=1e-13)
    assert_columns_close(np.concatenate(X2), svd_pca(np.concatenate([Y, Y]), 5)[:Y.shape[0]], what='init.pca, two ranks')


def test_streaming_pca_still_goes_through_pca_axes(tmp_path, monkeypatch):
    """gpu_MapReduce._streaming_pca calls init.pca_axes (the eigen part lives in one place)."""
    import os
    from gparml_amd import gpu_MapReduce as mr
    from gparml_amd import init
    shards = _data()
    os.makedirs(str(tmp_path / 'input'))
    names = ['s%d' % i for i in range(3)]
    for n, Y in zip(names, shards):
        np.savetxt(str(tmp_path / 'input' / n), Y, delimiter=',', fmt='%.17g')
    calls = []
    orig = init.pca_axes
    monkeypatch.setattr(init, 'pca_axes', lambda *a: (calls.append(a[0]), orig(*a))[1])
    project = mr._streaming_pca({'input': str(tmp_path / 'input'), 'Q': 5}, names)
    assert calls == [208]
    assert_columns_close(np.concatenate([project(n) for n in names]), svd_pca(np.concatenate(shards), 5), what='_streaming_pca')
