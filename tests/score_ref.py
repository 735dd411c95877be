"""numpy reference of held-out scoring (gp_predict_score): the Gaussian log density, squared error and normalised squared error of every observed
entry under a predictive mean and variance, the row sums and the five column sums.  ``score`` applies them to tests/predict_ref.py's prediction,
``score_from`` to any given (mean, var).  Shared by tests/test_score_ref_cpu.py and tests/test_gpu_score.py."""
import numpy as np

import predict_ref as R

LOG_2PI_FACTOR = 2.0 * np.pi


def terms(Y, mean, var, observed=None):
    """The per-entry terms (n, D), zero where not observed: e = y - mean, e2 = e e, q = e2 / var, half_log = 1/2 ln(2 pi var) and
    logp = -1/2 (ln(2 pi var) + q) -- the operation order of the device.  var (n, 1) or (n, D); observed None: every entry.  Entries that are
    not observed are never used (they may be NaN)."""
    Y, mean = np.atleast_2d(np.asarray(Y, dtype=float)), np.atleast_2d(np.asarray(mean, dtype=float))
    var = np.broadcast_to(np.asarray(var, dtype=float), mean.shape)
    o = np.ones(mean.shape, dtype=bool) if observed is None else (np.atleast_2d(np.asarray(observed)) != 0)
    assert Y.shape == mean.shape == o.shape
    e = np.where(o, np.where(o, Y, 0.0) - mean, 0.0)
    v = np.where(o, var, 1.0)
    e2 = e * e
    q = e2 / v
    log_part = np.where(o, np.log(LOG_2PI_FACTOR * v), 0.0)
    logp = -0.5 * (log_part + q)
    return dict(observed=o, e=e, e2=e2, q=q, half_log=0.5 * log_part, logp=logp, v=v)


def score_from(Y, mean, var, observed=None):
    """row_logp, row_sse, row_chi2 (n,) and cols (D, 5) = [count, sum e, sum e2, sum q, sum logp] from a given prediction; ``terms`` under 'terms'."""
    t = terms(Y, mean, var, observed)
    cols = np.stack([t['observed'].sum(axis=0).astype(float), t['e'].sum(axis=0), t['e2'].sum(axis=0), t['q'].sum(axis=0), t['logp'].sum(axis=0)], axis=1)
    return dict(row_logp=t['logp'].sum(axis=1), row_sse=t['e2'].sum(axis=1), row_chi2=t['q'].sum(axis=1), cols=cols, terms=t)


def score(Z, sf2, alpha, beta, Psi2, C, Y, X_mu, X_S=None, observed=None, include_noise=True):
    """The score of Y under predict_ref.predict at (X_mu, X_S) with the model of the statistics (Psi2, C)."""
    mean, var = R.predict(Z, sf2, alpha, beta, Psi2, C, X_mu, X_S, include_noise)
    out = score_from(Y, mean, var, observed)
    out['mean'], out['var'] = mean, var
    return out


def summary(cols):
    """count, bias, rmse, chi2_mean, nlpd per column from the column sums (NaN for a column without a scored entry)."""
    cols = np.asarray(cols, dtype=float)
    with np.errstate(invalid='ignore', divide='ignore'):
        cnt = np.where(cols[..., 0] > 0, cols[..., 0], np.nan)
        return dict(count=cols[..., 0], bias=cols[..., 1] / cnt, rmse=np.sqrt(cols[..., 2] / cnt), chi2_mean=cols[..., 3] / cnt, nlpd=-cols[..., 4] / cnt)
