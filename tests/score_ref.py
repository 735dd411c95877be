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


def cols_in_device_order(values, observed, seg=128):
    """The column sums (D,) of values (n, D) over the observed entries in the summation order the device documents (include/gparml_hip.h, DESIGN.md
    section 18), in plain float64: per column and per segment of ``seg`` rows by global index, the rows of the first and of the second half each
    summed one by one in ascending order from 0.0, hidden entries skipped; then half 0 + half 1; then the segments added one by one, ascending,
    into a total that starts at 0.0."""
    values, o = np.asarray(values, dtype=np.float64), np.asarray(observed) != 0
    n, D = values.shape
    assert o.shape == (n, D) and seg % 2 == 0
    out = np.empty(D)
    for d in range(D):
        total = 0.0
        for s0 in range(0, n, seg):
            halves = []
            for h0 in (s0, s0 + seg // 2):
                acc = 0.0
                for i in range(h0, min(h0 + seg // 2, n)):
                    if o[i, d]:
                        acc = acc + float(values[i, d])
                halves.append(acc)
            total = total + (halves[0] + halves[1])
        out[d] = total
    return out


def one_entry_mask(n, D, empty_row):
    """Every row observes exactly one column, (row mod D), and ``empty_row`` none: a row's three outputs are then the bits of its single entry's
    terms -- the lane sums and the butterfly add only zeros -- so the column sums can be rebuilt exactly from the row outputs."""
    o = np.zeros((n, D), dtype=bool)
    o[np.arange(n), np.arange(n) % D] = True
    o[empty_row] = False
    return o


def check_cols_order(row_logp, row_sse, row_chi2, cols, observed, what):
    """cols [D][5] of a call under a one_entry_mask against its own row outputs summed in the documented order: bit for bit."""
    o = np.asarray(observed) != 0
    assert np.array_equal(cols[:, 0], o.sum(axis=0).astype(float)), what + ': count'
    for k, rows in ((2, row_sse), (3, row_chi2), (4, row_logp)):
        assert np.all(np.isfinite(rows)), what
        want = cols_in_device_order(np.where(o, np.asarray(rows)[:, None], 0.0), o)
        assert np.array_equal(cols[:, k], want), '%s: cols[:, %d] is not the documented order: %r against %r' % (what, k, cols[:, k], want)


def summary(cols):
    """count, bias, rmse, chi2_mean, nlpd per column from the column sums (NaN for a column without a scored entry)."""
    cols = np.asarray(cols, dtype=float)
    with np.errstate(invalid='ignore', divide='ignore'):
        cnt = np.where(cols[..., 0] > 0, cols[..., 0], np.nan)
        return dict(count=cols[..., 0], bias=cols[..., 1] / cnt, rmse=np.sqrt(cols[..., 2] / cnt), chi2_mean=cols[..., 3] / cnt, nlpd=-cols[..., 4] / cnt)
