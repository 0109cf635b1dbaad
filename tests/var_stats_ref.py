"""NumPy reference of the statistics of household variables on the histogram (test
infrastructure only).

At node (s, j) of a period with lottery (lo, wlo) and prices (R, w), a' = wlo a[lo] + (1 - wlo) a[lo + 1]:

    consumption (R a_j + w lab_s) - a'      income (R - 1) a_j + w lab_s      earnings w lab_s
    cash R a_j + w lab_s                    saving a' - a_j                   wealth a_j

A distribution of a variable y[S][n_a] with weights mass[S][n_a] is ordered by a stable argsort of
the flattened keys (ties by state, then node) and its statistics are ``dist_stats_ref.marginal_stats``
of the sorted weights on the sorted keys.  Moments are two-pass with sequential sums.
"""
from __future__ import annotations

import numpy as np

from tests import dist_stats_ref as DR
from tests import welfare_ref as WR

VARIABLES = ("consumption", "income", "earnings", "cash", "saving", "wealth")


def variables(aGrid, lab, R, w, lo, wlo, which=VARIABLES):
    """dict name -> [S][n_a] of one calibration and period; lo is read as held to [0, n_a - 2]."""
    aGrid, lab = np.asarray(aGrid, dtype=np.float64), np.asarray(lab, dtype=np.float64)
    lo = np.clip(np.asarray(lo), 0, len(aGrid) - 2)
    ap = wlo * aGrid[lo] + (1.0 - wlo) * aGrid[lo + 1]
    full = lambda x: np.broadcast_to(x, ap.shape).copy()   # noqa: E731
    out = dict(consumption=WR.consumption(aGrid, lab, R, w, lo, wlo),
               income=(R - 1.0) * aGrid[None, :] + w * lab[:, None],
               earnings=full(w * lab[:, None]),
               cash=R * aGrid[None, :] + w * lab[:, None],
               saving=ap - aGrid[None, :],
               wealth=full(aGrid[None, :]))
    return {k: out[k] for k in which}


def merge(key, weight):
    """(key_sorted [S n_a], weight_sorted, rank [S][n_a]) of one distribution: the stable order."""
    key = np.asarray(key, dtype=np.float64)
    order = np.argsort(key.reshape(-1), kind="stable")
    rank = np.empty(order.size, dtype=np.int64)
    rank[order] = np.arange(order.size)
    return key.reshape(-1)[order], np.asarray(weight, dtype=np.float64).reshape(-1)[order], rank.reshape(key.shape)


def runs_nondecreasing(key):
    """Every run key[s] nondecreasing and free of NaN: what the merge requires."""
    key = np.asarray(key)
    return bool(np.all(key[..., :-1] <= key[..., 1:]))


def moments(values, weight):
    """(sum w, means [n_v], centred second moments [n_v][n_v]) of the variables ``values``
    (a list of arrays of weight's shape): two passes, sequential sums."""
    w = np.asarray(weight, dtype=np.float64).reshape(-1)
    ys = [np.asarray(y, dtype=np.float64).reshape(-1) for y in values]
    sw = float(np.cumsum(w)[-1])
    mean = np.array([np.cumsum(w * y)[-1] / sw for y in ys])
    cov = np.empty((len(ys), len(ys)))
    for u, yu in enumerate(ys):
        for v, yv in enumerate(ys):
            cov[u, v] = np.cumsum(w * ((yu - mean[u]) * (yv - mean[v])))[-1] / sw
    return sw, mean, cov


def variable_stats(key, weight, percentiles):
    """The fields of ``stats.VariableStats`` of one distribution, as a dict."""
    ks, ws, _ = merge(key, weight)
    out = DR.marginal_stats(ws, ks, percentiles)
    _, _, cov = moments([key], weight)
    out["std"] = float(np.sqrt(cov[0, 0]))
    with np.errstate(invalid="ignore", divide="ignore"):
        out["cv"] = out["std"] / abs(out["mean"])
    return out


def correlations(values, weight):
    _, _, cov = moments(values, weight)
    sd = np.sqrt(np.diag(cov))
    with np.errstate(invalid="ignore", divide="ignore"):
        return cov / (sd[:, None] * sd[None, :])


def gini_mean_difference(key, weight):
    """sum_ij p_i p_j |y_i - y_j| / (2 mu), p = weight / sum weight, over all nodes."""
    y = np.asarray(key, dtype=np.float64).reshape(-1)
    p = np.asarray(weight, dtype=np.float64).reshape(-1)
    p = p / np.sum(p)
    return np.sum(p[:, None] * p[None, :] * np.abs(y[:, None] - y[None, :])) / (2.0 * np.sum(p * y))
