"""NumPy reference of the wealth statistics of histogram distributions (test infrastructure
only).

For one distribution ``mass[S][n_a]`` over (state, beginning-of-period assets) on the ascending
grid ``a[n_a]``:

    g   = ((mass[0] + mass[1]) + ...) + mass[S-1]              the marginal, added in ascending s
    cw  = cumsum(g),  cd = cumsum(a g),  F = cw / cw[-1],  L = cd / cd[-1]
    lorenz(p)     = np.interp(p, F, L)                         = hark_utils.get_lorenz_shares(a, g, p, presorted)
    percentile(p) = interp1d(F, a, bounds_error=False)(p)      = hark_utils.get_percentiles(a, g, p, presorted)
    gini  = 1 - sum_j (F[j] - F[j-1]) (L[j] + L[j-1]),  F[-1] = L[-1] = 0   (area under the Lorenz polygon)
    total = cw[-1],  mean = cd[-1] / cw[-1],  bottom_share = g[0] / cw[-1]

The Lorenz shares and percentiles are taken from ``oracle.hark_utils`` itself, so the ties of F
(nodes without mass) are resolved by NumPy and SciPy.
"""
from __future__ import annotations

import numpy as np

from oracle import hark_utils as HU


def marginal(mass):
    """Sum over states in ascending s."""
    mass = np.asarray(mass, dtype=np.float64)
    g = mass[0].copy()
    for s in range(1, mass.shape[0]):
        g = g + mass[s]
    return g


def curves(g, a):
    """(F, L) of the marginal g on the grid a."""
    cw = np.cumsum(g)
    cd = np.cumsum(a * g)
    return cw / cw[-1], cd / cd[-1]


def gini(g, a):
    F, L = curves(g, a)
    Fp = np.concatenate([[0.0], F[:-1]])
    Lp = np.concatenate([[0.0], L[:-1]])
    return 1.0 - np.sum((F - Fp) * (L + Lp))


def gini_mean_difference(g, a):
    """sum_ij p_i p_j |a_i - a_j| / (2 mu) of the discrete distribution p = g / sum g."""
    p = g / np.sum(g)
    mu = np.sum(p * a)
    return np.sum(p[:, None] * p[None, :] * np.abs(a[:, None] - a[None, :])) / (2.0 * mu)


def marginal_stats(g, a, percentiles):
    """dict(lorenz[n_p], percentile_values[n_p], gini, mean, total, bottom_share) of one marginal."""
    g = np.asarray(g, dtype=np.float64)
    a = np.asarray(a, dtype=np.float64)
    p = np.asarray(percentiles, dtype=np.float64)
    cw = np.cumsum(g)
    cd = np.cumsum(a * g)
    with np.errstate(invalid="ignore", divide="ignore"):
        lor = HU.get_lorenz_shares(a, weights=g, percentiles=p, presorted=True)
        pct = HU.get_percentiles(a, weights=g, percentiles=p, presorted=True)
    return dict(lorenz=np.asarray(lor), percentile_values=np.asarray(pct), gini=gini(g, a), mean=cd[-1] / cw[-1],
                total=cw[-1], bottom_share=g[0] / cw[-1])


def dist_stats(mass, a, percentiles):
    """The statistics of one distribution mass[S][n_a]."""
    return marginal_stats(marginal(mass), a, percentiles)

