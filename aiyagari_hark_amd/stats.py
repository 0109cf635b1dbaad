"""Wealth-distribution statistics of the simulated panel on device.

The reference notebook compares the simulated wealth distribution with the SCF through
HARK's ``get_lorenz_shares`` and imports ``get_percentiles`` alongside it
(Aiyagari-HARK.py:298-316)::

    sim_Lorenz_points = get_lorenz_shares(sim_wealth, percentiles=pctiles)

These are HARK 0.12's two functions (``HARK.utilities``) with the same signature,
defaults and argument checks, computed by libaiyagari's ``aiy_wealth_stats``
(rocPRIM radix sort + scans + one interpolation kernel, ``csrc/stats.hip``) on a
device array -- e.g. ``agent.panel.a``, the 1e6-1e8 agents' assets, which then never
leave HBM.  Host arrays are copied to the device first.  Results equal HARK's to
rounding (tree-ordered sums instead of NumPy's sequential cumsum).

Histogram distributions: ``histogram_stats`` gives the same two statistics and
the Gini coefficient, mean, total and bottom share of masses on the ascending asset grid --
the stationary mass of a ``StationaryBatch`` (``batch_wealth_stats``) or the period marginals of
a transition path (``transition.path_wealth_stats``) -- without a sort: ``aiy_dist_marginal``
and ``aiy_dist_stats`` (``csrc/dist_stats.hip``), one launch for a whole stack.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

_MAX_PCT = 256


def _check_percentiles(percentiles):
    if percentiles is None:
        return np.array([0.5])
    if not isinstance(percentiles, (list, np.ndarray)) or min(percentiles) <= 0 or max(percentiles) >= 1:
        raise ValueError("Percentiles should be a list or numpy array of floats between 0 and 1")
    p = np.ascontiguousarray(percentiles, dtype=np.float64).ravel()
    if p.size > _MAX_PCT:
        raise ValueError(f"at most {_MAX_PCT} percentiles per call")
    return p


def _device_vector(x, device):
    if isinstance(x, torch.Tensor):
        t = x.detach()
        if t.device.type != "cuda":
            t = t.to(device if device is not None else "cuda")
    else:
        t = torch.as_tensor(np.asarray(x, dtype=np.float64).ravel()).to(device if device is not None else "cuda")
    return t.to(torch.float64).reshape(-1).contiguous()


def _stats(data, weights, percentiles, device):
    p = _check_percentiles(percentiles)
    d = _device_vector(data, device)
    w = None if weights is None else _device_vector(weights, d.device)
    if w is not None and w.numel() != d.numel():
        raise ValueError("weights must have the same size as data")
    n = d.numel()
    if n < 1:
        raise ValueError("data is empty")
    h = _lib.handle(d.device.index)
    lor = np.empty(p.size)
    pct = np.empty(p.size)
    dp = ctypes.POINTER(ctypes.c_double)
    h.check(h.lib.aiy_wealth_stats(h.h, _lib.ptr(d), None if w is None else _lib.ptr(w), n,
                                   p.ctypes.data_as(dp), p.size, lor.ctypes.data_as(dp), pct.ctypes.data_as(dp),
                                   _lib.stream_ptr()), "aiy_wealth_stats")
    return lor, pct


def get_lorenz_shares(data, weights=None, percentiles=None, presorted=False, device=None):
    """[HARK 0.12] utilities.get_lorenz_shares: cumulative share of total wealth held by
    the bottom p of the population, np.interp(p, cumsum(w)/sum(w), cumsum(a w)/sum(a w))
    over the wealth-sorted data.  ``presorted`` is accepted for signature parity (the
    device sort is run either way and gives the same order)."""
    return _stats(data, weights, percentiles, device)[0]


def get_percentiles(data, weights=None, percentiles=None, presorted=False, device=None):
    """[HARK 0.12] utilities.get_percentiles: the weighted inverse CDF,
    interp1d(cumsum(w)/sum(w), sorted data, bounds_error=False)(p) (NaN outside the
    support of the CDF)."""
    return _stats(data, weights, percentiles, device)[1]


# -------------------------------------------------------------------------------------
# Histogram distributions
# -------------------------------------------------------------------------------------
SLAB_BYTES = 256 << 20   # cap of aiy_dist_stats' cw / cd work space per call


@dataclass
class WealthStats:
    """Statistics of a stack of distributions of leading shape [...]."""
    lorenz: np.ndarray              # [..., n_p] Lorenz shares at ``percentiles``
    percentile_values: np.ndarray   # [..., n_p] wealth percentiles (NaN below the CDF's first value)
    gini: np.ndarray                # [...]
    mean: np.ndarray                # [...] sum a g / sum g
    total: np.ndarray               # [...] sum g
    bottom_share: np.ndarray        # [...] g[0] / sum g: the share of households on the lowest node
    percentiles: np.ndarray         # [n_p]


def _as_device(x, device):
    if isinstance(x, torch.Tensor):
        t = x.detach()
        if t.device.type != "cuda":
            t = t.to(device if device is not None else "cuda")
    else:
        t = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).to(device if device is not None else "cuda")
    return t.to(torch.float64).contiguous()


def _grid_stack(a_grid, lead, n_a, device):
    """(grids [n_grid][n_a] on device, n_grid) such that distribution d of the flattened stack
    uses grid d % n_grid: a grid shared by all, one per index of the trailing leading axes
    (e.g. [n_cal][n_a] under a [T+1][n_cal] stack), else the broadcast written out."""
    ag = _as_device(a_grid, device)
    if ag.dim() < 1 or ag.shape[-1] != n_a or ag.dim() > len(lead) + 1:
        raise ValueError(f"a_grid {tuple(ag.shape)} does not fit masses of leading shape {lead} and n_a={n_a}")
    ag = ag.reshape((1,) * (len(lead) + 1 - ag.dim()) + tuple(ag.shape))
    first = next((i for i in range(len(lead)) if ag.shape[i] != 1), len(lead))
    if tuple(ag.shape[first:-1]) == tuple(lead[first:]):
        n_grid = math.prod(lead[first:])
        return ag.reshape(n_grid, n_a), n_grid
    n_dist = math.prod(lead)
    return ag.expand(tuple(lead) + (n_a,)).reshape(n_dist, n_a).contiguous(), n_dist


def histogram_stats(mass, a_grid, percentiles=None, marginal=False, slab=None, device=None):
    """Wealth statistics of histogram distributions: ``mass`` [..., S, n_a] over (state,
    beginning-of-period assets), or the marginals [..., n_a] with ``marginal=True``, a device
    tensor or a NumPy array; ``a_grid`` [n_a] ascending, or broadcastable over the leading axes.
    Returns ``WealthStats`` of the leading shape; ``percentiles=None`` uses [0.5].

    The marginal over states is summed in ascending s (``aiy_dist_marginal``); Lorenz shares and
    percentiles are HARK's ``get_lorenz_shares`` / ``get_percentiles`` with weights = marginal and
    presorted = True, the Gini coefficient the area form of the piecewise-linear Lorenz curve.
    ``aiy_dist_stats`` keeps cw and cd of every distribution of a call (16 n_a bytes each), so
    the stack goes through it in slabs of ``slab`` distributions, by default the number whose
    work space stays within 256 MB; the results do not depend on the slab size."""
    p = _check_percentiles(percentiles)
    m = _as_device(mass, device)
    need = 1 if marginal else 2
    if m.dim() < need or m.shape[-1] < 2:
        raise ValueError(f"mass {tuple(m.shape)}: needs [..., {'n_a' if marginal else 'S, n_a'}] with n_a >= 2")
    n_a = int(m.shape[-1])
    lead = tuple(int(x) for x in m.shape[:-need])
    n_dist = math.prod(lead)
    if n_dist < 1:
        raise ValueError("no distribution")
    h = _lib.handle(m.device.index)
    grids, n_grid = _grid_stack(a_grid, lead, n_a, m.device)
    if marginal:
        g = m.reshape(n_dist, n_a)
    else:
        g = torch.empty((n_dist, n_a), dtype=torch.float64, device=m.device)
        h.check(h.lib.aiy_dist_marginal(h.h, n_dist, int(m.shape[-2]), n_a, _lib.ptr(m), _lib.ptr(g),
                                        _lib.stream_ptr()), "aiy_dist_marginal")
    if slab is None:
        slab = max(1, SLAB_BYTES // (16 * n_a))
    slab = max(1, min(int(slab), n_dist))
    work = _lib.work_space(m.device, "dist_stats", "", n_dist=slab, n_a=n_a)
    lor = np.empty((n_dist, p.size))
    pct = np.empty((n_dist, p.size))
    summ = np.empty((n_dist, 4))
    dp = _lib.c_double_p
    d0 = 0
    while d0 < n_dist:
        # a slab starts on a multiple of n_grid and holds whole rounds of the grids, or lies
        # inside one round (then it is given the grids from its first one on)
        r0 = d0 % n_grid
        n = slab // n_grid * n_grid if (r0 == 0 and slab >= n_grid) else min(slab, n_grid - r0)
        n = min(n, n_dist - d0)
        h.check(h.lib.aiy_dist_stats(h.h, n, n_grid - r0, n_a, _lib.ptr(g[d0:d0 + n]), _lib.ptr(grids[r0:]),
                                     p.ctypes.data_as(dp), p.size, _lib.ptr(work), lor[d0:].ctypes.data_as(dp),
                                     pct[d0:].ctypes.data_as(dp), summ[d0:].ctypes.data_as(dp), _lib.stream_ptr()),
                "aiy_dist_stats")
        d0 += n
    return WealthStats(lorenz=lor.reshape(lead + (p.size,)), percentile_values=pct.reshape(lead + (p.size,)),
                       gini=summ[:, 2].reshape(lead).copy(), mean=summ[:, 1].reshape(lead).copy(),
                       total=summ[:, 0].reshape(lead).copy(), bottom_share=summ[:, 3].reshape(lead).copy(),
                       percentiles=p)


def batch_wealth_stats(batch, percentiles=None):
    """``histogram_stats`` of ``batch.mass`` of a ``StationaryBatch`` on its grids: one row per
    calibration (the wealth statistics of a Table II cell)."""
    return histogram_stats(batch.mass, batch.d_a, percentiles)
