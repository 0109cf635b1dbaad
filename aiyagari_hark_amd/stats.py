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

Any household variable: consumption, income, earnings and cash on hand are
nondecreasing in assets within an income state, so a distribution of one of them is S sorted runs.
``variable_stats`` orders it by an S-way merge (``aiy_var_merge``, ``csrc/var_stats.hip``) and
hands the merged distribution to ``aiy_dist_stats``; ``household_variables`` makes the variables
from a lottery and prices, ``batch_inequality`` reports them for a steady state, with moments and
correlations (``aiy_var_moments``), and ``transition.path_variable_stats`` for every period of a path.
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


# -------------------------------------------------------------------------------------
# Any household variable on the histogram
# -------------------------------------------------------------------------------------
VARIABLES = tuple(_lib.AIY_VARIABLES)   # in the order of aiy_household_variables' output
_UNSORTABLE = {
    "saving": "saving a' - a is not monotone in assets within an income state once prices move (it turns at R "
              "1 % above the steady rate), and its mean is zero at a steady state, so its Lorenz curve means "
              "nothing: it gets moments only, not sorted statistics"}


@dataclass
class VariableStats:
    """Statistics of a household variable over a stack of distributions of leading shape [...]:
    the fields of ``WealthStats`` (the variable in place of wealth), then its dispersion."""
    lorenz: np.ndarray              # [..., n_p] Lorenz shares at ``percentiles``
    percentile_values: np.ndarray   # [..., n_p] percentiles of the variable (NaN below the CDF's first value)
    gini: np.ndarray                # [...]
    mean: np.ndarray                # [...] sum y w / sum w
    total: np.ndarray               # [...] sum w
    bottom_share: np.ndarray        # [...] the weight share of the lowest-ranked node
    percentiles: np.ndarray         # [n_p]
    std: np.ndarray                 # [...] sqrt(sum w (y - m)^2 / sum w), two passes
    cv: np.ndarray                  # [...] std / |mean|


@dataclass
class Inequality:
    """``batch_inequality``: one row per calibration."""
    stats: dict                     # name -> VariableStats [n_cal], the sortable variables
    moments: dict                   # name -> dict(mean, std, cv), each [n_cal], every variable asked for
    corr: np.ndarray                # [n_cal][n_v][n_v] weighted correlations, in the order of ``variables``
    variables: tuple                # the names asked for


def _check_variables(variables):
    names = tuple(variables)
    if not names or len(set(names)) != len(names) or any(n not in VARIABLES for n in names):
        raise ValueError(f"variables must be distinct names out of {VARIABLES}, got {names!r}")
    return names


def _moments(h, variables, weight, n_dist, S, n_a, work):
    """aiy_var_moments of the device tensors ``variables`` (each n_dist x S x n_a elements) on
    ``weight``: HOST [n_dist][1 + n_v + n_v^2]."""
    n_v = len(variables)
    out = np.empty((n_dist, 1 + n_v + n_v * n_v))
    ptrs = (_lib.vp * n_v)(*[_lib.ptr(v) for v in variables])
    h.check(h.lib.aiy_var_moments(h.h, n_dist, S, n_a, n_v, ptrs, _lib.ptr(weight), _lib.ptr(work),
                                  out.ctypes.data_as(_lib.c_double_p), _lib.stream_ptr()), "aiy_var_moments")
    return out


def variable_stats(values, mass, percentiles=None, slab=None, device=None):
    """Statistics of a household variable: ``values`` and ``mass`` [..., S, n_a], device tensors or
    NumPy arrays of one shape, ``values`` nondecreasing in assets within every state (consumption,
    income, earnings, cash on hand and wealth are; ``household_variables`` makes them).  Returns
    ``VariableStats`` of the leading shape; ``percentiles=None`` uses [0.5].

    Every distribution is S sorted runs: ``aiy_var_merge`` orders it by an S-way merge (stable:
    ties by state, then node) and the merged distribution goes to ``aiy_dist_stats`` as a marginal
    of S n_a nodes on its own ascending "grid"; ``std`` comes from ``aiy_var_moments``.  A run that
    decreases or holds a NaN is refused (AiyagariLibError, AIY_ERR_UNSUPPORTED).  The stack goes
    through in slabs of ``slab`` distributions, by default the number whose sorted stacks and
    ``aiy_dist_stats`` work space (32 S n_a bytes per distribution) stay within 256 MB; the results
    do not depend on the slab size."""
    p = _check_percentiles(percentiles)
    v = _as_device(values, device)
    m = _as_device(mass, v.device)
    if v.shape != m.shape:
        raise ValueError(f"values {tuple(v.shape)} and mass {tuple(m.shape)} must have one shape")
    if v.dim() < 2 or v.shape[-1] < 2 or not 1 <= v.shape[-2] <= _lib.AIY_MAX_STATES:
        raise ValueError(f"values {tuple(v.shape)}: needs [..., S, n_a] with n_a >= 2 and S <= {_lib.AIY_MAX_STATES}")
    S, n_a = int(v.shape[-2]), int(v.shape[-1])
    N = S * n_a
    lead = tuple(int(x) for x in v.shape[:-2])
    n_dist = math.prod(lead)
    if n_dist < 1:
        raise ValueError("no distribution")
    h = _lib.handle(v.device.index)
    if slab is None:
        slab = max(1, SLAB_BYTES // (32 * N))
    slab = max(1, min(int(slab), n_dist))
    work = _lib.work_space(v.device, "var", "", n_dist=slab, S=S, n_a=n_a)
    ds_work = _lib.work_space(v.device, "dist_stats", "", n_dist=slab, n_a=N)
    ks = torch.empty((slab, N), dtype=torch.float64, device=v.device)
    ws = torch.empty((slab, N), dtype=torch.float64, device=v.device)
    v, m = v.reshape(n_dist, S, n_a), m.reshape(n_dist, S, n_a)
    lor = np.empty((n_dist, p.size))
    pct = np.empty((n_dist, p.size))
    summ = np.empty((n_dist, 4))
    var = np.empty(n_dist)
    dp = _lib.c_double_p
    for d0 in range(0, n_dist, slab):
        n = min(slab, n_dist - d0)
        h.check(h.lib.aiy_var_merge(h.h, n, S, n_a, _lib.ptr(v[d0:d0 + n]), _lib.ptr(m[d0:d0 + n]), _lib.ptr(work),
                                    _lib.ptr(ks), _lib.ptr(ws), None, _lib.stream_ptr()), "aiy_var_merge")
        h.check(h.lib.aiy_dist_stats(h.h, n, n, N, _lib.ptr(ws), _lib.ptr(ks), p.ctypes.data_as(dp), p.size,
                                     _lib.ptr(ds_work), lor[d0:].ctypes.data_as(dp), pct[d0:].ctypes.data_as(dp),
                                     summ[d0:].ctypes.data_as(dp), _lib.stream_ptr()), "aiy_dist_stats")
        var[d0:d0 + n] = _moments(h, [v[d0:d0 + n]], m[d0:d0 + n], n, S, n_a, work)[:, 2]
    mean = summ[:, 1].reshape(lead).copy()
    std = np.sqrt(var).reshape(lead)
    with np.errstate(invalid="ignore", divide="ignore"):
        cv = std / np.abs(mean)
    return VariableStats(lorenz=lor.reshape(lead + (p.size,)), percentile_values=pct.reshape(lead + (p.size,)),
                         gini=summ[:, 2].reshape(lead).copy(), mean=mean, total=summ[:, 0].reshape(lead).copy(),
                         bottom_share=summ[:, 3].reshape(lead).copy(), percentiles=p, std=std, cv=cv)


def _variables_into(batch, lo, wlo, R_ptr, w_ptr, ld_price, n_t, mask, out):
    """aiy_household_variables into ``out`` (device, the variables of ``mask`` in bit order, each
    [n_t][n_cal][S][n_a]); R_ptr / w_ptr: device addresses of the first period's prices."""
    h = _lib.handle(batch.device.index)
    h.check(h.lib.aiy_household_variables(h.h, len(batch.cals), batch.S, batch.n_a, int(n_t), _lib.ptr(lo),
                                          _lib.ptr(wlo), R_ptr, w_ptr, int(ld_price), _lib.ptr(batch.d_a),
                                          _lib.ptr(batch.d_lab), int(mask), _lib.ptr(out), _lib.stream_ptr()),
            "aiy_household_variables")


def household_variables(batch, lo, wlo, R, w, which=VARIABLES):
    """The variables ``which`` (names out of ``VARIABLES``) of every node of the lotteries ``lo`` /
    ``wlo``, device [n_cal][S][n_a] with prices ``R``, ``w`` [n_cal], or [n_t][n_cal][S][n_a] with
    prices [n_cal][n_p], n_p >= n_t (period t at column t).  Returns a dict name -> device tensor
    of the lottery's shape (``aiy_household_variables``):

        consumption (R a + w lab) - a'    income (R - 1) a + w lab    earnings w lab
        cash R a + w lab    saving a' - a    wealth a,    a' = wlo a[lo] + (1 - wlo) a[lo + 1]."""
    names = _check_variables(which)
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    dR, dw = _as_device(R, batch.device), _as_device(w, batch.device)
    stacked = lo.dim() == 4
    n_t = int(lo.shape[0]) if stacked else 1
    want = ((n_t, n_cal, S, n_a) if stacked else (n_cal, S, n_a))
    if tuple(lo.shape) != want or tuple(wlo.shape) != want or lo.dtype != torch.int32:
        raise ValueError(f"lo (int32) and wlo must be [n_t][n_cal={n_cal}][S={S}][n_a={n_a}] or one period of it, "
                         f"got {tuple(lo.shape)} and {tuple(wlo.shape)}")
    if dR.shape != dw.shape or dR.shape[0] != n_cal or dR.dim() != (2 if stacked else 1) or \
            (stacked and dR.shape[1] < n_t):
        raise ValueError(f"prices {tuple(dR.shape)}, {tuple(dw.shape)} do not fit lotteries {tuple(lo.shape)}")
    mask = sum(_lib.AIY_VARIABLES[n] for n in names)
    out = torch.empty((len(names),) + want, dtype=torch.float64, device=batch.device)
    _variables_into(batch, lo, wlo, _lib.ptr(dR), _lib.ptr(dw), dR.shape[1] if stacked else 1, n_t, mask, out)
    order = [n for n in VARIABLES if n in names]
    return {n: out[order.index(n)] for n in names}


def _dispersion(mom, n_v):
    """(mean [n][n_v], std [n][n_v], cv, cov [n][n_v][n_v]) of aiy_var_moments' rows."""
    mean = mom[:, 1:1 + n_v]
    cov = mom[:, 1 + n_v:].reshape(-1, n_v, n_v)
    std = np.sqrt(np.einsum("nuu->nu", cov))
    with np.errstate(invalid="ignore", divide="ignore"):
        cv = std / np.abs(mean)
    return mean, std, cv, cov


def batch_inequality(batch, percentiles=None, variables=("wealth", "consumption", "income", "earnings"),
                     sorted_variables=None):
    """Inequality of a ``StationaryBatch`` at its steady state, one row per calibration: the
    variables of ``household_variables`` on ``steady_lottery(batch)`` weighted by ``batch.mass``.
    Returns ``Inequality``: ``stats[name]`` the ``VariableStats`` of every sortable variable named
    (``sorted_variables``, by default all of ``variables`` but ``saving``), ``moments[name]`` mean,
    std and cv of every variable named, ``saving`` included, and ``corr`` their weighted
    correlations (``aiy_var_moments``).  ``saving`` in ``sorted_variables``: ValueError."""
    from .transition import steady_lottery
    names = _check_variables(variables)
    if len(names) > _lib.AIY_VAR_MAX_MOMENTS:
        raise ValueError(f"at most {_lib.AIY_VAR_MAX_MOMENTS} variables")
    sortable = tuple(n for n in names if n not in _UNSORTABLE) if sorted_variables is None else tuple(sorted_variables)
    for n in sortable:
        if n in _UNSORTABLE:
            raise ValueError(_UNSORTABLE[n])
        if n not in names:
            raise ValueError(f"sorted variable {n!r} is not among variables {names!r}")
    p = _check_percentiles(percentiles)
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    lo, wlo, dR, dw = steady_lottery(batch)
    val = household_variables(batch, lo, wlo, dR, dw, names)
    mass = batch.mass.reshape(n_cal, S, n_a)
    stats = {n: variable_stats(val[n], mass, p) for n in sortable}
    h = _lib.handle(batch.device.index)
    work = _lib.work_space(batch.device, "var", "", n_dist=n_cal, S=S, n_a=n_a)
    mean, std, cv, cov = _dispersion(_moments(h, [val[n] for n in names], mass, n_cal, S, n_a, work), len(names))
    with np.errstate(invalid="ignore", divide="ignore"):
        corr = cov / (std[:, :, None] * std[:, None, :])
    moments = {n: dict(mean=mean[:, u].copy(), std=std[:, u].copy(), cv=cv[:, u].copy()) for u, n in enumerate(names)}
    return Inequality(stats=stats, moments=moments, corr=corr, variables=names)
