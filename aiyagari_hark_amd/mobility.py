"""Wealth and income mobility on the histogram: cohorts followed through the lotteries
(DESIGN.md §4s).

The Young lotteries and the forward step define the Markov chain on (s, a_j) exactly, so the
restriction of a distribution to a group of households -- a cohort -- pushed through them is
that group's exact later distribution: no Monte Carlo, no panel.  ``aiy_cohort_forward``
(``csrc/cohort.hip``) carries up to 16 cohorts through one lottery per period in one launch per
period and reports, for every period, each cohort's capital, consumption, and its mass by wealth
class and by income state.

``wealth_classes``    the nodes of the wealth classes between percentiles of a distribution
``cohorts_by_class``  the distribution split by wealth class, ``cohorts_by_state`` by income state
``cohort_forward``    the sweep: ``CohortPaths`` (K, C, occ, inc)
``mobility``          transition matrices between wealth classes, Shorrocks index, mean reversion
                      of wealth and the income composition of every cohort at a steady state

``solve_transition(..., cohorts=(0.2, 0.4, 0.6, 0.8))`` follows the wealth classes of the initial
distribution along the solved path (``TransitionResult.cohorts``).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from . import stats as _stats

F64 = torch.float64
MAX_PERCENTILES = _lib.AIY_MAX_COHORTS - 1


@dataclass
class CohortPaths:
    K: np.ndarray            # [n_cal][G][T+1] capital held by cohort g in period t
    C: np.ndarray | None     # [n_cal][G][T] its consumption (prices given)
    occ: np.ndarray          # [n_cal][G][T+1][Q] its mass in wealth class q
    inc: np.ndarray | None   # [n_cal][G][T+1][S] its mass in income state s
    edges: np.ndarray        # [n_cal][Q+1] int32: class q holds the nodes [edges[q], edges[q+1])


@dataclass
class MobilityResult:
    shares: np.ndarray            # [n_cal][G] mass of every cohort at the start
    thresholds: np.ndarray        # [n_cal][Q-1] the asset value at each inner edge (the upper class's first node)
    matrix: np.ndarray            # [n_cal][H][G][Q] P(class q after h periods | cohort g); NaN row for an empty cohort
    shorrocks: np.ndarray | None  # [n_cal][H] (Q - trace) / (Q - 1), by="wealth" only
    mean_wealth: np.ndarray       # [n_cal][G][hmax+1] K_g / share_g
    income: np.ndarray            # [n_cal][H][G][S] P(income state s after h periods | cohort g)
    horizons: np.ndarray          # [H]
    edges: np.ndarray             # [n_cal][Q+1]
    paths: CohortPaths            # the sweep behind the tables, hmax periods


def _check_class_percentiles(percentiles):
    """stats._check_percentiles (a tuple is taken as a list), strictly ascending, at most 15."""
    if isinstance(percentiles, tuple):
        percentiles = list(percentiles)
    if not isinstance(percentiles, (list, np.ndarray)) or len(percentiles) == 0:
        raise ValueError("Percentiles should be a list or numpy array of floats between 0 and 1")
    p = _stats._check_percentiles(percentiles)
    if p.size > MAX_PERCENTILES:
        raise ValueError(f"at most {MAX_PERCENTILES} percentiles (one cohort per class, {_lib.AIY_MAX_COHORTS} "
                         "cohorts per sweep)")
    if np.any(np.diff(p) <= 0):
        raise ValueError("percentiles must be strictly ascending")
    return p


def _check_horizons(horizons):
    try:
        hs = list(horizons)
    except TypeError:
        raise ValueError("horizons must be positive, strictly ascending integers") from None
    ok = len(hs) > 0 and all(isinstance(h, (int, np.integer)) and not isinstance(h, bool) and h > 0 for h in hs)
    if not ok or any(b <= a for a, b in zip(hs, hs[1:])):
        raise ValueError(f"horizons must be positive, strictly ascending integers, got {horizons!r}")
    return np.array(hs, dtype=np.int64)


def class_edges(g, p):
    """The class rule on one marginal g [n_a]: with F = cumsum(g) / sum(g) and F_prev = (0, F[:-1]),
    a node belongs to the class in which its first household falls, so the inner edges are
    searchsorted(F_prev, p, side="left").  Returns int32 [len(p) + 2]."""
    g = np.asarray(g, dtype=np.float64)
    F = np.cumsum(g) / np.sum(g)
    F_prev = np.concatenate(([0.0], F[:-1]))
    e = np.empty(len(p) + 2, dtype=np.int32)
    e[0], e[-1] = 0, g.size
    e[1:-1] = np.searchsorted(F_prev, p, side="left")
    return e


def _host_mass(batch, mass):
    m = batch.mass if mass is None else mass
    m = m.detach().cpu().numpy() if torch.is_tensor(m) else np.asarray(m, dtype=np.float64)
    return m.reshape(len(batch.cals), batch.S, batch.n_a)


def wealth_classes(batch, percentiles=(0.2, 0.4, 0.6, 0.8), mass=None):
    """``edges`` int32 [n_cal][Q+1], Q = len(percentiles) + 1: the wealth classes of ``mass``
    (default ``batch.mass``) between the percentiles, by ``class_edges`` on the marginal over
    assets (the sum over states, ascending, on the host).  A node that holds more than one band
    leaves classes empty (repeated edges)."""
    p = _check_class_percentiles(percentiles)
    m = _host_mass(batch, mass)
    return np.stack([class_edges(m[i].sum(axis=0), p) for i in range(m.shape[0])])


def _device_mass(batch, mass):
    m = batch.mass if mass is None else mass
    if not torch.is_tensor(m):
        m = torch.as_tensor(np.ascontiguousarray(m, dtype=np.float64))
    return m.to(batch.device).reshape(len(batch.cals), batch.S, batch.n_a)


def cohorts_by_class(batch, edges, mass=None):
    """Device tensor [Q][n_cal][S][n_a]: cohort q holds the elements of ``mass`` on the nodes of
    class q, copied and not rescaled, and zeros elsewhere -- every element in exactly one cohort."""
    edges = np.asarray(edges)
    n_cal, n_a = len(batch.cals), batch.n_a
    if edges.ndim != 2 or edges.shape[0] != n_cal or edges.shape[1] < 2:
        raise ValueError(f"edges must be [n_cal={n_cal}][Q+1], got {edges.shape}")
    Q = edges.shape[1] - 1
    # the class of node j: the number of upper edges at or below j
    cls = np.stack([np.searchsorted(edges[i, 1:], np.arange(n_a), side="right") for i in range(n_cal)])
    m = _device_mass(batch, mass)
    own = torch.as_tensor(cls).to(batch.device)[None, :, None, :] == \
        torch.arange(Q, device=batch.device)[:, None, None, None]
    return torch.where(own, m[None], torch.zeros((), dtype=F64, device=batch.device)).contiguous()


def cohorts_by_state(batch, mass=None):
    """Device tensor [S][n_cal][S][n_a]: cohort s holds row s of ``mass`` and zeros elsewhere."""
    m = _device_mass(batch, mass)
    out = torch.zeros((batch.S,) + tuple(m.shape), dtype=F64, device=batch.device)
    for s in range(batch.S):
        out[s, :, s, :] = m[:, s, :]
    return out


def cohort_forward(batch, lo, wlo, cohorts, T, edges, R=None, w=None, states=True, stream=None):
    """aiy_cohort_forward: the cohorts [G][n_cal][S][n_a] (device) advanced in place by T periods
    on the device lotteries ``lo`` / ``wlo`` [n_lot][n_cal][S][n_a], n_lot = T (a path) or 1 (one
    lottery for every period: a steady state).  ``edges`` [n_cal][Q+1]: the wealth classes of the
    occupancy; ``R``, ``w`` ([n_cal][T+1], NumPy or device): also the cohorts' consumption;
    ``states=False`` skips the occupancy by income state.  Returns ``CohortPaths``.  More than 16
    cohorts run as several calls of at most 16 -- cohorts do not interact.
    Raises AiyagariLibError (AIY_ERR_UNSUPPORTED, everything untouched) when a lottery row fails
    the monotone / range check."""
    T = int(T)
    if T < 1 or int(lo.shape[0]) not in (1, T):
        raise ValueError(f"lo must hold 1 or T={T} >= 1 lottery periods, got {int(lo.shape[0])}")
    if (R is None) != (w is None):
        raise ValueError("R and w must both be given or both be None")
    from .transition import _device
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    n_lot = int(lo.shape[0])
    dev = batch.device
    if tuple(lo.shape) != (n_lot, n_cal, S, n_a) or tuple(wlo.shape) != tuple(lo.shape) or lo.dtype != torch.int32:
        raise ValueError(f"lo / wlo must be [n_lot]{(n_cal, S, n_a)} (int32 / float64), got {tuple(lo.shape)} and "
                         f"{tuple(wlo.shape)}")
    if cohorts.dim() != 4 or tuple(cohorts.shape[1:]) != (n_cal, S, n_a) or cohorts.dtype != F64:
        raise ValueError(f"cohorts must be float64 [G]{(n_cal, S, n_a)}, got {tuple(cohorts.shape)}")
    edges = np.ascontiguousarray(edges, dtype=np.int32)
    if edges.ndim != 2 or edges.shape[0] != n_cal or not 1 <= edges.shape[1] - 1 <= _lib.AIY_MAX_CLASSES:
        raise ValueError(f"edges must be [n_cal={n_cal}][Q+1] with Q in 1..{_lib.AIY_MAX_CLASSES}, got {edges.shape}")
    G, Q = int(cohorts.shape[0]), edges.shape[1] - 1
    want_c = R is not None
    dR = dw = None
    if want_c:
        dR, dw = _device(R, dev), _device(w, dev)
        if tuple(dR.shape) != (n_cal, T + 1) or tuple(dw.shape) != (n_cal, T + 1):
            raise ValueError(f"price paths must be [n_cal][T+1] = {(n_cal, T + 1)}, got {tuple(dR.shape)} and "
                             f"{tuple(dw.shape)}")
    h = _lib.handle(dev.index)
    K = np.zeros((n_cal, G, T + 1))
    C = np.zeros((n_cal, G, T)) if want_c else None
    occ = np.zeros((n_cal, G, T + 1, Q))
    inc = np.zeros((n_cal, G, T + 1, S)) if states else None
    dp = _lib.c_double_p
    for g0 in range(0, G, _lib.AIY_MAX_COHORTS):
        n = min(_lib.AIY_MAX_COHORTS, G - g0)
        work = _lib.work_space(dev, "cohort", "cohort", n_cal=n_cal, S=S, n_a=n_a, n_lot=n_lot, G=n, Q=Q)
        k, o = np.zeros((n_cal, n, T + 1)), np.zeros((n_cal, n, T + 1, Q))
        c = np.zeros((n_cal, n, T)) if want_c else None
        i = np.zeros((n_cal, n, T + 1, S)) if states else None
        h.check(h.lib.aiy_cohort_forward(h.h, n_cal, S, n_a, T, n_lot, n, Q, _lib.ptr(lo), _lib.ptr(wlo),
                                         _lib.ptr(batch.d_P), _lib.ptr(batch.d_a), _lib.ptr(dR), _lib.ptr(dw),
                                         _lib.ptr(batch.d_lab) if want_c else None,
                                         edges.ctypes.data_as(_lib.c_int32_p), _lib.ptr(work),
                                         _lib.ptr(cohorts[g0:g0 + n]), k.ctypes.data_as(dp),
                                         c.ctypes.data_as(dp) if want_c else None, o.ctypes.data_as(dp),
                                         i.ctypes.data_as(dp) if states else None, _lib.stream_ptr(stream)),
                "aiy_cohort_forward")
        K[:, g0:g0 + n], occ[:, g0:g0 + n] = k, o
        if want_c:
            C[:, g0:g0 + n] = c
        if states:
            inc[:, g0:g0 + n] = i
    return CohortPaths(K=K, C=C, occ=occ, inc=inc, edges=edges)


def mobility(batch, percentiles=(0.2, 0.4, 0.6, 0.8), horizons=(1, 5, 10), by="wealth"):
    """Mobility tables of the steady state of ``batch`` (its ``mass`` and ``last_tables``): the
    cohorts -- the wealth classes between ``percentiles`` (by="wealth") or the S income states
    (by="income") -- swept max(horizons) periods on the steady lottery (n_lot = 1): the one
    ``capital_supply`` left in the batch, under which ``batch.mass`` was solved, else
    ``steady_lottery(batch)``.  Returns ``MobilityResult``; ``matrix`` is over wealth classes either
    way, and its row g and the row of ``income`` are the cohort's occupancies over its share (NaN
    for a cohort without mass).

    The batch's lottery is taken to belong to ``batch.mass``, which holds after ``capital_supply``
    and ``steady_state``.  A caller who has overwritten ``batch.mass`` (or ``batch.lo`` /
    ``batch.wlo``) since gets the tables of that mass on that lottery, not of a steady state: use
    ``cohort_forward`` with the lottery meant."""
    hs = _check_horizons(horizons)
    if by not in ("wealth", "income"):
        raise ValueError(f"by must be 'wealth' or 'income', got {by!r}")
    p = _check_class_percentiles(percentiles)
    from .transition import steady_lottery
    hmax = int(hs[-1])
    edges = wealth_classes(batch, p)
    cohorts = cohorts_by_class(batch, edges) if by == "wealth" else cohorts_by_state(batch)
    # the lottery batch.mass is stationary under: the one capital_supply left in the batch, else
    # (a batch cut out by transition.select) the lottery of its tables at the firm's rate
    if getattr(batch, "_mass_valid", False):
        lo, wlo = batch.lo, batch.wlo
    else:
        lo, wlo, _, _ = steady_lottery(batch)
    paths = cohort_forward(batch, lo[None], wlo[None], cohorts, hmax, edges)
    Q = edges.shape[1] - 1
    shares = paths.occ[:, :, 0, :].sum(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        matrix = np.swapaxes(paths.occ[:, :, hs, :], 1, 2) / shares[:, None, :, None]
        income = np.swapaxes(paths.inc[:, :, hs, :], 1, 2) / shares[:, None, :, None]
        mean_wealth = paths.K / shares[:, :, None]
        shorrocks = None
        if by == "wealth":
            shorrocks = (Q - np.trace(matrix, axis1=2, axis2=3)) / (Q - 1)
    inner = np.minimum(edges[:, 1:-1], batch.n_a - 1)
    thresholds = np.take_along_axis(batch.aGrid, inner.astype(np.int64), axis=1)
    return MobilityResult(shares=shares, thresholds=thresholds, matrix=matrix, shorrocks=shorrocks,
                          mean_wealth=mean_wealth, income=income, horizons=hs, edges=edges, paths=paths)
