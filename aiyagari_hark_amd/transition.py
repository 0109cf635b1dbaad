"""Perfect-foresight transition paths of the stationary economy.

Given a steady state (``steady_state``), a TFP path ``Z[0..T]`` with ``Z[T] = 1`` and an
initial distribution, ``solve_transition`` finds the capital path ``K[0..T]`` on which
households that foresee the prices

    r_t = Z_t alpha K_t^(alpha - 1) - delta,   w_t = Z_t (1 - alpha) K_t^alpha   (L = 1)

save exactly ``K``: a damped fixed point ``K <- (1 - lambda) K + lambda Ks(K)``, ``K[0]``
given by the initial distribution.  One evaluation ``Ks(K)`` is ``household_block``:

    backward  (m_{u-1}, c_{u-1}) = EGM step from (m_u, c_u) at R_u, w_u,  u = T .. 1,
              with the Young lottery of every period from the same interpolation
              (aiy_transition_backward, csrc/transition.hip);
    forward   mass_{t+1} = lottery step of mass_t, Ks[t] = sum mass_t a,
              C[t] = sum mass_t (q_t - a'_t)  (aiy_transition_forward).

``method="newton"`` replaces the damping by a quasi-Newton step on the whole path with the
sequence-space Jacobian of the block at the steady state (``household_jacobian``, the
fake-news algorithm of Auclert, Bardoczy, Rognlie and Straub 2021; DESIGN.md §4i,
csrc/transition_jac.hip); the same matrices give ``impulse_response``, the linear response
to a TFP path.

Everything per grid point runs in libaiyagari, batched over calibrations; the host only
prices the path and updates it (damping, or one T x T solve per calibration).  Several GPUs: split the calibrations with
``parallel.split_calibrations`` and solve each share on its device -- the calibrations of
a batch never interact.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
import time
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from . import setup_math as sm
from . import stats as _stats
from .stationary import StationaryBatch, _resolve_device, firm_prices, solve_table2

F64 = torch.float64


def steady_state(cals, n_a, aMin=0.001, aMax=50.0, aNestFac=2, device=None, egm_tol=1e-8, hist_tol=1e-12, accel=-1,
                 **solve_kw):
    """Steady state of every calibration: ``solve_table2`` for r*, then one
    ``StationaryBatch.capital_supply(r*)``.  Returns ``(batch, r, K)``: the batch keeps the
    converged tables (``batch.last_tables``) and the stationary mass (``batch.mass``) on
    device; ``K`` is the capital supply at r* (the capital the distribution holds)."""
    cals = list(cals)
    device = _resolve_device(device)
    solve_kw.setdefault("method", "brent")
    res = solve_table2(cals, n_a=n_a, aMin=aMin, aMax=aMax, aNestFac=aNestFac, egm_tol=egm_tol, hist_tol=hist_tol,
                       device=device, **solve_kw)
    batch = StationaryBatch(cals, sm.make_grid_exp_mult(aMin, aMax, n_a, aNestFac), device=device)
    K, _, _ = batch.capital_supply(res.r, egm_tol=egm_tol, hist_tol=hist_tol, accel=accel)
    return batch, np.array(res.r), K


def select(batch, idx):
    """The calibrations ``idx`` of ``batch`` as a batch of their own, with their converged
    tables and mass (one share of ``parallel.split_calibrations``, or a single calibration)."""
    idx = list(idx)
    sub = StationaryBatch([batch.cals[i] for i in idx], batch.aGrid[0], device=batch.device)
    if getattr(batch, "last_tables", None) is not None:
        sub.last_tables = tuple(t[idx].contiguous() for t in batch.last_tables)
    sub.mass.copy_(batch.mass[idx])
    return sub


def path_prices(K, Z, alpha, delta):
    """(r, w) [n_cal][T+1] of the Cobb-Douglas firm with L = 1 on a capital path K and a TFP
    path Z, element by element through libm's pow (as stationary.firm_prices)."""
    K = np.asarray(K, dtype=np.float64)
    Z = np.broadcast_to(np.asarray(Z, dtype=np.float64), K.shape)
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64).reshape(-1, 1), K.shape)
    delta = np.broadcast_to(np.asarray(delta, dtype=np.float64).reshape(-1, 1), K.shape)
    r = np.empty(K.shape)
    w = np.empty(K.shape)
    for i in np.ndindex(K.shape):
        a, k, z = float(alpha[i]), float(K[i]), float(Z[i])
        r[i] = z * a * math.pow(k, a - 1.0) - float(delta[i])
        w[i] = z * (1.0 - a) * math.pow(k, a)
    return r, w


def _device(x, dev):
    """A device tensor as it is; anything else as a float64 tensor on ``dev``."""
    if torch.is_tensor(x):
        return x
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).to(dev)


def _tables(t, n_cal, S, n_a):
    """A [n_cal][S][n_a+1] view of policy tables given with or without the n_M = 1 axis."""
    t = t.reshape(n_cal, S, n_a + 1)
    return t if t.is_contiguous() else t.contiguous()


@dataclass
class BlockResult:
    Ks: np.ndarray            # [n_cal][T+1]
    C: np.ndarray | None      # [n_cal][T]
    lo: torch.Tensor          # [T][n_cal][S][n_a] int32, device
    wlo: torch.Tensor         # [T][n_cal][S][n_a] device
    m0: torch.Tensor | None   # [n_cal][S][n_a+1] policy of period 0, device
    c0: torch.Tensor | None
    mass_T: torch.Tensor      # [n_cal][S][n_a] device
    marg: torch.Tensor | None = None   # [T+1][n_cal][n_a] device: the marginal over assets of every period
    masses: torch.Tensor | None = None   # [T+1][n_cal][S][n_a] device: every period's mass (masses=True)


class TransitionBuffers:
    """Device buffers of one (batch, T): the lotteries, the work space and a mass scratch,
    allocated once and reused by every block evaluation of a solve.  ``marginals=True`` adds
    the [T+1][n_cal][n_a] buffer of the period marginals (``household_block(marginals=True)``)."""

    def __init__(self, batch: StationaryBatch, T: int, marginals: bool = False):
        n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
        dev = batch.device
        self.T = int(T)
        self.work = _lib.work_space(dev, "transition", "transition", n_cal=n_cal, S=S, n_a=n_a, T=self.T)
        self.lo = torch.empty((self.T, n_cal, S, n_a), dtype=torch.int32, device=dev)
        self.wlo = torch.empty((self.T, n_cal, S, n_a), dtype=F64, device=dev)
        self.m0 = torch.empty((n_cal, S, n_a + 1), dtype=F64, device=dev)
        self.c0 = torch.empty((n_cal, S, n_a + 1), dtype=F64, device=dev)
        self.mass = torch.empty((n_cal, S, n_a), dtype=F64, device=dev)
        self.marg = torch.empty((self.T + 1, n_cal, n_a), dtype=F64, device=dev) if marginals else None
        self.masses = None   # [T+1][n_cal][S][n_a], allocated by household_block(masses=True) only


def transition_backward(batch, R, w, m_term, c_term, buffers, export_policy=True, stream=None):
    """aiy_transition_backward: fills buffers.lo / buffers.wlo (and m0 / c0).  R, w: device
    tensors [n_cal][T+1].  Asynchronous."""
    n_cal, S, n_a, T = len(batch.cals), batch.S, batch.n_a, buffers.T
    h = _lib.handle(batch.device.index)
    model = _lib.TransitionModel(n_cal, S, n_a, T, _lib.ptr(batch.d_a), _lib.ptr(batch.d_P), _lib.ptr(batch.d_lab),
                                 _lib.ptr(batch.d_beta), _lib.ptr(batch.d_crra), _lib.ptr(R), _lib.ptr(w),
                                 _lib.ptr(m_term), _lib.ptr(c_term))
    h.check(h.lib.aiy_transition_backward(h.h, ctypes.byref(model), _lib.ptr(buffers.work), _lib.ptr(buffers.lo),
                                          _lib.ptr(buffers.wlo), _lib.ptr(buffers.m0) if export_policy else None,
                                          _lib.ptr(buffers.c0) if export_policy else None, _lib.stream_ptr(stream)),
            "aiy_transition_backward")


def transition_forward(batch, lo, wlo, mass, T, work, R=None, w=None, want_c=True, stream=None, marg=None,
                       rows="monotone", mass_path=None):
    """aiy_transition_forward on device lotteries [T][n_cal][S][n_a]: advances ``mass`` in
    place from period 0 to period T and returns (Ks [n_cal][T+1], C [n_cal][T] or None).
    With ``marg`` (device [T+1][n_cal][n_a]) the sweep is aiy_transition_forward_marginals: the
    same results, and marg[t] = the sum over states of mass_t, t = 0 .. T.
    Raises AiyagariLibError (AIY_ERR_UNSUPPORTED) when a lottery row fails the monotone /
    range check; mass (and marg) is then untouched.

    ``rows="monotone"`` (the default) still refuses a lottery with a row that is not
    non-decreasing.  ``rows="any"`` is aiy_transition_forward_any: such rows run
    through the windowed pull, ``work`` must come from ``_lib.work_space(dev, "transition_any",
    ...)``, and the call returns ``(Ks, C, rows_turned)``, the number of rows with a decreasing
    pair.  It refuses (AIY_ERR_UNSUPPORTED, everything untouched) an entry outside [0, n_a - 2]
    and a row so disordered that its windows hold more than 4 (n_a + 1) sources; on monotone
    lotteries it gives the bits of the default.  Any other value: ValueError.

    With ``mass_path`` (device [T+1][n_cal][S][n_a]) the sweep is aiy_transition_forward_masses: the
    same results, and mass_path[t] = mass_t, t = 0 .. T, untouched when a row is
    refused.  It goes with neither ``marg`` nor ``rows="any"``."""
    if rows not in ("monotone", "any"):
        raise ValueError(f"rows must be 'monotone' or 'any', got {rows!r}")
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    h = _lib.handle(batch.device.index)
    Ks = np.zeros((n_cal, T + 1))
    C = np.zeros((n_cal, T)) if want_c else None
    args = (h.h, n_cal, S, n_a, int(T), _lib.ptr(lo), _lib.ptr(wlo), _lib.ptr(batch.d_P), _lib.ptr(batch.d_a),
            _lib.ptr(R) if want_c else None, _lib.ptr(w) if want_c else None,
            _lib.ptr(batch.d_lab) if want_c else None, _lib.ptr(work), _lib.ptr(mass),
            Ks.ctypes.data_as(_lib.c_double_p), C.ctypes.data_as(_lib.c_double_p) if want_c else None)
    if marg is not None and (tuple(marg.shape) != (T + 1, n_cal, n_a) or marg.dtype != F64):
        raise ValueError(f"marg must be float64 [T+1][n_cal][n_a] = {(T + 1, n_cal, n_a)}, got {tuple(marg.shape)}")
    if mass_path is not None:
        if marg is not None or rows == "any":
            raise ValueError("mass_path goes with neither marg nor rows='any'")
        if tuple(mass_path.shape) != (T + 1, n_cal, S, n_a) or mass_path.dtype != F64:
            raise ValueError(f"mass_path must be float64 [T+1][n_cal][S][n_a] = {(T + 1, n_cal, S, n_a)}, got "
                             f"{tuple(mass_path.shape)}")
        h.check(h.lib.aiy_transition_forward_masses(*args, _lib.ptr(mass_path), _lib.stream_ptr(stream)),
                "aiy_transition_forward_masses")
        return Ks, C
    if rows == "any":
        need = int(h.lib.aiy_transition_any_work_bytes(n_cal, S, n_a, int(T)))
        if work.numel() * work.element_size() < need:
            raise ValueError(f"rows='any' needs a 'transition_any' work space of {need} bytes, got "
                             f"{work.numel() * work.element_size()}")
        turned = ctypes.c_int32(0)
        h.check(h.lib.aiy_transition_forward_any(*args, _lib.ptr(marg), ctypes.byref(turned), _lib.stream_ptr(stream)),
                "aiy_transition_forward_any")
        return Ks, C, int(turned.value)
    if marg is None:
        h.check(h.lib.aiy_transition_forward(*args, _lib.stream_ptr(stream)), "aiy_transition_forward")
    else:
        h.check(h.lib.aiy_transition_forward_marginals(*args, _lib.ptr(marg), _lib.stream_ptr(stream)),
                "aiy_transition_forward_marginals")
    return Ks, C


def household_block(batch, R, w, m_term, c_term, mass0, want_c=True, export_policy=True, buffers=None, stream=None,
                    marginals=False, masses=False):
    """One household-block evaluation on the price paths R, w ([n_cal][T+1], NumPy or device):
    the backward sweep from the terminal policy (m_term, c_term), then the forward sweep from
    mass0 (left unchanged).  Returns BlockResult: Ks[n_cal][T+1], C[n_cal][T] and the device
    lotteries, period-0 policy and final mass (views of ``buffers``: the next evaluation with
    the same buffers overwrites them).  ``marginals=True`` also returns ``marg`` [T+1][n_cal][n_a],
    the marginal over assets of every period's mass (``path_wealth_stats`` reads it).
    ``masses=True`` instead returns ``masses`` [T+1][n_cal][S][n_a], every period's mass
    (``path_variable_stats`` reads it; 8 S n_a bytes per calibration and period)."""
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    dev = batch.device
    dR, dw = _device(R, dev), _device(w, dev)
    if dR.shape != dw.shape or dR.dim() != 2 or dR.shape[0] != n_cal or dR.shape[1] < 2:
        raise ValueError(f"price paths must be [n_cal][T+1], got {tuple(dR.shape)} and {tuple(dw.shape)}")
    T = dR.shape[1] - 1
    if buffers is None:
        buffers = TransitionBuffers(batch, T, marginals=marginals)
    elif buffers.T != T:
        raise ValueError(f"buffers hold T={buffers.T}, the price paths T={T}")
    if marginals and masses:
        raise ValueError("marginals=True and masses=True do not go together: the marginals are sums of the masses")
    if marginals and buffers.marg is None:
        buffers.marg = torch.empty((T + 1, n_cal, n_a), dtype=F64, device=dev)
    if masses and getattr(buffers, "masses", None) is None:
        buffers.masses = torch.empty((T + 1, n_cal, S, n_a), dtype=F64, device=dev)
    m_term = _tables(m_term, n_cal, S, n_a)
    c_term = _tables(c_term, n_cal, S, n_a)
    mass0 = _device(mass0, dev)
    transition_backward(batch, dR, dw, m_term, c_term, buffers, export_policy=export_policy, stream=stream)
    buffers.mass.copy_(mass0.reshape(n_cal, S, n_a))
    Ks, C = transition_forward(batch, buffers.lo, buffers.wlo, buffers.mass, T, buffers.work, dR, dw, want_c=want_c,
                               stream=stream, marg=buffers.marg if marginals else None,
                               mass_path=buffers.masses if masses else None)
    return BlockResult(Ks=Ks, C=C, lo=buffers.lo, wlo=buffers.wlo, m0=buffers.m0 if export_policy else None,
                       c0=buffers.c0 if export_policy else None, mass_T=buffers.mass,
                       marg=buffers.marg if marginals else None, masses=buffers.masses if masses else None)


def path_wealth_stats(batch, marg, percentiles=None):
    """Wealth statistics of every period of a path: ``marg`` [T+1][n_cal][n_a] (device, from
    ``household_block(marginals=True)``) on the grids of ``batch``.  Returns ``stats.WealthStats``
    of shape [n_cal][T+1]: the stack goes to ``stats.histogram_stats`` as it lies (period-major,
    distribution d on grid d % n_cal) and only the results are transposed, on the host."""
    n_cal, n_a = len(batch.cals), batch.n_a
    if marg.dim() != 3 or marg.shape[1] != n_cal or marg.shape[2] != n_a:
        raise ValueError(f"marg must be [T+1][n_cal={n_cal}][n_a={n_a}], got {tuple(marg.shape)}")
    ws = _stats.histogram_stats(marg, batch.d_a, percentiles, marginal=True)
    flip = lambda x: np.ascontiguousarray(np.swapaxes(x, 0, 1))   # noqa: E731
    return _stats.WealthStats(lorenz=flip(ws.lorenz), percentile_values=flip(ws.percentile_values),
                              gini=flip(ws.gini), mean=flip(ws.mean), total=flip(ws.total),
                              bottom_share=flip(ws.bottom_share), percentiles=ws.percentiles)


def path_variable_stats(batch, lo, wlo, R, w, masses, percentiles=None, variables=("consumption",)):
    """Statistics of household variables in every period of a path: the lotteries ``lo`` / ``wlo``
    [T][n_cal][S][n_a], the prices ``R``, ``w`` [n_cal][T+1] and the period masses ``masses``
    [T+1][n_cal][S][n_a] (device, from ``household_block(masses=True)``).  Returns ``(stats,
    moments)``: ``stats[name]`` a ``stats.VariableStats`` of shape [n_cal][T+1] for every sortable
    variable named, ``moments[name]`` a dict of mean, std and cv [n_cal][T+1] for every variable
    named (``saving`` gets moments only).  Period T has no lottery of its own: its consumption and
    saving take period T - 1's, with the prices of period T.  One variable is on the device at a time."""
    names = _stats._check_variables(variables)
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    dev = batch.device
    dR, dw = _device(R, dev), _device(w, dev)
    T = int(lo.shape[0])
    if tuple(masses.shape) != (T + 1, n_cal, S, n_a) or tuple(dR.shape) != (n_cal, T + 1) or dR.shape != dw.shape:
        raise ValueError(f"masses {tuple(masses.shape)} and prices {tuple(dR.shape)} do not fit T={T} lotteries")
    h = _lib.handle(dev.index)
    flip = lambda x: np.ascontiguousarray(np.swapaxes(x, 0, 1))   # noqa: E731
    val = torch.empty((T + 1, n_cal, S, n_a), dtype=F64, device=dev)
    work = _lib.work_space(dev, "var", "", n_dist=(T + 1) * n_cal, S=S, n_a=n_a)
    stats, moments = {}, {}
    for name in names:
        mask = _lib.AIY_VARIABLES[name]
        _stats._variables_into(batch, lo, wlo, _lib.ptr(dR), _lib.ptr(dw), T + 1, T, mask, val[:T])
        _stats._variables_into(batch, lo[T - 1], wlo[T - 1], dR.data_ptr() + 8 * T, dw.data_ptr() + 8 * T, T + 1, 1,
                               mask, val[T:])
        mom = _stats._moments(h, [val], masses, (T + 1) * n_cal, S, n_a, work)
        mean, std, cv, _ = _stats._dispersion(mom, 1)
        moments[name] = {k: flip(x.reshape(T + 1, n_cal)) for k, x in (("mean", mean), ("std", std), ("cv", cv))}
        if name in _stats._UNSORTABLE:
            continue
        vs = _stats.variable_stats(val, masses, percentiles)
        stats[name] = _stats.VariableStats(**{f.name: (vs.percentiles if f.name == "percentiles" else
                                                        flip(getattr(vs, f.name)))
                                              for f in dataclasses.fields(vs)})
    return stats, moments


@dataclass
class TransitionResult:
    K: np.ndarray            # [n_cal][T+1] capital path (K[:, 0] = sum mass0 a)
    r: np.ndarray            # [n_cal][T+1]
    w: np.ndarray            # [n_cal][T+1]
    C: np.ndarray            # [n_cal][T] aggregate consumption of the last evaluation
    iterations: np.ndarray   # [n_cal] block evaluations used
    residual: np.ndarray     # [n_cal] max_t |Ks_t - K_t| / K_0 of the last evaluation
    status: np.ndarray       # [n_cal] 0: converged; bit 1: stopped at max_iter
    stats: _stats.WealthStats | None = None   # [n_cal][T+1] wealth statistics of the path (percentiles=)
    welfare: object | None = None             # welfare.WelfareResult of the path against the steady state (welfare=True)
    cohorts: object | None = None             # mobility.CohortPaths of the wealth classes of mass0 (cohorts=)
    var_stats: dict | None = None             # name -> stats.VariableStats [n_cal][T+1] (variables=)
    var_moments: dict | None = None           # name -> dict(mean, std, cv) [n_cal][T+1] (variables=)


def solve_transition(batch, Z, T, damping=0.5, tol=1e-9, max_iter=100, mass0=None, m_term=None, c_term=None,
                     method="damped", jacobian=None, percentiles=None, welfare=False, cohorts=None, variables=None):
    """Equilibrium capital path of every calibration of ``batch`` after the TFP path Z
    ([T+1] or [n_cal][T+1], Z[T] = 1), from the distribution mass0 (default: batch.mass, the
    steady state) to the terminal policy (default: batch.last_tables).

    K starts at K[0] = sum mass0 a in every period; each iteration evaluates the household
    block on K's prices and moves K <- (1 - damping) K + damping Ks with K[0] held.  A
    calibration stops, and its path is no longer updated, once max_t |Ks_t - K_t| / K[0] < tol;
    one still running after max_iter evaluations gets status bit 1 (nothing is raised).

    method="newton" keeps the start, the stop test, the frozen calibrations and the status and
    replaces the update by K[1:] -= H^-1 (Ks[1:] - K[1:]), H the capital map of the household
    Jacobian at the steady state of ``batch`` (``jacobian``: a HouseholdJacobian of this batch
    and T to reuse, else one is built at r* = alpha K*^(alpha - 1) - delta, K* = sum batch.mass a).
    H is factorised once per calibration; ``damping`` is not used.

    ``percentiles`` (a list or array in (0, 1)): also ``TransitionResult.stats``, the
    ``path_wealth_stats`` of the solved path at these percentiles -- one more forward sweep, with
    marginals, from mass0 on the lotteries of the last evaluation (which solved every
    calibration at its final prices, the frozen ones included).

    ``welfare=True``: also ``TransitionResult.welfare``, the ``welfare.WelfareResult`` of living
    through the solved path from mass0 against staying at the steady state of ``batch``
    (DESIGN.md §4m): V_base = ``welfare.stationary_value(batch)``, V = ``welfare.path_value`` on
    the lotteries and prices of the last evaluation with V_base as the value from period T on.
    Nothing else of the result changes.

    ``cohorts`` (a tuple of percentiles in (0, 1), strictly ascending): also
    ``TransitionResult.cohorts``, the ``mobility.CohortPaths`` of the wealth classes of mass0
    between these percentiles (``mobility.wealth_classes``), swept from mass0 on the lotteries and
    prices of the last evaluation: every class's capital and consumption path
    and its mass by wealth class and income state.  Nothing else of the result changes.

    ``variables`` (names out of ``stats.VARIABLES``, with ``percentiles``): also
    ``TransitionResult.var_stats`` and ``.var_moments``, the ``path_variable_stats`` of the solved
    path -- one more forward sweep, keeping every period's mass, from mass0 on the
    lotteries of the last evaluation, exactly as ``percentiles`` alone does for wealth.  Period T
    has no lottery, so its consumption and saving take period T - 1's.  Without ``variables`` not
    one call more is made and both fields are None.  Nothing else of the result changes."""
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    T = int(T)
    if variables is not None:
        variables = _stats._check_variables(variables)
        if percentiles is None:
            raise ValueError("variables= needs percentiles=")
    if method not in ("damped", "newton"):
        raise ValueError(f"method must be 'damped' or 'newton', got {method!r}")
    if method == "damped" and jacobian is not None:
        raise ValueError("jacobian= is only used by method='newton'")
    if cohorts is not None:
        from . import mobility as _mobility
        cohorts = _mobility._check_class_percentiles(cohorts)
    Z = np.broadcast_to(np.asarray(Z, dtype=np.float64), (n_cal, T + 1))
    if m_term is None or c_term is None:
        if getattr(batch, "last_tables", None) is None:
            raise ValueError("no terminal policy: run steady_state / capital_supply first or pass m_term, c_term")
        m_term, c_term = batch.last_tables
    if mass0 is None:
        mass0 = batch.mass
    mass0 = _device(mass0, batch.device).reshape(n_cal, S, n_a).clone()
    K0 = np.sum(mass0.cpu().numpy() * batch.aGrid[:, None, :], axis=(1, 2))
    K = np.repeat(K0[:, None], T + 1, axis=1)
    newton = None
    if method == "newton":
        if jacobian is None:
            jacobian = household_jacobian(batch, steady_rate(batch), T, m_term=m_term, c_term=c_term)
        if jacobian.JR.shape != (n_cal, T, T + 1):
            raise ValueError(f"jacobian holds {jacobian.JR.shape}, the solve needs {(n_cal, T, T + 1)}")
        newton = jacobian.solver()
    buffers = TransitionBuffers(batch, T)
    active = np.ones(n_cal, dtype=bool)
    iterations = np.zeros(n_cal, dtype=np.int64)
    residual = np.full(n_cal, np.inf)
    C = np.zeros((n_cal, T))
    r, w = path_prices(K, Z, batch.alpha, batch.delta)
    for it in range(1, int(max_iter) + 1):
        rn, wn = path_prices(K, Z, batch.alpha, batch.delta)
        r[active], w[active] = rn[active], wn[active]
        out = household_block(batch, 1.0 + r, w, m_term, c_term, mass0, want_c=True, export_policy=False,
                              buffers=buffers)
        with np.errstate(invalid="ignore"):
            res = np.max(np.abs(out.Ks - K), axis=1) / K[:, 0]
        for c in np.flatnonzero(active):
            iterations[c] = it
            residual[c] = res[c]
            C[c] = out.C[c]
            if res[c] < tol:
                active[c] = False
            elif newton is not None:
                K[c, 1:] -= newton(c, out.Ks[c, 1:] - K[c, 1:])
            else:
                K[c, 1:] = (1.0 - damping) * K[c, 1:] + damping * out.Ks[c, 1:]
        if not active.any():
            break
    if active.any():   # the prices of the paths still moving when the loop ended
        rn, wn = path_prices(K, Z, batch.alpha, batch.delta)
        r[active], w[active] = rn[active], wn[active]
    status = np.where(active, 1, 0).astype(np.int32)
    path_stats = None
    if percentiles is not None:
        buffers.mass.copy_(mass0)
        marg = torch.empty((T + 1, n_cal, n_a), dtype=F64, device=batch.device)
        transition_forward(batch, buffers.lo, buffers.wlo, buffers.mass, T, buffers.work, want_c=False, marg=marg)
        path_stats = path_wealth_stats(batch, marg, percentiles)
    var_stats = var_moments = None
    if variables is not None:
        buffers.mass.copy_(mass0)
        masses = torch.empty((T + 1, n_cal, S, n_a), dtype=F64, device=batch.device)
        transition_forward(batch, buffers.lo, buffers.wlo, buffers.mass, T, buffers.work, want_c=False,
                           mass_path=masses)
        var_stats, var_moments = path_variable_stats(batch, buffers.lo, buffers.wlo, 1.0 + r, w, masses, percentiles,
                                                     variables)
    gains = None
    if welfare:
        from . import welfare as _welfare
        V_base = _welfare.stationary_value(batch)
        V = _welfare.path_value(batch, buffers.lo, buffers.wlo, 1.0 + r, w, V_base)
        gains = _welfare.welfare(batch, V, V_base, mass0)
    followed = None
    if cohorts is not None:
        edges = _mobility.wealth_classes(batch, cohorts, mass=mass0)
        followed = _mobility.cohort_forward(batch, buffers.lo, buffers.wlo,
                                            _mobility.cohorts_by_class(batch, edges, mass=mass0), T, edges, R=1.0 + r, w=w)
    return TransitionResult(K=K, r=r, w=w, C=C, iterations=iterations, residual=residual, status=status,
                            stats=path_stats, welfare=gains, cohorts=followed, var_stats=var_stats,
                            var_moments=var_moments)


def steady_rate(batch):
    """r* [n_cal]: the firm's rate at K* = sum batch.mass a."""
    K = np.sum(batch.mass.cpu().numpy() * batch.aGrid[:, None, :], axis=(1, 2))
    rs, _ = path_prices(K[:, None], np.ones((len(K), 1)), batch.alpha, batch.delta)
    return rs[:, 0]


def steady_lottery(batch, r=None, tables=None, lo=None, wlo=None):
    """The steady state's lottery and prices on device: ``(lo, wlo, R [n_cal], w [n_cal])`` by
    aiy_hist_lottery from ``tables`` (default ``batch.last_tables``) at the rate ``r`` (default
    ``steady_rate(batch)``), into ``lo`` / ``wlo`` [n_cal][S][n_a] where they are given."""
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    dev = batch.device
    if tables is None:
        if getattr(batch, "last_tables", None) is None:
            raise ValueError("no steady-state policy: run steady_state / capital_supply first")
        tables = batch.last_tables
    m, c = (_tables(t, n_cal, S, n_a) for t in tables)
    r = np.broadcast_to(np.asarray(steady_rate(batch) if r is None else r, dtype=np.float64), (n_cal,))
    w, _ = firm_prices(r, batch.alpha, batch.delta)
    dR, dw = _device(1.0 + r, dev), _device(w, dev)
    if lo is None:
        lo = torch.empty((n_cal, S, n_a), dtype=torch.int32, device=dev)
        wlo = torch.empty((n_cal, S, n_a), dtype=F64, device=dev)
    h = _lib.handle(dev.index)
    h.check(h.lib.aiy_hist_lottery(h.h, n_cal, S, n_a, _lib.ptr(m), _lib.ptr(c), _lib.ptr(batch.d_a), _lib.ptr(dR),
                                   _lib.ptr(dw), _lib.ptr(batch.d_lab), _lib.ptr(lo), _lib.ptr(wlo),
                                   _lib.stream_ptr()), "aiy_hist_lottery")
    return lo, wlo, dR, dw


# -------------------------------------------------------------------------------------
# Sequence-space Jacobian of the household block
# -------------------------------------------------------------------------------------
@dataclass
class HouseholdJacobian:
    JR: np.ndarray       # [n_cal][T][T+1]  d Ks[t+1] / d R_u
    Jw: np.ndarray       # [n_cal][T][T+1]  d Ks[t+1] / d w_u
    FR: np.ndarray       # [n_cal][T][T+1]  fake-news matrices F[t][s] = sum E_t dD_s
    Fw: np.ndarray
    h: float             # the step of the one-sided differences
    K: np.ndarray        # [n_cal] K* = sum D* a
    alpha: np.ndarray    # [n_cal]

    def capital_map(self):
        """H [n_cal][T][T] = J^R[:, 1:] R'(K*) + J^w[:, 1:] w'(K*) - I: the derivative of
        Ks[1:] - K[1:] with respect to K[1:] at the steady state (Z = 1; K[0] is given)."""
        T = self.JR.shape[1]
        a, K = self.alpha[:, None, None], self.K[:, None, None]
        dR = a * (a - 1.0) * K ** (a - 2.0)
        dw = a * (1.0 - a) * K ** (a - 1.0)
        return self.JR[:, :, 1:] * dR + self.Jw[:, :, 1:] * dw - np.eye(T)[None]

    def solver(self):
        """``solve(c, b) -> H_c^-1 b``; every H_c is LU-factorised once, on the host, one
        calibration at a time (a calibration's solve does not depend on the batch)."""
        H = self.capital_map()
        lu = [torch.linalg.lu_factor(torch.from_numpy(np.ascontiguousarray(H[c]))) for c in range(H.shape[0])]

        def solve(c, b):
            b = np.asarray(b, dtype=np.float64)
            x = torch.linalg.lu_solve(lu[c][0], lu[c][1], torch.from_numpy(np.ascontiguousarray(b)).reshape(-1, 1))
            return x.reshape(b.shape).numpy()
        return solve


def jacobian_from_fake_news(F):
    """J[..., t, u] = sum_{k = 0 .. min(t, u)} F[..., t - k, u - k]."""
    J = np.array(F, dtype=np.float64)
    for t in range(1, J.shape[-2]):
        J[..., t, 1:] += J[..., t - 1, :-1]
    return J


class JacobianBuffers:
    """Device buffers of one (batch, T) Jacobian.  At the Table II shape with T = 300 one
    [T+1][n_cal][S][n_a] array is 4 GB: the ghost steps and the two inputs' shocked steps are
    held at once (the differences are formed in place in the shocked ones, which are then the
    contraction's operands), E is a fourth, and the backward sweeps of the ghost and of both
    inputs share one set of lottery buffers (``TransitionBuffers`` of T + 1 periods)."""

    def __init__(self, batch: StationaryBatch, T: int):
        n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
        dev = batch.device
        self.T = int(T)
        self.work = _lib.work_space(dev, "jacobian", "Jacobian", n_cal=n_cal, S=S, n_a=n_a, T=self.T)
        self.sweep = TransitionBuffers(batch, self.T + 1)
        self.ghost = torch.empty((self.T + 1, n_cal, S, n_a), dtype=F64, device=dev)
        self.dD = [torch.empty_like(self.ghost), torch.empty_like(self.ghost)]   # R, w
        self.E = torch.empty((self.T, n_cal, S, n_a), dtype=F64, device=dev)
        self.lo = torch.empty((n_cal, S, n_a), dtype=torch.int32, device=dev)    # the steady lottery
        self.wlo = torch.empty((n_cal, S, n_a), dtype=F64, device=dev)
        self.F = torch.empty((n_cal, self.T, 2 * (self.T + 1)), dtype=F64, device=dev)


def jacobian_fanout(batch, lo, wlo, mass, out, work, T, stream=None):
    """aiy_jacobian_fanout: out[t] = lottery step of ``mass`` with (lo[t], wlo[t]) for every
    period of the device lottery [n_t][n_cal][S][n_a] (n_t <= T + 1, ``work`` sized for T).
    Raises AiyagariLibError (AIY_ERR_UNSUPPORTED) with ``out`` untouched when a row fails the
    monotone / range check."""
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    hd = _lib.handle(batch.device.index)
    hd.check(hd.lib.aiy_jacobian_fanout(hd.h, n_cal, S, n_a, int(T), int(lo.shape[0]), _lib.ptr(lo), _lib.ptr(wlo),
                                        _lib.ptr(batch.d_P), _lib.ptr(mass), _lib.ptr(work), _lib.ptr(out),
                                        _lib.stream_ptr(stream)), "aiy_jacobian_fanout")
    return out


def jacobian_expectation(batch, lo, wlo, E, work, stream=None):
    """aiy_jacobian_expectation: E[k] [T][n_cal][S][n_a] of the device lottery (lo, wlo)."""
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    hd = _lib.handle(batch.device.index)
    hd.check(hd.lib.aiy_jacobian_expectation(hd.h, n_cal, S, n_a, int(E.shape[0]), _lib.ptr(lo), _lib.ptr(wlo),
                                             _lib.ptr(batch.d_P), _lib.ptr(batch.d_a), _lib.ptr(work), _lib.ptr(E),
                                             _lib.stream_ptr(stream)), "aiy_jacobian_expectation")
    return E


def jacobian_contract(device, E, dD_R, dD_w, work, F=None, stream=None):
    """aiy_jacobian_contract: F [n_cal][T][2(T+1)] (device) of E [T][n_cal][S][n_a] and the two
    inputs' dD [T+1][n_cal][S][n_a]."""
    T, n_cal, S, n_a = E.shape
    hd = _lib.handle(device.index)
    if F is None:
        F = torch.empty((n_cal, T, 2 * (T + 1)), dtype=F64, device=E.device)
    hd.check(hd.lib.aiy_jacobian_contract(hd.h, n_cal, S, n_a, T, _lib.ptr(E), _lib.ptr(dD_R), _lib.ptr(dD_w),
                                          _lib.ptr(work), _lib.ptr(F), _lib.stream_ptr(stream)),
             "aiy_jacobian_contract")
    return F


def _shocked_backward(batch, Rs, w, T, h, shock, m_term, c_term, sweep):
    """One backward sweep of the Jacobians over T + 2 periods on the constant prices (Rs, w)
    [n_cal], with R[T] (shock "R") or w[T] (shock "w") moved by h, or neither (the ghost):
    fills the T + 1 lotteries of ``sweep`` (TransitionBuffers of T + 1 periods)."""
    R = np.repeat(Rs[:, None], T + 2, axis=1)
    W = np.repeat(np.asarray(w)[:, None], T + 2, axis=1)
    if shock == "R":
        R[:, T] += h
    elif shock == "w":
        W[:, T] += h
    dev = batch.device
    transition_backward(batch, torch.as_tensor(R).to(dev), torch.as_tensor(W).to(dev), m_term, c_term, sweep,
                        export_policy=False)


def household_jacobian(batch, r, T, h=1e-5, m_term=None, c_term=None, buffers=None, timings=None):
    """Sequence-space Jacobian of the household block of every calibration of ``batch`` at its
    steady state (interest rate ``r`` [n_cal], tables ``batch.last_tables``, mass ``batch.mass``)
    by the fake-news algorithm: J^x[t][u] = d Ks[t+1] / d x_u for x in {R, w}, t < T, u <= T.

    Three backward sweeps over T + 2 periods (a ghost on constant prices and one per input
    with x[T] += h), one fan-out lottery step of the steady mass per sweep, T - 1 expectation
    steps and one FP64 matrix-instruction contraction; the host only accumulates the fake-news
    matrices along their diagonals.  ``timings``: a dict that receives the milliseconds of
    every stage (each stage is then synchronised)."""
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    T = int(T)
    dev = batch.device
    if m_term is None or c_term is None:
        if getattr(batch, "last_tables", None) is None:
            raise ValueError("no steady-state policy: run steady_state / capital_supply first or pass m_term, c_term")
        m_term, c_term = batch.last_tables
    m_term = _tables(m_term, n_cal, S, n_a)
    c_term = _tables(c_term, n_cal, S, n_a)
    r = np.broadcast_to(np.asarray(r, dtype=np.float64), (n_cal,))
    w, _ = firm_prices(r, batch.alpha, batch.delta)
    Rs = 1.0 + r
    if buffers is None:
        buffers = JacobianBuffers(batch, T)
    elif buffers.T != T:
        raise ValueError(f"buffers hold T={buffers.T}, asked for T={T}")
    hd = _lib.handle(dev.index)
    mass = batch.mass.reshape(n_cal, S, n_a)
    t_last = [time.perf_counter()]

    def stage(name):
        if timings is not None:
            torch.cuda.synchronize(dev)
            now = time.perf_counter()
            timings[name] = timings.get(name, 0.0) + (now - t_last[0]) * 1e3
            t_last[0] = now

    def step_of_sweep(shock, out):
        _shocked_backward(batch, Rs, w, T, h, shock, m_term, c_term, buffers.sweep)
        stage("backward")
        jacobian_fanout(batch, buffers.sweep.lo, buffers.sweep.wlo, mass, out, buffers.work, T)
        stage("fanout")

    if timings is not None:
        torch.cuda.synchronize(dev)
        t_last[0] = time.perf_counter()
    step_of_sweep(None, buffers.ghost)
    for x, name in enumerate(("R", "w")):
        step_of_sweep(name, buffers.dD[x])
        hd.check(hd.lib.aiy_jacobian_diff(hd.h, buffers.ghost.numel(), _lib.ptr(buffers.dD[x]),
                                          _lib.ptr(buffers.ghost), float(h), _lib.stream_ptr()), "aiy_jacobian_diff")
        stage("diff")
    steady_lottery(batch, r, tables=(m_term, c_term), lo=buffers.lo, wlo=buffers.wlo)
    jacobian_expectation(batch, buffers.lo, buffers.wlo, buffers.E, buffers.work)
    stage("expectation")
    jacobian_contract(dev, buffers.E, buffers.dD[0], buffers.dD[1], buffers.work, F=buffers.F)
    stage("contraction")
    raw = buffers.F.cpu().numpy()
    # column c of an input is the lottery period c: the shock is s = T - c periods ahead
    FR = np.ascontiguousarray(raw[:, :, :T + 1][:, :, ::-1])
    Fw = np.ascontiguousarray(raw[:, :, T + 1:][:, :, ::-1])
    K = np.sum(mass.cpu().numpy() * batch.aGrid[:, None, :], axis=(1, 2))
    jac = HouseholdJacobian(JR=jacobian_from_fake_news(FR), Jw=jacobian_from_fake_news(Fw), FR=FR, Fw=Fw, h=float(h),
                            K=K, alpha=np.array(batch.alpha, dtype=np.float64))
    stage("host")
    return jac


def impulse_response(batch, jac, dZ):
    """Linear response (dK, dr, dw), each [n_cal][T+1], of the economy at the steady state of
    ``batch`` to the TFP path 1 + dZ (dZ [T+1] or [n_cal][T+1]): dK[0] = 0,
    dK[1:] = -H^-1 (J^R alpha K*^(alpha-1) + J^w (1 - alpha) K*^alpha) dZ, and the linearised
    firm's dr, dw."""
    n_cal, T = jac.JR.shape[0], jac.JR.shape[1]
    if n_cal != len(batch.cals):
        raise ValueError(f"jacobian holds {n_cal} calibrations, the batch {len(batch.cals)}")
    dZ = np.broadcast_to(np.asarray(dZ, dtype=np.float64), (n_cal, T + 1))
    solve = jac.solver()
    a, K = jac.alpha, jac.K
    rZ = a * K ** (a - 1.0)
    wZ = (1.0 - a) * K ** a
    dK = np.zeros((n_cal, T + 1))
    for c in range(n_cal):
        dK[c, 1:] = -solve(c, (jac.JR[c] * rZ[c] + jac.Jw[c] * wZ[c]) @ dZ[c])
    dr = rZ[:, None] * dZ + (a * (a - 1.0) * K ** (a - 2.0))[:, None] * dK
    dw = wZ[:, None] * dZ + (a * (1.0 - a) * K ** (a - 1.0))[:, None] * dK
    return dK, dr, dw
