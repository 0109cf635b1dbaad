"""Welfare on the histogram: values and consumption-equivalent gains.

The histogram of the stationary economy is a Markov chain on (s, a_j): a household at node
(s, j) of period t consumes

    c_t[s][j] = R_t a_j + w_t lab_s - (wlo a[lo] + (1 - wlo) a[lo + 1]),

moves to lo / lo + 1 with the Young lottery's weights and draws s' from P[s, .].  Its expected
discounted utility is therefore exactly

    V_t = u(c_t) + beta Lambda_t V_{t+1},    u(c) = log c (CRRA = 1), c^(1 - CRRA) / (1 - CRRA),

with Lambda_t the transpose of period t's forward step (``csrc/welfare.hip``).  This is the value
of the discretised economy, not an interpolated value of the continuous one; in exchange

    sum mass_0 V_0 = sum_{t<T} beta^t sum mass_t u(c_t) + beta^T sum mass_T V_T

holds to rounding on any path.

``stationary_value``  V* of the steady state of a batch (value iteration, ``aiy_value_stationary``)
``path_value``        V_0 (and every V_t) on the lotteries and prices of a transition path
``welfare``           mass-weighted welfare and consumption equivalents of V_new against V_base:
                      by node, by income state and behind the veil (``WelfareResult``)

``solve_transition(..., welfare=True)`` fills ``TransitionResult.welfare`` with the gains of the
solved path over staying at the steady state.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .transition import _device, steady_lottery  # noqa: F401  (steady_lottery: also imported from here)

F64 = torch.float64


def _work(batch):
    return _lib.work_space(batch.device, "value", "value", n_cal=len(batch.cals), S=batch.S, n_a=batch.n_a)


def path_value(batch, lo, wlo, R, w, V_term, keep_path=False, work=None, stream=None):
    """aiy_value_backward: V_0 [n_cal][S][n_a] (device) of households that live through the
    lotteries ``lo`` / ``wlo`` [T][n_cal][S][n_a] (device: a ``BlockResult``'s or
    ``TransitionBuffers``') at the prices R, w ([n_cal][T+1], NumPy or device; the last column
    is not read) and hold V_term from period T on.  ``keep_path=True`` returns
    ``(V_0, V_path [T][n_cal][S][n_a])``.  Asynchronous."""
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    dev = batch.device
    T = int(lo.shape[0])
    if tuple(lo.shape) != (T, n_cal, S, n_a) or tuple(wlo.shape) != (T, n_cal, S, n_a) or lo.dtype != torch.int32:
        raise ValueError(f"lo / wlo must be [T][n_cal][S][n_a] = [T]{(n_cal, S, n_a)} (int32 / float64), got "
                         f"{tuple(lo.shape)} and {tuple(wlo.shape)}")
    dR, dw = _device(R, dev), _device(w, dev)
    if tuple(dR.shape) != (n_cal, T + 1) or tuple(dw.shape) != (n_cal, T + 1):
        raise ValueError(f"price paths must be [n_cal][T+1] = {(n_cal, T + 1)}, got {tuple(dR.shape)} and "
                         f"{tuple(dw.shape)}")
    V_term = _device(V_term, dev).reshape(n_cal, S, n_a)
    if work is None:
        work = _work(batch)
    V0 = torch.empty((n_cal, S, n_a), dtype=F64, device=dev)
    V_path = torch.empty((T, n_cal, S, n_a), dtype=F64, device=dev) if keep_path else None
    h = _lib.handle(dev.index)
    h.check(h.lib.aiy_value_backward(h.h, n_cal, S, n_a, T, _lib.ptr(lo), _lib.ptr(wlo), _lib.ptr(batch.d_P),
                                     _lib.ptr(batch.d_a), _lib.ptr(dR), _lib.ptr(dw), _lib.ptr(batch.d_lab),
                                     _lib.ptr(batch.d_beta), _lib.ptr(batch.d_crra), _lib.ptr(V_term),
                                     _lib.ptr(work), _lib.ptr(V0), _lib.ptr(V_path), _lib.stream_ptr(stream)),
            "aiy_value_backward")
    return (V0, V_path) if keep_path else V0


def stationary_value(batch, r=None, tol=1e-10, max_iter=5000, chunk=0, info=None):
    """V* [n_cal][S][n_a] (device) of the steady state of ``batch``: the fixed point of
    V = u(c) + beta Lambda V on the steady lottery (``steady_lottery(batch, r)``), by
    aiy_value_stationary from V = u(c) / (1 - beta).  A calibration stops once
    max |V_new - V| <= tol (1 - beta) / beta max |V_new|, which bounds |V - V*| by tol max |V|;
    one still running after ``max_iter`` steps is reported, not raised: ``info`` (a dict)
    receives ``iterations`` and ``dist`` [n_cal]."""
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    dev = batch.device
    lo, wlo, dR, dw = steady_lottery(batch, r)
    work = _work(batch)
    # u(c): one period from a zero terminal value
    V = path_value(batch, lo[None], wlo[None], dR[:, None].repeat(1, 2).contiguous(),
                   dw[:, None].repeat(1, 2).contiguous(), torch.zeros((n_cal, S, n_a), dtype=F64, device=dev), work=work)
    V /= (1.0 - batch.d_beta)[:, None, None]
    beta = np.ascontiguousarray(batch.d_beta.cpu().numpy())
    iters = np.zeros(n_cal, dtype=np.int32)
    dist = np.zeros(n_cal)
    h = _lib.handle(dev.index)
    h.check(h.lib.aiy_value_stationary(h.h, n_cal, S, n_a, _lib.ptr(lo), _lib.ptr(wlo), _lib.ptr(batch.d_P),
                                       _lib.ptr(batch.d_a), _lib.ptr(dR), _lib.ptr(dw), _lib.ptr(batch.d_lab),
                                       _lib.ptr(batch.d_beta), _lib.ptr(batch.d_crra),
                                       beta.ctypes.data_as(_lib.c_double_p), float(tol), int(max_iter), int(chunk),
                                       _lib.ptr(V), _lib.ptr(work), iters.ctypes.data_as(_lib.c_int32_p),
                                       dist.ctypes.data_as(_lib.c_double_p), _lib.stream_ptr()),
            "aiy_value_stationary")
    if info is not None:
        info["iterations"] = iters
        info["dist"] = dist
    return V


def value_reduce(batch, mass, V):
    """aiy_value_reduce: W [n_cal][S] (NumPy) = sum_j mass[c][s][j] V[c][s][j].  Blocking."""
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    W = np.empty((n_cal, S))
    h = _lib.handle(batch.device.index)
    h.check(h.lib.aiy_value_reduce(h.h, n_cal, S, n_a, _lib.ptr(mass), _lib.ptr(V), W.ctypes.data_as(_lib.c_double_p),
                                   _lib.stream_ptr()), "aiy_value_reduce")
    return W


def consumption_equivalent(batch, V_new, V_base):
    """aiy_consumption_equivalent by node: g [n_cal][S][n_a] (device), the uniform proportional
    change of consumption that takes a household from V_base to V_new.  Asynchronous."""
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    g = torch.empty((n_cal, S, n_a), dtype=F64, device=batch.device)
    h = _lib.handle(batch.device.index)
    h.check(h.lib.aiy_consumption_equivalent(h.h, n_cal, S * n_a, _lib.ptr(V_new), _lib.ptr(V_base),
                                             _lib.ptr(batch.d_beta), _lib.ptr(batch.d_crra), _lib.ptr(g),
                                             _lib.stream_ptr()), "aiy_consumption_equivalent")
    return g


def ce_of_sums(W_new, W_base, share, beta, crra):
    """The two consumption-equivalent formulas on mass-weighted sums (NumPy, broadcasting):
    (W_new / W_base)^(1 / (1 - CRRA)) - 1, and exp((1 - beta)(W_new - W_base) / share) - 1 for
    CRRA = 1, ``share`` the mass the sums run over (it cancels in the ratio)."""
    W_new, W_base, share, beta, crra = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64)
                                                             for x in (W_new, W_base, share, beta, crra)))
    log = crra == 1.0
    with np.errstate(all="ignore"):
        g_log = np.exp((1.0 - beta) * (W_new - W_base) / share) - 1.0
        g_pow = (W_new / W_base) ** (1.0 / np.where(log, 2.0, 1.0 - crra)) - 1.0
    return np.where(log, g_log, g_pow)


@dataclass
class WelfareResult:
    V: torch.Tensor                # [n_cal][S][n_a] device: the value compared ...
    V_base: torch.Tensor           # ... and the value it is compared with
    ce: torch.Tensor               # [n_cal][S][n_a] device: consumption equivalent by node
    W: np.ndarray                  # [n_cal] sum mass V
    W_base: np.ndarray             # [n_cal] sum mass V_base
    W_by_state: np.ndarray         # [n_cal][S] sum_j mass V
    W_base_by_state: np.ndarray    # [n_cal][S]
    ce_aggregate: np.ndarray       # [n_cal] behind the veil: the formulas on W, W_base
    ce_by_state: np.ndarray        # [n_cal][S] conditional on the income state


def welfare(batch, V_new, V_base, mass):
    """Welfare of the households ``mass`` [n_cal][S][n_a] under V_new against V_base (device):
    ``WelfareResult`` with the consumption equivalent of every node and the same two formulas on
    the mass-weighted sums -- over everybody (the utilitarian gain behind the veil) and over
    each income state (the CRRA = 1 form divides by the state's share of ``mass``, which is the
    same under both values).  Raises ValueError when a sum is not finite: consumption c <= 0
    at some node made its value -inf or NaN."""
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    dev = batch.device
    V_new = _device(V_new, dev).reshape(n_cal, S, n_a)
    V_base = _device(V_base, dev).reshape(n_cal, S, n_a)
    mass = _device(mass, dev).reshape(n_cal, S, n_a)
    Ws = value_reduce(batch, mass, V_new)
    Wb = value_reduce(batch, mass, V_base)
    if not (np.all(np.isfinite(Ws)) and np.all(np.isfinite(Wb))):
        bad = sorted(set(np.flatnonzero(~(np.isfinite(Ws) & np.isfinite(Wb)).all(axis=1)).tolist()))
        raise ValueError(f"welfare is not finite for calibrations {bad}: consumption c <= 0 at some node of the path "
                         "(its utility, and every value that reaches it, is -inf or NaN)")
    share = value_reduce(batch, mass, torch.ones_like(mass))
    beta = batch.d_beta.cpu().numpy()
    crra = batch.d_crra.cpu().numpy()
    W, W_base = Ws.sum(axis=1), Wb.sum(axis=1)
    return WelfareResult(V=V_new, V_base=V_base, ce=consumption_equivalent(batch, V_new, V_base), W=W, W_base=W_base,
                         W_by_state=Ws, W_base_by_state=Wb,
                         ce_aggregate=ce_of_sums(W, W_base, share.sum(axis=1), beta, crra),
                         ce_by_state=ce_of_sums(Ws, Wb, share, beta[:, None], crra[:, None]))
