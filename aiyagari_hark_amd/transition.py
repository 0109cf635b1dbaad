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

Everything per grid point runs in libaiyagari, batched over calibrations; the host only
prices the path and damps it.  Several GPUs: split the calibrations with
``parallel.split_calibrations`` and solve each share on its device -- the calibrations of
a batch never interact.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from . import setup_math as sm
from .stationary import StationaryBatch, _resolve_device, solve_table2

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


class TransitionBuffers:
    """Device buffers of one (batch, T): the lotteries, the work space and a mass scratch,
    allocated once and reused by every block evaluation of a solve."""

    def __init__(self, batch: StationaryBatch, T: int):
        n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
        h = _lib.handle(batch.device.index)
        nbytes = int(h.lib.aiy_transition_work_bytes(n_cal, S, n_a, int(T)))
        if nbytes < 0:
            raise ValueError(f"transition sizes not supported: n_cal={n_cal} S={S} n_a={n_a} T={T}")
        dev = batch.device
        self.T = int(T)
        self.work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.lo = torch.empty((self.T, n_cal, S, n_a), dtype=torch.int32, device=dev)
        self.wlo = torch.empty((self.T, n_cal, S, n_a), dtype=F64, device=dev)
        self.m0 = torch.empty((n_cal, S, n_a + 1), dtype=F64, device=dev)
        self.c0 = torch.empty((n_cal, S, n_a + 1), dtype=F64, device=dev)
        self.mass = torch.empty((n_cal, S, n_a), dtype=F64, device=dev)


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


def transition_forward(batch, lo, wlo, mass, T, work, R=None, w=None, want_c=True, stream=None):
    """aiy_transition_forward on device lotteries [T][n_cal][S][n_a]: advances ``mass`` in
    place from period 0 to period T and returns (Ks [n_cal][T+1], C [n_cal][T] or None).
    Raises AiyagariLibError (AIY_ERR_UNSUPPORTED) when a lottery row fails the monotone /
    range check; mass is then untouched."""
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    h = _lib.handle(batch.device.index)
    Ks = np.zeros((n_cal, T + 1))
    C = np.zeros((n_cal, T)) if want_c else None
    h.check(h.lib.aiy_transition_forward(h.h, n_cal, S, n_a, int(T), _lib.ptr(lo), _lib.ptr(wlo), _lib.ptr(batch.d_P),
                                         _lib.ptr(batch.d_a), _lib.ptr(R) if want_c else None,
                                         _lib.ptr(w) if want_c else None, _lib.ptr(batch.d_lab) if want_c else None,
                                         _lib.ptr(work), _lib.ptr(mass), Ks.ctypes.data_as(_lib.c_double_p),
                                         C.ctypes.data_as(_lib.c_double_p) if want_c else None,
                                         _lib.stream_ptr(stream)), "aiy_transition_forward")
    return Ks, C


def household_block(batch, R, w, m_term, c_term, mass0, want_c=True, export_policy=True, buffers=None, stream=None):
    """One household-block evaluation on the price paths R, w ([n_cal][T+1], NumPy or device):
    the backward sweep from the terminal policy (m_term, c_term), then the forward sweep from
    mass0 (left unchanged).  Returns BlockResult: Ks[n_cal][T+1], C[n_cal][T] and the device
    lotteries, period-0 policy and final mass (views of ``buffers``: the next evaluation with
    the same buffers overwrites them)."""
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    dev = batch.device
    dR = torch.as_tensor(np.ascontiguousarray(R, dtype=np.float64)).to(dev) if not torch.is_tensor(R) else R
    dw = torch.as_tensor(np.ascontiguousarray(w, dtype=np.float64)).to(dev) if not torch.is_tensor(w) else w
    if dR.shape != dw.shape or dR.dim() != 2 or dR.shape[0] != n_cal or dR.shape[1] < 2:
        raise ValueError(f"price paths must be [n_cal][T+1], got {tuple(dR.shape)} and {tuple(dw.shape)}")
    T = dR.shape[1] - 1
    if buffers is None:
        buffers = TransitionBuffers(batch, T)
    elif buffers.T != T:
        raise ValueError(f"buffers hold T={buffers.T}, the price paths T={T}")
    m_term = _tables(m_term, n_cal, S, n_a)
    c_term = _tables(c_term, n_cal, S, n_a)
    if not torch.is_tensor(mass0):
        mass0 = torch.as_tensor(np.ascontiguousarray(mass0, dtype=np.float64)).to(dev)
    transition_backward(batch, dR, dw, m_term, c_term, buffers, export_policy=export_policy, stream=stream)
    buffers.mass.copy_(mass0.reshape(n_cal, S, n_a))
    Ks, C = transition_forward(batch, buffers.lo, buffers.wlo, buffers.mass, T, buffers.work, dR, dw, want_c=want_c,
                               stream=stream)
    return BlockResult(Ks=Ks, C=C, lo=buffers.lo, wlo=buffers.wlo, m0=buffers.m0 if export_policy else None,
                       c0=buffers.c0 if export_policy else None, mass_T=buffers.mass)


@dataclass
class TransitionResult:
    K: np.ndarray            # [n_cal][T+1] capital path (K[:, 0] = sum mass0 a)
    r: np.ndarray            # [n_cal][T+1]
    w: np.ndarray            # [n_cal][T+1]
    C: np.ndarray            # [n_cal][T] aggregate consumption of the last evaluation
    iterations: np.ndarray   # [n_cal] block evaluations used
    residual: np.ndarray     # [n_cal] max_t |Ks_t - K_t| / K_0 of the last evaluation
    status: np.ndarray       # [n_cal] 0: converged; bit 1: stopped at max_iter


def solve_transition(batch, Z, T, damping=0.5, tol=1e-9, max_iter=100, mass0=None, m_term=None, c_term=None):
    """Equilibrium capital path of every calibration of ``batch`` after the TFP path Z
    ([T+1] or [n_cal][T+1], Z[T] = 1), from the distribution mass0 (default: batch.mass, the
    steady state) to the terminal policy (default: batch.last_tables).

    K starts at K[0] = sum mass0 a in every period; each iteration evaluates the household
    block on K's prices and moves K <- (1 - damping) K + damping Ks with K[0] held.  A
    calibration stops, and its path is no longer updated, once max_t |Ks_t - K_t| / K[0] < tol;
    one still running after max_iter evaluations gets status bit 1 (nothing is raised)."""
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    T = int(T)
    Z = np.broadcast_to(np.asarray(Z, dtype=np.float64), (n_cal, T + 1))
    if m_term is None or c_term is None:
        if getattr(batch, "last_tables", None) is None:
            raise ValueError("no terminal policy: run steady_state / capital_supply first or pass m_term, c_term")
        m_term, c_term = batch.last_tables
    if mass0 is None:
        mass0 = batch.mass
    if not torch.is_tensor(mass0):
        mass0 = torch.as_tensor(np.ascontiguousarray(mass0, dtype=np.float64)).to(batch.device)
    mass0 = mass0.reshape(n_cal, S, n_a).clone()
    K0 = np.sum(mass0.cpu().numpy() * batch.aGrid[:, None, :], axis=(1, 2))
    K = np.repeat(K0[:, None], T + 1, axis=1)
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
            else:
                K[c, 1:] = (1.0 - damping) * K[c, 1:] + damping * out.Ks[c, 1:]
        if not active.any():
            break
    if active.any():   # the prices of the paths still moving when the loop ended
        rn, wn = path_prices(K, Z, batch.alpha, batch.delta)
        r[active], w[active] = rn[active], wn[active]
    status = np.where(active, 1, 0).astype(np.int32)
    return TransitionResult(K=K, r=r, w=w, C=C, iterations=iterations, residual=residual, status=status)
