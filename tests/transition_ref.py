"""NumPy reference of the perfect-foresight transition path (test infrastructure only).

One calibration at a time, written solely in terms of oracle.stationary's ``egm_step``,
``savings_lottery``, ``hist_step`` and ``prices``:

``block``  household block on price paths R[0..T], w[0..T]:
    backward  (m_{u-1}, c_{u-1}) = egm_step(m_u, c_u, ..., R_u, w_u, ...),  u = T .. 1
    lottery   (lo_t, wlo_t, a'_t) = savings_lottery(m_t, c_t, aGrid, R_t, w_t, lab), t < T
    forward   mass_{t+1} = hist_step(mass_t, lo_t, wlo_t, P),
              Ks[t] = sum mass_t a,  C[t] = sum mass_t (q_t - a'_t),  q = R_t a + w_t lab_s
``solve``  damped fixed point on K with K[0] = Ks[0] held:
    K <- (1 - damping) K + damping Ks  until  max_t |Ks_t - K_t| / K[0] < tol.

Prices on a path are r_t = Z_t alpha K_t^(alpha - 1) - delta, w_t = Z_t (1 - alpha) K_t^alpha
(L = 1); at Z = 1 that is ``oracle.stationary.prices`` read backwards (K = K_demand(r)),
which ``path_prices`` asserts on its last period.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import stationary as ST


def shock_path(T, size=0.01, decay=0.8):
    """Z_t = 1 + size decay^t for t < T, Z_T = 1."""
    Z = 1.0 + size * decay ** np.arange(T + 1)
    Z[T] = 1.0
    return Z


def path_prices(K, Z, alpha, delta):
    """(r, w) on the capital path K [T+1] and TFP path Z [T+1] (libm pow, element by element)."""
    K = np.asarray(K, dtype=np.float64)
    r = np.empty(K.shape)
    w = np.empty(K.shape)
    for t in range(K.size):
        r[t] = Z[t] * alpha * math.pow(K[t], alpha - 1.0) - delta
        w[t] = Z[t] * (1.0 - alpha) * math.pow(K[t], alpha)
    if Z[-1] == 1.0 and np.isfinite(K[-1]) and K[-1] > 0 and r[-1] + delta > 0:
        w_ss, K_ss = ST.prices(r[-1], alpha, delta)   # the steady-state firm, read backwards
        assert abs(K_ss - K[-1]) <= 1e-10 * K[-1] and abs(w_ss - w[-1]) <= 1e-10 * w[-1]
    return r, w


def block(aGrid, lab, P, beta, crra, R, w, m_term, c_term, mass0, keep=False):
    """Household block of one calibration.  Returns dict(Ks[T+1], C[T], lo[T][S][n_a],
    wlo, ap (the unclipped savings a'_t), m0, c0, mass_T; keep=True also m[t], c[t], mass[t])."""
    T = len(R) - 1
    m = [None] * (T + 1)
    c = [None] * (T + 1)
    m[T], c[T] = np.asarray(m_term), np.asarray(c_term)
    for u in range(T, 0, -1):
        m[u - 1], c[u - 1] = ST.egm_step(m[u], c[u], beta, crra, aGrid, R[u], w[u], lab, P)
    S, nA = mass0.shape
    lo = np.empty((T, S, nA), dtype=np.int64)
    wlo = np.empty((T, S, nA))
    ap = np.empty((T, S, nA))
    for t in range(T):
        lo[t], wlo[t], ap[t] = ST.savings_lottery(m[t], c[t], aGrid, R[t], w[t], lab)
    mass = np.array(mass0, dtype=np.float64)
    masses = [mass]
    Ks = np.empty(T + 1)
    C = np.empty(T)
    Ks[0] = np.sum(mass * aGrid[None, :])
    for t in range(T):
        q = R[t] * aGrid[None, :] + w[t] * lab[:, None]
        C[t] = np.sum(mass * (q - ap[t]))
        mass = ST.hist_step(mass, lo[t], wlo[t], P)
        Ks[t + 1] = np.sum(mass * aGrid[None, :])
        if keep:
            masses.append(mass)
    out = dict(Ks=Ks, C=C, lo=lo, wlo=wlo, ap=ap, m0=m[0], c0=c[0], mass_T=mass)
    if keep:
        out.update(m=m, c=c, mass=masses)
    return out


def solve(aGrid, lab, P, beta, crra, alpha, delta, Z, T, m_term, c_term, mass0, damping=0.5, tol=1e-9, max_iter=100,
          history=None):
    """Equilibrium path of one calibration.  Returns dict(K, r, w, C, iterations, residual,
    status, lo) -- status 1 when max_iter evaluations ran without meeting tol.  history: a list
    that receives a copy of K before every evaluation."""
    K0 = float(np.sum(mass0 * aGrid[None, :]))
    K = np.full(T + 1, K0)
    status, res, it, out = 1, np.inf, 0, None
    r, w = path_prices(K, Z, alpha, delta)
    for it in range(1, max_iter + 1):
        r, w = path_prices(K, Z, alpha, delta)
        if history is not None:
            history.append(K.copy())
        with np.errstate(all="ignore"):
            out = block(aGrid, lab, P, beta, crra, 1.0 + r, w, m_term, c_term, mass0)
            res = float(np.max(np.abs(out["Ks"] - K)) / K[0])
        if res < tol:
            status = 0
            break
        K[1:] = (1.0 - damping) * K[1:] + damping * out["Ks"][1:]
    if status:
        r, w = path_prices(K, Z, alpha, delta)
    return dict(K=K, r=r, w=w, C=out["C"], iterations=it, residual=res, status=status, lo=out["lo"])


def monotone(lo):
    """Every lottery row non-decreasing in the asset node."""
    return bool(np.all(np.diff(lo, axis=-1) >= 0))


def cpu_steady_state(labor_ar, labor_sd, crra, n_a, n_states=7, method="tauchen", beta=0.96, alpha=0.36, delta=0.08,
                     r_tol=1e-7):
    """CPU steady state of one calibration (oracle ge_bisect, then one capital_supply at r*):
    dict(aGrid, lab, P, beta, crra, alpha, delta, r, K, m, c, mass)."""
    aGrid = ST.make_stationary_grid(0.001, 50.0, n_a, 2)
    lab, P = ST.income_process(n_states, labor_ar, labor_sd, method)
    cal = dict(CapShare=alpha, DeprFac=delta, DiscFac=beta, CRRA=crra)
    ge = ST.ge_bisect(cal, aGrid, lab, P, r_tol=r_tol, fast=True)
    K, info = ST.capital_supply(ge["r"], cal, aGrid, lab, P, fast=True)
    return dict(aGrid=aGrid, lab=lab, P=P, beta=beta, crra=crra, alpha=alpha, delta=delta, r=ge["r"], K=K,
                m=info["m"], c=info["c"], mass=info["mass"])
