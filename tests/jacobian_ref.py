"""NumPy reference of the sequence-space Jacobian of the household block and of the Newton
solve built on it (test infrastructure only).

One calibration at a time, written solely in terms of oracle.stationary (``egm_step``,
``savings_lottery``, ``hist_step``, ``prices``) and tests/transition_ref.py (``block``,
``path_prices``).  ``ss`` is a steady state as ``transition_ref.cpu_steady_state`` returns it
(or the GPU's, as tests/test_gpu_transition.host_state builds it): aGrid, lab, P, beta, crra,
m, c, mass.

``fake_news``   steps 1-6: ghost and shocked backward sweeps over T + 2 periods, the
                distribution responses dD_s, the expectation vectors E_k, the fake-news
                matrix F[t][s] = sum E_t dD_s and J[t][u] = sum_k F[t - k][u - k] for both
                inputs x in {R, w};  J^x[t][u] = d Ks[t + 1] / d x_u, t < T, u <= T.
``brute``       the same Jacobian by one perturbed block evaluation per column.
``capital_map`` H = J^R[:, 1:] R'(K*) + J^w[:, 1:] w'(K*) - I.
``newton``      K[1:] -= H^-1 (Ks[1:] - K[1:]) with the start and the stop test of
                transition_ref.solve.
``impulse``     the linear response (dK, dr, dw) to a TFP path dZ[0..T].
"""
from __future__ import annotations

import numpy as np

from oracle import stationary as ST
from tests import transition_ref as TR


def steady_prices(ss, alpha, delta, r):
    """(R*, w*) of the steady state at r."""
    w, _ = ST.prices(r, alpha, delta)
    return 1.0 + r, w


def lotteries(ss, R, w):
    """Backward sweep on the paths R, w [n + 1] from (m*, c*): the lotteries of periods
    0 .. n - 1 (what aiy_transition_backward returns)."""
    n = len(R) - 1
    m, c = np.asarray(ss["m"]), np.asarray(ss["c"])
    out = [None] * n
    with np.errstate(all="ignore"):
        for u in range(n, 0, -1):
            m, c = ST.egm_step(m, c, ss["beta"], ss["crra"], ss["aGrid"], R[u], w[u], ss["lab"], ss["P"])
            lo, wlo, _ = ST.savings_lottery(m, c, ss["aGrid"], R[u - 1], w[u - 1], ss["lab"])
            out[u - 1] = (lo, wlo)
    return out


def expectation_step(E, lo, wlo, P):
    """E_{k+1}[s][j] = wlo G[s][lo] + (1 - wlo) G[s][lo + 1], G[s] = sum_{s'} P[s, s'] E_k[s']
    in ascending s': the transpose of hist_step."""
    S = P.shape[0]
    G = np.zeros_like(E)
    for s in range(S):
        for sp in range(S):
            G[s] += P[s, sp] * E[sp]
    return wlo * np.take_along_axis(G, lo, axis=1) + (1.0 - wlo) * np.take_along_axis(G, lo + 1, axis=1)


def expectation_vectors(ss, lo, wlo, n):
    """E_0 .. E_{n-1} [n][S][n_a] of the lottery (lo, wlo): E_0 = a."""
    S = ss["P"].shape[0]
    E = [np.broadcast_to(ss["aGrid"][None, :], (S, ss["aGrid"].size)).copy()]
    for _ in range(n - 1):
        E.append(expectation_step(E[-1], lo, wlo, ss["P"]))
    return np.stack(E)


def jacobian_from_fake_news(F):
    """J[t][u] = sum_{k = 0 .. min(t, u)} F[t - k][u - k]."""
    J = np.array(F, dtype=np.float64)
    for t in range(1, J.shape[0]):
        J[t, 1:] += J[t - 1, :-1]
    return J


def fake_news(ss, Rs, ws, T, h=1e-5):
    """dict(FR, Fw [T][T+1], JR, Jw [T][T+1], E [T][S][n_a], dD_R, dD_w [T+1][S][n_a])."""
    mass, P = np.asarray(ss["mass"]), ss["P"]
    R = np.full(T + 2, Rs)
    w = np.full(T + 2, ws)
    ghost = lotteries(ss, R, w)
    out = {}
    lo_s, wlo_s, _ = ST.savings_lottery(np.asarray(ss["m"]), np.asarray(ss["c"]), ss["aGrid"], Rs, ws, ss["lab"])
    E = expectation_vectors(ss, lo_s, wlo_s, T)
    out["E"] = E
    base = [ST.hist_step(mass, lo, wlo, P) for lo, wlo in ghost]
    for name in ("R", "w"):
        Rp, wp = R.copy(), w.copy()
        (Rp if name == "R" else wp)[T] += h
        shocked = lotteries(ss, Rp, wp)
        dD = np.stack([(ST.hist_step(mass, shocked[T - s][0], shocked[T - s][1], P) - base[T - s]) / h
                       for s in range(T + 1)])
        F = np.einsum("tsj,usj->tu", E, dD)
        out["dD_" + name] = dD
        out["F" + name] = F
        out["J" + name] = jacobian_from_fake_news(F)
    return out


def brute(ss, Rs, ws, T, h=1e-5):
    """(JR, Jw) [T][T+1] by finite differences of transition_ref.block: column u is
    (Ks(x_u + h)[1:] - Ks(x)[1:]) / h on the constant paths (R*, w*)."""
    R = np.full(T + 1, Rs)
    w = np.full(T + 1, ws)
    args = (ss["aGrid"], ss["lab"], ss["P"], ss["beta"], ss["crra"])
    with np.errstate(all="ignore"):
        base = TR.block(*args, R, w, ss["m"], ss["c"], ss["mass"])["Ks"]
        J = {}
        for name in ("R", "w"):
            Jx = np.empty((T, T + 1))
            for u in range(T + 1):
                Rp, wp = R.copy(), w.copy()
                (Rp if name == "R" else wp)[u] += h
                Jx[:, u] = (TR.block(*args, Rp, wp, ss["m"], ss["c"], ss["mass"])["Ks"][1:] - base[1:]) / h
            J[name] = Jx
    return J["R"], J["w"]


def capital_map(JR, Jw, K, alpha):
    """H [T][T]: d (Ks[1:] - K[1:]) / d K[1:] at the steady state (Z = 1)."""
    dR = alpha * (alpha - 1.0) * K ** (alpha - 2.0)
    dw = alpha * (1.0 - alpha) * K ** (alpha - 1.0)
    return JR[:, 1:] * dR + Jw[:, 1:] * dw - np.eye(JR.shape[0])


def newton(ss, alpha, delta, Z, T, H, tol=1e-9, max_iter=100, history=None):
    """transition_ref.solve with the quasi-Newton update in place of the damped one.
    history receives the residual of every evaluation."""
    mass0 = np.asarray(ss["mass"])
    K0 = float(np.sum(mass0 * ss["aGrid"][None, :]))
    K = np.full(T + 1, K0)
    status, res, it, out = 1, np.inf, 0, None
    for it in range(1, max_iter + 1):
        r, w = TR.path_prices(K, Z, alpha, delta)
        with np.errstate(all="ignore"):
            out = TR.block(ss["aGrid"], ss["lab"], ss["P"], ss["beta"], ss["crra"], 1.0 + r, w, ss["m"], ss["c"], mass0)
            res = float(np.max(np.abs(out["Ks"] - K)) / K[0])
        if history is not None:
            history.append(res)
        if res < tol:
            status = 0
            break
        K[1:] -= np.linalg.solve(H, out["Ks"][1:] - K[1:])
    r, w = TR.path_prices(K, Z, alpha, delta)
    return dict(K=K, r=r, w=w, C=out["C"], iterations=it, residual=res, status=status)


def impulse(JR, Jw, K, alpha, dZ):
    """(dK, dr, dw) [T+1] of the linearised economy after dZ[0..T]; dK[0] = 0."""
    dZ = np.asarray(dZ, dtype=np.float64)
    H = capital_map(JR, Jw, K, alpha)
    rZ = alpha * K ** (alpha - 1.0)
    wZ = (1.0 - alpha) * K ** alpha
    dK = np.zeros(dZ.size)
    dK[1:] = -np.linalg.solve(H, (JR * rZ + Jw * wZ) @ dZ)
    dr = rZ * dZ + alpha * (alpha - 1.0) * K ** (alpha - 2.0) * dK
    dw = wZ * dZ + alpha * (1.0 - alpha) * K ** (alpha - 1.0) * dK
    return dK, dr, dw
