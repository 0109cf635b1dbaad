"""NumPy reference of the economy with aggregate risk to first order (test infrastructure only;
DESIGN.md §4p).

One calibration at a time, written solely in terms of oracle.stationary (``savings_lottery``,
``hist_step``), tests/transition_ref.py and tests/jacobian_ref.py (``lotteries``, ``fake_news``,
``impulse``).  ``ss`` is a steady state as ``transition_ref.cpu_steady_state`` returns it (or the
GPU's, as tests/test_gpu_transition.host_state builds it).

``policy_jacobian``  a* and dA_x[u] = d a'(s, a_j) / d x_u, the response of the savings policy
                     the histogram uses (the mean of the Young lottery) to a price u periods
                     ahead, from the ghost and shocked backward sweeps of ``jacobian_ref``.
``linear_model``     the unit-innovation responses dZ, dK, dr, dw [T+1] (``jacobian_ref.impulse``).
``expectations``     X[t][x][u] = E_t[dx_{t+u}] after the innovations eps[0..t], the realised
                     prices and the pure moving-average capital path K_lin.
``lotteries_of``     one period's policy a* + sum_k op[k] X[k], clamped to the grid, and its
                     lottery by ``savings_lottery``'s locate.
``simulate``         the histogram moved through the lotteries of every period.
``moments``          analytic covariances of (Z, K, r, w, Y) of the linear model.
``saving_rule``      least squares of log K' on (1, log K, Z - 1).
"""
from __future__ import annotations

import numpy as np

from oracle import stationary as ST
from tests import jacobian_ref as JR


def lottery_mean(lo, wlo, aGrid):
    """wlo a[lo] + (1 - wlo) a[lo + 1]: the savings a lottery stands for."""
    return wlo * aGrid[lo] + (1.0 - wlo) * aGrid[lo + 1]


def policy_jacobian(ss, Rs, ws, T, h=1e-5):
    """dict(a_star [S][n_a], dA_R, dA_w [T+1][S][n_a]): dA_x[u] = (mean of the lottery of period
    T - u of the sweep with x[T] += h, minus the ghost's) / h."""
    a = ss["aGrid"]
    R = np.full(T + 2, Rs)
    w = np.full(T + 2, ws)
    ghost = [lottery_mean(lo, wlo, a) for lo, wlo in JR.lotteries(ss, R, w)]
    lo_s, wlo_s, _ = ST.savings_lottery(np.asarray(ss["m"]), np.asarray(ss["c"]), a, Rs, ws, ss["lab"])
    out = dict(a_star=lottery_mean(lo_s, wlo_s, a))
    for name in ("R", "w"):
        Rp, wp = R.copy(), w.copy()
        (Rp if name == "R" else wp)[T] += h
        shocked = [lottery_mean(lo, wlo, a) for lo, wlo in JR.lotteries(ss, Rp, wp)]
        out["dA_" + name] = np.stack([(shocked[T - u] - ghost[T - u]) / h for u in range(T + 1)])
    return out


def ar1(rho, T):
    return rho ** np.arange(T + 1)


def linear_model(ss, JRm, Jwm, K, alpha, delta, irf_Z):
    """dict(dZ, dK, dr, dw [T+1] per unit innovation, K, r, w, alpha) at the capital K."""
    dZ = np.asarray(irf_Z, dtype=np.float64)
    dK, dr, dw = JR.impulse(JRm, Jwm, K, alpha, dZ)
    return dict(dZ=dZ, dK=dK, dr=dr, dw=dw, K=K, r=alpha * K ** (alpha - 1.0) - delta, w=(1.0 - alpha) * K ** alpha,
                alpha=alpha)


def expectations(model, eps):
    """dict(X [n][2][T+1], dr [n], dw [n], Z [n], K_lin [n+1]) by the definition, term by term:
    X[t][x][u] = sum_{k = 0 .. min(t, T - u)} dx[u + k] eps[t - k]."""
    eps = np.asarray(eps, dtype=np.float64)
    n, T = eps.size, model["dZ"].size - 1
    X = np.zeros((n, 2, T + 1))
    Z = np.ones(n)
    K_lin = np.full(n + 1, float(model["K"]))
    for t in range(n):
        for x, d in enumerate((model["dr"], model["dw"])):
            for u in range(T + 1):
                for k in range(min(t, T - u) + 1):
                    X[t, x, u] += d[u + k] * eps[t - k]
        for k in range(min(t, T) + 1):
            Z[t] += model["dZ"][k] * eps[t - k]
    for t in range(1, n + 1):
        for k in range(1, min(t, T) + 1):   # dK[0] = 0: capital is given when the innovation arrives
            K_lin[t] += model["dK"][k] * eps[t - k]
    return dict(X=X, dr=X[:, 0, 0].copy(), dw=X[:, 1, 0].copy(), Z=Z, K_lin=K_lin)


def lotteries_of(pol, Xt, aGrid):
    """(lo, wlo, a') of one period: a' = a* + sum_k op[k] Xt[k] in ascending k (op = dA_R then
    dA_w), clamped to the grid; lo, wlo by the expressions of oracle.stationary.savings_lottery."""
    op = np.concatenate([pol["dA_R"], pol["dA_w"]])
    xs = np.asarray(Xt, dtype=np.float64).ravel()
    acc = np.zeros_like(pol["a_star"])
    for k in range(op.shape[0]):
        acc = acc + op[k] * xs[k]
    a1 = np.clip(pol["a_star"] + acc, aGrid[0], aGrid[-1])
    nA = aGrid.size
    j = np.clip(np.searchsorted(aGrid, a1, side="right") - 1, 0, nA - 2)
    wl = np.clip((aGrid[j + 1] - a1) / (aGrid[j + 1] - aGrid[j]), 0.0, 1.0)
    return j, wl, a1


def simulate(ss, model, pol, eps, mass0=None):
    """dict(K [n+1], C [n], Z, r, w, K_lin, marg [n+1][n_a], mass, monotone, gap)."""
    a, lab, P = ss["aGrid"], ss["lab"], ss["P"]
    ex = expectations(model, eps)
    n = ex["Z"].size
    mass = np.array(ss["mass"] if mass0 is None else mass0, dtype=np.float64)
    K = np.empty(n + 1)
    C = np.empty(n)
    marg = np.empty((n + 1, a.size))
    K[0] = np.sum(mass * a[None, :])
    marg[0] = mass.sum(axis=0)
    mono = True
    for t in range(n):
        lo, wlo, _ = lotteries_of(pol, ex["X"][t], a)
        mono = mono and bool(np.all(np.diff(lo, axis=-1) >= 0))
        q = (1.0 + model["r"] + ex["dr"][t]) * a[None, :] + (model["w"] + ex["dw"][t]) * lab[:, None]
        C[t] = np.sum(mass * (q - lottery_mean(lo, wlo, a)))
        mass = ST.hist_step(mass, lo, wlo, P)
        K[t + 1] = np.sum(mass * a[None, :])
        marg[t + 1] = mass.sum(axis=0)
    return dict(K=K, C=C, Z=ex["Z"], r=model["r"] + ex["dr"], w=model["w"] + ex["dw"], K_lin=ex["K_lin"], marg=marg,
                mass=mass, monotone=mono, gap=float(np.max(np.abs(K - ex["K_lin"])) / model["K"]))


def moments(model, sigma, lags):
    """cov[k][i][j] = sigma^2 sum_s dX^i_s dX^j_{s+k} for k = 0 .. lags, i, j over (Z, K, r, w, Y)
    with dY = K^alpha dZ + alpha K^(alpha - 1) dK: the covariance of X^i_t and X^j_{t+k} of the
    moving averages of white noise with variance sigma^2."""
    al, K = model["alpha"], model["K"]
    dY = K ** al * model["dZ"] + al * K ** (al - 1.0) * model["dK"]
    D = np.stack([model["dZ"], model["dK"], model["dr"], model["dw"], dY])
    n = D.shape[1]
    out = np.zeros((lags + 1, 5, 5))
    for k in range(min(lags, n - 1) + 1):
        out[k] = sigma ** 2 * D[:, :n - k] @ D[:, k:].T
    return out


def saving_rule(K, Z, burn=0):
    """(intercept, slope on log K, coefficient on Z - 1, R^2) of log K[t+1] on (1, log K[t], Z[t] - 1),
    t = burn .. n - 1."""
    K, Z = np.asarray(K, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    n = Z.size
    y = np.log(K[burn + 1:n + 1])
    A = np.stack([np.ones(n - burn), np.log(K[burn:n]), Z[burn:n] - 1.0], axis=1)
    coef, *_ = np.linalg.lstsq(A, y, rcond=None)
    res = y - A @ coef
    tot = y - y.mean()
    r2 = 1.0 - float(res @ res) / float(tot @ tot) if float(tot @ tot) > 0 else 1.0
    return float(coef[0]), float(coef[1]), float(coef[2]), r2
