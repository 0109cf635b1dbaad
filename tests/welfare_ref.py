"""NumPy reference of the welfare recursion on the histogram (test infrastructure only).

One calibration at a time, plain loops over states.  The histogram is a Markov chain on
(s, a_j): at node (s, j) of a period with lottery (lo, wlo) and prices (R, w) a household consumes

    c[s][j] = R a_j + w lab_s - (wlo a[lo] + (1 - wlo) a[lo + 1]),

moves to lo / lo + 1 with weights wlo / 1 - wlo and draws s' from P[s, .], so

    V_t[s][j] = u(c_t[s][j]) + beta (wlo G_{t+1}[s][lo] + (1 - wlo) G_{t+1}[s][lo + 1]),
    G_{t+1}[s][d] = sum over s' ascending of P[s, s'] V_{t+1}[s'][d],
    u(c) = log c (CRRA = 1), c^(1 - CRRA) / (1 - CRRA) otherwise; c = 0: -inf, c < 0: NaN.

``flow_utility`` / ``backward_step`` / ``path_values``   the recursion
``steady_value_dense``   (I - beta Lambda) V = u by np.linalg.solve, Lambda the chain's matrix
``steady_value_iter``    the plain iteration with the relative stopping rule
``forward_discounted``   sum_{t<T} beta^t sum mass_t u(c_t) + beta^T sum mass_T V_T, the masses
                         advanced by oracle.stationary.hist_step
``ce_nodes`` / ``ce_sums``   the consumption-equivalent formulas
"""
from __future__ import annotations

import numpy as np

from oracle import stationary as ST


def consumption(aGrid, lab, R, w, lo, wlo):
    """c [S][n_a] of one period."""
    return (R * aGrid[None, :] + w * lab[:, None]) - (wlo * aGrid[lo] + (1.0 - wlo) * aGrid[lo + 1])


def utility(c, crra):
    with np.errstate(all="ignore"):
        u = np.log(c) if crra == 1.0 else c ** (1.0 - crra) / (1.0 - crra)
    u = np.where(c == 0.0, -np.inf, u)
    return np.where(c < 0.0, np.nan, u)


def flow_utility(aGrid, lab, R, w, lo, wlo, crra, scale=1.0):
    """u(scale c) of one period."""
    return utility(scale * consumption(aGrid, lab, R, w, lo, wlo), crra)


def mix(P, V):
    """G[s] = sum over s' ascending of P[s, s'] V[s']."""
    S = P.shape[0]
    G = np.zeros_like(V)
    for s in range(S):
        acc = np.zeros(V.shape[1])
        for sp in range(S):
            acc = acc + P[s, sp] * V[sp]
        G[s] = acc
    return G


def backward_step(V_next, u, lo, wlo, P, beta):
    """V of a period with flow utility u and lottery (lo, wlo) from next period's V."""
    G = mix(P, V_next)
    V = np.empty_like(V_next)
    for s in range(P.shape[0]):
        V[s] = u[s] + beta * (wlo[s] * G[s][lo[s]] + (1.0 - wlo[s]) * G[s][lo[s] + 1])
    return V


def path_values(V_term, lo, wlo, P, aGrid, lab, R, w, beta, crra, scale=1.0):
    """[V_0, ..., V_{T-1}] on lotteries [T][S][n_a] and prices R, w [T+1] (the last not read)."""
    T = lo.shape[0]
    V = [None] * T
    nxt = np.asarray(V_term, dtype=np.float64)
    for t in range(T - 1, -1, -1):
        nxt = backward_step(nxt, flow_utility(aGrid, lab, R[t], w[t], lo[t], wlo[t], crra, scale), lo[t], wlo[t], P,
                            beta)
        V[t] = nxt
    return V


def chain_matrix(lo, wlo, P):
    """Lambda [S n_a][S n_a]: (Lambda V)[s][j] = wlo G[s][lo] + (1 - wlo) G[s][lo + 1], G = P V."""
    S, nA = lo.shape
    L = np.zeros((S * nA, S * nA))
    for s in range(S):
        for j in range(nA):
            for sp in range(S):
                L[s * nA + j, sp * nA + lo[s, j]] += wlo[s, j] * P[s, sp]
                L[s * nA + j, sp * nA + lo[s, j] + 1] += (1.0 - wlo[s, j]) * P[s, sp]
    return L


def steady_value_dense(u, lo, wlo, P, beta):
    """V* = (I - beta Lambda)^-1 u."""
    S, nA = lo.shape
    L = chain_matrix(lo, wlo, P)
    return np.linalg.solve(np.eye(S * nA) - beta * L, u.reshape(-1)).reshape(S, nA)


def stop_threshold(tol, beta, vmax):
    return tol * (1.0 - beta) / beta * vmax


def steady_value_iter(u, lo, wlo, P, beta, tol=1e-10, max_iter=5000, V0=None):
    """The plain iteration from u / (1 - beta), stopped once
    max |V_new - V| <= tol (1 - beta) / beta max |V_new|.  Returns (V, iterations, last distance)."""
    V = u / (1.0 - beta) if V0 is None else np.array(V0, dtype=np.float64)
    d = np.inf
    for it in range(1, max_iter + 1):
        new = backward_step(V, u, lo, wlo, P, beta)
        d = float(np.max(np.abs(new - V)))
        V = new
        if not d > stop_threshold(tol, beta, float(np.max(np.abs(V)))):
            return V, it, d
    return V, max_iter, d


def forward_discounted(mass0, lo, wlo, P, aGrid, lab, R, w, beta, crra, V_T, scale=1.0):
    """sum_{t<T} beta^t sum mass_t u(c_t) + beta^T sum mass_T V_T; also returns mass_T."""
    mass = np.array(mass0, dtype=np.float64)
    total, disc = 0.0, 1.0
    for t in range(lo.shape[0]):
        total += disc * float(np.sum(mass * flow_utility(aGrid, lab, R[t], w[t], lo[t], wlo[t], crra, scale)))
        mass = ST.hist_step(mass, lo[t], wlo[t], P)
        disc *= beta
    return total + disc * float(np.sum(mass * V_T)), mass


def ce_nodes(V_new, V_base, beta, crra):
    """Consumption equivalent by node."""
    if crra == 1.0:
        return np.exp((1.0 - beta) * (V_new - V_base)) - 1.0
    return (V_new / V_base) ** (1.0 / (1.0 - crra)) - 1.0


def ce_sums(W_new, W_base, share, beta, crra):
    """The same formulas on mass-weighted sums over households of total mass ``share``."""
    if crra == 1.0:
        return np.exp((1.0 - beta) * (W_new - W_base) / share) - 1.0
    return (W_new / W_base) ** (1.0 / (1.0 - crra)) - 1.0
