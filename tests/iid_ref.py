"""NumPy reference of the asset-grid distribution solve of an i.i.d.-income calibration
(csrc/hist_bicg.h, IID): with every row of P equal to pi, T x = pi (x) (M mu) for any x, where
mu[j] = sum_s x[s][j] and M = sum_s pi_s Push_s acts on the asset grid alone.
"""
import numpy as np

from oracle import stationary as ost


def rows_bit_identical(P):
    """The device's test: S >= 2 and every row of P equal to row 0 as 64-bit integers."""
    B = np.ascontiguousarray(P, dtype=np.float64).view(np.int64)
    return B.shape[0] >= 2 and bool(np.all(B == B[0]))


def setup(states, sigma, crra, method="tauchen", rho=0.0, n_a=300, r=0.03):
    """An economy at rate r: (P, lab, aGrid, EGM tables m and c, lottery lo and wlo)."""
    lab, P = ost.income_process(states, rho, sigma, method)
    aGrid = ost.make_stationary_grid(aCount=n_a)
    w, _ = ost.prices(r, 0.36, 0.08)
    m, c, _, _ = ost.egm_solve(0.96, crra, aGrid, 1.0 + r, w, lab, P, tol=1e-8)
    lo, wlo, _ = ost.savings_lottery(m, c, aGrid, 1.0 + r, w, lab)
    return dict(P=P, pi=P[0].copy(), lab=lab, aGrid=aGrid, m=m, c=c, lo=lo, wlo=wlo)


def m_step(mu, lo, wlo, pi):
    """M mu: state s pushes pi_s mu through its lottery; the states are summed, s ascending."""
    out = np.zeros(mu.size)
    for s in range(pi.size):
        T = np.zeros(mu.size)
        np.add.at(T, lo[s], wlo[s] * (pi[s] * mu))
        np.add.at(T, lo[s] + 1, (1.0 - wlo[s]) * (pi[s] * mu))
        out = out + T
    return out


def m_fixed_point(lo, wlo, pi, tol, max_iter=200000):
    """mu = M mu by the plain iteration under the scaled stopping rule
    max|M mu - mu| < tol / max(pi); returns (M mu, iterations)."""
    n = lo.shape[1]
    mu = np.full(n, 1.0 / n)
    for it in range(1, max_iter + 1):
        new = m_step(mu, lo, wlo, pi)
        d = np.max(np.abs(new - mu))
        mu = new
        if d < tol / np.max(pi):
            return mu, it
    return mu, max_iter
