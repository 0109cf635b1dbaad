"""NumPy model of the cohort sweep and of the class rule, independent of the
package: the sweep is oracle.stationary.hist_step chained cohort by cohort, with plain NumPy
sums for the classes and the states.  tests/test_mobility_ref.py pins it against a dense chain;
tests/test_gpu_cohort.py holds the device to it."""
import numpy as np

from oracle import stationary as ST


def class_edges(g, p):
    """int [len(p) + 2]: with F = cumsum(g) / sum(g) and F_prev = (0, F[:-1]) a node belongs to the
    class in which its first household falls: inner edges searchsorted(F_prev, p, 'left')."""
    g = np.asarray(g, dtype=np.float64)
    F = np.cumsum(g) / np.sum(g)
    F_prev = np.concatenate(([0.0], F[:-1]))
    return np.concatenate(([0], np.searchsorted(F_prev, np.asarray(p, dtype=np.float64), side="left"),
                           [g.size])).astype(np.int64)


def wealth_classes(mass, p):
    """[n_cal][Q+1] of masses [n_cal][S][n_a]."""
    return np.stack([class_edges(m.sum(axis=0), p) for m in mass])


def split_by_class(mass, edges):
    """[Q][S][n_a] of one calibration's mass [S][n_a]: cohort q keeps the nodes of class q."""
    Q = len(edges) - 1
    out = np.zeros((Q,) + mass.shape)
    for q in range(Q):
        out[q][:, edges[q]:edges[q + 1]] = mass[:, edges[q]:edges[q + 1]]
    return out


def split_by_state(mass):
    S = mass.shape[0]
    out = np.zeros((S,) + mass.shape)
    for s in range(S):
        out[s, s] = mass[s]
    return out


def class_sums(mass, edges):
    return np.array([mass[:, edges[q]:edges[q + 1]].sum() for q in range(len(edges) - 1)])


def sweep(cohort, lo, wlo, P, T, edges, aGrid):
    """One cohort [S][n_a] of one calibration through T periods of the lottery lo / wlo
    [n_lot][S][n_a] (n_lot 1 or T).  Returns (K [T+1], occ [T+1][Q], inc [T+1][S], mass_T)."""
    n_lot = lo.shape[0]
    assert n_lot in (1, T)
    m = np.array(cohort, dtype=np.float64)
    K, occ, inc = [], [], []
    for t in range(T + 1):
        K.append(np.sum(m * aGrid[None, :]))
        occ.append(class_sums(m, edges))
        inc.append(m.sum(axis=1))
        if t < T:
            tl = 0 if n_lot == 1 else t
            m = ST.hist_step(m, lo[tl], wlo[tl], P)
    return np.array(K), np.array(occ), np.array(inc), m


def mobility_matrix(mass, lo, wlo, P, p, horizons, aGrid, by="wealth"):
    """(shares [G], matrix [H][G][Q], edges) of one calibration at the lottery lo / wlo [S][n_a]."""
    edges = class_edges(mass.sum(axis=0), p)
    cohorts = split_by_class(mass, edges) if by == "wealth" else split_by_state(mass)
    hmax = max(horizons)
    shares = np.array([c.sum() for c in cohorts])
    matrix = np.full((len(horizons), len(cohorts), len(edges) - 1), np.nan)
    for g, c in enumerate(cohorts):
        _, occ, _, _ = sweep(c, lo[None], wlo[None], P, hmax, edges, aGrid)
        if shares[g] > 0:
            matrix[:, g, :] = occ[list(horizons)] / shares[g]
    return shares, matrix, edges


def dense_chain(lo, wlo, P):
    """M [(S n_a)][(S n_a)] with mass'.ravel() = mass.ravel() @ M for the lottery lo / wlo [S][n_a]."""
    S, n_a = lo.shape
    M = np.zeros((S * n_a, S * n_a))
    for s in range(S):
        for j in range(n_a):
            for sp in range(S):
                M[s * n_a + j, sp * n_a + lo[s, j]] += P[s, sp] * wlo[s, j]
                M[s * n_a + j, sp * n_a + lo[s, j] + 1] += P[s, sp] * (1.0 - wlo[s, j])
    return M
