"""Test-side reference of the stationary-distribution solve (aiy_hist_solve), plain NumPy.

The transition of one calibration is mass' = P^T push(mass) (oracle.stationary.hist_step): the
lottery (lo, wlo) pushes the mass of node j of state s onto nodes lo and lo + 1, then the income
chain mixes the states.  ``dense_T`` writes that map as the N x N matrix it is (N = S n_a,
column-stochastic), so every property a solve must have is read off a matrix: the residual of a
returned mass, the largest row sum that scales its sup norm, the exact stationary vector of one
dense solve.  Nothing here needs monotone rows.

The inputs are synthetic: the lottery of a linear saving rule a' = kappa_s a + b_s
(``rule_lottery``, with the oracle's arithmetic), in two families.  ``fast`` converges in 40-130
plain iterations, ``slow`` (a sticky income chain, kappa near 1) in thousands, which is where the
BiCGSTAB forms work.  Every calibration of a batch has its own lottery and its own P, so a
calibration that read a neighbour's inputs misses its reference.

``CASES`` names every batch the GPU tests use; tests/test_hist_ref.py pins the conditions they
rely on, on the CPU.
"""
from functools import lru_cache

import numpy as np

from oracle import stationary as ST

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
TOL = 1e-12
ITER_CAP = {"fast": 200, "slow": 6000}


def rule_lottery(S, aGrid, kappa, b):
    """Lottery of a' = kappa[s] a + b[s] onto aGrid with the arithmetic of
    oracle.stationary.savings_lottery: (lo[S, n_a] int64, wlo[S, n_a]).  Rows are monotone
    (kappa > 0); a' <= a_0 gives (0, 1.0), a' >= a_last gives (n_a - 2, 0.0)."""
    nA = aGrid.size
    lo = np.empty((S, nA), dtype=np.int64)
    wlo = np.empty((S, nA))
    for s in range(S):
        a1 = kappa[s] * aGrid + b[s]
        j = np.searchsorted(aGrid, a1, side="right") - 1
        j = np.clip(j, 0, nA - 2)
        wl = (aGrid[j + 1] - a1) / (aGrid[j + 1] - aGrid[j])
        lo[s] = j
        wlo[s] = np.clip(wl, 0.0, 1.0)
    return lo, wlo


def dense_T(lo, wlo, P):
    """The N x N matrix (N = S n_a, point (s, j) at s n_a + j) of mass' = P^T push(mass):
    column (s, j) holds P[s, s'] wlo at (s', lo) and P[s, s'] (1 - wlo) at (s', lo + 1)."""
    S, nA = lo.shape
    N = S * nA
    T = np.zeros((N, N))
    col = (np.arange(S)[:, None] * nA + np.arange(nA)[None, :])          # [s, j]
    cols = np.broadcast_to(col[None, :, :], (S, S, nA))                  # [s', s, j]
    rows = np.arange(S)[:, None, None] * nA + lo[None, :, :]
    Pt = P.T[:, :, None]                                                 # [s', s, 1] = P[s, s']
    np.add.at(T, (rows.ravel(), cols.ravel()), (Pt * wlo[None]).ravel())
    np.add.at(T, (rows.ravel() + 1, cols.ravel()), (Pt * (1.0 - wlo)[None]).ravel())
    return T


def stationary(T):
    """The exact stationary vector of T (sum 1): one dense solve of (T - I) pi = 0 with the last
    row replaced by ones."""
    N = T.shape[0]
    A = T - np.eye(N)
    A[-1, :] = 1.0
    rhs = np.zeros(N)
    rhs[-1] = 1.0
    return np.linalg.solve(A, rhs)


def csr(T):
    """The non-zeros of T row by row (row starts, columns, values in np.longdouble): what
    ``residuals`` sums.  Every row of a transition matrix built here has an entry or is skipped."""
    r, c = np.nonzero(T)
    rows, starts = np.unique(r, return_index=True)
    return rows, starts, c, T[r, c].astype(LD), T.shape[0]


def residuals(T, m):
    """(sum |T m - m|, max |T m - m|) with T m accumulated in np.longdouble.  T: the dense matrix
    or its ``csr``."""
    rows, starts, c, v, N = T if isinstance(T, tuple) else csr(T)
    x = np.asarray(m, dtype=np.float64).reshape(-1).astype(LD)
    Tm = np.zeros(N, dtype=LD)
    Tm[rows] = np.add.reduceat(v * x[c], starts)
    d = np.abs(Tm - x)
    return float(d.sum()), float(d.max())


def norm_inf(T):
    """The largest row sum of T (its entries are non-negative)."""
    return float(T.sum(axis=1).max())


def iterate(lo, wlo, P, tol=TOL, max_iter=100000, mass0=None):
    """The plain iterate: oracle.stationary.stationary_hist with hist_step_fast, unchanged.
    Returns (mass, iterations)."""
    mass, it, _ = ST.stationary_hist(lo, wlo, P, lo.shape[1], tol=tol, max_iter=max_iter, mass0=mass0,
                                     step=ST.hist_step_fast)
    return mass, it


# ------------------------------------------------------------------------------------------
# the two input families
# ------------------------------------------------------------------------------------------
def _cal_inputs(family, S, aGrid, seed, c, n_cal):
    """Inputs of calibration c of a batch: its numbers depend on (seed, c) and on the place of c
    in the batch (c = 0 the fastest rule, the last one the slowest), not on its neighbours."""
    rng = np.random.default_rng([seed, c])
    f = c / max(n_cal - 1, 1)                   # 0 .. 1 along the batch
    if family == "fast":
        P = rng.random((S, S)) + 0.05
        P /= P.sum(axis=1, keepdims=True)
        # kappa within 0.55 .. 0.97, slower along the batch
        kappa = rng.uniform(0.55 + 0.30 * f, 0.70 + 0.22 * f, S)
        b = np.sort(rng.uniform(-6.0, 9.0, S))
        if S >= 2:
            # state 0 dissaves onto the constraint, the last state saves past the top of the grid
            b[0] = -rng.uniform(1.0, 6.0)
            kappa[-1], b[-1] = 0.97, 9.0
        elif c % 2:
            # one state cannot do both (kappa < 1): the odd calibrations of a one-state batch sit
            # on the constraint, the even ones at the top
            kappa[0], b[0] = rng.uniform(0.90, 0.97), -rng.uniform(0.5, 1.5)
        else:
            kappa[0], b[0] = 0.97, 9.0 - 3.0 * f
    elif family == "slow":
        stay = 0.98 + 0.015 * f
        Q = rng.random((S, S)) + 0.05
        Q /= Q.sum(axis=1, keepdims=True)
        P = stay * np.eye(S) + (1.0 - stay) * Q
        kappa = rng.uniform(0.97, 0.975 + 0.02 * f, S)
        b = np.sort(rng.uniform(-0.6, 0.5, S))
        b[0] = -0.6
        kappa[-1], b[-1] = 0.995, 0.5
    else:
        raise ValueError(family)
    lo, wlo = rule_lottery(S, aGrid, kappa, b)
    return lo, wlo, P


def make_batch(family, S, n_a, n_cal, seed):
    """(aGrid[n_a], lo[n_cal, S, n_a] int64, wlo, P[n_cal, S, S]) of one batch."""
    aGrid = ST.make_stationary_grid(0.001, 50.0, n_a, 2)
    parts = [_cal_inputs(family, S, aGrid, seed, c, n_cal) for c in range(n_cal)]
    lo, wlo, P = (np.stack([p[k] for p in parts]) for k in range(3))
    return aGrid, lo, wlo, P


# name -> (family, S, n_a, calibrations, seed).  Dense cases stay at N = S n_a <= 4200.
CASES = {
    # push/mix and fused step: tiles of 256 destinations, SMAX 8 / 16 / 32 / 64
    "f1x255": ("fast", 1, 255, 4, 1),
    "f2x2": ("fast", 2, 2, 3, 302),
    "f7x256": ("fast", 7, 256, 3, 3),
    "f7x257": ("fast", 7, 257, 3, 4),
    "f8x256": ("fast", 8, 256, 3, 5),
    "f9x257": ("fast", 9, 257, 3, 6),
    "f16x257": ("fast", 16, 257, 3, 107),
    "f17x120": ("fast", 17, 120, 3, 208),
    "f32x100": ("fast", 32, 100, 3, 9),
    "f33x100": ("fast", 33, 100, 3, 110),
    "f64x64": ("fast", 64, 64, 3, 11),
    # cluster forms: 512-thread workgroups, one or two columns per thread
    "f1x1024": ("fast", 1, 1024, 4, 12),
    "f4x1024": ("fast", 4, 1024, 3, 244),
    "f2x1025": ("fast", 2, 1025, 3, 13),
    "f3x200": ("fast", 3, 200, 3, 14),
    "f8x512": ("fast", 8, 512, 3, 115),
    "f8x513": ("fast", 8, 513, 3, 16),
    "f6x513": ("fast", 6, 513, 3, 717),
    "f7x300": ("fast", 7, 300, 3, 18),
    "f7x520": ("fast", 7, 520, 3, 19),
    # many-state pull form: groups of kHpGrp = 5 states, full and ragged
    "f9x200": ("fast", 9, 200, 3, 20),
    "f10x150": ("fast", 10, 150, 3, 21),
    "f11x130": ("fast", 11, 130, 3, 22),
    "f15x100": ("fast", 15, 100, 3, 23),
    "f16x200": ("fast", 16, 200, 3, 24),
    "f25x100": ("fast", 25, 100, 3, 25),
    "f26x100": ("fast", 26, 100, 3, 26),
    # slow family
    "s7x300": ("slow", 7, 300, 3, 131),
    "s3x600": ("slow", 3, 600, 3, 32),
    "s12x150": ("slow", 12, 150, 3, 33),
    # more calibrations than one launch holds (the GPU test takes multi_processor_count + 3 of
    # them; the CPU test checks this many)
    "t2x16": ("fast", 2, 16, 259, 41),
    "t3x16": ("fast", 3, 16, 259, 42),
    "t9x16": ("fast", 9, 16, 259, 43),
}


@lru_cache(maxsize=None)
def batch(name, n_cal=None):
    family, S, n_a, nc, seed = CASES[name]
    return make_batch(family, S, n_a, nc if n_cal is None else n_cal, seed)


@lru_cache(maxsize=None)
def plain(name, n_cal=None):
    """The plain iterates of a batch from the uniform start: (mass[n_cal, S, n_a], iters[n_cal])."""
    _, lo, wlo, P = batch(name, n_cal)
    out = [iterate(lo[c], wlo[c], P[c]) for c in range(lo.shape[0])]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out])


def residual_bounds(N, ninf, tol=TOL, total=1.0):
    """Bounds on (sum |T m - m|, max |T m - m|) of a returned mass of the given total.  A plain
    iterate returns m' = T m with max|m' - m| < tol, a BiCGSTAB form T x with max|T x - x| < tol:
    the residual of the returned vector is T applied to a vector of sup norm < tol, so its 1-norm
    is below N tol (T has 1-norm 1) and its sup norm below norm_inf(T) tol.  Both carry 16 eps
    times the largest row sum per unit of mass for the rounding of the matvec itself."""
    allow = 16.0 * EPS * ninf * total
    return N * tol * total + allow, ninf * tol * total + allow
