"""Test-side references of one stationary EGM step (n_M = 1), plain NumPy, any S >= 1 and any CRRA.

``step64`` is the oracle's step itself: every operation in float64 and in the order the kernels
follow (csrc/common.h), so CRRA = 1 is compared with it bit for bit.  ``step_ld`` is the same
step in ``np.longdouble`` with the brackets of the float64 queries: the yardstick of the closed
power forms of CRRA 3 / 5 and of the device pow, whose last-ulp rounding NumPy's pow does not
share.  ``tile_spans`` says how many nodes of a next-period row the 64 queries of a tile span
(the kernel stages a 128-node window per row and tile), and ``dense_tables`` builds tables whose
tile 3 spans more than any window.
"""
import numpy as np

from oracle.stationary import egm_step as step64  # noqa: F401  (re-exported)
from oracle.hark_ks import BORROW_NODE

LD = np.longdouble
TILE = 64        # asset nodes per block (kTile)
WINDOW = 128     # nodes of a row staged per wave (kWin)


def queries(aGrid, R, w, lab):
    """The float64 queries m'[a, s'] = R a + w l(s') of a step."""
    return R * aGrid[:, None] + w * lab[None, :]


def brackets(x, q):
    """HARK LinearInterp's bracket index of the queries q in the row x."""
    return np.maximum(np.searchsorted(x[:-1], q), 1)


def step_ld(m_next, c_next, beta, rho, aGrid, R, w, lab, P):
    """oracle.stationary.egm_step in long double: the brackets of the float64 queries, then the
    queries, the interpolation, the powers and the expectation in long double; the result
    rounded to float64 at the end.  Tables [S][n_a + 1]; m_next None = the terminal c = m."""
    S, nA = P.shape[0], aGrid.size
    q64 = queries(aGrid, R, w, lab)
    a = aGrid.astype(LD)
    q = LD(R) * a[:, None] + LD(w) * lab.astype(LD)[None, :]
    rho_l = LD(rho)
    vP = np.empty((nA, S), dtype=LD)
    with np.errstate(all="ignore"):
        for sp in range(S):
            if m_next is None:
                c = q[:, sp]
            else:
                x, y = m_next[sp].astype(LD), c_next[sp].astype(LD)
                i = brackets(m_next[sp], q64[:, sp])
                al = (q[:, sp] - x[i - 1]) / (x[i] - x[i - 1])
                c = (LD(1) - al) * y[i - 1] + al * y[i]
                c[q64[:, sp] < m_next[sp][0]] = np.nan
            vP[:, sp] = c ** -rho_l
        E = LD(beta) * ((LD(R) * vP) @ P.astype(LD).T)
        cNow = E ** (LD(-1) / rho_l)
    mNow = a[:, None] + cNow
    m_out = np.empty((S, nA + 1))
    c_out = np.empty((S, nA + 1))
    m_out[:, 0] = BORROW_NODE
    c_out[:, 0] = BORROW_NODE
    m_out[:, 1:] = mNow.T.astype(np.float64)
    c_out[:, 1:] = cNow.T.astype(np.float64)
    return m_out, c_out


def tile_spans(m_next, aGrid, R, w, lab):
    """[S, tiles]: lb(last query) - lb(first query) of every (next-period row, 64-node tile),
    lb = searchsorted(x[:-1], q).  A tile's brackets fit a window only while this stays below
    WINDOW (less the nodes the window starts below the hint)."""
    S, nA = m_next.shape[0], aGrid.size
    q = queries(aGrid, R, w, lab)
    tiles = (nA + TILE - 1) // TILE
    out = np.empty((S, tiles), dtype=np.int64)
    for sp in range(S):
        lb = np.searchsorted(m_next[sp][:-1], q[:, sp])
        for t in range(tiles):
            out[sp, t] = lb[min(nA, (t + 1) * TILE) - 1] - lb[t * TILE]
    return out


def dense_tables(S, n_a, aGrid, R, w, lab, dense_tile=3, n_dense=300):
    """Synthetic next-period tables [S][n_a + 1] that defeat the window: in every row 300 nodes
    sit evenly spaced strictly inside the queries of tile 3 (asset nodes 192 ... 255), the other
    n_a - 300 are geomspace(0.01, 1.2 q_max), node 0 is the 1e-7 borrowing node; c is a smooth
    concave function of m."""
    assert n_a >= (dense_tile + 1) * TILE and n_a > n_dense
    q = queries(aGrid, R, w, lab)
    m = np.empty((S, n_a + 1))
    for sp in range(S):
        qs = q[:, sp]
        dense = np.linspace(qs[dense_tile * TILE], qs[(dense_tile + 1) * TILE - 1], n_dense + 2)[1:-1]
        rest = np.geomspace(0.01, 1.2 * qs.max(), n_a - n_dense)
        m[sp] = np.sort(np.concatenate(([BORROW_NODE], dense, rest)))
    c = 0.2 * m ** 0.8 + 0.05
    c[:, 0] = BORROW_NODE
    return m, c


def rel_gap(got, want):
    """max |got - want| / |want|."""
    return float(np.max(np.abs(got - want) / np.abs(want)))
