"""NumPy model of the forward step for lotteries whose rows are not monotone:
the two window arrays of a row and the windowed pull, written the way the device does them.

For a row L of n_a entries in [0, n_a - 2], with the prefix maximum M[j] = max L[0..j] and the
suffix minimum m[j] = min L[j..] (both non-decreasing in j),

    jlo[d] = first j with M[j] >= d,    jhi[d] = first j with m[j] > d,    d = 0 .. n_a

(n_a where there is none), so every source with L[j] == d lies in [jlo[d], jhi[d]).  On a sorted
row these are the inverse index jb[d] and jb[d + 1] of the monotone sweep."""
import numpy as np

CAP_FACTOR = 4   # a row is refused when its windows hold more than CAP_FACTOR (n_a + 1) sources


def windows(L):
    """(jlo, jhi), each [n_a + 1] int64, of one row."""
    L = np.asarray(L, dtype=np.int64)
    n = L.shape[0]
    if L.min() < 0 or L.max() > n - 2:
        raise ValueError("row leaves [0, n_a - 2]")
    d = np.arange(n + 1)
    M = np.maximum.accumulate(L)
    m = np.minimum.accumulate(L[::-1])[::-1]
    jlo = np.searchsorted(M, d, side="left")    # first j with M[j] >= d
    jhi = np.searchsorted(m, d, side="right")   # first j with m[j] > d
    jhi[n] = n
    return jlo, jhi


def inverse_index(L):
    """jb[d] = first j with L[j] >= d of a sorted row, d = 0 .. n_a (tr_range_kernel's array)."""
    L = np.asarray(L, dtype=np.int64)
    return np.searchsorted(L, np.arange(L.shape[0] + 1), side="left")


def window_sum(L):
    """sum over d of jhi[d] - jlo[d]: the sources the pull of this row visits."""
    jlo, jhi = windows(L)
    return int(np.sum(jhi - jlo))


def window_ratio(L):
    """window_sum / n_a: 1 on a sorted row."""
    return window_sum(L) / float(np.asarray(L).shape[0])


def within_cap(L):
    return window_sum(L) <= CAP_FACTOR * (np.asarray(L).shape[0] + 1)


def is_turned(L):
    """True when the row has at least one decreasing neighbouring pair."""
    L = np.asarray(L)
    return bool(np.any(L[1:] < L[:-1]))


def rows_turned(lo):
    """Number of rows (last axis) of a lottery with at least one decreasing pair."""
    lo = np.asarray(lo)
    return int(np.sum(np.any(lo[..., 1:] < lo[..., :-1], axis=-1)))


def pull_row(L, wl, q):
    """T[d] of one row by the windowed pull: for every column d the window of d in ascending j,
    adding wl q where L[j] == d, then the window of d - 1, adding (1 - wl) q where L[j] == d - 1."""
    L = np.asarray(L, dtype=np.int64)
    n = L.shape[0]
    jlo, jhi = windows(L)
    T = np.zeros(n)
    for d in range(n):
        ts = 0.0
        for j in range(jlo[d], jhi[d]):
            if L[j] == d:
                ts += wl[j] * q[j]
        if d > 0:
            for j in range(jlo[d - 1], jhi[d - 1]):
                if L[j] == d - 1:
                    ts += (1.0 - wl[j]) * q[j]
        T[d] = ts
    return T


def push_row(L, wl, q):
    """The same T by np.add.at (oracle.stationary.hist_step's two calls)."""
    T = np.zeros(np.asarray(L).shape[0])
    np.add.at(T, L, wl * q)
    np.add.at(T, np.asarray(L) + 1, (1.0 - wl) * q)
    return T


def disorder(rng, lo, frac=0.25, reach=3):
    """A copy of the lottery ``lo`` ([..., n_a], rows sorted) with about ``frac`` of every row's
    entries moved by up to +-``reach`` cells and clipped into [0, n_a - 2]."""
    lo = np.array(lo, dtype=np.int64)
    n = lo.shape[-1]
    k = max(1, int(n * frac))
    flat = lo.reshape(-1, n)
    for row in flat:
        idx = rng.choice(n, size=k, replace=False)
        row[idx] = np.clip(row[idx] + rng.integers(-reach, reach + 1, size=k), 0, n - 2)
    return flat.reshape(lo.shape)
