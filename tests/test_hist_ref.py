"""CPU tests of tests/hist_ref.py: the dense-matrix reference of the distribution solve against
the oracle's step, and the conditions that the GPU cases of tests/test_gpu_hist_forms.py rely on
(every batch of hist_ref.CASES: iteration caps, iteration counts of both parities, a fast and a
slow calibration, blocks of columns at the constraint and at the top, weights of exactly 1.0 and
0.0)."""
import numpy as np
import pytest

from oracle import stationary as ST
from tests import hist_ref as HR

EPS = HR.EPS


@pytest.mark.parametrize("shape", [(1, 33), (2, 2), (3, 40), (9, 21)])
def test_dense_T_is_the_oracle_step(shape):
    S, n_a = shape
    rng = np.random.default_rng(5)
    for family in ("fast", "slow"):
        _, lo, wlo, P = HR.make_batch(family, S, n_a, 2, 77)
        for c in range(2):
            T = HR.dense_T(lo[c], wlo[c], P[c])
            assert np.max(np.abs(T.sum(axis=0) - 1.0)) <= 4 * EPS        # column-stochastic
            assert T.min() >= 0.0
            m = rng.random((S, n_a))
            m /= m.sum()
            ref = ST.hist_step(m, lo[c], wlo[c], P[c])
            assert np.max(np.abs((T @ m.ravel()).reshape(S, n_a) - ref)) <= 8 * EPS * m.sum()
            assert np.max(np.abs(ST.hist_step_fast(m, lo[c], wlo[c], P[c]) - ref)) <= 8 * EPS * m.sum()
            pi = HR.stationary(T)
            assert pi.min() >= -1e-15 and abs(pi.sum() - 1.0) <= 1e-13
            s1, smax = HR.residuals(T, pi)
            assert smax <= 16 * EPS * HR.norm_inf(T)
            assert HR.norm_inf(T) >= 1.0 - 4 * EPS
            # the sparse and the dense form of the residual are the same sums
            assert HR.residuals(HR.csr(T), pi) == (s1, smax)


def test_dense_T_takes_any_rows():
    """Rows that are not monotone (a spike, swapped neighbours) are the same map."""
    _, lo, wlo, P = HR.make_batch("fast", 3, 60, 1, 9)
    lo, wlo, P = lo[0].copy(), wlo[0], P[0]
    lo[1, 30] = min(lo[1, 30] + 40, 58)
    lo[2, [10, 11]] = lo[2, [11, 10]]
    m = np.random.default_rng(1).random((3, 60))
    T = HR.dense_T(lo, wlo, P)
    assert np.max(np.abs((T @ m.ravel()).reshape(3, 60) - ST.hist_step(m, lo, wlo, P))) <= 8 * EPS * m.sum()


@pytest.mark.parametrize("name", sorted(HR.CASES))
def test_case_conditions(name):
    family, S, n_a, n_cal, _ = HR.CASES[name]
    _, lo, wlo, P = HR.batch(name)
    mass, iters = HR.plain(name)
    assert S * n_a <= 4200
    assert iters.max() <= HR.ITER_CAP[family], iters.max()
    assert set((iters % 2).tolist()) == {0, 1}, "final iteration counts of one parity only"
    assert 2 * iters.min() < iters.max(), (iters.min(), iters.max())
    at_con = ((lo == 0) & (wlo == 1.0)).reshape(n_cal, -1).sum(axis=1)
    at_top = ((lo == n_a - 2) & (wlo == 0.0)).reshape(n_cal, -1).sum(axis=1)
    if S >= 2:
        assert at_con.min() > 0 and at_top.min() > 0
    else:   # one state, kappa < 1: a rule reaches one end only; the batch holds both kinds
        assert at_con.max() > 0 and at_top.max() > 0 and np.all((at_con > 0) | (at_top > 0))
    assert np.all(np.diff(lo, axis=2) >= 0), "rule lotteries are monotone"
    assert lo.min() >= 0 and lo.max() <= n_a - 2
    for c in range(n_cal):
        T = HR.dense_T(lo[c], wlo[c], P[c])
        ninf = HR.norm_inf(T)
        b1, bmax = HR.residual_bounds(S * n_a, ninf)
        s1, smax = HR.residuals(T, mass[c])
        assert s1 <= b1 and smax <= bmax, (c, s1, b1, smax, bmax)
        # the rounding allowance of the bounds covers the reference's own float64 matvec
        x = mass[c].ravel()
        exact = HR.csr(T)
        Tm = np.zeros(x.size, dtype=HR.LD)
        Tm[exact[0]] = np.add.reduceat(exact[3] * x.astype(HR.LD)[exact[2]], exact[1])
        assert float(np.max(np.abs((T @ x).astype(HR.LD) - Tm))) <= 16 * EPS * ninf * x.sum()
        assert abs(x.sum() - 1.0) <= (S + 4) * EPS * (iters[c] + 1)


def test_families_differ_between_calibrations():
    """A calibration that reads a neighbour's lottery or P must miss its reference: no two of a
    batch share either."""
    for name in ("f7x300", "s7x300", "t2x16"):
        _, lo, wlo, P = HR.batch(name)
        n = min(lo.shape[0], 8)
        for a in range(n):
            for b in range(a + 1, n):
                assert not np.array_equal(wlo[a], wlo[b]) and not np.array_equal(P[a], P[b])
