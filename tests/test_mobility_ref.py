"""CPU tests that pin tests/mobility_ref.py, the NumPy model of the cohort sweep and of the class
rule: against the dense Markov chain, and the class rule on built marginals."""
import numpy as np

from tests import mobility_ref as MR


def small_chain(seed, S=3, n_a=12):
    rng = np.random.default_rng(seed)
    lo = np.sort(rng.integers(0, n_a - 1, size=(S, n_a)), axis=-1)
    wlo = rng.uniform(0.0, 1.0, size=(S, n_a))
    P = rng.dirichlet(np.ones(S), size=S)
    mass = rng.uniform(0.0, 1.0, size=(S, n_a))
    mass /= mass.sum()
    aGrid = np.linspace(0.0, 5.0, n_a) ** 2
    return lo, wlo, P, mass, aGrid


def test_sweep_equals_the_dense_chain():
    """S = 3, n_a = 12: the occupancy of every cohort and period equals the class sums of
    cohort @ M^t, M the [S n_a][S n_a] chain, to 1e-14."""
    lo, wlo, P, mass, aGrid = small_chain(0)
    S, n_a = lo.shape
    M = MR.dense_chain(lo, wlo, P)
    assert np.max(np.abs(M.sum(axis=1) - 1.0)) <= 1e-15
    edges = MR.class_edges(mass.sum(axis=0), (0.2, 0.4, 0.6, 0.8))
    T = 6
    worst = 0.0
    for cohorts in (MR.split_by_class(mass, edges), MR.split_by_state(mass)):
        assert np.array_equal(cohorts.sum(axis=0), mass)   # every element in exactly one cohort, copied
        for c in cohorts:
            K, occ, inc, mT = MR.sweep(c, lo[None], wlo[None], P, T, edges, aGrid)
            for t in range(T + 1):
                d = (c.ravel() @ np.linalg.matrix_power(M, t)).reshape(S, n_a)
                worst = max(worst, np.max(np.abs(occ[t] - MR.class_sums(d, edges))),
                            np.max(np.abs(inc[t] - d.sum(axis=1))), abs(K[t] - np.sum(d * aGrid[None, :])) / 25.0)
            assert np.max(np.abs(mT - d)) <= 1e-14
    print(f"dense chain: worst difference {worst:.2e}")
    assert worst <= 1e-14


def test_lottery_of_every_period():
    """n_lot = T takes lottery t in period t: T stacked copies give the bits of n_lot = 1."""
    lo, wlo, P, mass, aGrid = small_chain(1)
    edges = np.array([0, 5, 12])
    T = 4
    one = MR.sweep(mass, lo[None], wlo[None], P, T, edges, aGrid)
    many = MR.sweep(mass, np.repeat(lo[None], T, axis=0), np.repeat(wlo[None], T, axis=0), P, T, edges, aGrid)
    assert all(np.array_equal(a, b) for a, b in zip(one, many))


def test_mobility_matrix_rows_sum_to_one():
    for by in ("wealth", "income"):
        lo, wlo, P, mass, aGrid = small_chain(2)
        shares, matrix, edges = MR.mobility_matrix(mass, lo, wlo, P, (0.2, 0.4, 0.6, 0.8), (1, 5, 20), aGrid, by=by)
        live = shares > 0
        assert live.any() and abs(shares.sum() - 1.0) <= 1e-15
        assert np.max(np.abs(matrix[:, live, :].sum(axis=-1) - 1.0)) <= 1e-14
        assert np.all(np.isnan(matrix[:, ~live, :]))


def test_class_rule_on_built_marginals():
    p = (0.2, 0.4, 0.6, 0.8)
    # one node with more than 20 % of the mass: it holds the bands of two percentiles, a class is empty
    g = np.array([2.0, 12.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 4.0]) / 32.0
    e = MR.class_edges(g, p)
    assert e.tolist() == [0, 2, 2, 5, 8, 10]     # 32 F_prev = 0, 2, 14, 16, 18, 20, 22, 24, 26, 28; 32 p = 6.4, 12.8, ...
    assert np.all(np.diff(e) >= 0) and (np.diff(e) == 0).sum() == 1
    # F_prev equal to a percentile exactly (binary fractions): that node opens the upper class
    e = MR.class_edges(np.array([0.25, 0.25, 0.25, 0.25]), (0.25, 0.5, 0.75))
    assert e.tolist() == [0, 1, 2, 3, 4]
    e = MR.class_edges(np.array([0.5, 0.25, 0.125, 0.125]), (0.5,))
    assert e.tolist() == [0, 1, 4]
    # all mass on one node: it lies in the lowest class, the others are empty
    for k in (0, 3, 7):
        g = np.zeros(8)
        g[k] = 2.0
        e = MR.class_edges(g, p)
        assert e.tolist() == [0] + [k + 1] * 4 + [8]
        cohorts = MR.split_by_class(np.stack([g, g]), e)
        assert cohorts[0].sum() == 4.0 and cohorts[1:].sum() == 0.0
    # a scalar multiple of a marginal has the same classes
    g = np.random.default_rng(5).uniform(size=50)
    assert np.array_equal(MR.class_edges(g, p), MR.class_edges(4.0 * g, p))
