"""CPU tests of the NumPy reference of the histogram wealth statistics (tests/dist_stats_ref.py):
closed forms, the mean-difference Gini, and HARK's two functions on a steady state."""
import numpy as np

from oracle import hark_utils as HU
from tests import dist_stats_ref as DR
from tests import transition_ref as TR

PCT = np.linspace(0.01, 0.999, 15)      # the notebook's pctiles


def test_equal_wealth_has_gini_zero():
    a = np.array([0.5, 2.0, 7.0])
    g = np.array([0.0, 1.0, 0.0])       # everybody holds 2.0
    assert DR.gini(g, a) == 0.0
    mass = np.array([[0.0, 0.25, 0.0], [0.0, 0.75, 0.0]])
    st = DR.dist_stats(mass, a, [0.5])
    assert st["gini"] == 0.0 and st["mean"] == 2.0 and st["total"] == 1.0 and st["bottom_share"] == 0.0


def test_two_nodes_closed_form():
    a = np.array([0.0, 1.0])
    g = np.array([0.5, 0.5])
    F, L = DR.curves(g, a)
    assert np.array_equal(F, [0.5, 1.0]) and np.array_equal(L, [0.0, 1.0])
    st = DR.marginal_stats(g, a, [0.75])
    assert st["gini"] == 0.5
    assert st["lorenz"][0] == 0.5
    assert st["mean"] == 0.5 and st["bottom_share"] == 0.5


def test_trapezoid_gini_is_the_mean_difference_gini():
    rng = np.random.default_rng(3)
    worst = 0.0
    for n in (2, 5, 40, 300):
        for _ in range(5):
            a = np.sort(rng.uniform(0.0, 50.0, n))
            g = rng.uniform(0.0, 1.0, n)
            g[rng.uniform(size=n) < 0.3] = 0.0      # nodes without mass: ties in F
            g[rng.integers(n)] += 0.5
            worst = max(worst, abs(DR.gini(g, a) - DR.gini_mean_difference(g, a)))
    print(f"trapezoid vs mean-difference Gini: {worst:.1e}")
    assert worst <= 1e-12


def test_steady_state_needs_no_sort():
    ss = TR.cpu_steady_state(0.9, 0.4, 3.0, 120)
    a = ss["aGrid"]
    st = DR.dist_stats(ss["mass"], a, PCT)
    g = DR.marginal(ss["mass"])
    assert np.array_equal(st["lorenz"], HU.get_lorenz_shares(a, weights=g, percentiles=PCT, presorted=False))
    assert np.array_equal(st["percentile_values"], HU.get_percentiles(a, weights=g, percentiles=PCT, presorted=False))
    assert not np.any(np.isnan(st["percentile_values"]))
    print(f"A n_a=120: gini {st['gini']:.4f} bottom share {st['bottom_share']:.4f}")
    assert 0.3 < st["gini"] < 0.7
    assert abs(st["mean"] * st["total"] - np.sum(ss["mass"] * a[None, :])) <= 1e-12 * ss["K"]
