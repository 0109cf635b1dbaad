"""CPU tests of the NumPy reference of the household-variable statistics (tests/var_stats_ref.py):
the Gini of the merged distribution against the mean-difference Gini, the wealth case against
tests/dist_stats_ref.py, and the monotone runs the device merge relies on, on the oracle steady
states of the calibrations A to D of tests/test_gpu_dist_stats.py at n_a = 120."""
import numpy as np
import pytest

from tests import dist_stats_ref as DR
from tests import transition_ref as TR
from tests import var_stats_ref as VR

CALS = {"A": dict(labor_ar=0.9, labor_sd=0.4, crra=3.0), "B": dict(labor_ar=0.6, labor_sd=0.2, crra=3.0),
        "C": dict(labor_ar=0.3, labor_sd=0.4, crra=5.0), "D": dict(labor_ar=0.6, labor_sd=0.2, crra=1.0)}
PCT = np.linspace(0.01, 0.999, 15)


def test_merged_gini_is_the_mean_difference_gini():
    """Random positive keys, sorted within each run, with ties within and across runs and nodes
    without weight: 1e-12, the bound of test_dist_stats_ref."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for S, n in ((1, 2), (3, 5), (7, 40), (4, 90)):
        for _ in range(4):
            key = np.sort(np.round(rng.uniform(0.5, 30.0, (S, n)) * 2.0) / 2.0, axis=1)   # halves: many ties
            w = rng.uniform(0.0, 1.0, (S, n))
            w[rng.uniform(size=(S, n)) < 0.3] = 0.0
            w[rng.integers(S), rng.integers(n)] += 0.5
            assert VR.runs_nondecreasing(key)
            st = VR.variable_stats(key, w, PCT)
            worst = max(worst, abs(st["gini"] - VR.gini_mean_difference(key, w)))
    print(f"merged vs mean-difference Gini: {worst:.1e}")
    assert worst <= 1e-12


def test_merge_is_the_stable_order():
    key = np.array([[1.0, 2.0, 2.0], [0.5, 2.0, 3.0]])
    w = np.arange(6.0).reshape(2, 3)
    ks, ws, rank = VR.merge(key, w)
    assert np.array_equal(ks, [0.5, 1.0, 2.0, 2.0, 2.0, 3.0]) and np.array_equal(ws, [3.0, 0.0, 1.0, 2.0, 4.0, 5.0])
    assert np.array_equal(rank, [[1, 2, 3], [0, 4, 5]])
    assert not VR.runs_nondecreasing(np.array([[1.0, 0.5]])) and not VR.runs_nondecreasing(np.array([[1.0, np.nan]]))


def test_moments_closed_form():
    y = np.array([[1.0, 3.0]])
    w = np.array([[0.5, 0.5]])
    sw, mean, cov = VR.moments([y, -2.0 * y], w)
    assert sw == 1.0 and np.array_equal(mean, [2.0, -4.0])
    assert np.array_equal(cov, [[1.0, -2.0], [-2.0, 4.0]])
    assert np.array_equal(VR.correlations([y, -2.0 * y], w), [[1.0, -1.0], [-1.0, 1.0]])


def test_wealth_as_a_variable_matches_the_marginal():
    """key = the grid in every state (S equal keys at every node): Lorenz shares, Gini, mean and
    total equal dist_stats_ref.dist_stats of the same mass within 1e-12.  Percentiles are not
    compared: HARK's interpolation puts its breakpoints inside a group of ties."""
    rng = np.random.default_rng(5)
    for S, n in ((1, 2), (7, 60), (5, 133)):
        a = np.sort(rng.uniform(0.0, 50.0, n))
        mass = rng.uniform(0.0, 1.0, (S, n))
        mass[:, : n // 4] = 0.0
        mass /= mass.sum()
        st = VR.variable_stats(np.broadcast_to(a, (S, n)), mass, PCT)
        ref = DR.dist_stats(mass, a, PCT)
        for k in ("lorenz", "gini", "mean", "total"):
            assert np.max(np.abs(np.asarray(st[k]) - np.asarray(ref[k]))) <= 1e-12, (S, n, k)


@pytest.fixture(scope="module", params=sorted(CALS))
def state(request):
    return TR.cpu_steady_state(n_a=120, **CALS[request.param])


def test_steady_state_runs_are_monotone_and_consumption_adds_up(state):
    """Consumption, income and cash are nondecreasing in every state at the steady prices and at
    R (1 +- 0.01) on held tables -- the condition the device merge relies on -- and
    sum mass c equals the block's C within 1e-12."""
    ss = state
    aG, lab = ss["aGrid"], ss["lab"]
    R, w = 1.0 + ss["r"], TR.ST.prices(ss["r"], ss["alpha"], ss["delta"])[0]
    for f in (1.0, 1.01, 0.99):
        lo, wlo, _ = TR.ST.savings_lottery(ss["m"], ss["c"], aG, R * f, w, lab)
        val = VR.variables(aG, lab, R * f, w, lo, wlo)
        for name in ("consumption", "income", "cash", "earnings", "wealth"):
            assert VR.runs_nondecreasing(val[name]), (f, name)
        assert np.all(np.diff(val["consumption"], axis=1) > 0) and np.all(np.diff(val["income"], axis=1) > 0)
        if f == 1.0:
            blk = TR.block(aG, lab, ss["P"], ss["beta"], ss["crra"], np.array([R, R]), np.array([w, w]), ss["m"],
                           ss["c"], ss["mass"])
            val = VR.variables(aG, lab, R, w, blk["lo"][0], blk["wlo"][0])   # the block's own period-0 lottery
            assert VR.runs_nondecreasing(val["consumption"])
            C = float(np.sum(ss["mass"] * val["consumption"]))
            # the block sums q - a' with the unclipped a'; the variable is defined on the lottery, which
            # holds a' to the grid (the constrained households' a' lies below a_0): the difference is
            # exactly the clipped part, as in test_gpu_transition's bound on C
            ap = blk["ap"][0]
            C_block = blk["C"][0] + float(np.sum(ss["mass"] * (ap - np.clip(ap, aG[0], aG[-1]))))
            print(f"crra {ss['crra']}: sum mass c {C!r} block C {blk['C'][0]!r}, on the lottery {C_block!r}")
            assert abs(C - C_block) <= 1e-12
            st = VR.variable_stats(val["consumption"], ss["mass"], PCT)
            assert abs(st["mean"] * st["total"] - C_block) <= 1e-12
            assert 0.05 < st["gini"] < 0.95
