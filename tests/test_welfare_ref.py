"""CPU tests of the welfare reference (tests/welfare_ref.py) on the CPU steady states of the
calibrations A and D of tests/test_gpu_transition.py at n_a = 60: the properties the device
code is then held to."""
import numpy as np
import pytest

from tests import transition_ref as TR
from tests import welfare_ref as WR

CALS = {"A": dict(labor_ar=0.9, labor_sd=0.4, crra=3.0), "D": dict(labor_ar=0.6, labor_sd=0.2, crra=1.0)}
T = 10


@pytest.fixture(scope="module", params=sorted(CALS))
def state(request):
    """The steady state, its lottery and dense value, and a T = 10 block on wiggled prices."""
    ss = TR.cpu_steady_state(n_a=60, **CALS[request.param])
    aG, lab, P, beta, crra = ss["aGrid"], ss["lab"], ss["P"], ss["beta"], ss["crra"]
    R, w = 1.0 + ss["r"], TR.ST.prices(ss["r"], ss["alpha"], ss["delta"])[0]
    lo, wlo, _ = TR.ST.savings_lottery(ss["m"], ss["c"], aG, R, w, lab)
    u = WR.flow_utility(aG, lab, R, w, lo, wlo, crra)
    V_star = WR.steady_value_dense(u, lo, wlo, P, beta)
    Kp = ss["K"] * (1.0 + 0.01 * np.cos(0.9 * np.arange(T + 1)))
    rp, wp = TR.path_prices(Kp, TR.shock_path(T), ss["alpha"], ss["delta"])
    blk = TR.block(aG, lab, P, beta, crra, 1.0 + rp, wp, ss["m"], ss["c"], ss["mass"])
    return dict(ss=ss, lo=lo, wlo=wlo, u=u, V_star=V_star, Rp=1.0 + rp, wp=wp, blk=blk)


def test_iterated_steady_value_matches_dense_solve(state):
    """The iteration stopped at tol = 1e-10 by the relative rule is within 2e-10 max |V| of the
    dense solve: the rule's bound tol max |V| plus rounding of order (S + 4) 2^-53 / (1 - beta)."""
    ss = state["ss"]
    assert np.all(WR.consumption(ss["aGrid"], ss["lab"], 1.0 + ss["r"],
                                 TR.ST.prices(ss["r"], ss["alpha"], ss["delta"])[0], state["lo"], state["wlo"]) > 0)
    V, it, d = WR.steady_value_iter(state["u"], state["lo"], state["wlo"], ss["P"], ss["beta"], tol=1e-10)
    vmax = np.max(np.abs(state["V_star"]))
    err = np.max(np.abs(V - state["V_star"]))
    print(f"crra {ss['crra']}: {it} steps, last distance {d:.2e}, max |V| {vmax:.4g}, |V - V*| {err:.2e}")
    assert it < 5000
    assert err <= 2e-10 * vmax


def test_welfare_identity_on_a_path(state):
    """sum mass_0 V_0 = sum_t beta^t sum mass_t u(c_t) + beta^T sum mass_T V_T within 1e-13
    relative: the backward recursion is the adjoint of the forward step."""
    ss, blk = state["ss"], state["blk"]
    V = WR.path_values(state["V_star"], blk["lo"], blk["wlo"], ss["P"], ss["aGrid"], ss["lab"], state["Rp"],
                       state["wp"], ss["beta"], ss["crra"])
    lhs = float(np.sum(ss["mass"] * V[0]))
    rhs, mass_T = WR.forward_discounted(ss["mass"], blk["lo"], blk["wlo"], ss["P"], ss["aGrid"], ss["lab"],
                                        state["Rp"], state["wp"], ss["beta"], ss["crra"], state["V_star"])
    assert np.allclose(mass_T, blk["mass_T"], rtol=0, atol=1e-15)
    print(f"crra {ss['crra']}: lhs {lhs!r} rhs {rhs!r} rel {abs(lhs - rhs) / abs(lhs):.2e}")
    assert abs(lhs - rhs) <= 1e-13 * abs(lhs)


def test_no_change_is_no_gain(state):
    ss = state["ss"]
    V = state["V_star"]
    assert np.all(WR.ce_nodes(V, V, ss["beta"], ss["crra"]) == 0.0)
    W = float(np.sum(ss["mass"] * V))
    assert WR.ce_sums(W, W, 1.0, ss["beta"], ss["crra"]) == 0.0


@pytest.mark.parametrize("g", [0.01, -0.03])
def test_scaled_consumption_is_recovered(state, g):
    """Consumption scaled by 1 + g in every period (the terminal value included) gives back g by
    node and through the mass-weighted sums, within 1e-12."""
    ss, blk = state["ss"], state["blk"]
    beta, crra = ss["beta"], ss["crra"]
    args = (blk["lo"], blk["wlo"], ss["P"], ss["aGrid"], ss["lab"], state["Rp"], state["wp"], beta, crra)
    V_term = state["V_star"]
    V_term_g = V_term + np.log1p(g) / (1.0 - beta) if crra == 1.0 else (1.0 + g) ** (1.0 - crra) * V_term
    V0 = WR.path_values(V_term, *args)[0]
    V0_g = WR.path_values(V_term_g, *args, scale=1.0 + g)[0]
    assert np.max(np.abs(WR.ce_nodes(V0_g, V0, beta, crra) - g)) <= 1e-12
    mass = ss["mass"]
    share = float(np.sum(mass))
    assert abs(WR.ce_sums(np.sum(mass * V0_g), np.sum(mass * V0), share, beta, crra) - g) <= 1e-12
    for s in range(mass.shape[0]):
        got = WR.ce_sums(np.sum(mass[s] * V0_g[s]), np.sum(mass[s] * V0[s]), np.sum(mass[s]), beta, crra)
        assert abs(got - g) <= 1e-12
