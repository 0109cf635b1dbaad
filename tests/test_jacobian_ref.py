"""The NumPy sequence-space Jacobian reference (tests/jacobian_ref.py) on its own: the
fake-news Jacobian against brute-force finite differences of the block, the adjoint identity
of the expectation step, and the Newton solve on the calibration the damped loop cycles on."""
import numpy as np
import pytest

from oracle import stationary as ST
from tests import jacobian_ref as JR
from tests import transition_ref as TR

N_A, T, H_STEP = 120, 40, 1e-5
CALS = dict(A=(0.9, 0.4, 3.0), D=(0.6, 0.2, 1.0))
_cache = {}


def state(name):
    """Steady state, steady prices and fake-news matrices of one calibration, computed once."""
    if name not in _cache:
        ss = TR.cpu_steady_state(*CALS[name], N_A)
        Rs, ws = JR.steady_prices(ss, ss["alpha"], ss["delta"], ss["r"])
        _cache[name] = (ss, Rs, ws, JR.fake_news(ss, Rs, ws, T, H_STEP))
    return _cache[name]


@pytest.mark.parametrize("name", ["D", "A"])
def test_fake_news_matches_brute_force(name):
    """max|J_fake - J_brute| / max|J_brute| <= 1e-4 for both inputs: the error is O(h) (one-sided
    differences at h = 1e-5 on both sides); measured 1.12e-5 (D), 9.7e-7 (A) for R and
    <= 3.3e-7 for w, so the bound is 9x the worst case."""
    ss, Rs, ws, fn = state(name)
    bR, bw = JR.brute(ss, Rs, ws, T, H_STEP)
    for tag, fake, br in (("R", fn["JR"], bR), ("w", fn["Jw"], bw)):
        err = np.max(np.abs(fake - br)) / np.max(np.abs(br))
        print(f"{name} J^{tag}: max|fake - brute| / max|brute| = {err:.2e}")
        assert err <= 1e-4


@pytest.mark.parametrize("name", ["D", "A"])
def test_expectation_step_is_the_adjoint_of_hist_step(name):
    """sum E_1 D = sum a step(D) to 1e-13 relative, on the stationary mass and on a random one."""
    ss, Rs, ws, fn = state(name)
    lo, wlo, _ = ST.savings_lottery(ss["m"], ss["c"], ss["aGrid"], Rs, ws, ss["lab"])
    rng = np.random.default_rng(3)
    for D in (ss["mass"], rng.uniform(0.0, 1.0, size=ss["mass"].shape)):
        lhs = np.sum(fn["E"][1] * D)
        rhs = np.sum(ss["aGrid"][None, :] * ST.hist_step(D, lo, wlo, ss["P"]))
        assert abs(lhs - rhs) <= 1e-13 * abs(rhs)


def test_newton_converges_on_D():
    """D (log utility) cycles under damping 0.5; Newton reaches 1e-9 within 6 evaluations
    (measured: 4)."""
    ss, Rs, ws, fn = state("D")
    H = JR.capital_map(fn["JR"], fn["Jw"], ss["K"], ss["alpha"])
    hist = []
    out = JR.newton(ss, ss["alpha"], ss["delta"], TR.shock_path(T), T, H, tol=1e-9, max_iter=6, history=hist)
    print("D Newton residuals:", " ".join(f"{r:.1e}" for r in hist))
    assert out["status"] == 0 and out["iterations"] <= 6 and out["residual"] < 1e-9
    assert np.all(np.isfinite(out["K"]))


def test_impulse_is_the_first_order_term_of_the_newton_path():
    """The linear response against the Newton path at shock 1e-3: the second-order term is
    ~ size^2, so <= 1e-6 K* (measured worst case 1.4e-7)."""
    ss, Rs, ws, fn = state("A")
    H = JR.capital_map(fn["JR"], fn["Jw"], ss["K"], ss["alpha"])
    Z = TR.shock_path(T, size=1e-3)
    base = JR.newton(ss, ss["alpha"], ss["delta"], np.ones(T + 1), T, H, tol=1e-11, max_iter=8)
    out = JR.newton(ss, ss["alpha"], ss["delta"], Z, T, H, tol=1e-11, max_iter=8)
    dK, dr, dw = JR.impulse(fn["JR"], fn["Jw"], ss["K"], ss["alpha"], Z - 1.0)
    err = np.max(np.abs(out["K"] - base["K"] - dK)) / ss["K"]
    print(f"A impulse vs Newton at 1e-3: {err:.2e} K*")
    assert dK[0] == 0.0 and err <= 1e-6
