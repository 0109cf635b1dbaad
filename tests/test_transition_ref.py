"""The NumPy transition-path reference (tests/transition_ref.py) on its own: the damped fixed
point converges on the Table II-style calibrations A, B, C, and reports -- without raising --
the one it does not converge on at this damping (D, log utility)."""
import numpy as np
import pytest

from tests import transition_ref as TR

N_A, T = 120, 40
CALS = dict(A=(0.9, 0.4, 3.0), B=(0.6, 0.2, 3.0), C=(0.3, 0.4, 5.0), D=(0.6, 0.2, 1.0))


def run(name, max_iter, history=None):
    ss = TR.cpu_steady_state(*CALS[name], N_A)
    out = TR.solve(ss["aGrid"], ss["lab"], ss["P"], ss["beta"], ss["crra"], ss["alpha"], ss["delta"],
                   TR.shock_path(T), T, ss["m"], ss["c"], ss["mass"], damping=0.5, tol=1e-9, max_iter=max_iter,
                   history=history)
    return ss, out


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_reference_converges(name):
    ss, out = run(name, 40)
    assert out["status"] == 0 and out["iterations"] <= 40 and out["residual"] < 1e-9
    assert TR.monotone(out["lo"])
    assert np.all(out["lo"] >= 0) and np.all(out["lo"] <= N_A - 2)
    # capital rises after the TFP shock, then decays back
    dev = out["K"] / ss["K"] - 1.0
    assert 4e-3 <= dev.max() <= 1e-2 and 5 <= int(dev.argmax()) <= 12


def test_reference_reports_non_convergence():
    hist = []
    ss, out = run("D", 40, history=hist)
    assert out["status"] == 1 and out["iterations"] == 40 and not out["residual"] < 1e-9
    assert np.all(np.isfinite(out["K"])) and np.all(np.isfinite(out["C"]))
    assert TR.monotone(out["lo"])
    # a bounded cycle, not a blow-up
    tail = np.array(hist[-8:])
    assert 3.5 < tail.min() and tail.max() < 14.0
