"""CPU checks of the equivalences the i.i.d.-income path of the device-resident GE search rests
on (AIY_OPT_HIST_IID; csrc/hist_bicg.h IID, csrc/ge_resident.hip ge_egm_cycle), on a grid of
300 points, for rho = 0 Tauchen chains of 5 and 7 states and a Rouwenhorst chain.
"""
import numpy as np
import pytest

from oracle import stationary as ost
from tests import iid_ref as IR

CASES = [(7, 0.2, 1.0, "tauchen"), (5, 0.4, 3.0, "tauchen"), (7, 0.2, 5.0, "tauchen"), (7, 0.4, 3.0, "rouwenhorst")]
_SETUP = {}


def _setup(case):
    if case not in _SETUP:
        _SETUP[case] = IR.setup(*case)
    return _SETUP[case]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[3]}{c[0]}-sd{c[1]}-crra{c[2]:g}")
def test_rows_of_P_are_bit_identical(case):
    e = _setup(case)
    assert IR.rows_bit_identical(e["P"])
    assert abs(e["pi"].sum() - 1.0) < 1e-14
    # the package's own chain, which is what the device reads
    from aiyagari_hark_amd.stationary import Calibration
    _, P = Calibration(LaborAR=0.0, LaborSD=case[1], CRRA=case[2], LaborStatesNo=case[0], income=case[3]).income_process()
    assert IR.rows_bit_identical(P)
    # a persistent chain, and one a hair away from i.i.d., are not
    for rho in (0.6, 1e-9):
        _, Q = Calibration(LaborAR=rho, LaborSD=case[1], CRRA=case[2], LaborStatesNo=case[0],
                           income=case[3]).income_process()
        assert not IR.rows_bit_identical(Q)
    assert not IR.rows_bit_identical(np.ones((1, 1)))
    B = e["P"].copy()
    B[-1, -1] = np.nextafter(B[-1, -1], 2.0)   # one bit
    assert not IR.rows_bit_identical(B)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[3]}{c[0]}-sd{c[1]}-crra{c[2]:g}")
def test_egm_tables_are_bit_identical_across_states(case):
    e = _setup(case)
    for tab in (e["m"], e["c"]):
        bits = np.ascontiguousarray(tab).view(np.int64)
        assert np.all(bits == bits[0])
    # and after one more step from them (the step itself, not only the fixed point)
    w, _ = ost.prices(0.03, 0.36, 0.08)
    m2, c2 = ost.egm_step(e["m"], e["c"], 0.96, case[2], e["aGrid"], 1.03, w, e["lab"], e["P"])
    assert np.all(m2.view(np.int64) == m2.view(np.int64)[0]) and np.all(c2.view(np.int64) == c2.view(np.int64)[0])


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[3]}{c[0]}-sd{c[1]}-crra{c[2]:g}")
def test_asset_grid_operator_is_the_row_sum_of_hist_step(case):
    e = _setup(case)
    rng = np.random.default_rng(11)
    mu = rng.random(e["aGrid"].size)
    mu /= mu.sum()
    full = ost.hist_step(np.outer(e["pi"], mu), e["lo"], e["wlo"], e["P"])
    red = IR.m_step(mu, e["lo"], e["wlo"], e["pi"])
    # both are sums of the same nonnegative products in another order, at most S n_a of them into
    # one destination (the borrowing constraint): the reordering bound n eps of the largest entry
    bound = e["pi"].size * mu.size * np.finfo(float).eps
    assert np.max(np.abs(full.sum(axis=0) - red)) <= bound * np.max(red)
    assert np.max(np.abs(full - np.outer(e["pi"], red))) <= bound * np.max(red)
    # T x is pi (x) (its row sum) for ANY x, a tensor product or not: every fixed point is one
    x = rng.random((e["pi"].size, mu.size))
    x /= x.sum()
    tx = ost.hist_step(x, e["lo"], e["wlo"], e["P"])
    assert np.max(np.abs(tx - np.outer(e["pi"], tx.sum(axis=0)))) <= bound * np.max(tx)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[3]}{c[0]}-sd{c[1]}-crra{c[2]:g}")
def test_fixed_point_of_M_tensored_with_pi_is_stationary(case):
    e = _setup(case)
    tol = 1e-12
    mu, it = IR.m_fixed_point(e["lo"], e["wlo"], e["pi"], tol)
    x = np.outer(e["pi"], mu)
    res = np.max(np.abs(ost.hist_step(x, e["lo"], e["wlo"], e["P"]) - x))
    print(f"\n{case}: {it} iterations, residual of pi (x) mu in hist_step {res:.2e}")
    assert res < 1e-11
    assert abs(mu.sum() - 1.0) < 1e-12
    # the same fixed point as the full iteration's
    full, _, _ = ost.stationary_hist(e["lo"], e["wlo"], e["P"], mu.size, tol=tol)
    assert np.max(np.abs(full - x)) < 1e-9


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[3]}{c[0]}-sd{c[1]}-crra{c[2]:g}")
def test_scaled_stopping_rule_is_the_full_one(case):
    """max|T x - x| for x = pi (x) mu is max(pi) max|M mu - mu| (up to rounding), so the loop on
    mu at tol / max(pi) stops where the full vector's test at tol does."""
    e = _setup(case)
    rng = np.random.default_rng(5)
    mu = np.full(e["aGrid"].size, 1.0 / e["aGrid"].size)
    for k in range(40):
        new = IR.m_step(mu, e["lo"], e["wlo"], e["pi"])
        if k % 8 == 0:
            x = np.outer(e["pi"], mu)
            d_full = np.max(np.abs(ost.hist_step(x, e["lo"], e["wlo"], e["P"]) - x))
            d_red = np.max(np.abs(new - mu)) * np.max(e["pi"])
            # (each side's entries carry the reordering error n eps of the largest mass entry)
            assert abs(d_full - d_red) <= 2 * e["pi"].size * mu.size * np.finfo(float).eps * np.max(mu)
        mu = new + 1e-6 * rng.standard_normal(mu.size) * new   # keep it away from the fixed point
