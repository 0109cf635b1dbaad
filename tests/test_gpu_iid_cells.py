"""GPU tests of the i.i.d.-income path of the device-resident GE search (AIY_OPT_HIST_IID): a
calibration whose transition matrix has bit-identical rows collapses the income dimension, in the
household cycle (exact) and in the push form of the distribution solve (the asset-grid BiCGSTAB of
csrc/hist_bicg.h).

Shapes as tests/test_gpu_bicg_loop.py: n_a = 1437 (the last workgroup owns fewer columns),
clusters capped at 2 workgroups (two columns per thread) and at 4 (one), 7 labour states (the
Table II instantiations) and 5 (the generic ones).  Bounds: those of test_gpu_ge_resident.py.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_A = 1437
SHAPES = [(2, 7), (4, 7), (2, 5), (4, 5)]
_HOST = {}   # states -> host-driven search of the mixed cells (computed once, never changed)


def _cal(rho, sd, crra, states):
    from aiyagari_hark_amd.stationary import Calibration
    return Calibration(LaborAR=rho, LaborSD=sd, CRRA=crra, LaborStatesNo=states)


def _mixed(states):
    return [_cal(0.0, 0.2, 1.0, states), _cal(0.0, 0.4, 3.0, states), _cal(0.0, 0.2, 5.0, states),
            _cal(0.6, 0.2, 3.0, states)]


def _solve(gpu, cals, opts, resident=True):
    """(result, i.i.d. cells reported by the hook, launches, mid-solve stops) under handle options."""
    from aiyagari_hark_amd import _lib
    from aiyagari_hark_amd.stationary import solve_table2
    h = _lib.handle(gpu.index)
    prev = h.set_options(opts)
    try:
        res = solve_table2(cals, n_a=N_A, device=gpu, method="brent", groups=1, resident=resident)
        cells, launches, mid = ctypes.c_int32(-1), ctypes.c_int32(), ctypes.c_int32()
        h.check(h.lib.aiy_ge_last_iid_cells(h.h, ctypes.byref(cells)), "iid cells")
        if resident:
            h.check(h.lib.aiy_ge_last_rounds(h.h, ctypes.byref(launches), ctypes.byref(mid)), "rounds")
    finally:
        h.set_options(prev)
    return res, cells.value, launches.value, mid.value


def _close(a, b, what):
    dr = np.max(np.abs(a.r - b.r))
    dk = np.max(np.abs(a.KtoY - b.KtoY) / b.KtoY)
    print(f"{what}: max |dr| {dr:.2e}, max rel |dK/Y| {dk:.2e}")
    assert np.all(a.status == 0) and np.all(b.status == 0)
    assert dr <= 2e-7
    assert dk <= 2e-6


@pytest.mark.parametrize("cluster,states", SHAPES)
def test_mixed_launch(gpu, cluster, states):
    """Three i.i.d. cells and a persistent one in one launch: exactly the three take the reduced
    solve, and the roots are those of the general code and of the host-driven search."""
    from aiyagari_hark_amd import _lib
    cals = _mixed(states)
    base = {_lib.AIY_OPT_HIST_CLUSTER: cluster, _lib.AIY_OPT_HIST_PULL: 0}
    on, n_on, _, _ = _solve(gpu, cals, {**base, _lib.AIY_OPT_HIST_IID: 1})
    off, n_off, _, _ = _solve(gpu, cals, {**base, _lib.AIY_OPT_HIST_IID: 0})
    if states not in _HOST:
        _HOST[states], n_host, _, _ = _solve(gpu, cals, {}, resident=False)
        assert n_host == 0   # the host-driven loop has no reduced solve: the hook speaks of the last call
    print(f"\ncluster {cluster} states {states}: reduced solves on {n_on}, off {n_off}")
    assert n_on == 3 and n_off == 0
    _close(on, off, "on against off")
    _close(on, _HOST[states], "on against the host-driven search")


@pytest.mark.parametrize("cluster,states", SHAPES)
def test_near_iid_takes_the_general_path(gpu, cluster, states):
    """rho = 1e-9: the rows of P differ in their last bits, so the cell is not i.i.d."""
    from aiyagari_hark_amd import _lib
    cals = [_cal(1e-9, 0.2, 3.0, states)]
    base = {_lib.AIY_OPT_HIST_CLUSTER: cluster, _lib.AIY_OPT_HIST_PULL: 0}
    on, n_on, _, _ = _solve(gpu, cals, {**base, _lib.AIY_OPT_HIST_IID: 1})
    off, n_off, _, _ = _solve(gpu, cals, {**base, _lib.AIY_OPT_HIST_IID: 0})
    print(f"\ncluster {cluster} states {states}: reduced solves on {n_on}, off {n_off}")
    assert n_on == 0 and n_off == 0
    _close(on, off, "on against off")


@pytest.mark.parametrize("cluster,states", SHAPES)
def test_relaunch(gpu, cluster, states):
    """Six cells with rebalancing at its default: the stopped clusters -- i.i.d. ones among them,
    also inside a distribution solve -- go on in a second launch."""
    from aiyagari_hark_amd import _lib
    cals = [_cal(rho, 0.2, crra, states) for rho in (0.0, 0.3) for crra in (1.0, 3.0, 5.0)]
    base = {_lib.AIY_OPT_HIST_CLUSTER: cluster, _lib.AIY_OPT_HIST_PULL: 0}
    on, n_on, launches, mid = _solve(gpu, cals, {**base, _lib.AIY_OPT_HIST_IID: 1})
    off, n_off, launches_off, mid_off = _solve(gpu, cals, {**base, _lib.AIY_OPT_HIST_IID: 0})
    print(f"\ncluster {cluster} states {states}: on {launches} launches, {mid} mid-solve stops, {n_on} reduced; "
          f"off {launches_off} launches, {mid_off} mid-solve stops")
    assert n_on == 3 and n_off == 0
    assert launches >= 2
    _close(on, off, "on against off")


@pytest.mark.parametrize("cluster,states", SHAPES)
def test_household_collapse_is_exact(gpu, cluster, states):
    """Pull form, one launch: only the household collapse is active, and it changes no bit."""
    from aiyagari_hark_amd import _lib
    cals = _mixed(states)
    base = {_lib.AIY_OPT_HIST_CLUSTER: cluster, _lib.AIY_OPT_HIST_PULL: 1, _lib.AIY_OPT_GE_REBALANCE: 0}
    on, n_on, _, _ = _solve(gpu, cals, {**base, _lib.AIY_OPT_HIST_IID: 1})
    off, n_off, _, _ = _solve(gpu, cals, {**base, _lib.AIY_OPT_HIST_IID: 0})
    assert n_on == 0 and n_off == 0   # the pull form keeps the general distribution solve
    for f in ("r", "K", "K_supply", "KtoY"):
        assert np.array_equal(getattr(on, f).view(np.int64), getattr(off, f).view(np.int64)), f
    assert np.array_equal(on.status, off.status) and np.all(on.status == 0)
