"""GPU tests of the household solve of the device-resident GE search (csrc/ge_resident.hip:
ge_household_isolated, one separate function per CRRA kind that receives its arguments and the
kernel's dynamic LDS by value, and the Anderson ring written only in the cycles a mix reads).

Four calibrations in one launch, so that the four kinds of the marginal utility run side by side
in one kernel: CRRA 1, 3 and 5 (the Table II values, closed forms) and 2.5 (the general pow), at
n_a = 1437, an odd size: the last workgroup of a cluster owns fewer columns than the others.
Clusters capped at 2 workgroups run two columns per thread, at 4 one column per thread (the same
household functions under the other kernel); 5 labour states take the generic <8, 0, ...>
instantiations, 7 the Table II ones.  AIY_OPT_GE_ANDERSON at its default (12: 5 cycles of 12 are
kept in the ring), at 0 (no ring, the geometric extrapolation) and at 5 (every cycle is kept, a
mix at the first allowed cycle).  Each case is held to the host-driven search (resident=False)
with the bounds of test_gpu_bicg_loop.py.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_A = 1437
_REF = {}   # labour states -> the host-driven search's result (computed once, never changed)


def _cells(states):
    from aiyagari_hark_amd.stationary import Calibration, table2_calibrations
    cals = table2_calibrations(LaborStatesNo=states)
    pick = [next(c for c in cals if c.CRRA == 1.0), [c for c in cals if c.CRRA == 3.0][len(cals) // 6],
            [c for c in cals if c.CRRA == 5.0][-1]]
    return pick + [Calibration(LaborAR=0.3, LaborSD=0.4, CRRA=2.5, LaborStatesNo=states)]


def _host_reference(gpu, states):
    from aiyagari_hark_amd.stationary import solve_table2
    if states not in _REF:
        ref = solve_table2(_cells(states), n_a=N_A, device=gpu, method="brent", groups=1, resident=False)
        assert np.all(ref.status == 0)
        _REF[states] = ref
    return _REF[states]


def _resident(gpu, h, cals, options):
    """The resident search under `options`: (result, plan, launches, point-matvecs, EGM cycles)."""
    from aiyagari_hark_amd.stationary import resident_plan, solve_table2
    prev = h.set_options(options)
    try:
        plan = resident_plan(gpu, len(cals), cals[0].LaborStatesNo, N_A)
        h.check(h.lib.aiy_ge_launch_stats(h.h, None, None, None, None, 1), "reset")
        res = solve_table2(cals, n_a=N_A, device=gpu, method="brent", groups=1, resident=True)
        ms, n, pts, cyc = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        h.check(h.lib.aiy_ge_launch_stats(h.h, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(pts),
                                          ctypes.byref(cyc), 1), "stats")
    finally:
        h.set_options(prev)
    return res, plan, n.value, pts.value, cyc.value


@pytest.mark.parametrize("anderson", [None, 0, 5], ids=["aa-default", "aa-off", "aa-5"])
@pytest.mark.parametrize("cluster,states", [(2, 7), (4, 7), (2, 5), (4, 5)])
def test_four_crra_kinds_match_host_search(gpu, cluster, states, anderson):
    from aiyagari_hark_amd import _lib
    h = _lib.handle(gpu.index)
    cals = _cells(states)
    assert sorted(c.CRRA for c in cals) == [1.0, 2.5, 3.0, 5.0]
    ref = _host_reference(gpu, states)
    opts = {_lib.AIY_OPT_HIST_CLUSTER: cluster}
    if anderson is not None:
        opts[_lib.AIY_OPT_GE_ANDERSON] = anderson
    res, plan, n, pts, cyc = _resident(gpu, h, cals, opts)
    dr = np.max(np.abs(res.r - ref.r))
    dk = np.max(np.abs(res.KtoY - ref.KtoY) / ref.KtoY)
    print(f"\ncluster {cluster} states {states} anderson {anderson}: plan {plan}; {n} launch(es), {cyc:.0f} EGM "
          f"cycles, {pts:.3e} point-matvecs; max |dr| {dr:.2e}, max rel |dK/Y| {dk:.2e}")
    # G workgroups per cluster; two columns per thread at G = 2 (719 columns on 512 threads), one at G = 4
    assert plan is not None and plan[0] == cluster and plan[2] == (2 if cluster == 2 else 1)
    assert plan[1] * (cluster - 1) < N_A < plan[1] * cluster   # the last workgroup owns fewer columns
    assert n >= 1 and pts > 0 and cyc > 0                       # the resident kernel ran
    assert np.all(res.status == 0)
    assert dr <= 2e-7
    assert dk <= 2e-6


def test_ring_stores_leave_the_pull_form_reproducible(gpu):
    """The pull form without rebalancing is deterministic: with the Anderson mixing at its default
    period (most cycles pass no ring slot) two runs give the same bits and the same cycle count."""
    from aiyagari_hark_amd import _lib
    h = _lib.handle(gpu.index)
    cals = _cells(7)
    opts = {_lib.AIY_OPT_HIST_CLUSTER: 2, _lib.AIY_OPT_HIST_PULL: 1, _lib.AIY_OPT_GE_REBALANCE: 0}
    runs = [_resident(gpu, h, cals, opts) for _ in range(2)]
    (a, _, na, _, cyc_a), (b, _, nb, _, cyc_b) = runs
    print(f"\nr {a.r}; EGM cycles {cyc_a:.0f} / {cyc_b:.0f}")
    assert na >= 1 and nb >= 1 and cyc_a > 0
    assert np.all(a.status == 0) and np.all(b.status == 0)
    assert a.r.tobytes() == b.r.tobytes()
    assert cyc_a == cyc_b and int(a.egm_cycles[0][0]) == int(b.egm_cycles[0][0])
