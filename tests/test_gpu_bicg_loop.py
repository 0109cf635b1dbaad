"""GPU tests of the BiCGSTAB loop of the device-resident GE search (csrc/hist_bicg.h as
ge_resident.hip calls it: the solve as a separate function that receives the kernel's dynamic
LDS by address, and the same lambdas inlined for the pull form).

Three Table II cells at n_a = 1437, an odd size: the last workgroup of a cluster owns fewer
columns than the others, so threads with inactive points exist in every phase.  Clusters capped
at 2 workgroups run two columns per thread (a span boundary between the two workgroups), at 4
one column per thread (the form whose alpha reduction rides on the matvec barrier); 5 labour
states take the generic <8, 0, ...> instantiations, 7 the Table II ones.  Each case runs the
push form and the pull form (AIY_OPT_HIST_PULL) and is held to the host-driven search
(resident=False) with the bounds of test_gpu_ge_resident.py.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_A = 1437
_REF = {}   # labour states -> the host-driven search's result (computed once, never changed)


def _cells(states):
    from aiyagari_hark_amd.stationary import table2_calibrations
    cals = table2_calibrations(LaborStatesNo=states)
    return [cals[k] for k in np.linspace(0, len(cals) - 1, 3).astype(int)]


def _host_reference(gpu, states):
    from aiyagari_hark_amd.stationary import solve_table2
    if states not in _REF:
        ref = solve_table2(_cells(states), n_a=N_A, device=gpu, method="brent", groups=1, resident=False)
        assert np.all(ref.status == 0)
        _REF[states] = ref
    return _REF[states]


@pytest.mark.parametrize("pull", [0, 1], ids=["push", "pull"])
@pytest.mark.parametrize("cluster,states", [(2, 7), (4, 7), (2, 5), (4, 5)])
def test_resident_bicg_loop_matches_host_search(gpu, cluster, states, pull):
    from aiyagari_hark_amd import _lib
    from aiyagari_hark_amd.stationary import resident_plan, solve_table2
    h = _lib.handle(gpu.index)
    cals = _cells(states)
    ref = _host_reference(gpu, states)
    prev = h.set_options({_lib.AIY_OPT_HIST_CLUSTER: cluster, _lib.AIY_OPT_HIST_PULL: pull})
    try:
        plan = resident_plan(gpu, len(cals), states, N_A)
        h.check(h.lib.aiy_ge_launch_stats(h.h, None, None, None, None, 1), "reset")
        res = solve_table2(cals, n_a=N_A, device=gpu, method="brent", groups=1, resident=True)
        ms, n, pts, cyc = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        h.check(h.lib.aiy_ge_launch_stats(h.h, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(pts),
                                          ctypes.byref(cyc), 1), "stats")
    finally:
        h.set_options(prev)
    dr = np.max(np.abs(res.r - ref.r))
    dk = np.max(np.abs(res.KtoY - ref.KtoY) / ref.KtoY)
    print(f"\ncluster {cluster} states {states} pull {pull}: plan {plan}; {n.value} launch(es), {pts.value:.3e} "
          f"point-matvecs; max |dr| {dr:.2e}, max rel |dK/Y| {dk:.2e}")
    # G workgroups per cluster; two columns per thread at G = 2 (719 columns on 512 threads), one at G = 4
    assert plan is not None and plan[0] == cluster and plan[2] == (2 if cluster == 2 else 1)
    assert plan[1] * (cluster - 1) < N_A < plan[1] * cluster   # the last workgroup owns fewer columns
    assert n.value >= 1 and pts.value > 0 and cyc.value > 0     # the resident kernel ran
    assert np.all(res.status == 0)
    assert dr <= 2e-7
    assert dk <= 2e-6
