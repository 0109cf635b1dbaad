"""GPU test of the handle's owned scratch (csrc/owned.h, csrc/carve.h): every entry point that keeps
scratch on the handle runs on ONE fresh handle at a small shape, a larger one and the small one
again, so each buffer is created, regrown and reused below its capacity; the three users of the
resident histogram's second buffer (BiCGSTAB push, BiCGSTAB with the small pull matvec, the S > 8
pull form) follow one another.  Every result equals the same call on a second fresh handle that
only ever saw that shape: bit for bit, except the forms that sum with floating-point atomics,
which are held to the tolerances of their own tests (test_gpu_hist_resident.py: plain resident
masses 1e-13 / iterations +-1 / K 1e-12, BiCGSTAB push masses 1e-8 / K 1e-5;
test_gpu_ge_resident.py: r 2e-7, K/Y 2e-6).  Then the launch statistics of the fixed call
sequence, and a handle closed and created again on the same device."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = {"small": (1, 40), "large": (3, 300)}          # (n_cal, n_a)
ORDER = ("small", "large", "small")
# resident launches of the sequence `ORDER x USERS` below, counted on the commit before the
# handle's scratch became owning types: (aiy_hist_launch_stats, aiy_ge_launch_stats,
# aiy_panel_launch_stats launches, its periods)
PARENT_LAUNCHES = (12, 6, 3, 30)


@contextlib.contextmanager
def fresh_handle(gpu):
    """Every wrapper of the package takes the device's shared handle from _lib.handle(): a fresh
    handle stands in for it inside the block and is destroyed after it."""
    from aiyagari_hark_amd import _lib
    shared = _lib._handles.pop(gpu.index, None)
    h = _lib.Handle(gpu.index)
    _lib._handles[gpu.index] = h
    try:
        yield h
    finally:
        torch.cuda.synchronize()
        _lib._handles.pop(gpu.index, None)
        h.close()
        if shared is not None:
            _lib._handles[gpu.index] = shared


def _batch(gpu, shape, S=7):
    from aiyagari_hark_amd import setup_math as sm
    from aiyagari_hark_amd.stationary import Calibration, StationaryBatch
    n_cal, n_a = SHAPES[shape]
    income = "tauchen" if S == 7 else "rouwenhorst"
    cals = [Calibration(LaborAR=ar, LaborSD=0.2, CRRA=crra, LaborStatesNo=S, income=income)
            for ar, crra in ((0.3, 3.0), (0.0, 1.0), (0.6, 5.0))[:n_cal]]
    return StationaryBatch(cals, sm.make_grid_exp_mult(0.001, 50.0, n_a, 2), device=gpu)


def _stationary(gpu, shape, S, accel, pull):
    """aiy_egm_solve + aiy_hist_solve: (K, EGM cycles, iterations, mass, m table, c table)."""
    from aiyagari_hark_amd import _lib
    h = _lib.handle(gpu.index)
    b = _batch(gpu, shape, S)
    prev = h.set_options({_lib.AIY_OPT_HIST_PULL: int(pull)})
    try:
        K, cycles, iters = b.capital_supply(np.linspace(0.02, 0.035, len(b.cals)), accel=accel)
    finally:
        h.set_options(prev)
    return (K, cycles, iters, b.mass.cpu().numpy()) + tuple(t.cpu().numpy() for t in b.last_tables)


def _ge(gpu, shape, pull):
    """aiy_ge_stationary, device-resident: (r, K, K_s, status, K/Y up to the labour factor)."""
    from aiyagari_hark_amd import _lib
    from aiyagari_hark_amd.stationary import ge_stationary_native
    h = _lib.handle(gpu.index)
    b = _batch(gpu, shape)
    prev = h.set_options({_lib.AIY_OPT_HIST_PULL: int(pull)})
    try:
        r, K, Ks, steps, cyc, its, status = ge_stationary_native(
            b, "brent", 1e-7, 1e-8, 1e-12, 60, True, True, -1, secant=True, loose=True, extrapolate=True, resident=True)
    finally:
        h.set_options(prev)
    assert np.all(status == 0)
    return r, K, Ks, status, K ** (1.0 - b.alpha)


def _value_reduce(gpu, shape):
    from aiyagari_hark_amd.welfare import value_reduce
    b = _batch(gpu, shape)
    g = torch.Generator(device="cpu").manual_seed(7)
    mass = torch.rand(b.mass.shape, dtype=torch.float64, generator=g).to(gpu)
    V = torch.randn(b.mass.shape, dtype=torch.float64, generator=g).to(gpu)
    return (value_reduce(b, mass, V),)


def _wealth_stats(gpu, shape):
    from aiyagari_hark_amd.stats import get_lorenz_shares, get_percentiles
    n = SHAPES[shape][1] + 1   # (one scan block: the device scan is then order-stable)
    rng = np.random.default_rng(11)
    data, w = rng.lognormal(size=n), rng.random(n) + 0.1
    pct = np.array([0.2, 0.5, 0.9])
    return (get_lorenz_shares(data, w, pct, device=gpu), get_percentiles(data, w, pct, device=gpu),
            get_lorenz_shares(data, None, pct, device=gpu))


def _block_panel(gpu, shape):
    """aiy_sim_block_periods: n_cal calibrations in one block-engine launch."""
    from aiyagari_hark_amd.panel import BatchedPanel
    n_cal = SHAPES[shape][0]
    fxs = [np.load(os.path.join(GOLD, n + ".npz")) for n in ("egm_cfg1", "egm_cfg1_afunc2", "egm_ckpt")[:n_cal]]
    N, T = 201, 20
    dv = lambda x: torch.as_tensor(np.ascontiguousarray(x)).to(gpu)  # noqa: E731
    bp = BatchedPanel(n_cal, N, T, device=gpu)
    bp.bind_models(dv(np.stack([f["m"] for f in fxs])), dv(np.stack([f["c"] for f in fxs])),
                   dv(np.stack([f["Mgrid"] for f in fxs])), dv(np.stack([f["LSStates"] for f in fxs])),
                   dv(np.stack([f["cdf"] for f in fxs])),
                   dv(np.stack([f["Mrkv_hist"][:T].astype(np.int32) for f in fxs])),
                   [dict(CapShare=0.36, DeprFac=0.08, prod=(1.0, 1.0), agg_L=(1.0, 1.0))] * n_cal)
    bp.reset(np.array([float(f["KSS"]) for f in fxs]), np.random.default_rng(3).integers(0, 7, (n_cal, N)),
             [[float(f["MSS"]), float(f["KSS"]), 0, float(f["RSS"]), float(f["WSS"])] for f in fxs])
    bp.run(0, T, shock_mode="philox", seeds=(5, 17, 99)[:n_cal], ge_iter=3)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in (bp.lab, bp.a, bp.hist_A, bp.hist_M, bp.sow[:, :5]))


def _grid_panel(gpu, shape, sizes):
    """aiy_sim_periods with device Philox shocks: one launch of the persistent panel from 65 536
    agents, a captured graph of per-period launches below."""
    from aiyagari_hark_amd.panel import DevicePanel
    fx = np.load(os.path.join(GOLD, "egm_cfg1.npz"))
    N, T = sizes[shape], 10
    p = DevicePanel(N, device=gpu, act_T=T, engine="grid")
    p.bind_model(*(torch.as_tensor(fx[k]).to(gpu) for k in ("m", "c", "Mgrid", "LSStates", "cdf")),
                 torch.as_tensor(fx["Mrkv_hist"].astype(np.int32)).to(gpu),
                 dict(CapShare=0.36, DeprFac=0.08, prod=(1.0, 1.0), agg_L=(1.0, 1.0)))
    p.reset(float(fx["KSS"]), np.random.default_rng(5).integers(0, 7, N), float(fx["MSS"]), float(fx["KSS"]), 0,
            float(fx["RSS"]), float(fx["WSS"]))
    p.run(0, T, shock_mode="philox", seed=31, ge_iter=2)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in (p.lab, p.a, p.hist_A, p.hist_M, p.sow[:5]))


def _exact(got, ref):
    for k, (x, y) in enumerate(zip(got, ref)):
        assert np.array_equal(x, y), f"output {k} differs"


def _plain_hist(got, ref):
    (K, cyc, it, m), (K0, cyc0, it0, m0) = got[:4], ref[:4]
    _exact((cyc,) + got[4:], (cyc0,) + ref[4:])   # the household solve is order-stable
    assert np.max(np.abs(it - it0)) <= 1 and np.max(np.abs(m - m0)) < 1e-13 and np.max(np.abs(K - K0) / K0) < 1e-12


def _bicg_push(got, ref):
    (K, cyc, _, m), (K0, cyc0, _, m0) = got[:4], ref[:4]
    _exact((cyc,) + got[4:], (cyc0,) + ref[4:])
    assert np.max(np.abs(m - m0)) < 1e-8 and np.max(np.abs(K - K0) / K0) < 1e-5


def _ge_push(got, ref):
    assert np.max(np.abs(got[0] - ref[0])) <= 2e-7 and np.max(np.abs(got[4] - ref[4]) / ref[4]) <= 2e-6


# name -> (call, comparison with the single-shape handle's result); the order is the call sequence
USERS = {
    "hist_plain": (lambda gpu, s: _stationary(gpu, s, 7, 0, False), _plain_hist),
    "hist_bicg_push": (lambda gpu, s: _stationary(gpu, s, 7, -1, False), _bicg_push),
    "hist_bicg_pull": (lambda gpu, s: _stationary(gpu, s, 7, -1, True), _exact),
    "hist_pull_9_states": (lambda gpu, s: _stationary(gpu, s, 9, -1, False), _exact),
    "ge_push": (lambda gpu, s: _ge(gpu, s, False), _ge_push),
    "ge_pull": (lambda gpu, s: _ge(gpu, s, True), _exact),
    "value_reduce": (_value_reduce, _exact),
    "wealth_stats": (_wealth_stats, _exact),
    "block_panel": (_block_panel, _exact),
    "period_panel": (lambda gpu, s: _grid_panel(gpu, s, {"small": 7001, "large": 40003}), _exact),
    "resident_panel": (lambda gpu, s: _grid_panel(gpu, s, {"small": 65537, "large": 131075}), _exact),
}


def _launch_stats(h):
    ms, n = ctypes.c_double(), ctypes.c_int64()
    n_ge, n_res, periods = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    h.check(h.lib.aiy_hist_launch_stats(h.h, ctypes.byref(ms), ctypes.byref(n), 1), "hist stats")
    h.check(h.lib.aiy_ge_launch_stats(h.h, ctypes.byref(ms), ctypes.byref(n_ge), None, None, 1), "ge stats")
    h.check(h.lib.aiy_panel_launch_stats(h.h, ctypes.byref(ms), ctypes.byref(n_res), ctypes.byref(periods), 1),
            "panel stats")
    return n.value, n_ge.value, n_res.value, periods.value


@pytest.fixture(scope="module")
def grown(gpu):
    """The whole sequence on one handle: results[(user, visit)] and the launch statistics."""
    results = {}
    with fresh_handle(gpu) as h:
        for visit, shape in enumerate(ORDER):
            for name, (call, _) in USERS.items():
                results[name, visit] = call(gpu, shape)
        stats = _launch_stats(h)
        again = _launch_stats(h)
    return results, stats, again


@pytest.mark.parametrize("name", list(USERS))
def test_grown_handle_equals_single_shape_handle(gpu, grown, name):
    call, same = USERS[name]
    ref = {}
    for shape in SHAPES:
        with fresh_handle(gpu):
            ref[shape] = call(gpu, shape)
    for visit, shape in enumerate(ORDER):
        same(grown[0][name, visit], ref[shape])


def test_launch_statistics(grown):
    _, stats, again = grown
    print(f"\nlaunches (hist, GE, panel, panel periods) = {stats}")
    assert stats == PARENT_LAUNCHES
    assert again == (0, 0, 0, 0)   # read-and-reset


def test_handle_closed_and_created_again(gpu):
    out = []
    for _ in range(2):
        with fresh_handle(gpu):
            out.append(_stationary(gpu, "small", 7, -1, True))
    _exact(out[1], out[0])
