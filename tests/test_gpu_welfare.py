"""GPU tests of the welfare entry points (csrc/welfare.hip, aiyagari_hark_amd/welfare.py) against
the NumPy reference tests/welfare_ref.py, which is always fed the device's own lotteries, and
against the adjoint identity sum mass_0 V_0 = sum_t beta^t sum mass_t u(c_t) + beta^T sum mass_T V_T.

n_a = 120 leaves a partial last block of 56 columns; S = 7 leaves the states unevenly over the
4 waves of a block; the synthetic lotteries reach lo = 0, wlo = 1 and lo = n_a - 2, wlo = 0."""
import types

import numpy as np
import pytest

from oracle import stationary as ST
from tests import transition_ref as TR
from tests import welfare_ref as WR
from tests.test_gpu_transition import A, B, C, D, R25, synthetic_problem, wiggle_prices

pytestmark = pytest.mark.gpu

CRRAS = np.array([1.0, 3.0, 5.0, 2.5])
BETAS = np.array([0.96, 0.95, 0.96, 0.9])


@pytest.fixture(scope="module")
def ss120(gpu):
    from aiyagari_hark_amd.stationary import Calibration
    from aiyagari_hark_amd.transition import steady_state
    return steady_state([Calibration(**k) for k in (A, B, C, D)], 120, device=gpu)


@pytest.fixture(scope="module")
def ss25(gpu):
    from aiyagari_hark_amd.stationary import Calibration
    from aiyagari_hark_amd.transition import steady_state
    return steady_state([Calibration(**R25), Calibration(**R25)], 1000, device=gpu)


@pytest.fixture(scope="module")
def vstar120(ss120):
    """V* of ss120 at tol = 1e-10 and the solve's report: computed once, never modified."""
    from aiyagari_hark_amd.welfare import stationary_value
    info = {}
    return stationary_value(ss120[0], info=info), info


def up(dev, x, dt=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x)).to(dt or torch.float64).to(dev)


def fake_batch(dev, P, aGrid, lab, beta, crra):
    """What the welfare wrappers read of a StationaryBatch, for uploaded problems."""
    n_cal, S = lab.shape
    return types.SimpleNamespace(cals=[None] * n_cal, S=S, n_a=aGrid.shape[1], device=dev, d_P=up(dev, P),
                                 d_a=up(dev, aGrid), d_lab=up(dev, lab), d_beta=up(dev, beta), d_crra=up(dev, crra))


def host_lottery(batch, r=None):
    from aiyagari_hark_amd.welfare import steady_lottery
    lo, wlo, dR, dw = steady_lottery(batch, r)
    return lo.cpu().numpy().astype(np.int64), wlo.cpu().numpy(), dR.cpu().numpy(), dw.cpu().numpy()


@pytest.mark.parametrize("S,n_a", [(7, 120), (7, 1000), (25, 120), (25, 1000)])
@pytest.mark.parametrize("variant", ["head", "tail"])
def test_synthetic_recursion(gpu, S, n_a, variant):
    """1: V0 and every V_path[t] within 1e-12 max |V| of the reference (about ten times the
    per-step bound (S + 4) 2^-53 accumulated over 1 / (1 - beta) <= 25) for CRRA 1, 3, 5 and 2.5;
    V_path[0] is V0 bit for bit; the last two periods and the last one alone, re-run from V_term,
    reproduce V_path[T - 2] and V_path[T - 1] bit for bit."""
    import torch

    from aiyagari_hark_amd.welfare import path_value
    n_cal, T = 4, 5
    rng = np.random.default_rng(1000 * S + n_a + (variant == "tail"))
    lo, wlo, P, _, aGrid = synthetic_problem(rng, n_cal, S, n_a, T, variant)
    if variant == "head":
        wlo[:, :, 0, :5] = 1.0        # all of the mass on node 0
    else:
        wlo[:, :, S - 1, -5:] = 0.0   # all of it on node n_a - 1
    lab = rng.uniform(0.5, 1.5, size=(n_cal, S))
    R = 1.0 + rng.uniform(0.01, 0.05, size=(n_cal, T + 1))
    w = (1.2 * aGrid[:, -1:] / lab.min(axis=1, keepdims=True)) * rng.uniform(1.0, 1.1, size=(n_cal, T + 1))
    assert np.all(w * lab.min(axis=1, keepdims=True) > aGrid[:, -1:])   # so c > 0 at every node
    # a terminal value of the size of the flow utilities' discounted sum, so that max |V| does not
    # hide u(c) (c is 60 to 170 here: u is ~1e-8 for CRRA = 5)
    scale = np.abs([float(WR.utility(np.float64(60.0), g)) for g in CRRAS]) / (1.0 - BETAS)
    V_term = rng.normal(size=(n_cal, S, n_a)) * scale[:, None, None]
    fb = fake_batch(gpu, P, aGrid, lab, BETAS, CRRAS)
    d_lo, d_wlo, d_R, d_w, d_Vt = up(gpu, lo, torch.int32), up(gpu, wlo), up(gpu, R), up(gpu, w), up(gpu, V_term)
    V0, V_path = path_value(fb, d_lo, d_wlo, d_R, d_w, d_Vt, keep_path=True)
    V0_only = path_value(fb, d_lo, d_wlo, d_R, d_w, d_Vt)
    tail2 = path_value(fb, d_lo[T - 2:].contiguous(), d_wlo[T - 2:].contiguous(), d_R[:, T - 2:].contiguous(),
                       d_w[:, T - 2:].contiguous(), d_Vt)
    tail1 = path_value(fb, d_lo[T - 1:].contiguous(), d_wlo[T - 1:].contiguous(), d_R[:, T - 1:].contiguous(),
                       d_w[:, T - 1:].contiguous(), d_Vt)   # T = 1
    torch.cuda.synchronize()
    assert torch.equal(V_path[0], V0) and torch.equal(V0_only, V0)
    assert torch.equal(tail2, V_path[T - 2]) and torch.equal(tail1, V_path[T - 1])
    got = V_path.cpu().numpy()
    for i in range(n_cal):
        ref = np.array(WR.path_values(V_term[i], lo[:, i], wlo[:, i], P[i], aGrid[i], lab[i], R[i], w[i], BETAS[i],
                                      CRRAS[i]))
        assert np.all(np.isfinite(ref))
        err = np.max(np.abs(got[:, i] - ref)) / np.max(np.abs(ref))
        print(f"{variant} S={S} n_a={n_a} crra={CRRAS[i]}: max |V| {np.max(np.abs(ref)):.4g}  rel err {err:.2e}")
        assert err <= 1e-12


def test_batch_independence(ss120, vstar120):
    """2: each calibration alone gives V0 and V* (and its step count) bit-identical to its slice
    of the batch run."""
    import torch

    from aiyagari_hark_amd.transition import household_block, select
    from aiyagari_hark_amd.welfare import path_value, stationary_value
    batch, _, K = ss120
    V_star, info = vstar120
    R, w = wiggle_prices(K, 5)
    out = household_block(batch, R, w, *batch.last_tables, batch.mass)
    V0 = path_value(batch, out.lo, out.wlo, R, w, V_star)
    for i in range(len(batch.cals)):
        sub = select(batch, [i])
        one = {}
        Vs = stationary_value(sub, info=one)
        assert torch.equal(Vs[0], V_star[i]) and one["iterations"][0] == info["iterations"][i]
        V0_i = path_value(sub, out.lo[:, i:i + 1].contiguous(), out.wlo[:, i:i + 1].contiguous(), R[i:i + 1],
                          w[i:i + 1], Vs)
        assert torch.equal(V0_i[0], V0[i])


def test_steady_value_small(ss120, vstar120):
    """3 (n_a = 120): V* within 2e-10 max |V| of the dense solve (I - beta Lambda) V = u on the
    device's own lottery (the stopping rule's bound tol max |V| plus rounding), before max_iter;
    5 periods at the steady prices and lottery from V* give V* back within 1e-10 max |V|
    (|T^5 V - V| <= 5 (1 - beta) tol max |V| by the stopping rule)."""
    from aiyagari_hark_amd.welfare import path_value, steady_lottery
    batch, _, _ = ss120
    V_star, info = vstar120
    V = V_star.cpu().numpy()
    lo, wlo, R, w = host_lottery(batch)
    for i, cal in enumerate(batch.cals):
        u = WR.flow_utility(batch.aGrid[i], batch.levels[i], R[i], w[i], lo[i], wlo[i], cal.CRRA)
        assert np.min(WR.consumption(batch.aGrid[i], batch.levels[i], R[i], w[i], lo[i], wlo[i])) > 0
        ref = WR.steady_value_dense(u, lo[i], wlo[i], batch.P[i], cal.DiscFac)
        vmax = np.max(np.abs(ref))
        err = np.max(np.abs(V[i] - ref))
        print(f"cal {i}: {info['iterations'][i]} steps, dist {info['dist'][i]:.2e}, max |V| {vmax:.5g}, "
              f"|V - V*| / max |V| {err / vmax:.2e}")
        assert info["iterations"][i] < 5000
        assert err <= 2e-10 * vmax
    d_lo, d_wlo, dR, dw = steady_lottery(batch)
    T = 5
    again = path_value(batch, d_lo[None].repeat(T, 1, 1, 1), d_wlo[None].repeat(T, 1, 1, 1),
                       dR[:, None].repeat(1, T + 1), dw[:, None].repeat(1, T + 1), V_star).cpu().numpy()
    for i in range(len(batch.cals)):
        assert np.max(np.abs(again[i] - V[i])) <= 1e-10 * np.max(np.abs(V[i]))


def test_steady_value_large(ss25):
    """3 (S = 25, n_a = 1000, too large for a dense solve): V* at tol = 1e-10 within 2e-10 max |V|
    of the reference iteration run to 1e-12 on the device's lottery."""
    from aiyagari_hark_amd.welfare import path_value, stationary_value, steady_lottery
    batch, _, _ = ss25
    info = {}
    V_dev = stationary_value(batch, tol=1e-10, info=info)
    V = V_dev.cpu().numpy()
    lo, wlo, R, w = host_lottery(batch)
    ref = None
    for i, cal in enumerate(batch.cals):
        if ref is None or not (np.array_equal(lo[i], lo[0]) and np.array_equal(wlo[i], wlo[0]) and R[i] == R[0]
                               and w[i] == w[0]):
            u = WR.flow_utility(batch.aGrid[i], batch.levels[i], R[i], w[i], lo[i], wlo[i], cal.CRRA)
            ref, it, _ = WR.steady_value_iter(u, lo[i], wlo[i], batch.P[i], cal.DiscFac, tol=1e-12)
            assert it < 5000
        vmax = np.max(np.abs(ref))
        err = np.max(np.abs(V[i] - ref))
        print(f"R25 cal {i}: {info['iterations'][i]} steps, max |V| {vmax:.5g}, |V - V*| / max |V| {err / vmax:.2e}")
        assert info["iterations"][i] < 5000
        assert err <= 2e-10 * vmax
    d_lo, d_wlo, dR, dw = steady_lottery(batch)
    T = 5
    again = path_value(batch, d_lo[None].repeat(T, 1, 1, 1), d_wlo[None].repeat(T, 1, 1, 1),
                       dR[:, None].repeat(1, T + 1), dw[:, None].repeat(1, T + 1), V_dev).cpu().numpy()
    for i in range(len(batch.cals)):
        assert np.max(np.abs(again[i] - V[i])) <= 1e-10 * np.max(np.abs(V[i]))


def test_adjoint_identity_on_a_real_path(ss120, vstar120):
    """4: sum mass_0 V_0 by aiy_value_reduce equals the discounted sum of NumPy forward steps on
    the device's lotteries plus beta^T sum mass_T V*, within 1e-11 relative."""
    from aiyagari_hark_amd.transition import household_block
    from aiyagari_hark_amd.welfare import path_value, value_reduce
    batch, _, K = ss120
    V_star, _ = vstar120
    T = 40
    R, w = wiggle_prices(K, T)
    out = household_block(batch, R, w, *batch.last_tables, batch.mass)
    V0 = path_value(batch, out.lo, out.wlo, R, w, V_star)
    lhs = value_reduce(batch, batch.mass, V0).sum(axis=1)
    lo, wlo = out.lo.cpu().numpy().astype(np.int64), out.wlo.cpu().numpy()
    mass, Vs = batch.mass.cpu().numpy(), V_star.cpu().numpy()
    for i, cal in enumerate(batch.cals):
        rhs, _ = WR.forward_discounted(mass[i], lo[:, i], wlo[:, i], batch.P[i], batch.aGrid[i], batch.levels[i],
                                       R[i], w[i], cal.DiscFac, cal.CRRA, Vs[i])
        rel = abs(lhs[i] - rhs) / abs(rhs)
        print(f"cal {i}: sum mass_0 V_0 {lhs[i]!r}  forward {rhs!r}  rel {rel:.2e}")
        assert rel <= 1e-11


def test_consumption_equivalents(gpu):
    """5: by node within 1e-13 absolute of the NumPy formulas for CRRA 1, 3, 5 and 2.5 and exactly
    0 for V_new = V_base; ce_aggregate / ce_by_state are the formulas on the reduced sums and
    agree with NumPy sums within 1e-12 relative."""
    import torch

    from aiyagari_hark_amd.welfare import consumption_equivalent, welfare
    n_cal, S, n_a = 4, 7, 120
    rng = np.random.default_rng(5)
    P = rng.dirichlet(np.ones(S), size=(n_cal, S))
    aGrid = np.broadcast_to(ST.make_stationary_grid(0.001, 50.0, n_a, 2), (n_cal, n_a)).copy()
    fb = fake_batch(gpu, P, aGrid, rng.uniform(0.5, 1.5, size=(n_cal, S)), BETAS, CRRAS)
    V_base = -rng.uniform(1.0, 100.0, size=(n_cal, S, n_a))
    V_new = V_base * rng.uniform(0.97, 1.03, size=V_base.shape)
    V_base[0] = rng.uniform(1.0, 30.0, size=(S, n_a))          # CRRA = 1: levels, not ratios
    # gains of either sign by node, but no state's sum is a near-cancellation: a relative bound on
    # exp((1 - beta) dW / share) - 1 says nothing where dW itself is rounding
    V_new[0] = V_base[0] + rng.uniform(-0.2, 0.5, size=(S, n_a))
    mass = rng.uniform(0.0, 1.0, size=(n_cal, S, n_a))
    mass /= mass.sum(axis=(1, 2), keepdims=True)
    d_new, d_base, d_mass = up(gpu, V_new), up(gpu, V_base), up(gpu, mass)
    g = consumption_equivalent(fb, d_new, d_base).cpu().numpy()
    zero = consumption_equivalent(fb, d_base, d_base)
    assert bool(torch.all(zero == 0.0))
    res = welfare(fb, d_new, d_base, d_mass)
    assert torch.equal(res.ce, consumption_equivalent(fb, d_new, d_base))
    for i in range(n_cal):
        err = np.max(np.abs(g[i] - WR.ce_nodes(V_new[i], V_base[i], BETAS[i], CRRAS[i])))
        print(f"crra {CRRAS[i]}: ce by node abs err {err:.2e}")
        assert err <= 1e-13
        Wn, Wb, share = np.sum(mass[i] * V_new[i], axis=1), np.sum(mass[i] * V_base[i], axis=1), mass[i].sum(axis=1)
        assert np.allclose(res.W_by_state[i], Wn, rtol=1e-12, atol=0)
        assert np.allclose(res.W_base_by_state[i], Wb, rtol=1e-12, atol=0)
        assert np.isclose(res.W[i], Wn.sum(), rtol=1e-12, atol=0) and np.isclose(res.W_base[i], Wb.sum(), rtol=1e-12)
        assert np.allclose(res.ce_by_state[i], WR.ce_sums(Wn, Wb, share, BETAS[i], CRRAS[i]), rtol=1e-12, atol=0)
        assert np.isclose(res.ce_aggregate[i], WR.ce_sums(Wn.sum(), Wb.sum(), share.sum(), BETAS[i], CRRAS[i]),
                          rtol=1e-12, atol=0)
        if CRRAS[i] != 1.0:   # ... and they are the formula on the reduced sums themselves
            assert np.array_equal(res.ce_by_state[i],
                                  WR.ce_sums(res.W_by_state[i], res.W_base_by_state[i], 1.0, BETAS[i], CRRAS[i]))


def test_solve_transition_with_welfare(ss120, vstar120):
    """6: welfare=True changes nothing else of the result (bit for bit); the gain of a positive
    TFP shock is finite and positive on every calibration; V re-derived by path_value from the
    result's prices is the result's V bit for bit."""
    import torch

    from aiyagari_hark_amd.transition import household_block, solve_transition
    from aiyagari_hark_amd.welfare import path_value
    batch, _, _ = ss120
    T = 40
    Z = TR.shock_path(T)
    plain = solve_transition(batch, Z, T, method="newton")
    res = solve_transition(batch, Z, T, method="newton", welfare=True)
    assert plain.welfare is None and np.all(res.status == 0)
    for name in ("K", "r", "w", "C", "iterations", "residual"):
        assert np.array_equal(getattr(plain, name), getattr(res, name)), name
    wf = res.welfare
    print("ce_aggregate", wf.ce_aggregate, "ce by node", float(wf.ce.min()), float(wf.ce.max()))
    assert np.all(np.isfinite(wf.ce_aggregate)) and np.all(wf.ce_aggregate > 0)
    assert np.all(np.isfinite(wf.ce_by_state))
    assert torch.equal(wf.V_base, vstar120[0])
    out = household_block(batch, 1.0 + res.r, res.w, *batch.last_tables, batch.mass)
    assert torch.equal(path_value(batch, out.lo, out.wlo, 1.0 + res.r, res.w, wf.V_base), wf.V)


def test_refusals(ss120, vstar120):
    """7: T = 0, a null V_term and tol = 1e-14 give AIY_ERR_ARG with the outputs untouched; a path
    priced with w = 0 runs normally and welfare() raises ValueError naming c <= 0."""
    import torch

    from aiyagari_hark_amd import _lib
    from aiyagari_hark_amd.transition import household_block
    from aiyagari_hark_amd.welfare import path_value, steady_lottery, welfare
    batch, _, K = ss120
    V_star, _ = vstar120
    n_cal, S, n_a, T = len(batch.cals), batch.S, batch.n_a, 5
    R, w = wiggle_prices(K, T)
    out = household_block(batch, R, w, *batch.last_tables, batch.mass)
    dev = batch.device
    dR, dw = up(dev, R), up(dev, w)
    h = _lib.handle(dev.index)
    work = torch.empty(int(h.lib.aiy_value_work_bytes(n_cal, S, n_a)), dtype=torch.uint8, device=dev)
    V0 = torch.full((n_cal, S, n_a), -7.0, dtype=torch.float64, device=dev)
    Vp = torch.full((T, n_cal, S, n_a), -7.0, dtype=torch.float64, device=dev)

    def backward(T_arg, V_term):
        return h.lib.aiy_value_backward(h.h, n_cal, S, n_a, T_arg, _lib.ptr(out.lo), _lib.ptr(out.wlo),
                                        _lib.ptr(batch.d_P), _lib.ptr(batch.d_a), _lib.ptr(dR), _lib.ptr(dw),
                                        _lib.ptr(batch.d_lab), _lib.ptr(batch.d_beta), _lib.ptr(batch.d_crra),
                                        _lib.ptr(V_term), _lib.ptr(work), _lib.ptr(V0), _lib.ptr(Vp), _lib.stream_ptr())
    assert backward(0, V_star) == -1 and _lib.ERRORS[-1] == "AIY_ERR_ARG"
    assert backward(T, None) == -1
    torch.cuda.synchronize()
    assert bool(torch.all(V0 == -7.0)) and bool(torch.all(Vp == -7.0))
    lo, wlo, sR, sw = steady_lottery(batch)
    V = torch.full((n_cal, S, n_a), -7.0, dtype=torch.float64, device=dev)
    beta = np.ascontiguousarray(batch.d_beta.cpu().numpy())
    iters, dist = np.full(n_cal, -7, dtype=np.int32), np.full(n_cal, -7.0)
    rc = h.lib.aiy_value_stationary(h.h, n_cal, S, n_a, _lib.ptr(lo), _lib.ptr(wlo), _lib.ptr(batch.d_P),
                                    _lib.ptr(batch.d_a), _lib.ptr(sR), _lib.ptr(sw), _lib.ptr(batch.d_lab),
                                    _lib.ptr(batch.d_beta), _lib.ptr(batch.d_crra), beta.ctypes.data_as(_lib.c_double_p),
                                    1e-14, 100, 0, _lib.ptr(V), _lib.ptr(work), iters.ctypes.data_as(_lib.c_int32_p),
                                    dist.ctypes.data_as(_lib.c_double_p), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and b"tol" in h.lib.aiy_last_error(h.h)
    assert bool(torch.all(V == -7.0)) and np.all(iters == -7) and np.all(dist == -7.0)
    assert backward(T, V_star) == 0   # the good call still runs
    torch.cuda.synchronize()
    assert bool(torch.all(torch.isfinite(V0))) and torch.equal(Vp[0], V0)
    bad = path_value(batch, out.lo, out.wlo, R, np.zeros_like(w), V_star)   # c = R a - a' <= 0 where a' > R a
    torch.cuda.synchronize()
    assert not bool(torch.all(torch.isfinite(bad)))
    with pytest.raises(ValueError, match="c <= 0"):
        welfare(batch, bad, V_star, batch.mass)
