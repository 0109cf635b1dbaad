"""GPU tests of the economy with aggregate risk to first order (csrc/aggregate.hip,
aiyagari_hark_amd/aggregate.py): the two device entry points against NumPy, the
policy derivatives and the simulation against tests/aggregate_ref.py, and the properties the
scheme rests on (no drift without shocks, second-order error, independence of batch and
chunking).  The reference is always fed the GPU's own steady-state tables and mass."""
import numpy as np
import pytest

from tests import aggregate_ref as AR
from tests import dist_stats_ref as DR
from tests import jacobian_ref as JR
from tests.test_gpu_transition import A, ALPHA, B, C, D, DELTA, host_state, synthetic_problem

pytestmark = pytest.mark.gpu

T_PATH, H, RHO = 40, 1e-5, 0.8
# the gaps against the reference measured on the MI355X on first run (see the docstrings), times 10
TOL_DA = 10 * 1.32e-9
TOL_SIM_K = 10 * 3.31e-13
TOL_SIM_C = 10 * 3.40e-13
TOL_SIM_GINI = 10 * 5.89e-13
TOL_A_STAR = 4e-16   # three roundings of a lottery mean, as in test_lottery_mean_matches_numpy


def up(dev, x, dt=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(x))
    return (t if dt is None else t.to(dt)).to(dev)


@pytest.fixture(scope="module")
def ss120(gpu):
    """[A, B, C, D] at n_a = 120: (batch, r*, K*)."""
    from aiyagari_hark_amd.stationary import Calibration
    from aiyagari_hark_amd.transition import steady_state
    return steady_state([Calibration(**k) for k in (A, B, C, D)], 120, device=gpu)


@pytest.fixture(scope="module")
def jac120(ss120):
    from aiyagari_hark_amd.transition import household_jacobian
    batch, r, _ = ss120
    return household_jacobian(batch, r, T_PATH, h=H)


@pytest.fixture(scope="module")
def pol120(ss120, jac120):
    """The policy derivatives, built after the Jacobian."""
    from aiyagari_hark_amd.aggregate import policy_jacobian
    batch, r, _ = ss120
    return policy_jacobian(batch, r, T_PATH, h=H)


@pytest.fixture(scope="module")
def model120(ss120, jac120):
    from aiyagari_hark_amd.aggregate import ar1, linear_model
    return linear_model(ss120[0], jac120, ar1(RHO, T_PATH))


@pytest.fixture(scope="module")
def ref120(ss120, jac120, model120):
    """Per calibration (host state, reference policy derivatives, the device model as the
    reference's dict): computed once."""
    batch, r, K = ss120
    out = []
    for i, hs in enumerate(host_state(batch, K)):
        Rs, ws = JR.steady_prices(hs, ALPHA, DELTA, r[i])
        with np.errstate(all="ignore"):
            pol = AR.policy_jacobian(hs, Rs, ws, T_PATH, H)
        model = dict(dZ=model120.dZ[i], dK=model120.dK[i], dr=model120.dr[i], dw=model120.dw[i], K=model120.K[i],
                     r=model120.r[i], w=model120.w[i], alpha=model120.alpha[i])
        out.append((hs, pol, model))
    return out


# -------------------------------------------------------------------------------------
# aiy_lottery_mean
# -------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,n_a", [(S, n_a) for S in (7, 25) for n_a in (120, 1000)])
def test_lottery_mean_matches_numpy(gpu, S, n_a):
    """wlo a[lo] + (1 - wlo) a[lo + 1] within 4e-16 relative of NumPy's."""
    import torch

    from aiyagari_hark_amd.aggregate import lottery_mean
    from tests.test_gpu_jacobian import fake_batch
    n_t, n_cal = 5, 2
    lo, wlo, P, _, aGrid = synthetic_problem(np.random.default_rng(21), n_cal, S, n_a, n_t, "head")
    aGrid[1] *= 1.25   # every calibration reads its own grid
    fake = fake_batch(gpu, P, aGrid, S, n_a)
    out = lottery_mean(fake, up(gpu, lo, torch.int32), up(gpu, wlo)).cpu().numpy()
    ref = np.stack([AR.lottery_mean(lo[:, i], wlo[:, i], aGrid[i]) for i in range(n_cal)], axis=1)
    err = np.max(np.abs(out - ref) / np.abs(ref))
    print(f"S={S} n_a={n_a}: lottery mean rel {err:.2e}")
    assert out.shape == (n_t, n_cal, S, n_a) and err <= 4e-16
    one = lottery_mean(fake, up(gpu, lo[2], torch.int32), up(gpu, wlo[2])).cpu().numpy()   # [n_cal][S][n_a]
    assert np.array_equal(one, out[2])


# -------------------------------------------------------------------------------------
# aiy_aggregate_lotteries
# -------------------------------------------------------------------------------------
def synthetic_operands(rng, n_cal, S, n_a, T, n_p):
    from oracle import stationary as ST
    aGrid = np.broadcast_to(ST.make_stationary_grid(0.001, 50.0, n_a, 2), (n_cal, n_a)).copy()
    a_star = np.sort(rng.uniform(aGrid[0, 0], aGrid[0, -1], size=(n_cal, S, n_a)), axis=-1)
    dA = [rng.standard_normal((T + 1, n_cal, S, n_a)) for _ in range(2)]
    X = 1e-2 * rng.standard_normal((n_cal, n_p, 2 * (T + 1)))
    return aGrid, a_star, dA, X


def synthesise(dev, aGrid, a_star, dA, X):
    """(lo, wlo) device tensors of aiy_aggregate_lotteries through the package's wrapper."""
    import types

    import torch

    from aiyagari_hark_amd.aggregate import PolicyJacobian, aggregate_lotteries
    n_cal, S, n_a = a_star.shape
    n_p = X.shape[1]
    fake = types.SimpleNamespace(cals=[None] * n_cal, S=S, n_a=n_a, device=dev, d_a=up(dev, aGrid))
    pol = PolicyJacobian(a_star=up(dev, a_star), dA_R=up(dev, dA[0]), dA_w=up(dev, dA[1]), h=H)
    lo = torch.full((n_p, n_cal, S, n_a), -7, dtype=torch.int32, device=dev)
    wlo = torch.full((n_p, n_cal, S, n_a), -7.0, dtype=torch.float64, device=dev)
    aggregate_lotteries(fake, pol, up(dev, X), lo, wlo)
    return lo, wlo


@pytest.mark.parametrize("n_p", [1, 7, 65])
@pytest.mark.parametrize("T", [5, 40])
@pytest.mark.parametrize("S,n_a", [(S, n_a) for S in (7, 25) for n_a in (120, 1000)])
def test_synthesis_matches_reference(gpu, S, n_a, T, n_p):
    """The mean of the device lottery against the clamped a' of NumPy: within the dot-product
    bound (2 (T + 1) + 4) 2^-53 (|a*| + sum |op X|) plus 2 ulp of a' for the locate; lo in
    [0, n_a - 2] and wlo in [0, 1] everywhere.  T = 40: 82 columns, not a multiple of 4; S n_a and
    n_p are off the tile edges."""
    n_cal = 2
    aGrid, a_star, dA, X = synthetic_operands(np.random.default_rng(100 * T + S + n_p), n_cal, S, n_a, T, n_p)
    lo, wlo = synthesise(gpu, aGrid, a_star, dA, X)
    lo, wlo = lo.cpu().numpy(), wlo.cpu().numpy()
    assert lo.min() >= 0 and lo.max() <= n_a - 2 and wlo.min() >= 0.0 and wlo.max() <= 1.0
    op = np.concatenate(dA)                                    # [2(T+1)][n_cal][S][n_a]
    raw = a_star[None] + np.einsum("kcsj,cpk->pcsj", op, X)
    mag = np.abs(a_star)[None] + np.einsum("kcsj,cpk->pcsj", np.abs(op), np.abs(X))
    ref = np.clip(raw, aGrid[None, :, None, :1], aGrid[None, :, None, -1:])
    g = np.broadcast_to(aGrid[None, :, None, :], lo.shape)
    mean = wlo * np.take_along_axis(g, lo, axis=-1) + (1.0 - wlo) * np.take_along_axis(g, lo + 1, axis=-1)
    bound = (2 * (T + 1) + 4) * 2.0 ** -53 * mag + 2.0 * np.spacing(ref)
    worst = float(np.max(np.abs(mean - ref) / bound))
    clamped = float(np.mean((raw < aGrid[0, 0]) | (raw > aGrid[0, -1])))
    print(f"S={S} n_a={n_a} T={T} n_p={n_p}: worst |mean - a'| / bound {worst:.2e}, {clamped:.1%} clamped")
    assert worst <= 1.0


def test_synthesis_clamps_exactly(gpu):
    """Rows pushed below a_0 and above a_last by a large X: (lo, wlo) = (0, 1) and (n_a - 2, 0)."""
    n_cal, S, n_a, T = 2, 7, 120, 5
    aGrid, a_star, dA, X = synthetic_operands(np.random.default_rng(7), n_cal, S, n_a, T, 3)
    dA[0][0] = 1.0
    X[:, 0, 0], X[:, 2, 0] = -1e3, 1e3
    lo, wlo = synthesise(gpu, aGrid, a_star, dA, X)
    assert bool((lo[0] == 0).all()) and bool((wlo[0] == 1.0).all())
    assert bool((lo[2] == n_a - 2).all()) and bool((wlo[2] == 0.0).all())
    assert int(lo[1].min()) < int(lo[1].max())   # the period between them is an ordinary one


def test_synthesis_bits_do_not_depend_on_the_batch(gpu):
    """Period p of an n_p = 65 call equals the n_p = 1 call on that period's X row, and
    calibration 1 of the batch equals the same calibration alone (torch.equal on lo and wlo)."""
    import torch
    n_cal, S, n_a, T, n_p = 2, 7, 1000, 40, 65
    aGrid, a_star, dA, X = synthetic_operands(np.random.default_rng(8), n_cal, S, n_a, T, n_p)
    aGrid[1] *= 1.25
    a_star[1] *= 1.25
    lo, wlo = synthesise(gpu, aGrid, a_star, dA, X)
    for p in (0, 15, 16, 33, 63, 64):
        lo1, wlo1 = synthesise(gpu, aGrid, a_star, dA, X[:, p:p + 1])
        assert torch.equal(lo1[0], lo[p]) and torch.equal(wlo1[0], wlo[p])
    lo_c, wlo_c = synthesise(gpu, aGrid[1:], a_star[1:], [d[:, 1:] for d in dA], X[1:])
    assert torch.equal(lo_c[:, 0], lo[:, 1]) and torch.equal(wlo_c[:, 0], wlo[:, 1])
    lo_r, wlo_r = synthesise(gpu, aGrid, a_star, dA, X)   # and a second run has the same bits
    assert torch.equal(lo_r, lo) and torch.equal(wlo_r, wlo)


def test_synthesis_argument_checks(gpu):
    """n_p < 1, T < 1 and null buffers return -1 with the outputs untouched."""
    import torch

    from aiyagari_hark_amd import _lib
    n_cal, S, n_a, T, n_p = 2, 7, 120, 5, 3
    aGrid, a_star, dA, X = synthetic_operands(np.random.default_rng(9), n_cal, S, n_a, T, n_p)
    d = dict(a_star=up(gpu, a_star), dA_R=up(gpu, dA[0]), dA_w=up(gpu, dA[1]), X=up(gpu, X), a=up(gpu, aGrid))
    lo = torch.full((n_p, n_cal, S, n_a), -7, dtype=torch.int32, device=gpu)
    wlo = torch.full((n_p, n_cal, S, n_a), -7.0, dtype=torch.float64, device=gpu)
    h = _lib.handle(gpu.index)

    def call(T=T, n_p=n_p, n_a=n_a, S=S, **null):
        p = {k: (None if k in null else _lib.ptr(v)) for k, v in d.items()}
        return h.lib.aiy_aggregate_lotteries(h.h, n_cal, S, n_a, T, n_p, p["a_star"], p["dA_R"], p["dA_w"], p["X"], p["a"],
                                             None if "lo" in null else _lib.ptr(lo),
                                             None if "wlo" in null else _lib.ptr(wlo), _lib.stream_ptr())
    assert call(n_p=0) == -1 and call(n_p=-3) == -1 and call(T=0) == -1 and call(n_a=1) == -1 and call(S=65) == -1
    for name in ("a_star", "dA_R", "dA_w", "X", "a", "lo", "wlo"):
        assert call(**{name: True}) == -1
        assert b"null" in h.lib.aiy_last_error(h.h)
    assert h.lib.aiy_lottery_mean(h.h, n_cal, S, n_a, 0, _lib.ptr(lo), _lib.ptr(wlo), _lib.ptr(d["a"]), _lib.ptr(wlo),
                                  _lib.stream_ptr()) == -1
    assert h.lib.aiy_lottery_mean(h.h, n_cal, S, n_a, n_p, _lib.ptr(lo), None, _lib.ptr(d["a"]), _lib.ptr(wlo),
                                  _lib.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((lo == -7).all()) and bool((wlo == -7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert int(lo.min()) >= 0 and float(wlo.min()) >= 0.0


# -------------------------------------------------------------------------------------
# policy_jacobian
# -------------------------------------------------------------------------------------
def test_policy_jacobian_matches_reference(ss120, jac120, pol120, ref120):
    """a* and dA_x of [A, B, C, D] at n_a = 120, T = 40 against tests/aggregate_ref.py on the
    GPU's steady state.  dA_x: the gap measured on the MI355X on first run times 10, as a
    fraction of max |dA_x| (the rounding of a lottery mean is divided by h = 1e-5) -- measured:
    dA_R 4.4e-11 (max |dA_R| = 48.6), dA_w 1.32e-9 (max |dA_w| = 1.6; calibration D: 0 for both).
    a*: the rounding of a lottery mean (measured: identical).  Then the first row of the
    fake-news matrices: sum mass dA_x[u] = F^x[0][u] of the device Jacobian to 1e-9 absolute
    (measured: at most 3.5e-11 on a scale of 7.3)."""
    batch, _, _ = ss120
    a_star, dA = pol120.a_star.cpu().numpy(), (pol120.dA_R.cpu().numpy(), pol120.dA_w.cpu().numpy())
    assert dA[0].shape == (T_PATH + 1, 4, batch.S, batch.n_a) and pol120.h == H
    mass = batch.mass.cpu().numpy()
    for i, (hs, pol, _) in enumerate(ref120):
        e_a = np.max(np.abs(a_star[i] - pol["a_star"])) / np.max(np.abs(pol["a_star"]))
        print(f"cal {i}: max|a* - ref| / max|a*| = {e_a:.2e}")
        assert e_a <= TOL_A_STAR
        for x, name in enumerate(("R", "w")):
            ref = pol["dA_" + name]
            e_d = np.max(np.abs(dA[x][:, i] - ref)) / np.max(np.abs(ref))
            row = np.einsum("sj,usj->u", mass[i], dA[x][:, i])
            F = (jac120.FR, jac120.Fw)[x][i, 0]
            e_f = np.max(np.abs(row - F))
            print(f"cal {i} dA_{name}: max|d - ref| / max|d| = {e_d:.2e}  max|dA_{name}| = {np.max(np.abs(ref)):.2e}  "
                  f"first row gap {e_f:.2e} on {np.max(np.abs(F)):.2e}")
            assert e_d <= TOL_DA
            assert e_f <= 1e-9


def test_household_jacobian_is_unchanged_by_policy_jacobian(ss120, jac120, pol120):
    """household_jacobian before and after a policy_jacobian call returns identical arrays."""
    from aiyagari_hark_amd.aggregate import policy_jacobian
    from aiyagari_hark_amd.transition import household_jacobian
    batch, r, _ = ss120
    again = policy_jacobian(batch, r, T_PATH, h=H)
    import torch
    assert torch.equal(again.dA_R, pol120.dA_R) and torch.equal(again.dA_w, pol120.dA_w)
    assert torch.equal(again.a_star, pol120.a_star)
    after = household_jacobian(batch, r, T_PATH, h=H)
    for name in ("JR", "Jw", "FR", "Fw", "K"):
        assert np.array_equal(getattr(after, name), getattr(jac120, name))


# -------------------------------------------------------------------------------------
# simulate
# -------------------------------------------------------------------------------------
def test_zero_shocks_stay_at_the_steady_state(ss120, pol120, model120):
    from aiyagari_hark_amd.aggregate import AggregateSimulation, simulate
    batch, _, _ = ss120
    sim = simulate(batch, model120, pol120, np.zeros(10))
    assert isinstance(sim, AggregateSimulation) and sim.K.shape == (4, 11) and sim.C.shape == (4, 10)
    err = np.max(np.abs(sim.K - model120.K[:, None]), axis=1) / model120.K
    print("zero shocks: max |K - K*| / K*", err)
    assert np.all(err <= 1e-8)
    assert np.all(sim.Z == 1.0) and np.array_equal(sim.gap, err) and sim.stats is None


def test_single_innovation_is_the_impulse_response_to_second_order(ss120, jac120, pol120, model120):
    from aiyagari_hark_amd.aggregate import ar1, simulate
    from aiyagari_hark_amd.transition import impulse_response
    batch, _, _ = ss120
    dK, _, _ = impulse_response(batch, jac120, ar1(RHO, T_PATH))
    err = {}
    for size in (1e-2, 1e-3):
        eps = np.zeros(T_PATH)
        eps[0] = size
        sim = simulate(batch, model120, pol120, eps, want_c=False)
        err[size] = np.max(np.abs(sim.K - model120.K[:, None] - size * dK), axis=1) / model120.K
        assert sim.C is None
    scale = np.max(np.abs(1e-3 * dK), axis=1) / model120.K
    print("err(1e-2)", err[1e-2], "err(1e-3)", err[1e-3], "response at 1e-3", scale)
    assert np.all(err[1e-3] <= err[1e-2] / 50.0)
    assert np.all(err[1e-3] <= 1e-3 * scale)


@pytest.fixture(scope="module")
def stochastic(ss120, pol120, model120):
    """60 periods at sigma = 0.007, seed 0, chunk 16, percentiles 0.5 and 0.9."""
    from aiyagari_hark_amd.aggregate import simulate
    eps = 0.007 * np.random.default_rng(0).standard_normal(60)
    return eps, simulate(ss120[0], model120, pol120, eps, chunk=16, percentiles=[0.5, 0.9])


def test_stochastic_run_matches_reference(ss120, pol120, model120, ref120, stochastic):
    """K, C and the Gini path of 60 periods against aggregate_ref.simulate fed the device's
    policy derivatives' reference twin (its own a*, dA from the same host state).  Tolerances:
    the gaps measured on the MI355X on first run times 10 -- measured: K 3.31e-13 and C 3.40e-13
    relative, Gini 5.89e-13 absolute (calibration D: 3e-16, 3e-16, 8e-16).  |sum mass - 1| <= 1e-11, and K[:, 0] is K* (to the rounding of two
    orders of summing 840 terms, 1e-13 relative)."""
    eps, sim = stochastic
    assert sim.K.shape == (4, 61) and sim.C.shape == (4, 60) and sim.stats.gini.shape == (4, 61)
    assert sim.stats.percentile_values.shape == (4, 61, 2)
    mass = sim.mass.cpu().numpy()
    assert np.all(np.abs(mass.sum(axis=(1, 2)) - 1.0) <= 1e-11)
    assert np.all(np.abs(sim.K[:, 0] - model120.K) <= 1e-13 * model120.K)
    from aiyagari_hark_amd.aggregate import simulate
    still = simulate(ss120[0], model120, pol120, np.zeros(1), want_c=False)   # the forward sweep's own sum of the steady mass
    assert np.array_equal(sim.K[:, 0], still.K[:, 0])
    for i, (hs, pol, model) in enumerate(ref120):
        ref = AR.simulate(hs, model, pol, eps)
        assert ref["monotone"]
        e_K = np.max(np.abs(sim.K[i] - ref["K"]) / ref["K"])
        e_C = np.max(np.abs(sim.C[i] - ref["C"]) / ref["C"])
        gini = np.array([DR.gini(g, hs["aGrid"]) for g in ref["marg"]])
        e_G = np.max(np.abs(sim.stats.gini[i] - gini))
        print(f"cal {i}: K rel {e_K:.2e}  C rel {e_C:.2e}  Gini abs {e_G:.2e}  gap {sim.gap[i]:.2e} "
              f"(reference {ref['gap']:.2e})  sd(K)/K* {np.std(sim.K[i]) / model['K']:.2e}")
        assert np.allclose(sim.Z[i], ref["Z"], rtol=1e-14, atol=0) and np.allclose(sim.K_lin[i], ref["K_lin"], rtol=1e-14)
        assert np.allclose(sim.r[i], ref["r"], rtol=1e-13, atol=0) and np.allclose(sim.w[i], ref["w"], rtol=1e-13, atol=0)
        assert e_K <= TOL_SIM_K and e_C <= TOL_SIM_C and e_G <= TOL_SIM_GINI


def test_chunking_does_not_change_a_bit(ss120, pol120, model120, stochastic):
    """chunk = 7 and chunk = 60 give K, C and the final mass bit for bit equal to chunk = 16."""
    import torch

    from aiyagari_hark_amd.aggregate import simulate
    eps, sim = stochastic
    for chunk in (7, 60):
        other = simulate(ss120[0], model120, pol120, eps, chunk=chunk)
        assert np.array_equal(other.K, sim.K) and np.array_equal(other.C, sim.C)
        assert torch.equal(other.mass, sim.mass)


def test_simulation_on_a_500_point_grid(gpu):
    """[A, B, C, D] at n_a = 500, the finest grid of DESIGN.md §4p's sweep on which the linearised
    policies keep every row monotone at sigma = 0.007: 64 periods at T = 40 in chunks of 64 and of
    24 run, with the same bits; mass stays 1 to 1e-11; without shocks K stays at K* to 1e-8; and a
    single innovation of 1e-3 is the impulse response to 1e-3 of its size (the bounds of the
    n_a = 120 tests)."""
    import torch

    from aiyagari_hark_amd.aggregate import ar1, linear_model, policy_jacobian, simulate
    from aiyagari_hark_amd.stationary import Calibration
    from aiyagari_hark_amd.transition import household_jacobian, steady_state
    batch, r, _ = steady_state([Calibration(**k) for k in (A, B, C, D)], 500, device=gpu)
    jac = household_jacobian(batch, r, T_PATH, h=H)
    model = linear_model(batch, jac, ar1(RHO, T_PATH))
    pol = policy_jacobian(batch, r, T_PATH, h=H)
    eps = 0.007 * np.random.default_rng(0).standard_normal(64)
    sim = simulate(batch, model, pol, eps, chunk=64, percentiles=[0.5, 0.9])
    other = simulate(batch, model, pol, eps, chunk=24)
    assert np.array_equal(other.K, sim.K) and np.array_equal(other.C, sim.C) and torch.equal(other.mass, sim.mass)
    assert np.all(np.abs(sim.mass.cpu().numpy().sum(axis=(1, 2)) - 1.0) <= 1e-11)
    assert np.all(np.isfinite(sim.stats.gini)) and np.all(sim.C > 0)
    still = simulate(batch, model, pol, np.zeros(10), want_c=False)
    drift = np.max(np.abs(still.K - model.K[:, None]), axis=1) / model.K
    one = np.zeros(T_PATH)
    one[0] = 1e-3
    err = simulate(batch, model, pol, one, want_c=False).gap
    scale = np.max(np.abs(1e-3 * model.dK), axis=1) / model.K
    print("n_a=500: gap", sim.gap, "drift", drift, "err(1e-3)", err, "response", scale)
    assert np.all(drift <= 1e-8) and np.all(err <= 1e-3 * scale)


def test_a_shock_too_large_is_refused(ss120, pol120, model120):
    """A PolicyJacobian whose dA turns one row's a' around (decreasing in assets) makes simulate
    raise the forward sweep's AIY_ERR_UNSUPPORTED from its row check."""
    import torch

    from aiyagari_hark_amd._lib import AiyagariLibError
    from aiyagari_hark_amd.aggregate import PolicyJacobian, simulate
    batch, _, _ = ss120
    eps = np.array([0.01, 0.0, 0.0])
    x0 = model120.dr[1, 0] * eps[0]          # the realised dR of period 0 in calibration 1
    dA_R, dA_w = torch.zeros_like(pol120.dA_R), torch.zeros_like(pol120.dA_w)
    row = pol120.a_star[1, 3]
    dA_R[0, 1, 3] = (row.flip(0) - row) / x0
    bad = PolicyJacobian(a_star=pol120.a_star, dA_R=dA_R, dA_w=dA_w, h=H)
    with pytest.raises(AiyagariLibError) as info:
        simulate(batch, model120, bad, eps)
    assert "AIY_ERR_UNSUPPORTED" in str(info.value) and "monotone" in str(info.value)
    good = PolicyJacobian(a_star=pol120.a_star, dA_R=torch.zeros_like(dA_R), dA_w=dA_w, h=H)
    assert np.all(simulate(batch, model120, good, eps).gap < 1e-2)   # the steady policy in every period still runs
