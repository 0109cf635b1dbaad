"""GPU tests of the sequence-space Jacobian (csrc/transition_jac.hip,
aiyagari_hark_amd/transition.py): every device stage against the existing entry points (bit
for bit) or NumPy, the assembled Jacobian against the fake-news reference
tests/jacobian_ref.py, and the Newton solve and the linear impulse response built on it.  The
reference is always fed the GPU's own steady-state tables and mass."""
import types

import numpy as np
import pytest

from oracle import stationary as ST
from tests import jacobian_ref as JR
from tests import transition_ref as TR
from tests.test_gpu_transition import A, ALPHA, B, C, D, DELTA, R25, host_state, pick, synthetic_problem

pytestmark = pytest.mark.gpu

T_PATH = 40
SYNTHETIC = [(S, n_a, variant) for S in (7, 25) for n_a in (120, 1000) for variant in ("head", "tail")]


@pytest.fixture(scope="module")
def ss120(gpu):
    """[A, B, C, D] at n_a = 120: (batch, r*, K*)."""
    from aiyagari_hark_amd.stationary import Calibration
    from aiyagari_hark_amd.transition import steady_state
    return steady_state([Calibration(**k) for k in (A, B, C, D)], 120, device=gpu)


@pytest.fixture(scope="module")
def jac120(ss120):
    """The Jacobian of [A, B, C, D] at T = 40, h = 1e-5."""
    from aiyagari_hark_amd.transition import household_jacobian
    batch, r, _ = ss120
    return household_jacobian(batch, r, T_PATH, h=1e-5)


def up(dev, x, dt=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(x))
    return (t if dt is None else t.to(dt)).to(dev)


def fake_batch(dev, P, aGrid, S, n_a):
    return types.SimpleNamespace(cals=[None] * P.shape[0], S=S, n_a=n_a, device=dev, d_P=up(dev, P), d_a=up(dev, aGrid),
                                 d_lab=None)


def jac_work(dev, n_cal, S, n_a, T):
    import torch

    from aiyagari_hark_amd import _lib
    h = _lib.handle(dev.index)
    return torch.empty(int(h.lib.aiy_jacobian_work_bytes(n_cal, S, n_a, T)), dtype=torch.uint8, device=dev)


@pytest.mark.parametrize("S,n_a,variant", SYNTHETIC)
def test_fanout_equals_single_forward_steps(gpu, S, n_a, variant):
    """1: every out[t] has the bits of aiy_transition_forward with T = 1 on that period's
    lottery, and is within 1e-12 of hist_step."""
    import torch

    from aiyagari_hark_amd import _lib
    from aiyagari_hark_amd.transition import jacobian_fanout, transition_forward
    n_t, n_cal = 5, 2
    lo, wlo, P, mass, aGrid = synthetic_problem(np.random.default_rng(11), n_cal, S, n_a, n_t, variant)
    fake = fake_batch(gpu, P, aGrid, S, n_a)
    d_lo, d_wlo, d_mass = up(gpu, lo, torch.int32), up(gpu, wlo), up(gpu, mass)
    out = torch.full((n_t, n_cal, S, n_a), -7.0, dtype=torch.float64, device=gpu)
    jacobian_fanout(fake, d_lo, d_wlo, d_mass, out, jac_work(gpu, n_cal, S, n_a, n_t - 1), n_t - 1)
    assert torch.equal(d_mass, up(gpu, mass))   # the source is read only
    h = _lib.handle(gpu.index)
    twork = torch.empty(int(h.lib.aiy_transition_work_bytes(n_cal, S, n_a, 1)), dtype=torch.uint8, device=gpu)
    host = out.cpu().numpy()
    for t in range(n_t):
        m1 = d_mass.clone()
        transition_forward(fake, d_lo[t:t + 1].contiguous(), d_wlo[t:t + 1].contiguous(), m1, 1, twork, want_c=False)
        assert torch.equal(out[t], m1)
        for i in range(n_cal):
            err = np.max(np.abs(host[t, i] - ST.hist_step(mass[i], lo[t, i], wlo[t, i], P[i])))
            assert err <= 1e-12


def test_fanout_refuses_a_bad_row(gpu):
    """1 (bad row): one decreasing pair in one row of one period: AIY_ERR_UNSUPPORTED, the
    outputs untouched, the error names the check; the untouched lottery still runs."""
    import torch

    from aiyagari_hark_amd import _lib
    n_t, n_cal, S, n_a = 5, 2, 7, 120
    lo, wlo, P, mass, aGrid = synthetic_problem(np.random.default_rng(12), n_cal, S, n_a, n_t, "head")
    bad = lo.copy()
    row = bad[2, 1, 3]
    j = int(np.flatnonzero(row >= 1)[0]) + 1
    row[j] = row[j - 1] - 1
    assert bad.min() >= 0 and bad.max() <= n_a - 2
    d_wlo, d_mass, d_P = up(gpu, wlo), up(gpu, mass), up(gpu, P)
    out = torch.full((n_t, n_cal, S, n_a), -7.0, dtype=torch.float64, device=gpu)
    work = jac_work(gpu, n_cal, S, n_a, n_t - 1)
    h = _lib.handle(gpu.index)

    def call(d_lo, T=n_t - 1, count=n_t):
        return h.lib.aiy_jacobian_fanout(h.h, n_cal, S, n_a, T, count, _lib.ptr(d_lo), _lib.ptr(d_wlo), _lib.ptr(d_P),
                                         _lib.ptr(d_mass), _lib.ptr(work), _lib.ptr(out), _lib.stream_ptr())
    rc = call(up(gpu, bad, torch.int32))
    torch.cuda.synchronize()
    assert rc == -4 and _lib.ERRORS[rc] == "AIY_ERR_UNSUPPORTED"
    assert bool(torch.all(out == -7.0))
    assert b"monotone" in h.lib.aiy_last_error(h.h)
    good = up(gpu, lo, torch.int32)
    assert call(good, count=n_t + 1) == -1 and call(good, T=0, count=1) == -1   # argument checks run before any launch
    assert bool(torch.all(out == -7.0))
    assert call(good) == 0
    torch.cuda.synchronize()
    assert bool(torch.all(out >= 0.0))


@pytest.mark.parametrize("S,n_a,variant", SYNTHETIC)
def test_expectation_matches_numpy_and_is_the_adjoint(gpu, S, n_a, variant):
    """2: E_k within 1e-12 relative of the NumPy recursion for 5 steps, and sum E_k mass =
    Ks[k] of a forward sweep on the repeated lottery to 1e-12 relative."""
    import torch

    from aiyagari_hark_amd import _lib
    from aiyagari_hark_amd.transition import jacobian_expectation, transition_forward
    steps, n_cal = 5, 2
    lo, wlo, P, mass, aGrid = synthetic_problem(np.random.default_rng(13), n_cal, S, n_a, 1, variant)
    lo, wlo = lo[0], wlo[0]
    fake = fake_batch(gpu, P, aGrid, S, n_a)
    d_lo, d_wlo = up(gpu, lo, torch.int32), up(gpu, wlo)
    E = torch.empty((steps + 1, n_cal, S, n_a), dtype=torch.float64, device=gpu)
    jacobian_expectation(fake, d_lo, d_wlo, E, jac_work(gpu, n_cal, S, n_a, steps + 1))
    E = E.cpu().numpy()
    h = _lib.handle(gpu.index)
    twork = torch.empty(int(h.lib.aiy_transition_work_bytes(n_cal, S, n_a, steps)), dtype=torch.uint8, device=gpu)
    rep = lambda x: x[None].expand(steps, *x.shape).contiguous()  # noqa: E731
    Ks, _ = transition_forward(fake, rep(d_lo), rep(d_wlo), up(gpu, mass), steps, twork, want_c=False)
    for i in range(n_cal):
        ref = np.broadcast_to(aGrid[i][None, :], (S, n_a)).copy()
        for k in range(steps + 1):
            err = np.max(np.abs(E[k, i] - ref) / np.abs(ref))
            adj = abs(np.sum(E[k, i] * mass[i]) - Ks[i, k]) / Ks[i, k]
            assert err <= 1e-12 and adj <= 1e-12, (k, err, adj)
            ref = JR.expectation_step(ref, lo[i], wlo[i], P[i])


@pytest.mark.parametrize("S,n_a", [(7, 120), (25, 1000), (7, 1301)])
@pytest.mark.parametrize("T", [1, 5, 17, 40])
def test_contraction_on_random_operands(gpu, T, S, n_a):
    """3: long index 840, 25 000 and 9107 = 2 chunks of 4096 + 915 (not divisible by 4).
    |F - F_numpy| <= 2 N 2^-53 (|E| |dD|^T) elementwise: the dot-product bound of any summation
    order, once for each side.  Two runs are bit-identical, and a calibration alone has the
    bits it has in the batch."""
    import torch

    from aiyagari_hark_amd.transition import jacobian_contract
    n_cal, N = 2, S * n_a
    rng = np.random.default_rng(1000 * T + S)
    E = rng.normal(size=(T, n_cal, S, n_a))
    dD = [rng.normal(size=(T + 1, n_cal, S, n_a)) for _ in range(2)]
    d_E, d_D = up(gpu, E), [up(gpu, x) for x in dD]
    work = jac_work(gpu, n_cal, S, n_a, T)
    runs = [jacobian_contract(gpu, d_E, d_D[0], d_D[1], work).cpu().numpy() for _ in range(2)]
    assert np.array_equal(runs[0], runs[1])
    F = runs[0]
    assert F.shape == (n_cal, T, 2 * (T + 1))
    worst = 0.0
    for i in range(n_cal):
        Ei = E[:, i].reshape(T, N)
        Di = np.concatenate([x[:, i].reshape(T + 1, N) for x in dD])
        bound = 2.0 * N * 2.0 ** -53 * (np.abs(Ei) @ np.abs(Di).T)
        err = np.abs(F[i] - Ei @ Di.T)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound)
        alone = jacobian_contract(gpu, d_E[:, i:i + 1].contiguous(), d_D[0][:, i:i + 1].contiguous(),
                                  d_D[1][:, i:i + 1].contiguous(), jac_work(gpu, 1, S, n_a, T)).cpu().numpy()
        assert np.array_equal(alone[0], F[i])
    print(f"T={T} N={N}: worst |F - F_numpy| / bound {worst:.2e}")


def check_against_reference(batch, r, K, jac, T, tag):
    for i, hs in enumerate(host_state(batch, K)):
        Rs, ws = JR.steady_prices(hs, ALPHA, DELTA, r[i])
        with np.errstate(all="ignore"):
            ref = JR.fake_news(hs, Rs, ws, T, jac.h)
        for name, mine, theirs in (("R", jac.JR[i], ref["JR"]), ("w", jac.Jw[i], ref["Jw"])):
            err = np.max(np.abs(mine - theirs)) / np.max(np.abs(theirs))
            print(f"{tag} cal {i} J^{name}: max|dJ| / max|J| = {err:.2e}")
            assert err <= 1e-5


def test_household_jacobian_matches_reference(ss120, jac120):
    """4: against the reference's fake-news J on [A, C, D] at n_a = 120, T = 40:
    max|dJ| / max|J| <= 1e-5, a tenth of the method's own 1e-4 budget against brute force (the
    device must add nothing material to it).  Measured: see DESIGN.md §4i."""
    from aiyagari_hark_amd.transition import HouseholdJacobian, household_jacobian
    idx = [0, 2, 3]
    batch, r, K = pick(ss120, idx)
    jac = household_jacobian(batch, r, T_PATH, h=1e-5)
    assert isinstance(jac, HouseholdJacobian) and jac.JR.shape == (3, T_PATH, T_PATH + 1) and jac.h == 1e-5
    for name in ("JR", "Jw", "FR", "Fw"):   # a calibration does not see its batch
        assert np.array_equal(getattr(jac, name), getattr(jac120, name)[idx])
    assert jac.capital_map().shape == (3, T_PATH, T_PATH)
    check_against_reference(batch, r, K, jac, T_PATH, "n_a=120 T=40")


def test_household_jacobian_matches_reference_25_states(gpu):
    """4: R25 (25 Rouwenhorst states) at n_a = 1000, T = 3, the same bound."""
    from aiyagari_hark_amd.stationary import Calibration
    from aiyagari_hark_amd.transition import household_jacobian, steady_state
    batch, r, K = steady_state([Calibration(**R25)], 1000, device=gpu)
    jac = household_jacobian(batch, r, 3, h=1e-5)
    check_against_reference(batch, r, K, jac, 3, "R25 n_a=1000 T=3")


def test_newton_converges_on_all_four(ss120, jac120):
    """5: [A, B, C, D], T = 40, tol 1e-9, max_iter 10: all converge (D cycles for ever under
    damping 0.5) within 6 evaluations; A, B, C within 1e-8 K* of the damped solution; the
    reference block's residual at the GPU path <= 2e-9 (test_equilibrium_path's bounds); a
    calibration solved alone has the bits it has in the batch."""
    from aiyagari_hark_amd.transition import select, solve_transition
    batch, r, K = ss120
    Z = TR.shock_path(T_PATH)
    res = solve_transition(batch, Z, T_PATH, tol=1e-9, max_iter=10, method="newton", jacobian=jac120)
    print("Newton iterations", res.iterations, "residuals", res.residual)
    assert np.all(res.status == 0) and np.all(res.residual < 1e-9)
    assert np.all(res.iterations <= 6)
    built = solve_transition(batch, Z, T_PATH, tol=1e-9, max_iter=10, method="newton")   # builds its own Jacobian
    assert np.all(built.status == 0) and np.all(built.iterations <= 6)
    damped = solve_transition(pick(ss120, [0, 1, 2])[0], Z, T_PATH, damping=0.5, tol=1e-9, max_iter=40)
    assert np.all(damped.status == 0)
    print("damped iterations", damped.iterations)
    for i, hs in enumerate(host_state(batch, K)):
        if i < 3:
            d_K = np.max(np.abs(res.K[i] - damped.K[i])) / K[i]
            print(f"cal {i}: |K_newton - K_damped| / K* {d_K:.2e}")
            assert d_K <= 1e-8
        rr, ww = TR.path_prices(res.K[i], Z, ALPHA, DELTA)
        with np.errstate(all="ignore"):
            blk = TR.block(hs["aGrid"], hs["lab"], hs["P"], hs["beta"], hs["crra"], 1.0 + rr, ww, hs["m"], hs["c"],
                           hs["mass"])
        resid = np.max(np.abs(blk["Ks"] - res.K[i])) / res.K[i, 0]
        print(f"cal {i}: ref residual at K_gpu {resid:.2e}")
        assert resid <= 2e-9
        alone = solve_transition(select(batch, [i]), Z, T_PATH, tol=1e-9, max_iter=10, method="newton")
        assert np.array_equal(alone.K[0], built.K[i]) and np.array_equal(alone.C[0], built.C[i])
        assert alone.residual[0] == built.residual[i] and alone.iterations[0] == built.iterations[i]


def test_impulse_response_is_the_first_order_term(ss120, jac120):
    """6: the linear response against the Newton path, measured from the Z = 1 Newton path:
    <= 1e-6 K* at shock size 1e-3 and <= 1e-4 K* at 1e-2 (CPU worst cases 1.4e-7 and 1.4e-5:
    the 100x is the second-order term)."""
    from aiyagari_hark_amd.transition import impulse_response, solve_transition
    batch, r, K = ss120
    kw = dict(tol=1e-10, max_iter=10, method="newton", jacobian=jac120)
    base = solve_transition(batch, np.ones(T_PATH + 1), T_PATH, **kw)
    assert np.all(base.status == 0)
    for size, bound in ((1e-3, 1e-6), (1e-2, 1e-4)):
        Z = TR.shock_path(T_PATH, size=size)
        res = solve_transition(batch, Z, T_PATH, **kw)
        assert np.all(res.status == 0)
        dK, dr, dw = impulse_response(batch, jac120, Z - 1.0)
        assert dK.shape == dr.shape == dw.shape == (4, T_PATH + 1) and np.all(dK[:, 0] == 0.0)
        err = np.max(np.abs(res.K - base.K - dK), axis=1) / K
        print(f"shock {size:g}: |K_newton - K_base - dK| / K* {err}")
        assert np.all(err <= bound)
        # the linearised firm: dr, dw are the first-order prices of (dZ, dK)
        a = batch.alpha
        assert np.allclose(dr, (a * K ** (a - 1.0))[:, None] * (Z - 1.0) + (a * (a - 1.0) * K ** (a - 2.0))[:, None] * dK,
                           rtol=1e-9, atol=1e-15)
        assert np.allclose(dw, ((1.0 - a) * K ** a)[:, None] * (Z - 1.0) + (a * (1.0 - a) * K ** (a - 1.0))[:, None] * dK,
                           rtol=1e-9, atol=1e-15)


def test_default_method_is_the_damped_loop(ss120):
    """7: solve_transition without ``method`` is bit-identical to method="damped"."""
    from aiyagari_hark_amd.transition import solve_transition
    batch, _, _ = pick(ss120, [0, 3])
    Z = TR.shock_path(5)
    a = solve_transition(batch, Z, 5, max_iter=3)
    b = solve_transition(batch, Z, 5, max_iter=3, method="damped")
    for name in ("K", "r", "w", "C", "iterations", "residual", "status"):
        assert np.array_equal(getattr(a, name), getattr(b, name))
    with pytest.raises(ValueError):
        solve_transition(batch, Z, 5, method="secant")
