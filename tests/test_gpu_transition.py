"""GPU tests of the perfect-foresight transition path (csrc/transition.hip,
aiyagari_hark_amd/transition.py) against the existing entry points (bit for bit) and the NumPy
reference tests/transition_ref.py.  The reference is always fed the GPU's own steady-state
tables and mass, so only the new code is compared."""
import ctypes
import types

import numpy as np
import pytest

from oracle import stationary as ST
from tests import transition_ref as TR

pytestmark = pytest.mark.gpu

A = dict(LaborAR=0.9, LaborSD=0.4, CRRA=3.0)
B = dict(LaborAR=0.6, LaborSD=0.2, CRRA=3.0)
C = dict(LaborAR=0.3, LaborSD=0.4, CRRA=5.0)
D = dict(LaborAR=0.6, LaborSD=0.2, CRRA=1.0)
R25 = dict(LaborAR=0.9, LaborSD=0.4, CRRA=5.0, LaborStatesNo=25, income="rouwenhorst")
ALPHA, DELTA = 0.36, 0.08


def host_state(batch, K):
    """The GPU steady state on the host: per calibration the inputs of the reference."""
    m, c = (t.cpu().numpy()[:, :, 0, :] for t in batch.last_tables)
    mass = batch.mass.cpu().numpy()
    return [dict(aGrid=batch.aGrid[i], lab=batch.levels[i], P=batch.P[i], beta=batch.cals[i].DiscFac,
                 crra=batch.cals[i].CRRA, m=m[i], c=c[i], mass=mass[i], K=K[i]) for i in range(len(batch.cals))]


@pytest.fixture(scope="module")
def ss120(gpu):
    """[A, B, C, D] at n_a = 120: (batch, r*, K*)."""
    from aiyagari_hark_amd.stationary import Calibration
    from aiyagari_hark_amd.transition import steady_state
    return steady_state([Calibration(**k) for k in (A, B, C, D)], 120, device=gpu)


@pytest.fixture(scope="module")
def ss25(gpu):
    """[R25, R25] at n_a = 1000 (the second one gets another price path)."""
    from aiyagari_hark_amd.stationary import Calibration
    from aiyagari_hark_amd.transition import steady_state
    return steady_state([Calibration(**R25), Calibration(**R25)], 1000, device=gpu)


def pick(ss, idx):
    from aiyagari_hark_amd.transition import select
    batch, r, K = ss
    return select(batch, idx), r[idx], K[idx]


def wiggle_prices(K, T):
    """Prices of a capital path +-1 % around K*, another phase per calibration."""
    from aiyagari_hark_amd.transition import path_prices
    n = len(K)
    t = np.arange(T + 1)
    Kp = K[:, None] * (1.0 + 0.01 * np.cos(0.9 * t[None, :] + 1.3 * np.arange(n)[:, None]))
    Z = np.broadcast_to(TR.shock_path(T), (n, T + 1))
    r, w = path_prices(Kp, Z, np.full(n, ALPHA), np.full(n, DELTA))
    return 1.0 + r, w


def shapes(ss120, ss25):
    return [pick(ss120, [0, 2, 3]) + (5,), pick(ss120, [0, 2, 3]) + (1,), pick(ss25, [0, 1]) + (3,)]


def chained(batch, R, w, m_term, c_term, T):
    """The backward sweep from the existing entry points: aiy_egm_step (n_M = 1) and
    aiy_hist_lottery with every period's prices."""
    import torch

    from aiyagari_hark_amd import _lib
    from aiyagari_hark_amd.egm import EgmBatch, egm_step
    dev = batch.device
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    m = [None] * (T + 1)
    c = [None] * (T + 1)
    m[T], c[T] = m_term, c_term
    for u in range(T, 0, -1):
        Rn = torch.as_tensor(np.repeat(R[:, u, None, None], S, axis=2)).to(dev)
        Wn = torch.as_tensor(np.repeat(w[:, u, None, None], S, axis=2)).to(dev)
        eb = EgmBatch(batch.d_a, torch.zeros((n_cal, 1), dtype=torch.float64, device=dev), batch.d_P, Rn, Wn,
                      torch.zeros_like(Rn), batch.d_lab, batch.d_beta, batch.d_crra)
        m[u - 1], c[u - 1] = egm_step(eb, m[u], c[u])
    h = _lib.handle(dev.index)
    lo = torch.empty((T, n_cal, S, n_a), dtype=torch.int32, device=dev)
    wlo = torch.empty((T, n_cal, S, n_a), dtype=torch.float64, device=dev)
    for t in range(T):
        dR = torch.as_tensor(np.ascontiguousarray(R[:, t])).to(dev)
        dw = torch.as_tensor(np.ascontiguousarray(w[:, t])).to(dev)
        h.check(h.lib.aiy_hist_lottery(h.h, n_cal, S, n_a, _lib.ptr(m[t]), _lib.ptr(c[t]), _lib.ptr(batch.d_a),
                                       _lib.ptr(dR), _lib.ptr(dw), _lib.ptr(batch.d_lab), _lib.ptr(lo[t]),
                                       _lib.ptr(wlo[t]), _lib.stream_ptr()), "aiy_hist_lottery")
    return m[0], c[0], lo, wlo


def test_backward_equals_existing_entry_points_bit_for_bit(ss120, ss25):
    """1: m0 / c0 and every lo[t], wlo[t] equal the chained aiy_egm_step + aiy_hist_lottery,
    zero tolerance (same helpers, no contraction).  T = 1 runs one step and the lottery-only
    launch."""
    import torch

    from aiyagari_hark_amd.transition import household_block
    for batch, _, K, T in shapes(ss120, ss25):
        R, w = wiggle_prices(K, T)
        m_term, c_term = batch.last_tables
        out = household_block(batch, R, w, m_term, c_term, batch.mass)
        m0, c0, lo, wlo = chained(batch, R, w, m_term, c_term, T)
        torch.cuda.synchronize()
        assert torch.equal(out.m0, m0[:, :, 0, :]) and torch.equal(out.c0, c0[:, :, 0, :])
        assert torch.equal(out.lo, lo) and torch.equal(out.wlo, wlo)
        assert bool(torch.all(torch.isfinite(out.wlo)))


def test_block_matches_reference(ss120, ss25):
    """2: Ks within 1e-10 relative and c_0 within 1e-8 relative of the NumPy block (the bounds
    of test_stationary_capital_supply_matches_oracle and the README).  C differs from the
    reference's only where the lottery clips a' onto the grid: the GPU sums q - (wlo a[lo] +
    (1 - wlo) a[lo + 1]), so |dC_t| <= sum mass_t |a' - clip(a')| (+ 1e-10 relative)."""
    from aiyagari_hark_amd.transition import household_block
    for batch, _, K, T in shapes(ss120, ss25):
        R, w = wiggle_prices(K, T)
        out = household_block(batch, R, w, *batch.last_tables, batch.mass)
        c0 = out.c0.cpu().numpy()
        lo = out.lo.cpu().numpy()
        for i, hs in enumerate(host_state(batch, K)):
            ref = TR.block(hs["aGrid"], hs["lab"], hs["P"], hs["beta"], hs["crra"], R[i], w[i], hs["m"], hs["c"],
                           hs["mass"], keep=True)
            e_K = np.max(np.abs(out.Ks[i] - ref["Ks"]) / ref["Ks"])
            e_c = np.max(np.abs(c0[i] - ref["c0"]) / np.abs(ref["c0"]))
            print(f"S={batch.S} n_a={batch.n_a} T={T} cal {i}: Ks rel {e_K:.2e}  c0 rel {e_c:.2e}")
            assert e_K <= 1e-10 and e_c <= 1e-8
            assert np.array_equal(lo[:, i], ref["lo"])
            aG = hs["aGrid"]
            for t in range(T):
                clip = np.sum(ref["mass"][t] * np.abs(ref["ap"][t] - np.clip(ref["ap"][t], aG[0], aG[-1])))
                assert abs(out.C[i, t] - ref["C"][t]) <= clip + 1e-10 * abs(ref["C"][t])


def synthetic_problem(rng, n_cal, S, n_a, T, variant):
    """A random monotone in-range lottery [T][n_cal][S][n_a], a stochastic P and a mass."""
    lo = np.sort(rng.integers(0, n_a - 1, size=(T, n_cal, S, n_a)), axis=-1)
    if variant == "head":       # the first min(500, n_a - 10) sources of one row share lo = 0
        lo[:, :, 0, :min(500, n_a - 10)] = 0
    elif variant == "tail":     # the last state's rows are all n_a - 2
        lo[:, :, S - 1, :] = n_a - 2
    wlo = rng.uniform(0.0, 1.0, size=lo.shape)
    P = rng.dirichlet(np.ones(S), size=(n_cal, S))
    mass = rng.uniform(0.0, 1.0, size=(n_cal, S, n_a))
    mass /= mass.sum(axis=(1, 2), keepdims=True)
    aGrid = np.broadcast_to(ST.make_stationary_grid(0.001, 50.0, n_a, 2), (n_cal, n_a)).copy()
    return lo, wlo, P, mass, aGrid


def forward_against_hist_step(dev, lo, wlo, P, mass0, aGrid, tag):
    import torch

    from aiyagari_hark_amd import _lib
    from aiyagari_hark_amd.transition import transition_forward
    T, n_cal, S, n_a = lo.shape
    up = lambda x, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(x)).to(dt).to(dev)  # noqa: E731
    fake = types.SimpleNamespace(cals=[None] * n_cal, S=S, n_a=n_a, device=dev, d_P=up(P), d_a=up(aGrid), d_lab=None)
    h = _lib.handle(dev.index)
    work = torch.empty(int(h.lib.aiy_transition_work_bytes(n_cal, S, n_a, T)), dtype=torch.uint8, device=dev)
    d_lo, d_wlo = up(lo, torch.int32), up(wlo)
    runs = []
    for _ in range(2):
        mass = up(mass0)
        Ks, _ = transition_forward(fake, d_lo, d_wlo, mass, T, work, want_c=False)
        runs.append((Ks, mass.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])   # 4: deterministic
    Ks, mT = runs[0]
    for i in range(n_cal):
        m = mass0[i].copy()
        Kr = [np.sum(m * aGrid[i][None, :])]
        for t in range(T):
            m = ST.hist_step(m, lo[t, i], wlo[t, i], P[i])
            Kr.append(np.sum(m * aGrid[i][None, :]))
        Kr = np.array(Kr)
        e_m = np.max(np.abs(mT[i] - m))
        e_K = np.max(np.abs(Ks[i] - Kr) / Kr)
        e_s = abs(mT[i].sum() - mass0[i].sum())
        print(f"{tag} cal {i}: mass_T abs {e_m:.2e}  Ks rel {e_K:.2e}  sum drift {e_s:.2e}")
        assert e_m <= 1e-12 and e_K <= 1e-10 and e_s < 1e-12


def test_forward_alone_matches_hist_step(gpu):
    """3 (and the forward half of 4): the forward sweep on lotteries uploaded from NumPy."""
    from aiyagari_hark_amd.stationary import Calibration
    from aiyagari_hark_amd.transition import path_prices, steady_state
    T = 5
    # the reference lotteries of B at n_a = 1000: destination 0 of state 0 has more than a wave of sources
    batch, r, K = steady_state([Calibration(**B)], 1000, device=gpu)
    hs = host_state(batch, K)[0]
    Kp = K[:, None] * (1.0 + 0.01 * np.cos(0.9 * np.arange(T + 1)))[None, :]
    rp, wp = path_prices(Kp, TR.shock_path(T)[None, :], np.full(1, ALPHA), np.full(1, DELTA))
    ref = TR.block(hs["aGrid"], hs["lab"], hs["P"], hs["beta"], hs["crra"], 1.0 + rp[0], wp[0], hs["m"], hs["c"],
                   hs["mass"])
    assert int(np.sum(ref["lo"][0, 0] == 0)) > 64
    forward_against_hist_step(gpu, ref["lo"][:, None], ref["wlo"][:, None], hs["P"][None], hs["mass"][None],
                              hs["aGrid"][None], "B n_a=1000")
    rng = np.random.default_rng(11)
    for S in (7, 25):
        for n_a in (120, 1000):
            for variant in ("head", "tail"):
                lo, wlo, P, mass, aGrid = synthetic_problem(rng, 2, S, n_a, T, variant)
                forward_against_hist_step(gpu, lo, wlo, P, mass, aGrid, f"{variant} S={S} n_a={n_a}")


def test_determinism_and_batch_independence(ss120):
    """4: two block evaluations are bit-identical, and each calibration of [A, C, D] gives
    bit-identical Ks solved in the batch and solved alone."""
    import torch

    from aiyagari_hark_amd.transition import household_block, select, solve_transition
    batch, _, K = pick(ss120, [0, 2, 3])
    R, w = wiggle_prices(K, 5)
    runs = []
    for _ in range(2):
        out = household_block(batch, R, w, *batch.last_tables, batch.mass)
        runs.append((out.Ks.copy(), out.C.copy(), out.lo.clone(), out.wlo.clone(), out.m0.clone(), out.c0.clone(),
                     out.mass_T.clone()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert all(torch.equal(x, y) for x, y in zip(runs[0][2:], runs[1][2:]))
    Z = TR.shock_path(5)
    together = solve_transition(batch, Z, 5, max_iter=3)
    for i in range(3):
        alone = solve_transition(select(batch, [i]), Z, 5, max_iter=3)
        assert np.array_equal(alone.K[0], together.K[i]) and np.array_equal(alone.C[0], together.C[i])
        assert alone.residual[0] == together.residual[i]


def test_bad_lottery_is_refused(ss120):
    """5: one decreasing pair (every entry still in [0, n_a - 2]) in one row of one period:
    AIY_ERR_UNSUPPORTED, Ks_out and mass unchanged, the error names the check."""
    import torch

    from aiyagari_hark_amd import _lib
    from aiyagari_hark_amd.transition import TransitionBuffers, household_block
    batch, _, K = pick(ss120, [0, 2, 3])
    T = 5
    R, w = wiggle_prices(K, T)
    buf = TransitionBuffers(batch, T)
    household_block(batch, R, w, *batch.last_tables, batch.mass, buffers=buf)
    lo = buf.lo.clone()
    row = lo[2, 1, 3]
    j = int(torch.nonzero(row >= 1)[0]) + 1          # lo[j - 1] >= 1: lo[j] = lo[j - 1] - 1 stays in range
    row[j] = row[j - 1] - 1
    assert int(lo.min()) >= 0 and int(lo.max()) <= batch.n_a - 2
    mass = batch.mass.clone()
    n_cal = len(batch.cals)
    Ks = np.full((n_cal, T + 1), -7.0)
    h = _lib.handle(batch.device.index)
    rc = h.lib.aiy_transition_forward(h.h, n_cal, batch.S, batch.n_a, T, _lib.ptr(lo), _lib.ptr(buf.wlo),
                                      _lib.ptr(batch.d_P), _lib.ptr(batch.d_a), None, None, None, _lib.ptr(buf.work),
                                      _lib.ptr(mass), Ks.ctypes.data_as(_lib.c_double_p), None, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -4 and _lib.ERRORS[rc] == "AIY_ERR_UNSUPPORTED"
    assert np.all(Ks == -7.0) and torch.equal(mass, batch.mass)
    assert b"monotone" in h.lib.aiy_last_error(h.h)
    # the untouched lottery still runs
    assert h.lib.aiy_transition_forward(h.h, n_cal, batch.S, batch.n_a, T, _lib.ptr(buf.lo), _lib.ptr(buf.wlo),
                                        _lib.ptr(batch.d_P), _lib.ptr(batch.d_a), None, None, None, _lib.ptr(buf.work),
                                        _lib.ptr(mass), Ks.ctypes.data_as(_lib.c_double_p), None,
                                        _lib.stream_ptr()) == 0
    assert np.all(Ks > 0)
    # argument checks run before any launch
    assert h.lib.aiy_transition_forward(h.h, n_cal, batch.S, batch.n_a, 0, _lib.ptr(buf.lo), _lib.ptr(buf.wlo),
                                        _lib.ptr(batch.d_P), _lib.ptr(batch.d_a), None, None, None, _lib.ptr(buf.work),
                                        _lib.ptr(mass), Ks.ctypes.data_as(_lib.c_double_p), None,
                                        _lib.stream_ptr()) == -1


def test_equilibrium_path(ss120):
    """6: [A, B, C], n_a = 120, T = 40, damping 0.5, tol 1e-9, max_iter 40 against the
    reference solve.  Two solves each within tol / (1 - 0.5) of the fixed point are within
    4e-9 of each other; the 1e-8 bound adds a 2.5x margin."""
    from aiyagari_hark_amd.transition import solve_transition
    batch, _, K = pick(ss120, [0, 1, 2])
    T = 40
    Z = TR.shock_path(T)
    res = solve_transition(batch, Z, T, damping=0.5, tol=1e-9, max_iter=40)
    assert np.all(res.status == 0) and np.all(res.residual < 1e-9)
    for i, hs in enumerate(host_state(batch, K)):
        ref = TR.solve(hs["aGrid"], hs["lab"], hs["P"], hs["beta"], hs["crra"], ALPHA, DELTA, Z, T, hs["m"], hs["c"],
                       hs["mass"], damping=0.5, tol=1e-9, max_iter=40)
        assert ref["status"] == 0
        d_K = np.max(np.abs(res.K[i] - ref["K"])) / K[i]
        rr, ww = TR.path_prices(res.K[i], Z, ALPHA, DELTA)
        blk = TR.block(hs["aGrid"], hs["lab"], hs["P"], hs["beta"], hs["crra"], 1.0 + rr, ww, hs["m"], hs["c"],
                       hs["mass"])
        resid = np.max(np.abs(blk["Ks"] - res.K[i])) / res.K[i, 0]
        dev = res.K[i] / K[i] - 1.0
        print(f"cal {i}: iterations {res.iterations[i]} (ref {ref['iterations']})  |K - K_ref| / K* {d_K:.2e}  "
              f"ref residual at K_gpu {resid:.2e}  peak {dev.max():.2e} at t = {int(dev.argmax())}")
        assert abs(int(res.iterations[i]) - ref["iterations"]) <= 1
        assert d_K <= 1e-8
        assert resid <= 2e-9
        assert 4e-3 <= dev.max() <= 1e-2 and 5 <= int(dev.argmax()) <= 12
        assert np.allclose(res.r[i], rr, rtol=0, atol=1e-15) and np.allclose(res.w[i], ww, rtol=1e-15, atol=0)


def test_non_convergence_is_reported_not_raised(ss120):
    """7: [A, D] with max_iter 8: D has status bit 1 and a finite path; A's path is
    bit-identical to A's first 8 iterations solved alone."""
    from aiyagari_hark_amd.transition import solve_transition
    T = 40
    Z = TR.shock_path(T)
    both, _, _ = pick(ss120, [0, 3])
    res = solve_transition(both, Z, T, damping=0.5, tol=1e-9, max_iter=8)
    assert res.status[1] & 1 and res.iterations[1] == 8
    assert np.all(np.isfinite(res.K[1])) and np.all(np.isfinite(res.C[1]))
    alone, _, _ = pick(ss120, [0])
    ra = solve_transition(alone, Z, T, damping=0.5, tol=1e-9, max_iter=8)
    assert np.array_equal(ra.K[0], res.K[0]) and ra.status[0] == res.status[0] == 1
    assert ra.residual[0] == res.residual[0]
