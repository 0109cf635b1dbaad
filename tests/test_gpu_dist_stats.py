"""GPU tests of the wealth statistics of histogram distributions and paths (csrc/dist_stats.hip,
aiy_transition_forward_marginals in csrc/transition.hip, stats.histogram_stats,
transition.path_wealth_stats) against the NumPy reference tests/dist_stats_ref.py.  The
reference is always fed the GPU's own masses, so only the new code is compared.

Bounds (those of tests/test_gpu_stats.py, where the device sums are chunk-ordered and NumPy's
sequential): Lorenz shares, Gini, mean and total 1e-10 relative, percentile values 1e-8 relative
with an equal NaN pattern, bottom share 1e-12 relative."""
import types

import numpy as np
import pytest

from oracle import stationary as ST
from tests import dist_stats_ref as DR
from tests import transition_ref as TR

pytestmark = pytest.mark.gpu

A = dict(LaborAR=0.9, LaborSD=0.4, CRRA=3.0)
B = dict(LaborAR=0.6, LaborSD=0.2, CRRA=3.0)
C = dict(LaborAR=0.3, LaborSD=0.4, CRRA=5.0)
D = dict(LaborAR=0.6, LaborSD=0.2, CRRA=1.0)
R25 = dict(LaborAR=0.9, LaborSD=0.4, CRRA=5.0, LaborStatesNo=25, income="rouwenhorst")
ALPHA, DELTA = 0.36, 0.08
PCT = np.linspace(0.01, 0.999, 15)      # the notebook's pctiles
RTOL = 1e-10
PCTL_RTOL_CUMSUM = 1e-8
BOTTOM_RTOL = 1e-12
FIELDS = ("lorenz", "percentile_values", "gini", "mean", "total", "bottom_share")


@pytest.fixture(scope="module")
def ss120(gpu):
    """[A, B, C, D] at n_a = 120: (batch, r*, K*)."""
    from aiyagari_hark_amd.stationary import Calibration
    from aiyagari_hark_amd.transition import steady_state
    return steady_state([Calibration(**k) for k in (A, B, C, D)], 120, device=gpu)


@pytest.fixture(scope="module")
def ss25(gpu):
    """[R25, R25] at n_a = 1000."""
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


def rel_err(dev, ref):
    """Largest relative error; NaN on both sides counts as equal, on one side as infinite."""
    dev, ref = np.asarray(dev, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert dev.shape == ref.shape, (dev.shape, ref.shape)
    nd, nr = np.isnan(dev), np.isnan(ref)
    if not np.array_equal(nd, nr):
        return np.inf
    ok = ~nr
    if not ok.any():
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs(dev[ok] - ref[ok]) / np.maximum(np.abs(ref[ok]), 1e-300)
    e[dev[ok] == ref[ok]] = 0.0
    return float(np.max(e))


def compare(ws, ref, tag):
    """ws: WealthStats of leading shape [n]; ref: dict of stacked reference arrays.  Prints
    every error before it asserts."""
    errs = {k: rel_err(getattr(ws, k), ref[k]) for k in FIELDS}
    print(tag + ": " + "  ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert np.array_equal(np.isnan(ws.percentile_values), np.isnan(ref["percentile_values"]))
    for k in ("lorenz", "gini", "mean", "total"):
        assert errs[k] <= RTOL, (tag, k, errs[k])
    assert errs["percentile_values"] <= PCTL_RTOL_CUMSUM, (tag, errs["percentile_values"])
    assert errs["bottom_share"] <= BOTTOM_RTOL, (tag, errs["bottom_share"])


def same_bits(x, y):
    return all(np.array_equal(getattr(x, k), getattr(y, k), equal_nan=True) for k in FIELDS)


def test_steady_states_match_reference(ss120, ss25):
    """1: batch_wealth_stats of both fixtures at the notebook's percentiles."""
    from aiyagari_hark_amd.stats import batch_wealth_stats
    for name, (batch, _, _) in (("n_a=120", ss120), ("n_a=1000", ss25)):
        ws = batch_wealth_stats(batch, PCT)
        mass = batch.mass.cpu().numpy()
        ref = [DR.dist_stats(mass[i], batch.aGrid[i], PCT) for i in range(len(batch.cals))]
        ref = {k: np.stack([r[k] for r in ref]) for k in FIELDS}
        assert ws.gini.shape == (len(batch.cals),) and ws.lorenz.shape == (len(batch.cals), PCT.size)
        compare(ws, ref, "steady state " + name)
        print("  gini", np.round(ws.gini, 4), "bottom share", np.round(ws.bottom_share, 4))
        if batch.n_a == 120:                                  # A and D: no NaN at the notebook's percentiles
            assert not np.any(np.isnan(ws.percentile_values[[0, 3]]))
        assert np.all((ws.gini > 0.05) & (ws.gini < 0.95))
        assert np.array_equal(ws.percentiles, PCT)


def synthetic_stack(rng, S, n_a):
    """[3][2][S][n_a] random masses: leading, interior and trailing runs of exact zeros, a point
    mass on one node and two plain ones; two grids [2][n_a]."""
    mass = rng.uniform(0.0, 1.0, size=(6, S, n_a))
    run = max(1, n_a // 4)
    mass[0, :, :run] = 0.0                                   # leading run
    if n_a > 2:
        mass[1, :, n_a // 3:n_a // 3 + run] = 0.0            # interior run
    mass[2, :, n_a - run:] = 0.0                             # trailing run
    node = n_a // 2
    mass[3, :, :node] = 0.0                                  # a point mass on one node
    mass[3, :, node + 1:] = 0.0
    mass /= mass.sum(axis=(1, 2), keepdims=True)
    grids = np.stack([ST.make_stationary_grid(0.001, 50.0, n_a, 2), 0.01 + 30.0 * np.linspace(0.0, 1.0, n_a) ** 2])
    return mass.reshape(3, 2, S, n_a), grids


@pytest.mark.parametrize("n_a", [2, 120, 257, 1000])
@pytest.mark.parametrize("S", [1, 7, 64])
def test_synthetic_stacks_match_reference(gpu, S, n_a):
    """2: the chunking (n_a below, at and above 256 threads, no multiple of them), the empty
    tail threads, the chunk-boundary Gini term and the tie rules of F on nodes without mass."""
    import torch

    from aiyagari_hark_amd.stats import histogram_stats
    rng = np.random.default_rng(1000 * S + n_a)
    mass, grids = synthetic_stack(rng, S, n_a)
    ws = histogram_stats(torch.as_tensor(mass).to(gpu), grids, PCT)
    assert ws.gini.shape == (3, 2) and ws.percentile_values.shape == (3, 2, PCT.size)
    flat = types.SimpleNamespace(**{k: getattr(ws, k).reshape((6,) + getattr(ws, k).shape[2:]) for k in FIELDS})
    ref = [DR.dist_stats(mass[i, k], grids[k], PCT) for i in range(3) for k in range(2)]
    ref = {k: np.stack([r[k] for r in ref]) for k in FIELDS}
    compare(flat, ref, f"S={S} n_a={n_a}")
    assert ref["gini"][3] == 0.0 and flat.gini[3] == 0.0      # the point mass
    # a host array and marginals given directly take the same path
    g = np.stack([DR.marginal(m) for m in mass.reshape(6, S, n_a)]).reshape(3, 2, n_a)
    assert same_bits(histogram_stats(g, torch.as_tensor(grids).to(gpu), PCT, marginal=True, device=gpu), ws)


def sweep(batch, buf, T, marg):
    """One forward sweep from batch.mass on the lotteries of buf: (Ks, C, mass_T)."""
    from aiyagari_hark_amd.transition import transition_forward
    mass = batch.mass.clone()
    Ks, C = transition_forward(batch, buf.lo, buf.wlo, mass, T, buf.work, buf.R, buf.w, want_c=True, marg=marg)
    return Ks, C, mass


def path_problem(batch, K, T):
    """Lotteries of a wiggled price path in fresh buffers (with the device prices attached)."""
    import torch

    from aiyagari_hark_amd.transition import TransitionBuffers, household_block
    R, w = wiggle_prices(K, T)
    buf = TransitionBuffers(batch, T)
    household_block(batch, R, w, *batch.last_tables, batch.mass, buffers=buf)
    buf.R = torch.as_tensor(np.ascontiguousarray(R)).to(batch.device)
    buf.w = torch.as_tensor(np.ascontiguousarray(w)).to(batch.device)
    return buf


def period_masses(batch, buf, T):
    """mass_0 .. mass_T by T successive aiy_transition_forward calls with T = 1."""
    from aiyagari_hark_amd.transition import transition_forward
    mass = batch.mass.clone()
    out = [mass.clone()]
    for t in range(T):
        transition_forward(batch, buf.lo[t:t + 1], buf.wlo[t:t + 1], mass, 1, buf.work, want_c=False)
        out.append(mass.clone())
    return out


def test_sweep_keeps_its_bits_and_path_stats_match_reference(ss120, ss25):
    """3 and 4: Ks, C and mass_T of the marginals entry equal aiy_transition_forward's bit for bit,
    marg[t] is the ascending-s sum of the period masses, and path_wealth_stats of the marginals
    matches the reference applied to those masses."""
    import torch

    from aiyagari_hark_amd.transition import path_wealth_stats
    for batch, _, K, T in shapes(ss120, ss25):
        n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
        buf = path_problem(batch, K, T)
        Ks0, C0, mT0 = sweep(batch, buf, T, None)
        marg = torch.full((T + 1, n_cal, n_a), -7.0, dtype=torch.float64, device=batch.device)
        Ks1, C1, mT1 = sweep(batch, buf, T, marg)
        assert np.array_equal(Ks0, Ks1) and np.array_equal(C0, C1) and torch.equal(mT0, mT1)
        masses = period_masses(batch, buf, T)
        assert torch.equal(masses[T], mT0)
        for t in range(T + 1):
            g = masses[t][:, 0].clone()
            for s in range(1, S):
                g = g + masses[t][:, s]
            assert torch.equal(marg[t], g), (T, t)
        ws = path_wealth_stats(batch, marg, PCT)
        assert ws.gini.shape == (n_cal, T + 1) and ws.lorenz.shape == (n_cal, T + 1, PCT.size)
        host = [m.cpu().numpy() for m in masses]
        for i in range(n_cal):
            ref = [DR.dist_stats(host[t][i], batch.aGrid[i], PCT) for t in range(T + 1)]
            ref = {k: np.stack([r[k] for r in ref]) for k in FIELDS}
            one = types.SimpleNamespace(**{k: getattr(ws, k)[i] for k in FIELDS})
            compare(one, ref, f"path S={S} n_a={n_a} T={T} cal {i}")
        assert np.max(np.abs(ws.mean * ws.total - Ks1) / Ks1) <= RTOL


def test_determinism_batch_and_slab_independence(ss120):
    """5: two runs are bit-identical; a calibration selected alone gives the bits it gives in the
    batch, marginals and every statistic; the slab size does not change a bit."""
    import torch

    from aiyagari_hark_amd.stats import histogram_stats
    from aiyagari_hark_amd.transition import household_block, path_wealth_stats, select
    batch, _, K = pick(ss120, [0, 2, 3])
    T = 5
    R, w = wiggle_prices(K, T)
    runs = []
    for _ in range(2):
        out = household_block(batch, R, w, *batch.last_tables, batch.mass, marginals=True)
        runs.append((out.marg.clone(), path_wealth_stats(batch, out.marg, PCT)))
    assert torch.equal(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1])
    marg, ws = runs[0]
    for i in range(3):
        sub = select(batch, [i])
        alone = household_block(sub, R[i:i + 1], w[i:i + 1], *sub.last_tables, sub.mass, marginals=True)
        assert torch.equal(alone.marg[:, 0], marg[:, i])
        wa = path_wealth_stats(sub, alone.marg, PCT)
        assert all(np.array_equal(getattr(wa, k)[0], getattr(ws, k)[i], equal_nan=True) for k in FIELDS)
    # 18 distributions on 3 grids: one per call, inside a round of the grids, a slab that is
    # cut down to whole rounds, the whole stack
    whole = histogram_stats(marg, batch.d_a, PCT, marginal=True, slab=marg.shape[0] * marg.shape[1])
    for slab in (1, 2, 4, 7):
        assert same_bits(histogram_stats(marg, batch.d_a, PCT, marginal=True, slab=slab), whole), slab
    assert same_bits(histogram_stats(marg, batch.d_a, PCT, marginal=True), whole)
    assert all(np.array_equal(np.swapaxes(getattr(whole, k), 0, 1), getattr(ws, k), equal_nan=True) for k in FIELDS)


def test_refusals(ss120):
    """6: a decreasing lottery row is refused with marg, mass, Ks and C untouched; a percentile of
    1.0 and 257 percentiles are refused before any device work."""
    import torch

    from aiyagari_hark_amd import _lib
    from aiyagari_hark_amd.stats import histogram_stats
    from aiyagari_hark_amd.transition import transition_forward
    batch, _, K = pick(ss120, [0, 2, 3])
    T = 5
    buf = path_problem(batch, K, T)
    lo = buf.lo.clone()
    row = lo[2, 1, 3]
    j = int(torch.nonzero(row >= 1)[0]) + 1          # lo[j - 1] >= 1: lo[j] = lo[j - 1] - 1 stays in range
    row[j] = row[j - 1] - 1
    assert int(lo.min()) >= 0 and int(lo.max()) <= batch.n_a - 2
    n_cal, n_a = len(batch.cals), batch.n_a
    mass = batch.mass.clone()
    marg = torch.full((T + 1, n_cal, n_a), -7.0, dtype=torch.float64, device=batch.device)
    Ks = np.full((n_cal, T + 1), -7.0)
    Cc = np.full((n_cal, T), -7.0)
    h = _lib.handle(batch.device.index)

    def call(lottery):
        return h.lib.aiy_transition_forward_marginals(
            h.h, n_cal, batch.S, n_a, T, _lib.ptr(lottery), _lib.ptr(buf.wlo), _lib.ptr(batch.d_P),
            _lib.ptr(batch.d_a), _lib.ptr(buf.R), _lib.ptr(buf.w), _lib.ptr(batch.d_lab), _lib.ptr(buf.work),
            _lib.ptr(mass), Ks.ctypes.data_as(_lib.c_double_p), Cc.ctypes.data_as(_lib.c_double_p), _lib.ptr(marg),
            _lib.stream_ptr())

    rc = call(lo)
    torch.cuda.synchronize()
    assert rc == -4 and _lib.ERRORS[rc] == "AIY_ERR_UNSUPPORTED"
    with pytest.raises(_lib.AiyagariLibError, match="monotone"):
        h.check(rc, "aiy_transition_forward_marginals")
    assert np.all(Ks == -7.0) and np.all(Cc == -7.0) and torch.equal(mass, batch.mass)
    assert bool(torch.all(marg == -7.0))
    with pytest.raises(_lib.AiyagariLibError):
        transition_forward(batch, lo, buf.wlo, mass, T, buf.work, buf.R, buf.w, marg=marg)
    assert bool(torch.all(marg == -7.0)) and torch.equal(mass, batch.mass)
    # the untouched lottery still runs
    assert call(buf.lo) == 0
    assert np.all(Ks > 0) and np.all(Cc > 0) and bool(torch.all(marg >= 0.0))

    # percentiles: the Python layer and the C entry both refuse
    for bad in ([0.5, 1.0], list(np.linspace(0.001, 0.999, 257))):
        with pytest.raises(ValueError):
            histogram_stats(batch.mass, batch.d_a, bad)
    g = marg[0].contiguous()
    work = torch.empty(int(h.lib.aiy_dist_stats_work_bytes(n_cal, n_a)), dtype=torch.uint8, device=batch.device)
    dp = _lib.c_double_p
    for pct, n_p, want in ((np.array([0.5, 1.0]), 2, -1), (np.array([0.0]), 1, -1),
                           (np.linspace(0.001, 0.999, 257), 257, -4)):
        out = np.full((3, n_cal, max(n_p, 4)), -7.0)
        rc = h.lib.aiy_dist_stats(h.h, n_cal, n_cal, n_a, _lib.ptr(g), _lib.ptr(batch.d_a), pct.ctypes.data_as(dp), n_p,
                                  _lib.ptr(work), out[0].ctypes.data_as(dp), out[1].ctypes.data_as(dp),
                                  out[2].ctypes.data_as(dp), _lib.stream_ptr())
        assert rc == want and np.all(out == -7.0)
    # n_p = 0: the summary alone
    summ = np.full((n_cal, 4), -7.0)
    assert h.lib.aiy_dist_stats(h.h, n_cal, n_cal, n_a, _lib.ptr(g), _lib.ptr(batch.d_a), None, 0, _lib.ptr(work),
                                None, None, summ.ctypes.data_as(dp), _lib.stream_ptr()) == 0
    assert np.all(np.abs(summ[:, 0] - 1.0) < 1e-9) and np.all((summ[:, 2] > 0.05) & (summ[:, 2] < 0.95))


def test_solve_transition_with_percentiles(ss120):
    """7: [A, B], T = 5, Newton: the path is the one solved without percentiles, stats[:, 0] is the
    steady state's, and mean x total is the final block's Ks."""
    from aiyagari_hark_amd.stats import batch_wealth_stats
    from aiyagari_hark_amd.transition import household_block, household_jacobian, solve_transition
    batch, r, _ = pick(ss120, [0, 1])
    T = 5
    Z = TR.shock_path(T)
    jac = household_jacobian(batch, r, T)
    plain = solve_transition(batch, Z, T, method="newton", jacobian=jac)
    res = solve_transition(batch, Z, T, method="newton", jacobian=jac, percentiles=PCT)
    assert plain.stats is None
    for k in ("K", "r", "w", "C", "iterations", "residual", "status"):
        assert np.array_equal(getattr(plain, k), getattr(res, k)), k
    assert res.stats.gini.shape == (2, 6) and res.stats.lorenz.shape == (2, 6, PCT.size)
    ss = batch_wealth_stats(batch, PCT)
    assert all(np.array_equal(getattr(res.stats, k)[:, 0], getattr(ss, k), equal_nan=True) for k in FIELDS)
    assert np.all(res.status == 0)
    last = household_block(batch, 1.0 + res.r, res.w, *batch.last_tables, batch.mass)
    e = np.max(np.abs(res.stats.mean * res.stats.total - last.Ks) / last.Ks)
    print(f"mean x total against the final block's Ks: {e:.1e}; gini path of A {np.round(res.stats.gini[0], 5)}")
    assert e <= RTOL
