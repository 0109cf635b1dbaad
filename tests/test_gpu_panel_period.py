"""GPU tests of ONE period of the agent panel on its three engines -- sim_period_kernel
(csrc/panel.hip), panel_block_kernel<2|4> (csrc/panel_block.hip) and the instantiations of
sim_resident_kernel (csrc/panel_resident.hip) -- against the scalar float64 reference of
tests/panel_ref.py: the labour draw, m = R a + W l, the merged-table lookup tab_policy_t with the
device index decode brk_slot / brk_resolve, a' = m - c, the mean and the price update.

Agents are placed through the market state: at Rnow = 1, Wnow = 0 the kernel's m is the asset
itself, so an agent sits on any chosen double -- every node of both rows, the doubles 1 to 5000
ulp either side, values in every kind of index bucket (tests/panel_ref.py names the path of each
query; tests/test_panel_ref.py asserts that every path is reached).  A second reset with generic
prices holds the m arithmetic.

Held bit for bit: the labour states and every agent's a' (values and NaN masks), on every engine,
count and option.  Two tolerances only:
  * hist_A[0] against the exactly rounded mean: (N - 1) 2^-53 sum|a'| / N, the worst case of any
    summation order (derived); the observed gaps are printed.
  * Mnow, Rnow, Wnow against calc_R_and_W in long double AT the device's own hist_A[0]: the
    kernels form K^al and K^(al - 1) from one exp(al log K) where the reference calls pow twice.
    Largest relative gaps measured on the MI355X over the 291 checked periods of this module on
    the first run: Mnow 2.374e-16 (block engine, N = 2049), Rnow 1.782e-16 (per-period engine,
    N = 5), Wnow 1.070e-15 (block engine, n_a = 2, K = 2.7e9 with the agents parked at 1e12:
    al log K = 7.8 carries its rounding into the exponent); the bound is ten times the largest
    (drift of the device math library), as in tests/test_gpu_egm_step.py.  Per engine: per-period
    2.27e-16 / 1.78e-16 / 1.06e-15, block 2.37e-16 / 1.64e-16 / 1.07e-15, resident 1.48e-16 /
    1.68e-16 / 7.85e-16.  The mean came within 2.1 % of its bound at the most (block engine).
Every a' and every labour state was bit-equal on the first run; so was the case of unequal first
nodes (test_unequal_first_nodes).
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import hark_ks as H
from oracle import philox as PX
from tests import panel_ref as PR

pytestmark = pytest.mark.gpu

# measured on the MI355X (first run of this module), relative to the long-double price update
PRICE_GAP_M, PRICE_GAP_R, PRICE_GAP_W = 2.374e-16, 1.782e-16, 1.070e-15
PRICE_TOL = 10 * max(PRICE_GAP_M, PRICE_GAP_R, PRICE_GAP_W)
assert PRICE_TOL <= 1e-13

GENERIC = (1.03, 1.2)     # Rnow, Wnow of the second reset
WORST = {}                # engine -> [sum gap / bound, price gaps M, R, W]


def dv(dev, x):
    import torch
    return torch.as_tensor(np.array(x, order="C")).to(dev)   # (a copy: the family's arrays are read-only)


class Rig:
    """A DevicePanel bound to one family member; every run starts from its own reset."""

    def __init__(self, dev, fam, N, engine, unemployed=False, agent_offset=0):
        from aiyagari_hark_amd.panel import DevicePanel
        self.dev, self.fam, self.N = dev, fam, N
        self.p = DevicePanel(N, device=dev, agent_offset=agent_offset, act_T=fam.mrkv_hist.size, engine=engine)
        self.p.bind_model(dv(dev, fam.m), dv(dev, fam.c), dv(dev, fam.Mgrid), dv(dev, fam.lvl), dv(dev, fam.cdf),
                          dv(dev, fam.mrkv_hist), PR.MARKET, unemployed=unemployed)

    def run(self, a0, lab0, U, sow0, emp=None, periods=1, **philox):
        """sow0 = (Mnow, Mrkv, Rnow, Wnow); U [periods][N] host uniforms (None: Philox)."""
        import torch
        Mnow, Mrkv, R, W = sow0
        self.p.reset(a0, lab0, Mnow, -1.0, Mrkv, R, W)
        if U is None:
            self.p.run(0, periods, shock_mode="philox", **philox)
        else:
            U = np.array(U, dtype=np.float64).reshape(-1, self.N)    # (copies: the cached cases are read-only)
            E = None if emp is None else np.array(np.broadcast_to(np.asarray(emp, dtype=np.uint8), U.shape))
            self.p.run(0, periods, shock_mode="numpy", u_host_source=lambda n: U[:n],
                       emp_source=None if E is None else (lambda n: E[:n]))
        torch.cuda.synchronize()
        return collect(self.p)


def collect(p, k=None):
    g = (lambda t: t.cpu().numpy()) if k is None else (lambda t: t[k].cpu().numpy())
    return dict(a=g(p.a), lab=g(p.lab), sow=g(p.sow), hist_A=g(p.hist_A), hist_M=g(p.hist_M))


def bits_equal(x, y):
    nx, ny = np.isnan(x), np.isnan(y)
    return np.array_equal(nx, ny) and np.array_equal(x[~nx].view(np.int64), y[~ny].view(np.int64))


def check(tag, engine, out, fam, a0, lab0, u, sow0, emp=None, fast=False, t=0, market=PR.MARKET, ref=None):
    """Hold one period's outcome to the reference.  Returns the reference (a', l')."""
    Mnow, Mrkv, R, W = sow0
    e = np.ones(len(a0), dtype=np.int64) if emp is None else np.asarray(emp, dtype=np.int64)
    if ref is None:
        ref = (PR.period_fast if fast else PR.period)(a0, lab0, e, u, R, W, Mnow, Mrkv, fam.lvl, fam.cdf, fam.m,
                                                      fam.c, fam.Mgrid)[:2]
    a_ref, l_ref = ref
    assert np.array_equal(out["lab"], l_ref), tag
    bad = np.flatnonzero(~((out["a"] == a_ref) | (np.isnan(out["a"]) & np.isnan(a_ref))))
    assert bits_equal(out["a"], a_ref), (tag, bad[:8], out["a"][bad[:8]], a_ref[bad[:8]])
    sow, K = out["sow"], out["hist_A"][t]
    nxt = int(fam.mrkv_hist[t])
    w = WORST.setdefault(engine, [0.0, 0.0, 0.0, 0.0])
    if np.isnan(a_ref).any():
        assert np.isnan(K) and np.isnan(out["hist_M"][t]) and np.isnan(sow[[0, 1, 3, 4]]).all(), tag
    else:
        assert K > 0
        gap, bound = abs(K - PR.mean_fsum(a_ref)), PR.sum_bound(a_ref)
        want = PR.prices_ld(K, nxt, market)
        pg = [PR.rel_gap_ld(sow[i], x) for i, x in zip((0, 3, 4), want)]
        print(f"{tag}: mean gap {gap:.3e} (bound {bound:.3e})  prices M {pg[0]:.3e} R {pg[1]:.3e} W {pg[2]:.3e}")
        if bound > 0:
            w[0] = max(w[0], gap / bound)
        for i in range(3):
            w[1 + i] = max(w[1 + i], pg[i])
        assert gap <= bound, (tag, gap, bound)
        assert max(pg) <= PRICE_TOL, (tag, pg)
        assert sow[1] == K and out["hist_M"][t] == sow[0], tag
    assert sow[2] == nxt and sow[5] == 0.0 and sow[7] == t + 1, (tag, sow)
    return ref


def report(engine):
    w = WORST.get(engine)
    if w:
        print(f"[{engine}] worst so far: mean gap / bound {w[0]:.3e}  price gaps M {w[1]:.3e} R {w[2]:.3e} "
              f"W {w[3]:.3e}")


def both_prices(rig, tag, engine, fam, Mnow, Mrkv, agents, emp=None):
    """The placed run (m == a) and the same agents at generic prices."""
    a0, lab0, u, _ = agents
    for R, W in ((1.0, 0.0), GENERIC):
        sow0 = (Mnow, Mrkv, R, W)
        check(f"{tag} R={R} W={W}", engine, rig.run(a0, lab0, u, sow0, emp), fam, a0, lab0, u, sow0, emp)
    report(engine)


def resident_periods(h):
    ms, n, p = ctypes.c_double(), ctypes.c_int64(), ctypes.c_int64()
    h.check(h.lib.aiy_panel_launch_stats(h.h, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(p), 0), "stats")
    return int(p.value)


# ---------------------------------------------------------------------------------------
# Lookup paths, index widths, below the grid
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_lab", (2, 7))
@pytest.mark.parametrize("n_a,octaves,n_M", PR.LOOKUP)
@pytest.mark.parametrize("engine", ("grid", "block"))
def test_lookup_paths(gpu, engine, n_a, octaves, n_M, n_lab):
    """One agent per query of the section-2 set, both Mrkv values; n_lab = 2 runs the block
    engine at 2 agents per lane, n_lab = 7 at 4."""
    for Mrkv in (0, 1):
        fam, Mnow, agents = PR.lookup_case(n_a, octaves, n_M, n_lab, Mrkv)
        N = agents[0].size
        assert (N <= 2048) if n_lab == 2 else (2048 < N <= 12288)
        rig = Rig(gpu, fam, N, engine)
        both_prices(rig, f"{engine} n_a={n_a} oct={octaves} n_M={n_M} n_lab={n_lab} Mrkv={Mrkv} N={N}", engine, fam,
                    Mnow, Mrkv, agents)


@pytest.mark.parametrize("n_a,n_M", PR.WIDTHS)
def test_index_widths(gpu, n_a, n_M):
    """lg changes between 16|17 (and at every power of two up to 4096|4097, where a one-node
    entry resolves exactly: w == shift); n_a = 2 is the ABI minimum."""
    fam, Mnow, Mrkv, agents = PR.width_case(n_a, n_M)
    N = agents[0].size
    for engine in ("grid", "block") if N <= 12288 else ("grid",):
        both_prices(Rig(gpu, fam, N, engine), f"{engine} n_a={n_a} n_M={n_M} N={N}", engine, fam, Mnow, Mrkv, agents)


@pytest.mark.parametrize("n_M", (1, 3))
@pytest.mark.parametrize("engine", ("grid", "block"))
def test_below_the_grid(gpu, engine, n_M):
    """Queries <= 0, 1e-9, 5e-8 and the double below the first node are NaN on both sides, the
    first node itself is not; the period's mean and prices are NaN."""
    fam = PR.Family(7, n_M, 32, 14)
    rng = np.random.default_rng([17, n_M])
    Mnow = fam.M_inside(1)
    per = [np.concatenate([PR.queries(*fam.rows(l, 1, 1, Mnow), rng, steps=(1,), n_rand=60), PR.queries_below()])
           for l in range(7)]
    a0, lab0, u, _ = PR.place(fam, per, rng)
    sow0 = (Mnow, 1, 1.0, 0.0)
    out = Rig(gpu, fam, a0.size, engine).run(a0, lab0, u, sow0)
    a_ref, _ = check(f"{engine} below n_M={n_M}", engine, out, fam, a0, lab0, u, sow0)
    assert np.isnan(a_ref).sum() == 7 * 6 and np.isnan(out["hist_A"][0])


@pytest.mark.parametrize("order", ((1e-7, 2e-7), (2e-7, 1e-7)))
@pytest.mark.parametrize("engine", ("grid", "block"))
def test_unequal_first_nodes(gpu, engine, order):
    """Two M rows whose first nodes differ: brk_resolve counts the lower bound below the first
    bucket from {min, max} of the rows' first nodes; agents at both and at their ulp neighbours.
    Between the two, and below, one row is NaN and so is the blend."""
    fam = PR.Family(2, 2, 32, 6, first=order)
    rng = np.random.default_rng(19)
    Mnow = fam.M_inside(1)
    foot = np.concatenate([PR.ulps(np.array([1e-7, 2e-7]), k) for k in (0, 1, -1, 3, -3, 100, -100)] +
                          [np.array([1.5e-7, 1e-3, 0.04])])
    per = [np.concatenate([PR.queries(*fam.rows(l, 0, 1, Mnow), rng, steps=(1,), n_rand=60), foot]) for l in range(2)]
    a0, lab0, u, _ = PR.place(fam, per, rng)
    sow0 = (Mnow, 0, 1.0, 0.0)
    out = Rig(gpu, fam, a0.size, engine).run(a0, lab0, u, sow0)
    a_ref, _ = check(f"{engine} first nodes {order}", engine, out, fam, a0, lab0, u, sow0)
    # NaN: everything below 2e-7 (10 of the 14 neighbours, and 1.5e-7)
    assert np.isnan(a_ref).sum() == 2 * 11 and not np.isnan(a_ref[a0 == 2e-7]).any()


# ---------------------------------------------------------------------------------------
# M bracket, labour draw, Krusell-Smith mode
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_M", (2, 3, 5))
@pytest.mark.parametrize("engine", ("grid", "block"))
def test_M_bracket(gpu, engine, n_M):
    """Mnow below, on and above the M grid: the bracket is clipped and alpha leaves [0, 1]."""
    fam = PR.Family(2, n_M, 33, 6)
    rng = np.random.default_rng([23, n_M])
    Mg = fam.Mgrid
    per = [np.concatenate([PR.queries(*fam.rows(l, 1, 1, fam.M_inside(j)), rng, steps=(1,), n_rand=80)
                           for j in sorted({1, n_M - 1})]) for l in range(2)]
    a0, lab0, u, _ = PR.place(fam, per, rng)
    rig = Rig(gpu, fam, a0.size, engine)
    Ms = [0.6 * Mg[0], Mg[0], fam.M_inside(n_M - 1), Mg[-1], 1.4 * Mg[-1]] + ([Mg[1], Mg[n_M - 2]] if n_M > 2 else [])
    for Mnow in Ms:
        for R, W in ((1.0, 0.0), GENERIC):
            sow0 = (float(Mnow), 1, R, W)
            check(f"{engine} n_M={n_M} Mnow={Mnow:.4g} R={R}", engine, rig.run(a0, lab0, u, sow0), fam, a0, lab0, u,
                  sow0)
    report(engine)


def draw_agents(fam, N, rng):
    """Uniforms on every CDF entry of the agent's row, the doubles next to them, 0 and the
    double below 1 (u < 1: the last entry, 1.0, is met from below only); tiled to N agents."""
    lab0, u = [], []
    for l in range(fam.n_lab):
        row = fam.cdf[l]
        us = np.concatenate([row, PR.ulps(row, 1), PR.ulps(row, -1), [0.0, np.nextafter(1.0, 0.0)]])
        us = us[us < 1.0]
        lab0.append(np.full(us.size, l))
        u.append(us)
    lab0, u = np.concatenate(lab0), np.concatenate(u)
    perm = rng.permutation(np.resize(np.arange(u.size), N))
    return np.exp(rng.uniform(np.log(0.05), np.log(40.0), N)), lab0[perm], u[perm]


@pytest.mark.parametrize("n_lab", (1, 7, 16))
@pytest.mark.parametrize("engine", ("grid", "block", "resident"))
def test_labour_draw_edges(gpu, engine, n_lab):
    """searchsorted(cdf[l], u, 'right') at u on a CDF entry; the resident kernel draws in
    draw_slice, the others in agent_step (csrc/panel_common.h)."""
    from aiyagari_hark_amd import _lib
    fam = PR.Family(n_lab, 2, 17, 6)
    rng = np.random.default_rng([29, n_lab])
    N = {"grid": 3001, "block": 3001, "resident": 65539}[engine]
    a0, lab0, u = draw_agents(fam, N, rng)
    sow0 = (fam.M_inside(1), 0) + GENERIC
    h = _lib.handle(gpu.index)
    before = resident_periods(h)
    out = Rig(gpu, fam, N, "grid" if engine == "resident" else engine).run(a0, lab0, u, sow0)
    assert resident_periods(h) - before == (1 if engine == "resident" else 0)
    check(f"{engine} draw n_lab={n_lab}", engine, out, fam, a0, lab0, u, sow0)
    want = H.draw_labor(lab0, u, fam.cdf)
    assert np.array_equal(out["lab"], want) and want.max() == n_lab - 1
    report(engine)


@pytest.mark.parametrize("n_a,octaves,n_M,n_lab", ((32, 14, 3, 7), (33, 6, 1, 2)))
@pytest.mark.parametrize("engine", ("grid", "block"))
def test_krusell_smith_mode(gpu, engine, n_a, octaves, n_M, n_lab):
    """Employment mixed per agent: the unemployed sub-states' own rows, and W (l 0) in m."""
    fam = PR.Family(n_lab, n_M, n_a, octaves)
    rng = np.random.default_rng([31, n_a, n_M])
    Mnow, Mrkv = fam.M_inside(1), 1
    assert not np.array_equal(fam.m[4 * 1 + 2 * Mrkv + 1], fam.m[4 * 1 + 2 * Mrkv])
    # queries of the employed and of the unemployed rows; an agent is either, whichever it sits on
    per = [np.concatenate([PR.queries(*fam.rows(l, Mrkv, e, Mnow), rng, steps=(1, 100), n_rand=100)
                           for e in (1, 0)]) for l in range(n_lab)]
    a0, lab0, u, tgt = PR.place(fam, per, rng)
    emp = rng.integers(0, 2, a0.size)
    rig = Rig(gpu, fam, a0.size, engine, unemployed=True)
    both_prices(rig, f"{engine} KS n_a={n_a} n_M={n_M}", engine, fam, Mnow, Mrkv, (a0, lab0, u, tgt), emp)


# ---------------------------------------------------------------------------------------
# Counts and dispatch edges
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def count_family(n_M=3):
    fam = PR.Family(7, n_M, 32, 14)
    Mnow = fam.M_inside(1)
    per = tuple(PR.queries(*fam.rows(l, 0, 1, Mnow), np.random.default_rng(37 + l)) for l in range(7))
    return fam, Mnow, per


def count_case(N, n_M=3):
    fam, Mnow, per = count_family(n_M)
    return fam, Mnow, PR.fill(fam, N, per, np.random.default_rng([41, N, n_M]))


@pytest.mark.parametrize("N", (1, 2, 3, 5, 1023, 1024, 1025, 2049))
def test_grid_counts(gpu, N):
    """sim_period_kernel: a lone agent, a ragged pair, one workgroup's 1024 agents +- 1, three."""
    fam, Mnow, agents = count_case(N)
    both_prices(Rig(gpu, fam, N, "grid"), f"grid N={N}", "grid", fam, Mnow, 0, agents)


def test_grid_second_stride_pass(gpu):
    """8192 x 1024 + 5 agents on the per-period kernel: a second grid-stride pass with a ragged
    pair (vectorised reference)."""
    from aiyagari_hark_amd import _lib
    N = 8192 * 1024 + 5
    fam, Mnow, (a0, lab0, u, _) = count_case(N)
    h = _lib.handle(gpu.index)
    prev = h.set_options({_lib.AIY_OPT_RESIDENT: 0})
    try:
        before = resident_periods(h)
        sow0 = (Mnow, 0, 1.0, 0.0)
        out = Rig(gpu, fam, N, "grid").run(a0, lab0, u, sow0)
        assert resident_periods(h) == before
    finally:
        h.set_options(prev)
    check(f"grid N={N}", "grid", out, fam, a0, lab0, u, sow0, fast=True)
    report("grid")


@pytest.mark.parametrize("N", (1, 2, 3, 63, 64, 65, 129, 2047, 2048, 2049, 2050, 12287, 12288))
def test_block_counts(gpu, N):
    """panel_block_kernel: <2> up to 2048 agents, <4> to the cap; ragged groups and waves."""
    fam, Mnow, agents = count_case(N)
    both_prices(Rig(gpu, fam, N, "block"), f"block N={N}", "block", fam, Mnow, 0, agents)


def test_block_refuses_above_its_cap(gpu):
    from aiyagari_hark_amd import _lib
    N = 12289
    fam, Mnow, (a0, lab0, u, _) = count_case(N)
    rig = Rig(gpu, fam, N, "block")
    with pytest.raises(_lib.AiyagariLibError, match="AIY_ERR_UNSUPPORTED"):
        rig.run(a0, lab0, u, (Mnow, 0, 1.0, 0.0))
    out = collect(rig.p)
    assert np.array_equal(out["a"], a0) and np.array_equal(out["lab"], lab0)
    assert np.array_equal(out["sow"], [Mnow, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0])


def test_batched_panel_three_calibrations(gpu):
    """Three calibrations with their own tables, M grids, labour processes and markets in one
    block launch, host uniforms [3][1][N]: each held to its own reference."""
    import torch

    from aiyagari_hark_amd.panel import BatchedPanel
    N, n_lab, n_M, n_a = 2051, 7, 3, 32
    fams = [PR.Family(n_lab, n_M, n_a, o, seed=k, M_scale=1.0 + 0.01 * k, hist_roll=k)
            for k, o in enumerate((14, 6, 10))]
    mks = [dict(CapShare=0.36 - 0.02 * k, DeprFac=0.08 + 0.01 * k, prod=(0.99 - 0.01 * k, 1.01 + 0.01 * k),
                agg_L=(0.93, 0.96 - 0.02 * k)) for k in range(3)]
    ag, sows = [], []
    for k, fam in enumerate(fams):
        rng = np.random.default_rng([43, k])
        Mnow = fam.M_inside(1 + k % 2)
        per = [PR.queries(*fam.rows(l, k % 2, 1, Mnow), rng) for l in range(n_lab)]
        ag.append(PR.fill(fam, N, per, rng))
        sows.append((Mnow, k % 2) + ((1.0, 0.0) if k < 2 else GENERIC))
    assert len({int(f.mrkv_hist[0]) for f in fams}) == 2
    bp = BatchedPanel(3, N, fams[0].mrkv_hist.size, device=gpu)
    st = lambda name: dv(gpu, np.stack([getattr(f, name) for f in fams]))  # noqa: E731
    bp.bind_models(st("m"), st("c"), st("Mgrid"), st("lvl"), st("cdf"), st("mrkv_hist"), mks)
    bp.reset(np.stack([x[0] for x in ag]), np.stack([x[1] for x in ag]),
             [[s[0], -1.0, s[1], s[2], s[3]] for s in sows])
    U = np.stack([x[2] for x in ag])[:, None, :]
    bp.run(0, 1, shock_mode="numpy", u_host_source=lambda n: U[:, :n])
    torch.cuda.synchronize()
    for k, fam in enumerate(fams):
        check(f"batched cal {k}", "block", collect(bp, k), fam, *ag[k][:3], sows[k], market=mks[k])
    report("block")


# ---------------------------------------------------------------------------------------
# Resident engine
# ---------------------------------------------------------------------------------------
RES_N = (65536, 65537, 65539)


@functools.lru_cache(maxsize=None)
def resident_case(N, n_M):
    """Agents, start and reference of one resident case (the reference is shared by the forms)."""
    fam, Mnow, (a0, lab0, u, _) = count_case(N, n_M)
    sow0 = (Mnow, 0) + GENERIC
    ref = PR.period(a0, lab0, np.ones(N, dtype=np.int64), u, *GENERIC, Mnow, 0, fam.lvl, fam.cdf, fam.m, fam.c,
                    fam.Mgrid)[:2]
    for x in (a0, lab0, u) + ref:
        x.setflags(write=False)
    return fam, a0, lab0, u, sow0, ref


# (AIY_OPT_RESIDENT_SHAPE, AIY_OPT_RESIDENT_STREAM, AIY_OPT_RESIDENT_SHAPE_STREAM)
FORMS = {"lds 512x8 quad": (0, 0, -1), "lds 1024x4 quad": (1, 0, -1), "lds 512x8 lane": (2, 0, -1),
         "stream 1024x4 quad": (0, 1, 1), "stream 512x8 quad": (0, 1, 0), "stream 512x8 lane": (2, 1, 2)}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_resident_forms(gpu, form):
    """Every workgroup shape and record-load form, agents in LDS and streamed, at the threshold,
    an odd count and a ragged last workgroup; blended and one-row tables; generic prices."""
    from aiyagari_hark_amd import _lib
    h = _lib.handle(gpu.index)
    shape, stream, sstream = FORMS[form]
    prev = h.set_options({_lib.AIY_OPT_RESIDENT: 1, _lib.AIY_OPT_RESIDENT_SHAPE: shape,
                          _lib.AIY_OPT_RESIDENT_STREAM: stream, _lib.AIY_OPT_RESIDENT_SHAPE_STREAM: sstream})
    try:
        for n_M in (3, 1):
            for N in RES_N:
                fam, a0, lab0, u, sow0, ref = resident_case(N, n_M)
                before = resident_periods(h)
                out = Rig(gpu, fam, N, "grid").run(a0, lab0, u, sow0)
                assert resident_periods(h) == before + 1
                check(f"resident {form} n_M={n_M} N={N}", "resident", out, fam, a0, lab0, u, sow0, ref=ref)
    finally:
        h.set_options(prev)
    report("resident")


def test_resident_placed_queries(gpu):
    """The lookup paths on the resident kernel's own call of tab_policy_t: m == a at R = 1,
    W = 0, the query set tiled over 65 539 agents, blended and one-row."""
    from aiyagari_hark_amd import _lib
    h = _lib.handle(gpu.index)
    for n_M in (3, 1):
        N = 65539
        fam, Mnow, (a0, lab0, u, _) = count_case(N, n_M)
        sow0 = (Mnow, 0, 1.0, 0.0)
        before = resident_periods(h)
        out = Rig(gpu, fam, N, "grid").run(a0, lab0, u, sow0)
        assert resident_periods(h) == before + 1
        check(f"resident placed n_M={n_M}", "resident", out, fam, a0, lab0, u, sow0)
    report("resident")


def test_resident_threshold_below(gpu):
    """65 535 agents take the per-period kernel and give the bits of the reference too."""
    from aiyagari_hark_amd import _lib
    h = _lib.handle(gpu.index)
    N = 65535
    fam, Mnow, (a0, lab0, u, _) = count_case(N)
    sow0 = (Mnow, 0) + GENERIC
    before = resident_periods(h)
    out = Rig(gpu, fam, N, "grid").run(a0, lab0, u, sow0)
    assert resident_periods(h) == before
    check(f"grid N={N}", "grid", out, fam, a0, lab0, u, sow0)


def test_resident_second_base_pass(gpu):
    """Just above 256 x 4096 agents a workgroup's slice exceeds one pass of 4096: a second
    `base` pass with a handful of agents (vectorised reference)."""
    from aiyagari_hark_amd import _lib
    h = _lib.handle(gpu.index)
    N = 1_050_001
    fam, Mnow, (a0, lab0, u, _) = count_case(N)
    sow0 = (Mnow, 0, 1.0, 0.0)
    before = resident_periods(h)
    out = Rig(gpu, fam, N, "grid").run(a0, lab0, u, sow0)
    assert resident_periods(h) == before + 1
    check(f"resident N={N}", "resident", out, fam, a0, lab0, u, sow0, fast=True)
    report("resident")


def test_resident_philox_period(gpu):
    """One period on device Philox uniforms against oracle.philox (shape 0)."""
    N, seed, ge = 65537, 77, 3
    fam, a0, lab0, _, sow0, _ = resident_case(N, 3)
    out = Rig(gpu, fam, N, "grid").run(a0, lab0, None, sow0, seed=seed, ge_iter=ge)
    u = PX.uniform(ge << 20, np.arange(N, dtype=np.uint64), seed)
    check("resident philox", "resident", out, fam, a0, lab0, u, sow0)


def test_single_rank_offset_philox_period(gpu):
    """One rank whose agents start at global index 2: the Philox draws are those of indices
    2 + i, so the call runs the per-period kernel (the resident kernel's single-rank forms draw at
    offset 0) although AIY_OPT_RESIDENT is on and the count is above its threshold."""
    from aiyagari_hark_amd import _lib
    N, off, seed, ge = 65539, 2, 77, 3
    fam, a0, lab0, _, sow0, _ = resident_case(N, 3)
    h = _lib.handle(gpu.index)
    prev = h.set_options({_lib.AIY_OPT_RESIDENT: 1})
    try:
        before = resident_periods(h)
        out = Rig(gpu, fam, N, "grid", agent_offset=off).run(a0, lab0, None, sow0, seed=seed, ge_iter=ge)
        after = resident_periods(h)
    finally:
        h.set_options(prev)
    u = PX.uniform(ge << 20, off + np.arange(N, dtype=np.uint64), seed)
    assert np.array_equal(out["lab"], H.draw_labor(lab0, u, fam.cdf))
    check("grid philox offset 2", "grid", out, fam, a0, lab0, u, sow0)
    assert after == before


# ---------------------------------------------------------------------------------------
# A second period, without a tolerance
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine,N", (("grid", 3001), ("block", 3001), ("resident", 65539)))
def test_second_period(gpu, engine, N):
    """Two periods in one call == the reference's second period fed the device's own period-1
    agents and prices, bit for bit."""
    fam, Mnow, (a0, lab0, _, _) = count_case(N)
    a0 = np.clip(a0, None, 50.0)    # (a 1e12 agent would own the mean and the next prices)
    rng = np.random.default_rng([47, N])
    U = rng.random((2, N))
    sow0 = (Mnow, 0) + GENERIC
    rig = Rig(gpu, fam, N, "grid" if engine == "resident" else engine)
    one = rig.run(a0, lab0, U[:1], sow0)
    check(f"{engine} period 1", engine, one, fam, a0, lab0, U[0], sow0)
    two = rig.run(a0, lab0, U, sow0, periods=2)
    s1 = one["sow"]
    a2, l2 = PR.period(one["a"], one["lab"], np.ones(N, dtype=np.int64), U[1], s1[3], s1[4], s1[0], int(s1[2]),
                       fam.lvl, fam.cdf, fam.m, fam.c, fam.Mgrid)[:2]
    assert np.array_equal(two["lab"], l2) and bits_equal(two["a"], a2)
    assert two["hist_A"][0] == one["hist_A"][0] and two["hist_M"][0] == one["hist_M"][0] and two["sow"][7] == 2
    assert not np.isnan(a2).any()
    gap, bound = abs(two["hist_A"][1] - PR.mean_fsum(a2)), PR.sum_bound(a2)
    print(f"{engine} period 2: mean gap {gap:.3e} (bound {bound:.3e})")
    assert gap <= bound
