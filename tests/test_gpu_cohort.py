"""GPU tests of the cohort sweep (aiy_cohort_forward, csrc/cohort.hip) and of the
mobility interface on it: the bits of aiy_transition_forward cohort by cohort, the occupancy
against tests/mobility_ref.py (oracle.stationary.hist_step chained), independence of the cohorts,
conservation, the refusals, a natural steady state and a solved path."""
import types

import numpy as np
import pytest

from oracle import stationary as ST
from tests import mobility_ref as MR

pytestmark = pytest.mark.gpu


def synthetic_problem(rng, n_cal, S, n_a, T, variant):
    """test_gpu_forward_any.synthetic_problem: a random monotone in-range lottery
    [T][n_cal][S][n_a], a stochastic P and a mass of sum 1 per calibration."""
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


def prices(rng, n_cal, S, T):
    """R, w [n_cal][T + 1] and lab [n_cal][S]."""
    return (1.0 + rng.uniform(0.01, 0.05, size=(n_cal, T + 1)), rng.uniform(1.0, 1.4, size=(n_cal, T + 1)),
            rng.uniform(0.3, 2.0, size=(n_cal, S)))


def split(rng, mass, G):
    """[G][n_cal][S][n_a]: every element of the mass shared out among G cohorts at random."""
    if G == 1:
        return mass[None].copy()
    f = rng.dirichlet(np.ones(G), size=mass.shape)            # [...][G]
    return np.ascontiguousarray(np.moveaxis(f, -1, 0) * mass[None])


def even_edges(n_cal, n_a, Q):
    return np.broadcast_to(np.linspace(0, n_a, Q + 1).astype(np.int32), (n_cal, Q + 1)).copy()


class Problem:
    """One lottery on the device with everything a sweep takes; ``sel``: a subset of calibrations."""

    def __init__(self, dev, lo, wlo, P, mass, aGrid, R, w, lab, sel=None):
        import torch
        sel = slice(None) if sel is None else sel
        self.host = dict(lo=lo[:, sel], wlo=wlo[:, sel], P=P[sel], mass=mass[sel], aGrid=aGrid[sel], R=R[sel], w=w[sel],
                         lab=lab[sel])
        self.up = lambda x, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(x)).to(dt).to(dev)  # noqa: E731
        h, up = self.host, self.up
        self.T, self.n_cal, self.S, self.n_a = h["lo"].shape
        self.dev = dev
        self.lo, self.wlo, self.R, self.w = up(h["lo"], torch.int32), up(h["wlo"]), up(h["R"]), up(h["w"])
        self.batch = types.SimpleNamespace(cals=[None] * self.n_cal, S=self.S, n_a=self.n_a, device=dev, d_P=up(h["P"]),
                                           d_a=up(h["aGrid"]), d_lab=up(h["lab"]))

    def single(self, mass):
        """(Ks, C, mass_T) of aiy_transition_forward on one mass [n_cal][S][n_a]."""
        import torch

        from aiyagari_hark_amd import _lib
        from aiyagari_hark_amd.transition import transition_forward
        work = _lib.work_space(self.dev, "transition", "transition", n_cal=self.n_cal, S=self.S, n_a=self.n_a, T=self.T)
        m = self.up(mass)
        Ks, C = transition_forward(self.batch, self.lo, self.wlo, m, self.T, work, self.R, self.w)
        torch.cuda.synchronize()
        return Ks, C, m.cpu().numpy()

    def cohorts(self, cohorts, edges, lo=None, wlo=None, T=None):
        """(CohortPaths, mass_T [G][n_cal][S][n_a]) of the sweep with consumption and states."""
        import torch

        from aiyagari_hark_amd.mobility import cohort_forward
        T = self.T if T is None else T
        m = self.up(cohorts)
        out = cohort_forward(self.batch, self.lo if lo is None else lo, self.wlo if wlo is None else wlo, m, T, edges,
                             R=self.R[:, :T + 1].contiguous(), w=self.w[:, :T + 1].contiguous())
        torch.cuda.synchronize()
        return out, m.cpu().numpy()


def same_paths(a, b, sel=slice(None)):
    """Bit equality of two (CohortPaths, mass_T), of b's cohorts ``sel``."""
    (pa, ma), (pb, mb) = a, b
    return (np.array_equal(pa.K, pb.K[:, sel]) and np.array_equal(pa.C, pb.C[:, sel]) and
            np.array_equal(pa.occ, pb.occ[:, sel]) and np.array_equal(pa.inc, pb.inc[:, sel]) and
            np.array_equal(ma, mb[sel]))


# -------------------------------------------------------------------------------------
# 1: the bits of the single sweep
# -------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,n_a,G,variant", [(7, 120, 5, "tail"), (7, 1000, 5, "head"), (7, 1000, 16, "head"),
                                             (25, 120, 1, "tail"), (25, 1000, 5, "head"), (64, 65, 16, "tail"),
                                             (1, 2, 1, "tail")])
def test_every_cohort_has_the_bits_of_the_single_sweep(gpu, S, n_a, G, variant):
    """mass_T[g], K[:, g] and C[:, g] equal aiy_transition_forward's on cohort g alone, bit for bit:
    "head" is the whole-wave path (500 sources on one destination), (64, 65, 16) runs 8 chunks of 2
    cohorts and a second column block with one live column, (1, 2, 1) the smallest sizes."""
    rng = np.random.default_rng(100000 * G + 1000 * S + n_a)
    n_cal, T = 2, 5
    prob = synthetic_problem(rng, n_cal, S, n_a, T, variant)
    p = Problem(gpu, *prob, *prices(rng, n_cal, S, T))
    co = split(rng, prob[3], G)
    paths, mT = p.cohorts(co, even_edges(n_cal, n_a, 5))
    assert paths.K.shape == (n_cal, G, T + 1) and paths.C.shape == (n_cal, G, T)
    assert paths.occ.shape == (n_cal, G, T + 1, 5) and paths.inc.shape == (n_cal, G, T + 1, S)
    for g in range(G):
        Ks, C, m = p.single(co[g])
        assert np.array_equal(mT[g], m), g
        assert np.array_equal(paths.K[:, g], Ks) and np.array_equal(paths.C[:, g], C), g
    assert np.all(paths.K > 0) and np.all(paths.occ >= 0.0)


# -------------------------------------------------------------------------------------
# 2: one lottery for every period
# -------------------------------------------------------------------------------------
def test_one_lottery_gives_the_bits_of_its_copies(gpu):
    """n_lot = 1 against the same lottery stacked T times: every output, bit for bit."""
    import torch
    rng = np.random.default_rng(2)
    n_cal, S, n_a, G, T = 2, 7, 120, 5, 6
    lo, wlo, P, mass, aGrid = synthetic_problem(rng, n_cal, S, n_a, 1, "tail")
    p = Problem(gpu, np.repeat(lo, T, axis=0), np.repeat(wlo, T, axis=0), P, mass, aGrid, *prices(rng, n_cal, S, T))
    assert p.T == T and torch.equal(p.lo[0], p.lo[T - 1])
    co, edges = split(rng, mass, G), even_edges(n_cal, n_a, 4)
    stacked = p.cohorts(co, edges)
    one = p.cohorts(co, edges, lo=p.lo[:1].contiguous(), wlo=p.wlo[:1].contiguous(), T=T)
    assert same_paths(one, stacked)
    assert not np.array_equal(stacked[1], co)


# -------------------------------------------------------------------------------------
# 3: occupancy
# -------------------------------------------------------------------------------------
Q32 = sorted([0, 1, 2, 2, 2, 3, 10, 10, 31, 32, 33, 63, 64, 64, 65, 66, 90, 100, 101, 127, 128, 128, 129, 129, 130,
              130] + [40, 41, 42, 50, 77])
EDGE_SETS = {"Q1": [0, 130], "Q5": [0, 63, 64, 65, 128, 130], "Q32": [0] + Q32 + [130]}


@pytest.fixture(scope="module")
def occupancy_case():
    """The n_a = 130 problem of test 3 and its reference chain per cohort, computed once:
    ref[cal][g] = the masses of periods 0 .. T."""
    rng = np.random.default_rng(3)
    n_cal, S, n_a, G, T = 2, 7, 130, 3, 5
    prob = synthetic_problem(rng, n_cal, S, n_a, T, "head")
    pr = prices(rng, n_cal, S, T)
    co = split(rng, prob[3], G)
    lo, wlo, P = prob[0], prob[1], prob[2]
    chain = [[[co[g, i]] for g in range(G)] for i in range(n_cal)]
    for i in range(n_cal):
        for g in range(G):
            for t in range(T):
                chain[i][g].append(ST.hist_step(chain[i][g][-1], lo[t, i], wlo[t, i], P[i]))
    return prob, pr, co, chain


@pytest.mark.parametrize("name", list(EDGE_SETS))
def test_occupancy_matches_the_reference_chain(gpu, occupancy_case, name):
    """occ and inc of every period within 1e-12 absolute of the class and state sums of the chain,
    K within 1e-10 relative; at t = 0 within 1e-15 of the NumPy sums of the cohorts as given.
    Q5 has its inner edges on the column-block boundaries (63, 64, 65, 128); Q32 has repeated
    edges (empty classes) and single-node classes."""
    prob, pr, co, chain = occupancy_case
    e = np.array(EDGE_SETS[name], dtype=np.int32)
    Q = len(e) - 1
    assert Q == {"Q1": 1, "Q5": 5, "Q32": 32}[name] and np.all(np.diff(e) >= 0)
    if name == "Q32":
        assert (np.diff(e) == 0).sum() >= 5 and (np.diff(e) == 1).sum() >= 8
    n_cal, G, T = prob[3].shape[0], co.shape[0], prob[0].shape[0]
    p = Problem(gpu, *prob, *pr)
    paths, _ = p.cohorts(co, np.broadcast_to(e, (n_cal, Q + 1)).copy())
    worst = dict(occ=0.0, inc=0.0, K=0.0, occ0=0.0, inc0=0.0)
    for i in range(n_cal):
        a = prob[4][i]
        for g in range(G):
            for t in range(T + 1):
                m = chain[i][g][t]
                worst["occ"] = max(worst["occ"], np.max(np.abs(paths.occ[i, g, t] - MR.class_sums(m, e))))
                worst["inc"] = max(worst["inc"], np.max(np.abs(paths.inc[i, g, t] - m.sum(axis=1))))
                Kr = np.sum(m * a[None, :])
                worst["K"] = max(worst["K"], abs(paths.K[i, g, t] - Kr) / Kr)
            worst["occ0"] = max(worst["occ0"], np.max(np.abs(paths.occ[i, g, 0] - MR.class_sums(co[g, i], e))))
            worst["inc0"] = max(worst["inc0"], np.max(np.abs(paths.inc[i, g, 0] - co[g, i].sum(axis=1))))
    print(f"{name}: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["occ"] <= 1e-12 and worst["inc"] <= 1e-12 and worst["K"] <= 1e-10
    assert worst["occ0"] <= 1e-15 and worst["inc0"] <= 1e-15


# -------------------------------------------------------------------------------------
# 4: independence
# -------------------------------------------------------------------------------------
def test_a_cohort_does_not_depend_on_the_others(gpu):
    """One cohort alone (G = 1), in two places of G = 5 among different others, and last of
    G = 16 (the second chunk): the same bits in every output; and a calibration alone against
    the batch of 3."""
    rng = np.random.default_rng(4)
    n_cal, S, n_a, T = 3, 7, 120, 4
    prob = synthetic_problem(rng, n_cal, S, n_a, T, "tail")
    pr = prices(rng, n_cal, S, T)
    p = Problem(gpu, *prob, *pr)
    edges = even_edges(n_cal, n_a, 5)
    x = split(rng, prob[3], 3)[1]                      # the cohort followed
    others = lambda G: split(rng, prob[3] * rng.uniform(0.1, 2.0), G)   # noqa: E731
    alone = p.cohorts(x[None], edges)
    for G, place in ((5, 0), (5, 3), (16, 15), (16, 7), (16, 8)):
        co = others(G)
        co[place] = x
        assert same_paths(alone, p.cohorts(co, edges), slice(place, place + 1)), (G, place)
    co = others(5)
    whole = p.cohorts(co, edges)
    sub = Problem(gpu, *prob, *pr, sel=slice(1, 2))
    (ps, ms), (pw, mw) = sub.cohorts(co[:, 1:2], edges[1:2]), whole
    assert np.array_equal(ps.K, pw.K[1:2]) and np.array_equal(ps.C, pw.C[1:2]) and np.array_equal(ps.occ, pw.occ[1:2])
    assert np.array_equal(ps.inc, pw.inc[1:2]) and np.array_equal(ms, mw[:, 1:2])


def test_more_than_sixteen_cohorts_run_as_several_calls(gpu):
    """S = 25 income states as cohorts (cohorts_by_state): 16 + 9 in two calls.  Every cohort has the
    bits of aiy_transition_forward on it alone, and starts in its own state."""
    from aiyagari_hark_amd.mobility import cohorts_by_state
    rng = np.random.default_rng(25)
    n_cal, S, n_a, T = 2, 25, 120, 3
    prob = synthetic_problem(rng, n_cal, S, n_a, T, "tail")
    p = Problem(gpu, *prob, *prices(rng, n_cal, S, T))
    co = cohorts_by_state(p.batch, p.up(prob[3])).cpu().numpy()
    assert co.shape == (S, n_cal, S, n_a) and np.array_equal(co.sum(axis=0), prob[3])
    paths, mT = p.cohorts(co, even_edges(n_cal, n_a, 5))
    assert paths.K.shape == (n_cal, S, T + 1) and paths.inc.shape == (n_cal, S, T + 1, S)
    for g in (0, 15, 16, 24):
        Ks, C, m = p.single(co[g])
        assert np.array_equal(mT[g], m) and np.array_equal(paths.K[:, g], Ks) and np.array_equal(paths.C[:, g], C), g
    for i in range(n_cal):
        assert np.all(paths.inc[i, :, 0, :][~np.eye(S, dtype=bool)] == 0.0) and np.all(np.diag(paths.inc[i, :, 0, :]) > 0)


# -------------------------------------------------------------------------------------
# 5: conservation
# -------------------------------------------------------------------------------------
def test_mass_is_conserved(gpu):
    """sum_q occ, sum_s inc and the cohort's total at t = 0 agree within 1e-13 in every period;
    the cohorts' mass_T add up to aiy_transition_forward's of the full mass within 1e-14."""
    rng = np.random.default_rng(5)
    n_cal, S, n_a, G, T = 2, 7, 130, 5, 5
    prob = synthetic_problem(rng, n_cal, S, n_a, T, "head")
    p = Problem(gpu, *prob, *prices(rng, n_cal, S, T))
    co = split(rng, prob[3], G)
    paths, mT = p.cohorts(co, np.broadcast_to(np.array(EDGE_SETS["Q5"], dtype=np.int32), (n_cal, 6)).copy())
    total0 = np.moveaxis(co.sum(axis=(2, 3)), 0, 1)     # [n_cal][G]
    d_occ = np.max(np.abs(paths.occ.sum(axis=-1) - total0[:, :, None]))
    d_inc = np.max(np.abs(paths.inc.sum(axis=-1) - total0[:, :, None]))
    d_both = np.max(np.abs(paths.occ.sum(axis=-1) - paths.inc.sum(axis=-1)))
    _, _, full = p.single(prob[3])
    d_mass = np.max(np.abs(mT.sum(axis=0) - full))
    print(f"conservation: occ {d_occ:.2e}  inc {d_inc:.2e}  occ - inc {d_both:.2e}  sum of cohorts {d_mass:.2e}")
    assert d_occ <= 1e-13 and d_inc <= 1e-13 and d_both <= 1e-13 and d_mass <= 1e-14


# -------------------------------------------------------------------------------------
# 6: refusals
# -------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(gpu):
    """One decreasing pair in one row: AIY_ERR_UNSUPPORTED; edges that decrease, do not start at 0
    or do not end at n_a: AIY_ERR_ARG.  The cohorts and the sentinel-filled outputs stay as they
    were, and the unmodified call still runs."""
    import torch

    from aiyagari_hark_amd import _lib
    rng = np.random.default_rng(6)
    n_cal, S, n_a, G, Q, T = 2, 7, 120, 5, 5, 5
    prob = synthetic_problem(rng, n_cal, S, n_a, T, "head")
    p = Problem(gpu, *prob, *prices(rng, n_cal, S, T))
    co0 = p.up(split(rng, prob[3], G))
    co = co0.clone()
    h = _lib.handle(gpu.index)
    work = _lib.work_space(gpu, "cohort", "cohort", n_cal=n_cal, S=S, n_a=n_a, n_lot=T, G=G, Q=Q)
    K, C = np.full((n_cal, G, T + 1), -7.0), np.full((n_cal, G, T), -7.0)
    occ, inc = np.full((n_cal, G, T + 1, Q), -7.0), np.full((n_cal, G, T + 1, S), -7.0)
    good = even_edges(n_cal, n_a, Q)
    dp = _lib.c_double_p

    def call(lot, edges):
        edges = np.ascontiguousarray(edges, dtype=np.int32)
        rc = h.lib.aiy_cohort_forward(h.h, n_cal, S, n_a, T, T, G, Q, _lib.ptr(lot), _lib.ptr(p.wlo),
                                      _lib.ptr(p.batch.d_P), _lib.ptr(p.batch.d_a), _lib.ptr(p.R), _lib.ptr(p.w),
                                      _lib.ptr(p.batch.d_lab), edges.ctypes.data_as(_lib.c_int32_p), _lib.ptr(work),
                                      _lib.ptr(co), K.ctypes.data_as(dp), C.ctypes.data_as(dp), occ.ctypes.data_as(dp),
                                      inc.ctypes.data_as(dp), _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, h.lib.aiy_last_error(h.h)

    def untouched():
        return (all(np.all(x == -7.0) for x in (K, C, occ, inc)) and torch.equal(co, co0))

    turned = p.lo.clone()
    row = turned[3, 1, 4]
    j = int(torch.nonzero(row[1:] > row[:-1])[0]) + 1     # row[j - 1] < row[j]: swap them
    row[j - 1], row[j] = row[j].clone(), row[j - 1].clone()
    assert int((turned != p.lo).sum()) == 2
    rc, msg = call(turned, good)
    assert rc == -4 and b"monotone" in msg and untouched()
    for bad in ([0, 30, 20, 60, 90, 120], [0, 24, 48, 72, 96, 119], [0, 24, 48, 72, 96, 121], [1, 24, 48, 72, 96, 120]):
        e = good.copy()
        e[1] = bad
        rc, msg = call(p.lo, e)
        assert rc == -1 and b"edges" in msg and untouched(), bad
    rc, _ = call(p.lo, good)
    assert rc == 0 and np.all(K > 0) and np.all(occ >= 0.0) and np.all(inc >= 0.0) and not torch.equal(co, co0)


# -------------------------------------------------------------------------------------
# 7: a natural case
# -------------------------------------------------------------------------------------
def test_mobility_of_three_steady_states(gpu):
    """n_a = 300, three calibrations through capital_supply at r = (0.035, 0.035, 0.02) with
    hist_tol = 1e-12, mobility(batch, horizons=(1, 5, 20)): rows sum to 1 within 1e-12; the matrix
    within 1e-12 of tests/mobility_ref on the device's own mass and lottery; the stationary mass is
    invariant: |sum_g share_g matrix[h][g][q] - share_q| <= h S n_a hist_tol (the lottery step does
    not expand L1 distance and the solve stops at a max-norm of hist_tol per element);
    0 <= shorrocks <= 1 + 1e-12."""
    from aiyagari_hark_amd.mobility import mobility
    from aiyagari_hark_amd.stationary import Calibration, StationaryBatch
    n_a, hist_tol, horizons = 300, 1e-12, (1, 5, 20)
    cals = [Calibration(LaborAR=0.6, LaborSD=0.2, CRRA=3.0), Calibration(LaborAR=0.0, LaborSD=0.2, CRRA=1.0),
            Calibration(LaborAR=0.9, LaborSD=0.4, CRRA=5.0)]
    batch = StationaryBatch(cals, ST.make_stationary_grid(0.001, 50.0, n_a, 2), device=gpu)
    batch.capital_supply(np.array([0.035, 0.035, 0.02]), hist_tol=hist_tol)
    res = mobility(batch, horizons=horizons)
    S = batch.S
    assert res.matrix.shape == (3, 3, 5, 5) and res.shorrocks.shape == (3, 3) and res.income.shape == (3, 3, 5, S)
    assert res.mean_wealth.shape == (3, 5, 21) and res.thresholds.shape == (3, 4) and res.shares.shape == (3, 5)
    mass, lo, wlo = batch.mass.cpu().numpy(), batch.lo.cpu().numpy(), batch.wlo.cpu().numpy()
    for i in range(3):
        shares, matrix, edges = MR.mobility_matrix(mass[i], lo[i], wlo[i], batch.P[i], (0.2, 0.4, 0.6, 0.8), horizons,
                                                   batch.aGrid[i])
        assert np.array_equal(edges, res.edges[i])
        live = shares > 0
        assert np.array_equal(live, res.shares[i] > 0) and np.all(np.isnan(res.matrix[i][:, ~live, :]))
        assert np.array_equal(res.thresholds[i], batch.aGrid[i][np.minimum(edges[1:-1], n_a - 1)])
        d_ref = np.max(np.abs(res.matrix[i][:, live, :] - matrix[:, live, :]))
        d_row = np.max(np.abs(res.matrix[i][:, live, :].sum(axis=-1) - 1.0))
        d_share = np.max(np.abs(res.shares[i] - shares))
        print(f"cal {i}: edges {edges.tolist()} shares {np.round(res.shares[i], 4).tolist()}  matrix - ref "
              f"{d_ref:.2e}  rows - 1 {d_row:.2e}  shares - ref {d_share:.2e}  shorrocks {res.shorrocks[i].tolist()}")
        assert d_ref <= 1e-12 and d_row <= 1e-12 and d_share <= 1e-12
        for k, hz in enumerate(horizons):
            back = np.nansum(res.shares[i][:, None] * res.matrix[i, k], axis=0)
            resid = np.max(np.abs(back - res.shares[i]))
            print(f"   h = {hz}: invariance residual {resid:.2e}  bound {hz * S * n_a * hist_tol:.2e}")
            assert resid <= hz * S * n_a * hist_tol
        assert np.all(res.shorrocks[i] >= 0.0) and np.all(res.shorrocks[i] <= 1.0 + 1e-12)
        d_inc = np.max(np.abs(res.income[i][:, live, :].sum(axis=-1) - 1.0))
        assert d_inc <= 1e-12
        assert np.max(np.abs(res.mean_wealth[i][live, 0] * res.shares[i][live] - res.paths.K[i][live, 0])) <= 1e-12
    by_state = mobility(batch, horizons=(1, 5), by="income")
    assert by_state.matrix.shape == (3, 2, S, 5) and by_state.shorrocks is None
    assert np.max(np.abs(by_state.matrix.sum(axis=-1) - 1.0)) <= 1e-12


# -------------------------------------------------------------------------------------
# 8: a solved path
# -------------------------------------------------------------------------------------
def test_cohorts_on_a_solved_path(gpu):
    """steady_state of the first calibration at n_a = 200, a 1 % TFP shock of persistence 0.8,
    T = 30: the cohorts' K and C add up to the path's within 1e-10 relative (the path converged to
    1e-12, so its K is its last evaluation's to that order), and every other field of the result
    has the bits of the call without cohorts=."""
    from aiyagari_hark_amd.stationary import Calibration
    from aiyagari_hark_amd.transition import solve_transition, steady_state
    T = 30
    batch, _, _ = steady_state([Calibration(LaborAR=0.6, LaborSD=0.2, CRRA=3.0)], 200, device=gpu)
    Z = 1.0 + 0.01 * 0.8 ** np.arange(T + 1)
    Z[T] = 1.0
    kw = dict(tol=1e-12, max_iter=200)
    plain = solve_transition(batch, Z, T, **kw)
    res = solve_transition(batch, Z, T, cohorts=(0.2, 0.4, 0.6, 0.8), **kw)
    assert plain.cohorts is None and np.all(res.status == 0)
    for name in ("K", "r", "w", "C", "iterations", "residual", "status"):
        assert np.array_equal(getattr(plain, name), getattr(res, name)), name
    co = res.cohorts
    assert co.K.shape == (1, 5, T + 1) and co.C.shape == (1, 5, T) and co.occ.shape == (1, 5, T + 1, 5)
    d_K = np.max(np.abs(co.K.sum(axis=1) - res.K) / res.K)
    d_C = np.max(np.abs(co.C.sum(axis=1) - res.C) / res.C)
    print(f"path: iterations {res.iterations.tolist()} residual {res.residual.tolist()}  sum K_g - K {d_K:.2e}  "
          f"sum C_g - C {d_C:.2e}  K_g[0] {co.K[0, :, 0].tolist()}")
    assert d_K <= 1e-10 and d_C <= 1e-10
    # at t = 0 every cohort sits in its own class
    assert np.all(co.occ[0, :, 0, :][~np.eye(5, dtype=bool)] == 0.0) and np.all(np.diag(co.occ[0, :, 0, :]) >= 0.0)
    assert np.max(np.abs(co.occ.sum(axis=-1) - co.occ[:, :, :1, :].sum(axis=-1))) <= 1e-13
