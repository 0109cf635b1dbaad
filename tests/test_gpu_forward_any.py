"""GPU tests of the forward sweep for lotteries whose rows need not be monotone
(aiy_transition_forward_any, csrc/transition.hip): the bits of
aiy_transition_forward_marginals where that one runs, oracle.stationary.hist_step chained where
it refuses, the two refusals of its own, and the simulation with aggregate risk on a grid where
the linearised policies turn rows.  The NumPy model tests/forward_any_ref.py keeps every
disordered input inside the work cap by the reference alone."""
import types

import numpy as np
import pytest

from oracle import stationary as ST
from tests import forward_any_ref as FR

pytestmark = pytest.mark.gpu

B = dict(LaborAR=0.6, LaborSD=0.2, CRRA=3.0)
NATURAL_N_A = 3000   # the natural case's grid (test_natural_case_runs_where_the_default_refuses)


def synthetic_problem(rng, n_cal, S, n_a, T, variant):
    """test_gpu_transition.synthetic_problem: a random monotone in-range lottery
    [T][n_cal][S][n_a], a stochastic P and a mass."""
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


class Problem:
    """One lottery on the device with everything a sweep takes; ``sel``: a subset of calibrations."""

    def __init__(self, dev, lo, wlo, P, mass, aGrid, R, w, lab, sel=None):
        import torch
        sel = slice(None) if sel is None else sel
        self.host = dict(lo=lo[:, sel], wlo=wlo[:, sel], P=P[sel], mass=mass[sel], aGrid=aGrid[sel], R=R[sel], w=w[sel],
                         lab=lab[sel])
        up = lambda x, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(x)).to(dt).to(dev)  # noqa: E731
        h = self.host
        self.T, self.n_cal, self.S, self.n_a = h["lo"].shape
        self.dev = dev
        self.lo, self.wlo, self.R, self.w = up(h["lo"], torch.int32), up(h["wlo"]), up(h["R"]), up(h["w"])
        self.mass0 = up(h["mass"])
        self.batch = types.SimpleNamespace(cals=[None] * self.n_cal, S=self.S, n_a=self.n_a, device=dev, d_P=up(h["P"]),
                                           d_a=up(h["aGrid"]), d_lab=up(h["lab"]))

    def run(self, rows):
        """(Ks, C, mass_T, marg, rows_turned) of one sweep with consumption and marginals."""
        import torch

        from aiyagari_hark_amd import _lib
        from aiyagari_hark_amd.transition import transition_forward
        what = "transition_any" if rows == "any" else "transition"
        work = _lib.work_space(self.dev, what, what, n_cal=self.n_cal, S=self.S, n_a=self.n_a, T=self.T)
        mass = self.mass0.clone()
        marg = torch.full((self.T + 1, self.n_cal, self.n_a), -7.0, dtype=torch.float64, device=self.dev)
        out = transition_forward(self.batch, self.lo, self.wlo, mass, self.T, work, self.R, self.w, marg=marg,
                                 rows=rows)
        torch.cuda.synchronize()
        return out[0], out[1], mass.cpu().numpy(), marg.cpu().numpy(), (out[2] if rows == "any" else None)


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))


def against_hist_step(p, run, tag):
    """The bounds of test_gpu_transition.forward_against_hist_step, and C against
    sum mass (q - lottery mean) to 1e-10 relative."""
    Ks, C, mT, marg, _ = run
    h = p.host
    for i in range(p.n_cal):
        a = h["aGrid"][i]
        m = h["mass"][i].copy()
        Kr, Cr = [np.sum(m * a[None, :])], []
        for t in range(p.T):
            lo, wl = h["lo"][t, i], h["wlo"][t, i]
            q = h["R"][i, t] * a[None, :] + h["w"][i, t] * h["lab"][i][:, None]
            Cr.append(np.sum(m * (q - (wl * a[lo] + (1.0 - wl) * a[lo + 1]))))
            assert np.max(np.abs(marg[t, i] - m.sum(axis=0))) <= 1e-12
            m = ST.hist_step(m, lo, wl, h["P"][i])
            Kr.append(np.sum(m * a[None, :]))
        Kr, Cr = np.array(Kr), np.array(Cr)
        e_m = np.max(np.abs(mT[i] - m))
        e_K = np.max(np.abs(Ks[i] - Kr) / Kr)
        e_C = np.max(np.abs(C[i] - Cr) / np.abs(Cr))
        e_s = abs(mT[i].sum() - h["mass"][i].sum())
        print(f"{tag} cal {i}: mass_T abs {e_m:.2e}  Ks rel {e_K:.2e}  C rel {e_C:.2e}  sum drift {e_s:.2e}")
        assert e_m <= 1e-12 and e_K <= 1e-10 and e_s < 1e-12 and e_C <= 1e-10


# -------------------------------------------------------------------------------------
# 1: monotone lotteries
# -------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["head", "tail"])
@pytest.mark.parametrize("S,n_a", [(S, n_a) for S in (7, 25) for n_a in (120, 1000)])
def test_monotone_lotteries_give_the_bits_of_the_monotone_sweep(gpu, S, n_a, variant):
    """Ks, C, mass and marg of aiy_transition_forward_any equal aiy_transition_forward_marginals'
    bit for bit ("head": a destination with 500 sources, the whole-wave path), rows_turned = 0."""
    rng = np.random.default_rng(1000 * S + n_a + (variant == "head"))
    n_cal, T = 2, 5
    p = Problem(gpu, *synthetic_problem(rng, n_cal, S, n_a, T, variant), *prices(rng, n_cal, S, T))
    mono, any_ = p.run("monotone"), p.run("any")
    assert same_bits(mono, any_)
    assert any_[4] == 0 and np.all(any_[0] > 0) and np.all(any_[3] >= 0.0)


# -------------------------------------------------------------------------------------
# 2: disordered lotteries
# -------------------------------------------------------------------------------------
def moved_lottery(rng, n_cal, S, n_a, T):
    """A sorted lottery with n_a / 4 entries of every row moved by up to +-3 cells."""
    lo, wlo, P, mass, aGrid = synthetic_problem(rng, n_cal, S, n_a, T, "none")
    return FR.disorder(rng, lo), wlo, P, mass, aGrid


def placed_lottery(rng, n_cal, S, n_a, T):
    """A sorted lottery with single turns placed where the kernels change path; every other row
    stays monotone.  Returns the problem and the names of the turns placed."""
    lo, wlo, P, mass, aGrid = synthetic_problem(rng, n_cal, S, n_a, T, "none")
    done = []
    row = lo[2, 0, S - 1]                       # the first two sources of a row
    row[0], row[1] = 1, 0
    done.append("first two")
    row = lo[3, 1, 0]                           # the last two sources of a row
    row[n_a - 2], row[n_a - 1] = n_a - 2, n_a - 3 if n_a > 3 else 0
    done.append("last two")
    if n_a >= 65:                               # sources 63 and 64: two waves of the row's scan at n_a = 65
        row = lo[0, 0, 0]
        v = min(int(row[63]), n_a - 3)
        row[63], row[64] = v + 1, v
        done.append("sources 63, 64")
    if n_a >= 1000:
        row = lo[1, 1, min(1, S - 1)]           # destinations 64 then 63: two blocks of columns
        j = int(np.searchsorted(row, 64))
        row[j], row[j + 1] = 64, 63
        done.append("destinations 63, 64")
        row = lo[1, 0, 0]                       # 500 sources on destination 0, some of them on 1 and 2
        row[:] = np.sort(rng.integers(3, n_a - 1, size=n_a))
        row[:500] = 0
        row[rng.choice(np.arange(5, 495), size=40, replace=False)] = rng.integers(1, 3, size=40)
        assert np.sum(row[:500] == 1) > 3 and np.sum(row[:500] == 2) > 3
        done.append("head with strangers")
    return (lo, wlo, P, mass, aGrid), done


@pytest.mark.parametrize("kind", ["moved", "placed"])
@pytest.mark.parametrize("S,n_a", [(S, n_a) for n_a in (3, 64, 65, 1000) for S in (1, 7, 25)])
def test_disordered_lotteries_match_hist_step(gpu, S, n_a, kind):
    """Rows the default refuses, against oracle.stationary.hist_step chained: mass 1e-12
    absolute, Ks 1e-10 relative, sum drift 1e-12, C 1e-10 relative.  n_a = 3 is the smallest
    grid, 64 one full block of columns, 65 a second block with one live column.  Two runs give
    the same bits, and a calibration alone gives the bits it gives in the batch of 3."""
    from aiyagari_hark_amd._lib import AiyagariLibError
    rng = np.random.default_rng(7000 + 100 * S + n_a + (kind == "placed"))
    n_cal, T = 3, 4
    if kind == "moved":
        prob, done = moved_lottery(rng, n_cal, S, n_a, T), []
    else:
        prob, done = placed_lottery(rng, n_cal, S, n_a, T)
        assert {"first two", "last two"} <= set(done)
        assert n_a < 65 or "sources 63, 64" in done
        assert n_a < 1000 or {"destinations 63, 64", "head with strangers"} <= set(done)
    lo = prob[0]
    assert lo.min() >= 0 and lo.max() <= n_a - 2
    ratios = np.array([FR.window_ratio(r) for r in lo.reshape(-1, n_a)])
    assert ratios.max() <= 3.0                      # inside the work cap by the reference alone
    n_turned = FR.rows_turned(lo)
    assert n_turned > 0 and (kind == "moved" or n_turned == len(done))   # placed: the other rows are monotone
    p = Problem(gpu, *prob, *prices(rng, n_cal, S, T))
    with pytest.raises(AiyagariLibError, match="monotone"):
        p.run("monotone")
    run = p.run("any")
    print(f"{kind} S={S} n_a={n_a}: {n_turned} rows turned, window ratio at most {ratios.max():.3f}, placed {done}")
    assert run[4] == n_turned
    against_hist_step(p, run, f"{kind} S={S} n_a={n_a}")
    assert same_bits(run, p.run("any"))
    alone = Problem(gpu, *prob, p.host["R"], p.host["w"], p.host["lab"], sel=slice(1, 2)).run("any")
    assert all(np.array_equal(x, y) for x, y in zip(alone[:3], (run[0][1:2], run[1][1:2], run[2][1:2])))
    assert np.array_equal(alone[3], run[3][:, 1:2]) and alone[4] == FR.rows_turned(lo[:, 1:2])


# -------------------------------------------------------------------------------------
# 3: refusals
# -------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(gpu):
    """A reversed row is "too disordered"; an entry of n_a - 1 or -1 "leaves [0, n_a - 2]"; neither
    message says "monotone".  Ks (prefilled), mass and marg stay as they were and the unmodified
    lottery still runs; T = 0 and null buffers are AIY_ERR_ARG before any launch."""
    import torch

    from aiyagari_hark_amd import _lib
    rng = np.random.default_rng(3)
    n_cal, S, n_a, T = 2, 7, 120, 5
    good = synthetic_problem(rng, n_cal, S, n_a, T, "head")
    p = Problem(gpu, *good, *prices(rng, n_cal, S, T))
    h = _lib.handle(gpu.index)
    work = _lib.work_space(gpu, "transition_any", "transition_any", n_cal=n_cal, S=S, n_a=n_a, T=T)
    mass = p.mass0.clone()
    marg = torch.full((T + 1, n_cal, n_a), -7.0, dtype=torch.float64, device=gpu)
    Ks, C = np.full((n_cal, T + 1), -7.0), np.full((n_cal, T), -7.0)
    turned = np.full(1, -7, dtype=np.int32)

    def call(lot, T=T, **null):
        a = dict(lo=_lib.ptr(lot), wlo=_lib.ptr(p.wlo), P=_lib.ptr(p.batch.d_P), a=_lib.ptr(p.batch.d_a),
                 work=_lib.ptr(work), mass=_lib.ptr(mass), Ks=Ks.ctypes.data_as(_lib.c_double_p))
        a.update({k: None for k in null})
        rc = h.lib.aiy_transition_forward_any(h.h, n_cal, S, n_a, T, a["lo"], a["wlo"], a["P"], a["a"], _lib.ptr(p.R),
                                              _lib.ptr(p.w), _lib.ptr(p.batch.d_lab), a["work"], a["mass"], a["Ks"],
                                              C.ctypes.data_as(_lib.c_double_p), _lib.ptr(marg),
                                              turned.ctypes.data_as(_lib.c_int32_p), _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, h.lib.aiy_last_error(h.h)

    def untouched():
        return (np.all(Ks == -7.0) and np.all(C == -7.0) and torch.equal(mass, p.mass0) and bool((marg == -7.0).all())
                and turned[0] == -7)

    reversed_ = p.lo.clone()
    reversed_[2, 1, 3] = torch.flip(reversed_[2, 1, 3], dims=(0,))
    assert not FR.within_cap(reversed_[2, 1, 3].cpu().numpy())
    rc, msg = call(reversed_)
    assert rc == -4 and b"too disordered" in msg and str(4 * (n_a + 1)).encode() in msg and b"monotone" not in msg
    assert untouched()
    for value in (n_a - 1, -1):
        out = p.lo.clone()
        out[4, 0, 6, 77] = value
        rc, msg = call(out)
        assert rc == -4 and b"leaves [0, n_a - 2]" in msg and b"monotone" not in msg and b"disordered" not in msg
        assert untouched()
    assert call(p.lo, T=0)[0] == -1
    for name in ("lo", "wlo", "P", "a", "work", "mass", "Ks"):
        rc, msg = call(p.lo, **{name: True})
        assert rc == -1 and b"null" in msg
    assert untouched()
    rc, _ = call(p.lo)   # the unmodified lottery still runs, with the default's bits
    assert rc == 0 and turned[0] == 0 and np.all(Ks > 0) and bool((marg >= 0.0).all())
    mono = p.run("monotone")
    assert np.array_equal(Ks, mono[0]) and np.array_equal(C, mono[1]) and np.array_equal(mass.cpu().numpy(), mono[2])


# -------------------------------------------------------------------------------------
# 4: a natural case
# -------------------------------------------------------------------------------------
def test_natural_case_runs_where_the_default_refuses(gpu):
    """Calibration B at n_a = NATURAL_N_A, T = 40, h = 1e-5, ar1(0.8), 24 innovations of sigma =
    0.007: the linearised policies turn rows, the default simulate raises, rows="any" runs.
    Against the chain that downloads the device's own lotteries and applies hist_step, with the
    bounds of test 2; |sum mass - 1| <= 1e-11; chunk = 7 and chunk = 24 give the same bits."""
    import torch

    from aiyagari_hark_amd._lib import AiyagariLibError
    from aiyagari_hark_amd.aggregate import (aggregate_lotteries, ar1, expectations, linear_model, policy_jacobian,
                                             simulate)
    from aiyagari_hark_amd.stationary import Calibration
    from aiyagari_hark_amd.transition import household_jacobian, steady_state
    T, n = 40, 24
    batch, r, _ = steady_state([Calibration(**B)], NATURAL_N_A, device=gpu)
    jac = household_jacobian(batch, r, T, h=1e-5)
    model = linear_model(batch, jac, ar1(0.8, T))
    del jac
    pol = policy_jacobian(batch, r, T, h=1e-5)
    eps = 0.007 * np.random.default_rng(0).standard_normal(n)
    S, n_a = batch.S, batch.n_a
    # the device's own lotteries of the 24 periods
    ex = expectations(model, eps)
    d_lo = torch.empty((n, 1, S, n_a), dtype=torch.int32, device=gpu)
    d_wlo = torch.empty((n, 1, S, n_a), dtype=torch.float64, device=gpu)
    aggregate_lotteries(batch, pol, torch.as_tensor(np.ascontiguousarray(ex.X)).to(gpu), d_lo, d_wlo)
    lo, wlo = d_lo.cpu().numpy()[:, 0], d_wlo.cpu().numpy()[:, 0]
    turned = [(t, s) for t in range(n) for s in range(S) if FR.is_turned(lo[t, s])]
    ratios = [FR.window_ratio(lo[t, s]) for t, s in turned]
    print(f"n_a={n_a}: turned (period, state) rows {turned}, window ratios {ratios}")
    assert len(turned) > 0 and max(ratios) <= 3.0   # not monotone at this shape, and far inside the cap
    with pytest.raises(AiyagariLibError, match="monotone"):
        simulate(batch, model, pol, eps, chunk=24)
    sim = simulate(batch, model, pol, eps, chunk=24, rows="any")
    assert sim.rows_turned == len(turned)
    # the chain on the host
    a, lab, P = batch.aGrid[0], batch.levels[0], batch.P[0]
    m = batch.mass.cpu().numpy()[0].copy()
    Kr, Cr = [np.sum(m * a[None, :])], []
    for t in range(n):
        q = (1.0 + model.r[0] + ex.dr[0, t]) * a[None, :] + (model.w[0] + ex.dw[0, t]) * lab[:, None]
        Cr.append(np.sum(m * (q - (wlo[t] * a[lo[t]] + (1.0 - wlo[t]) * a[lo[t] + 1]))))
        m = ST.hist_step(m, lo[t], wlo[t], P)
        Kr.append(np.sum(m * a[None, :]))
    Kr, Cr = np.array(Kr), np.array(Cr)
    mT = sim.mass.cpu().numpy()[0]
    e_m, e_K = np.max(np.abs(mT - m)), np.max(np.abs(sim.K[0] - Kr) / Kr)
    e_C, e_s = np.max(np.abs(sim.C[0] - Cr) / np.abs(Cr)), abs(mT.sum() - batch.mass.cpu().numpy()[0].sum())
    print(f"natural: mass abs {e_m:.2e}  K rel {e_K:.2e}  C rel {e_C:.2e}  sum drift {e_s:.2e}  gap {sim.gap[0]:.2e}")
    assert e_m <= 1e-12 and e_K <= 1e-10 and e_C <= 1e-10 and e_s < 1e-12
    assert abs(mT.sum() - 1.0) <= 1e-11
    other = simulate(batch, model, pol, eps, chunk=7, rows="any")
    assert np.array_equal(other.K, sim.K) and np.array_equal(other.C, sim.C) and torch.equal(other.mass, sim.mass)
    assert other.rows_turned == sim.rows_turned
    assert simulate(batch, model, pol, np.zeros(3), rows="monotone").rows_turned is None


def test_rows_longer_than_the_staged_window(gpu):
    """The window pass keeps a row of up to 12 288 entries in LDS and reads a longer one from
    memory: n_a = 12 289 takes the second form.  A monotone lottery has the default's bits, a
    moved one matches hist_step chained."""
    n_cal, S, n_a, T = 1, 2, 12289, 2
    rng = np.random.default_rng(12289)
    p = Problem(gpu, *synthetic_problem(rng, n_cal, S, n_a, T, "head"), *prices(rng, n_cal, S, T))
    any_ = p.run("any")
    assert same_bits(p.run("monotone"), any_) and any_[4] == 0
    prob = moved_lottery(rng, n_cal, S, n_a, T)
    assert max(FR.window_ratio(r) for r in prob[0].reshape(-1, n_a)) <= 3.0
    p = Problem(gpu, *prob, *prices(rng, n_cal, S, T))
    run = p.run("any")
    assert run[4] == FR.rows_turned(prob[0]) == T * n_cal * S
    against_hist_step(p, run, f"moved S={S} n_a={n_a}")
