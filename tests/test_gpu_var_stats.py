"""GPU tests of the statistics of household variables (csrc/var_stats.hip, the masses entry of
csrc/transition.hip, stats.variable_stats / household_variables / batch_inequality,
transition.path_variable_stats) against the NumPy reference tests/var_stats_ref.py.  The reference
is always fed the GPU's own inputs, so only the new code is compared.

Bounds (those of tests/test_gpu_dist_stats.py): Lorenz shares, Gini, mean and total 1e-10
relative, percentile values 1e-8 relative with an equal NaN pattern, bottom share 1e-12; std and
cv 1e-10 relative; correlations 1e-10 absolute.  The merge itself is compared bit for bit.

Two synthetic patterns are built so that a relative bound on the Gini coefficient has a meaning.
The point mass sits on one node of one state (gini = 1 - 1 exactly on both sides).  With all keys
equal the keys are 2.0 and the weights integers over a power-of-two total: L = F bit for bit,
every F is a multiple of 2^-20 and every term and sum of the area is exact, so gini = 0.0 on both
sides (with arbitrary weights both sides would return their own rounding of 1 - 1).  At n_a = 2
the zero runs leave key = grid one grid value, S tied keys that hold all the weight: there the
grid is [0.5, 32.0] and the weights are the integer ones, so that cd = a cw exactly and again L = F."""
import types

import numpy as np
import pytest

from oracle import stationary as ST
from tests import dist_stats_ref as DR
from tests import transition_ref as TR
from tests import var_stats_ref as VR

pytestmark = pytest.mark.gpu

A = dict(LaborAR=0.9, LaborSD=0.4, CRRA=3.0)
B = dict(LaborAR=0.6, LaborSD=0.2, CRRA=3.0)
C = dict(LaborAR=0.3, LaborSD=0.4, CRRA=5.0)
D = dict(LaborAR=0.6, LaborSD=0.2, CRRA=1.0)
R25 = dict(LaborAR=0.9, LaborSD=0.4, CRRA=5.0, LaborStatesNo=25, income="rouwenhorst")
ALPHA, DELTA = 0.36, 0.08
PCT = np.linspace(0.01, 0.999, 15)      # the notebook's pctiles
RTOL = 1e-10
PCTL_RTOL = 1e-8
BOTTOM_RTOL = 1e-12
CORR_ATOL = 1e-10
FIELDS = ("lorenz", "percentile_values", "gini", "mean", "total", "bottom_share", "std", "cv")
SORTABLE = ("wealth", "consumption", "income", "earnings", "cash")
PATTERNS = ("interleaved", "descending", "ties", "equal", "grid")


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


WORST = {}


def compare(vs, ref, tag, fields=FIELDS):
    """vs: VariableStats of leading shape [n] (or a namespace of its fields); ref: dict of stacked
    reference arrays.  Prints every error before it asserts."""
    errs = {k: rel_err(getattr(vs, k), ref[k]) for k in fields}
    for k, v in errs.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print(tag + ": " + "  ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    if "percentile_values" in fields:
        assert np.array_equal(np.isnan(vs.percentile_values), np.isnan(ref["percentile_values"]))
        assert errs["percentile_values"] <= PCTL_RTOL, (tag, errs["percentile_values"])
    for k in ("lorenz", "gini", "mean", "total", "std", "cv"):
        if k in fields:
            assert errs[k] <= RTOL, (tag, k, errs[k])
    if "bottom_share" in fields:
        assert errs["bottom_share"] <= BOTTOM_RTOL, (tag, errs["bottom_share"])


def ref_stack(key, weight, pct=PCT):
    """The reference of every distribution of host stacks [n][S][n_a], stacked by field."""
    ref = [VR.variable_stats(key[i], weight[i], pct) for i in range(key.shape[0])]
    return {k: np.stack([np.asarray(r[k]) for r in ref]) for k in FIELDS}


def same_bits(x, y, fields=FIELDS):
    return all(np.array_equal(getattr(x, k), getattr(y, k), equal_nan=True) for k in fields)


def merge_call(gpu, key, weight, rank=True):
    """aiy_var_merge on device stacks [n][S][n_a] with every output at a sentinel first:
    (rc, key_sorted, weight_sorted, rank)."""
    import torch

    from aiyagari_hark_amd import _lib
    n, S, n_a = key.shape
    h = _lib.handle(gpu.index)
    ks = torch.full((n, S * n_a), -7.0, dtype=torch.float64, device=gpu)
    ws = torch.full((n, S * n_a), -7.0, dtype=torch.float64, device=gpu)
    rk = torch.full((n, S, n_a), -7, dtype=torch.int32, device=gpu)
    work = _lib.work_space(gpu, "var", "", n_dist=n, S=S, n_a=n_a)
    rc = h.lib.aiy_var_merge(h.h, n, S, n_a, _lib.ptr(key), _lib.ptr(weight), _lib.ptr(work), _lib.ptr(ks),
                             _lib.ptr(ws), _lib.ptr(rk) if rank else None, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, ks, ws, rk


def synthetic_weights(rng, S, n_a, integer=False):
    """[6][S][n_a]: leading, interior and trailing runs of exact zeros, a point mass on one node
    of one state and two plain ones; integer: integers over a total of 2^20 (see the module)."""
    w = np.floor(rng.uniform(0.0, 16.0, size=(6, S, n_a))) if integer else rng.uniform(0.0, 1.0, size=(6, S, n_a))
    run = max(1, n_a // 4)
    w[0, :, :run] = 0.0
    if n_a > 2:
        w[1, :, n_a // 3:n_a // 3 + run] = 0.0
    w[2, :, n_a - run:] = 0.0
    w[3] = 0.0
    w[3, S // 2, n_a // 2] = 1.0
    if integer:
        for i in range(6):                                   # top the total up to 2^20 on one node
            w[i, S // 2, n_a // 2] += 2.0 ** 20 - w[i].sum()
        return w / 2.0 ** 20
    return w / w.sum(axis=(1, 2), keepdims=True)


def synthetic_keys(rng, pattern, S, n_a, grid):
    """[6][S][n_a] keys, every run nondecreasing."""
    if pattern == "interleaved":       # strictly increasing runs whose ranges overlap
        return np.sort(rng.uniform(0.5, 40.0, size=(6, S, n_a)), axis=2)
    if pattern == "descending":        # disjoint ranges, all of run s above run s + 1
        base = np.sort(rng.uniform(0.1, 0.9, size=(6, S, n_a)), axis=2)
        return base + (S - np.arange(S))[None, :, None]
    if pattern == "ties":              # small integers: ties within and across runs
        return np.sort(rng.integers(1, 6, size=(6, S, n_a)).astype(np.float64), axis=2)
    if pattern == "equal":
        return np.full((6, S, n_a), 2.0)
    return np.broadcast_to(grid, (6, S, n_a)).copy()         # key = the grid in every state


@pytest.mark.parametrize("n_a", [2, 120, 257, 1000])
@pytest.mark.parametrize("S", [1, 7, 64])
def test_merge_synthetic(gpu, S, n_a):
    """1: the rank is the inverse of NumPy's stable argsort, key_sorted and weight_sorted are the
    gathered inputs bit for bit, the statistics are within the bounds, and with key = grid Lorenz
    shares, Gini, mean and total agree with histogram_stats of the same mass within 1e-10."""
    import torch

    from aiyagari_hark_amd.stats import histogram_stats, variable_stats
    rng = np.random.default_rng(1000 * S + n_a)
    grid = ST.make_stationary_grid(0.001, 50.0, n_a, 2) if n_a > 2 else np.array([0.5, 32.0])
    for pattern in PATTERNS:
        key = synthetic_keys(rng, pattern, S, n_a, grid)
        w = synthetic_weights(rng, S, n_a, integer=pattern == "equal" or (pattern == "grid" and n_a == 2))
        dk, dw = torch.as_tensor(key).to(gpu), torch.as_tensor(w).to(gpu)
        rc, ks, ws, rk = merge_call(gpu, dk, dw)
        assert rc == 0
        for i in range(6):
            rks, rws, rrank = VR.merge(key[i], w[i])
            assert np.array_equal(rk[i].cpu().numpy(), rrank), (pattern, i)
            assert np.array_equal(ks[i].cpu().numpy(), rks) and np.array_equal(ws[i].cpu().numpy(), rws), (pattern, i)
        _, ks2, ws2, _ = merge_call(gpu, dk, dw, rank=False)     # rank_out is optional
        assert torch.equal(ks2, ks) and torch.equal(ws2, ws)
        vs = variable_stats(dk.reshape(3, 2, S, n_a), dw.reshape(3, 2, S, n_a), PCT)
        assert vs.gini.shape == (3, 2) and vs.lorenz.shape == (3, 2, PCT.size) and vs.std.shape == (3, 2)
        flat = types.SimpleNamespace(**{k: getattr(vs, k).reshape((6,) + getattr(vs, k).shape[2:]) for k in FIELDS})
        ref = ref_stack(key, w)
        compare(flat, ref, f"S={S} n_a={n_a} {pattern}")
        assert flat.gini[3] == 0.0 and ref["gini"][3] == 0.0          # the point mass
        if pattern == "equal":
            assert np.all(flat.gini == 0.0) and np.all(ref["gini"] == 0.0) and np.all(flat.std == 0.0)
        if pattern == "grid":
            hs = histogram_stats(dw, grid, PCT)
            # below the first node's share HARK's np.interp returns L[0], and the first point of the
            # merged curve is one state's part of that node: those entries differ by definition
            keep = PCT[None, :] >= w[:, :, 0].sum(axis=1)[:, None]
            assert keep[:, 1:].all() or n_a == 2
            for k in ("lorenz", "gini", "mean", "total"):
                got, want = getattr(flat, k), getattr(hs, k)
                e = rel_err(np.where(keep, got, 0.0), np.where(keep, want, 0.0)) if k == "lorenz" else rel_err(got, want)
                print(f"  key = grid against histogram_stats: {k} {e:.1e}")
                assert e <= RTOL, (k, e)
        # a host array takes the same path
        if pattern == "ties":
            assert same_bits(variable_stats(key.reshape(3, 2, S, n_a), w.reshape(3, 2, S, n_a), PCT, device=gpu), vs)


@pytest.mark.parametrize("bad", ["decreasing", "nan"])
def test_refusal(gpu, bad):
    """2: one decreasing pair (or one NaN key) in one run of one distribution of a stack, at the
    first pair, the last pair, a pair that straddles two threads' chunks of the merge (16 nodes), a
    wave of the check (64), its block (256) and a wave of the merge (1024): AIY_ERR_UNSUPPORTED
    with every output at its sentinel.  aiy_var_moments still runs on the same stack."""
    import torch

    from aiyagari_hark_amd import _lib
    from aiyagari_hark_amd.stats import _moments, variable_stats
    S, n_a, n = 3, 1100, 4
    rng = np.random.default_rng(7)
    key = np.sort(rng.uniform(0.5, 40.0, size=(n, S, n_a)), axis=2)
    w = rng.uniform(0.0, 1.0, size=(n, S, n_a))
    dw = torch.as_tensor(w).to(gpu)
    h = _lib.handle(gpu.index)
    pairs = (1, n_a - 1, 16, 64, 256, 1024)             # the pair (j - 1, j)
    for j in pairs if bad == "decreasing" else (0, n_a - 1, 15, 16, 63, 64, 255, 256, 1023, 1024):
        k = key.copy()
        if bad == "decreasing":
            k[2, 1, j - 1], k[2, 1, j] = k[2, 1, j], k[2, 1, j - 1]
            assert k[2, 1, j] < k[2, 1, j - 1]
        else:
            k[2, 1, j] = np.nan
        dk = torch.as_tensor(k).to(gpu)
        rc, ks, ws, rk = merge_call(gpu, dk, dw)
        assert rc == -4 and _lib.ERRORS[rc] == "AIY_ERR_UNSUPPORTED", (j, rc)
        with pytest.raises(_lib.AiyagariLibError, match="nondecreasing"):
            h.check(rc, "aiy_var_merge")
        assert bool(torch.all(ks == -7.0)) and bool(torch.all(ws == -7.0)) and bool(torch.all(rk == -7)), j
        with pytest.raises(_lib.AiyagariLibError):
            variable_stats(dk, dw, PCT)
        if bad == "decreasing":
            work = _lib.work_space(gpu, "var", "", n_dist=n, S=S, n_a=n_a)
            mom = _moments(h, [dk], dw, n, S, n_a, work)
            for i in range(n):
                sw, mean, cov = VR.moments([k[i]], w[i])
                assert rel_err(mom[i], np.array([sw, mean[0], cov[0, 0]])) <= RTOL, (j, i)
    # the untouched stack still merges; a NaN in the last key of the last run of the stack is seen
    assert merge_call(gpu, torch.as_tensor(key).to(gpu), dw)[0] == 0
    k = key.copy()
    k[-1, -1, -1] = np.nan
    assert merge_call(gpu, torch.as_tensor(k).to(gpu), dw)[0] == -4
    # bad sizes and null buffers: AIY_ERR_ARG before any launch
    dk = torch.as_tensor(key).to(gpu)
    work = _lib.work_space(gpu, "var", "", n_dist=n, S=S, n_a=n_a)
    ks = torch.full((n, S * n_a), -7.0, dtype=torch.float64, device=gpu)
    for args in ((0, S, n_a), (n, 0, n_a), (n, 65, n_a), (n, S, 1)):
        assert h.lib.aiy_var_merge(h.h, *args, _lib.ptr(dk), _lib.ptr(dw), _lib.ptr(work), _lib.ptr(ks), _lib.ptr(ks),
                                   None, _lib.stream_ptr()) == -1, args
    assert h.lib.aiy_var_merge(h.h, n, S, n_a, _lib.ptr(dk), _lib.ptr(dw), _lib.ptr(work), None, _lib.ptr(ks), None,
                               _lib.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert bool(torch.all(ks == -7.0))


def path_problem(batch, K, T):
    """Lotteries of a wiggled price path in fresh buffers (with the device prices attached)."""
    import torch

    from aiyagari_hark_amd.transition import TransitionBuffers, household_block
    R, w = wiggle_prices(K, T)
    buf = TransitionBuffers(batch, T)
    household_block(batch, R, w, *batch.last_tables, batch.mass, buffers=buf)
    buf.R = torch.as_tensor(np.ascontiguousarray(R)).to(batch.device)
    buf.w = torch.as_tensor(np.ascontiguousarray(w)).to(batch.device)
    buf.hR, buf.hw = R, w
    return buf


def test_bits_runs_stack_and_slabs(ss120):
    """3: two runs are bit-identical; a distribution alone gives the bits it gives in the stack; the
    slab size does not change a bit (18 consumption distributions of a T = 5 path)."""
    from aiyagari_hark_amd.stats import household_variables, variable_stats
    from aiyagari_hark_amd.transition import household_block
    batch, _, K = pick(ss120, [0, 2, 3])
    T = 5
    R, w = wiggle_prices(K, T)
    out = household_block(batch, R, w, *batch.last_tables, batch.mass, masses=True)
    assert tuple(out.masses.shape) == (T + 1, 3, batch.S, batch.n_a)
    c = household_variables(batch, out.lo, out.wlo, R[:, :T], w[:, :T], ("consumption",))["consumption"]
    mass = out.masses[:T]
    whole = variable_stats(c, mass, PCT, slab=3 * T)
    assert whole.gini.shape == (T, 3)
    assert same_bits(variable_stats(c, mass, PCT, slab=3 * T), whole)
    for slab in (1, 2, 4, 7):
        assert same_bits(variable_stats(c, mass, PCT, slab=slab), whole), slab
    assert same_bits(variable_stats(c, mass, PCT), whole)
    for t, i in ((0, 0), (3, 1), (4, 2)):
        alone = variable_stats(c[t, i], mass[t, i], PCT)
        assert all(np.array_equal(getattr(alone, k), getattr(whole, k)[t, i], equal_nan=True) for k in FIELDS), (t, i)
    # 18 distributions: the full [T + 1] stack with period T on the lottery of T - 1
    import torch
    c18 = torch.cat([c, c[T - 1:]])
    w18 = variable_stats(c18, out.masses, PCT, slab=18)
    for slab in (1, 2, 4, 7):
        assert same_bits(variable_stats(c18, out.masses, PCT, slab=slab), w18), slab


def host_variables(batch, lo, wlo, R, w, names):
    """The NumPy expressions on the GPU's own lottery [n_cal][S][n_a] with prices R, w [n_cal]."""
    lo, wlo = lo.cpu().numpy(), wlo.cpu().numpy()
    out = [VR.variables(batch.aGrid[i], batch.levels[i], R[i], w[i], lo[i], wlo[i], names) for i in range(len(R))]
    return {k: np.stack([o[k] for o in out]) for k in names}


def test_steady_states(ss120, ss25):
    """4: every variable bit-equal to the NumPy expression on the GPU's own lottery,
    batch_inequality within the bounds of the reference, mean(consumption) x total within 1e-12 of
    aiy_transition_forward's C at T = 1, the wealth entry within 1e-10 of batch_wealth_stats, and
    corr(wealth, wealth) = 1 to 1e-12."""
    from aiyagari_hark_amd import _lib
    from aiyagari_hark_amd.stats import VARIABLES, batch_inequality, batch_wealth_stats, household_variables
    from aiyagari_hark_amd.transition import steady_lottery, transition_forward
    for tag, (batch, _, _) in (("n_a=120", ss120), ("n_a=1000", ss25)):
        n_cal = len(batch.cals)
        lo, wlo, dR, dw = steady_lottery(batch)
        R, w = dR.cpu().numpy(), dw.cpu().numpy()
        val = household_variables(batch, lo, wlo, dR, dw)
        host = host_variables(batch, lo, wlo, R, w, VARIABLES)
        for name in VARIABLES:
            assert np.array_equal(val[name].cpu().numpy(), host[name]), (tag, name)
        for name in SORTABLE:
            assert VR.runs_nondecreasing(host[name]), (tag, name)
        names = ("wealth", "consumption", "income", "earnings", "cash", "saving")
        ineq = batch_inequality(batch, PCT, names)
        assert set(ineq.stats) == set(SORTABLE) and set(ineq.moments) == set(names)
        assert ineq.corr.shape == (n_cal, 6, 6)
        mass = batch.mass.cpu().numpy()
        for name in SORTABLE:
            compare(ineq.stats[name], ref_stack(host[name], mass), f"steady state {tag} {name}")
            assert np.array_equal(ineq.stats[name].std, ineq.moments[name]["std"])
        worst = 0.0
        for i in range(n_cal):
            sw, mean, cov = VR.moments([host[n][i] for n in names], mass[i])
            corr = VR.correlations([host[n][i] for n in names], mass[i])
            worst = max(worst, float(np.max(np.abs(ineq.corr[i] - corr))))
            for u, n in enumerate(names):
                sd = np.sqrt(cov[u, u])
                assert rel_err(ineq.moments[n]["std"][i], sd) <= RTOL
                if n == "saving":      # its mean is zero at a steady state: the error is measured in its std
                    assert abs(ineq.moments[n]["mean"][i] - mean[u]) <= RTOL * sd
                else:
                    assert rel_err(ineq.moments[n]["mean"][i], mean[u]) <= RTOL
                    assert rel_err(ineq.moments[n]["cv"][i], sd / abs(mean[u])) <= RTOL
        WORST["corr"] = max(WORST.get("corr", 0.0), worst)
        print(f"steady state {tag}: correlations {worst:.1e}; gini of consumption "
              f"{np.round(ineq.stats['consumption'].gini, 4)} income {np.round(ineq.stats['income'].gini, 4)} "
              f"wealth {np.round(ineq.stats['wealth'].gini, 4)}")
        assert worst <= CORR_ATOL
        assert np.max(np.abs(ineq.corr[:, 0, 0] - 1.0)) <= 1e-12 and np.all(np.abs(ineq.corr) <= 1.0 + 1e-12)
        # aggregate consumption: one forward step on the same lottery
        m = batch.mass.clone()
        work = _lib.work_space(batch.device, "transition", "", n_cal=n_cal, S=batch.S, n_a=batch.n_a, T=1)
        _, Cagg = transition_forward(batch, lo[None], wlo[None], m, 1, work, dR[:, None].repeat(1, 2).contiguous(),
                                     dw[:, None].repeat(1, 2).contiguous(), want_c=True)
        cs = ineq.stats["consumption"]
        e = np.max(np.abs(cs.mean * cs.total - Cagg[:, 0]))
        print(f"  mean(c) x total against the forward sweep's C: {e:.1e}")
        assert e <= 1e-12
        ws = batch_wealth_stats(batch, PCT)
        for k in ("lorenz", "gini", "mean"):
            e = rel_err(getattr(ineq.stats["wealth"], k), getattr(ws, k))
            print(f"  wealth against batch_wealth_stats: {k} {e:.1e}")
            assert e <= RTOL
        with pytest.raises(ValueError, match="not monotone"):
            batch_inequality(batch, PCT, names, sorted_variables=("wealth", "saving"))


def sweep(batch, buf, T, mass_path):
    """One forward sweep from batch.mass on the lotteries of buf: (Ks, C, mass_T)."""
    from aiyagari_hark_amd.transition import transition_forward
    mass = batch.mass.clone()
    Ks, Cc = transition_forward(batch, buf.lo, buf.wlo, mass, T, buf.work, buf.R, buf.w, want_c=True,
                                mass_path=mass_path)
    return Ks, Cc, mass


def test_masses_sweep_and_path_stats(ss120, ss25):
    """5: Ks, C and mass_T of the masses entry equal aiy_transition_forward's bit for bit,
    mass_path[t] has the bits of T calls with T = 1, a decreasing lottery row leaves everything at
    its sentinels, and path_variable_stats matches the reference applied to those masses."""
    import torch

    from aiyagari_hark_amd import _lib
    from aiyagari_hark_amd.transition import path_variable_stats, transition_forward
    for batch, _, K, T in shapes(ss120, ss25):
        n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
        buf = path_problem(batch, K, T)
        Ks0, C0, mT0 = sweep(batch, buf, T, None)
        masses = torch.full((T + 1, n_cal, S, n_a), -7.0, dtype=torch.float64, device=batch.device)
        Ks1, C1, mT1 = sweep(batch, buf, T, masses)
        assert np.array_equal(Ks0, Ks1) and np.array_equal(C0, C1) and torch.equal(mT0, mT1)
        mass = batch.mass.clone()
        assert torch.equal(masses[0], mass)
        for t in range(T):
            transition_forward(batch, buf.lo[t:t + 1], buf.wlo[t:t + 1], mass, 1, buf.work, want_c=False)
            assert torch.equal(masses[t + 1], mass), (T, t)
        assert torch.equal(masses[T], mT0)
        # the statistics of consumption, income and saving along the path
        names = ("consumption", "income", "saving")
        stats, moments = path_variable_stats(batch, buf.lo, buf.wlo, buf.R, buf.w, masses, PCT, names)
        assert set(stats) == {"consumption", "income"} and set(moments) == set(names)
        assert stats["income"].gini.shape == (n_cal, T + 1) and stats["income"].lorenz.shape == (n_cal, T + 1, PCT.size)
        hm = masses.cpu().numpy()
        lo, wlo = buf.lo.cpu().numpy(), buf.wlo.cpu().numpy()
        for i in range(n_cal):
            per = [VR.variables(batch.aGrid[i], batch.levels[i], buf.hR[i, t], buf.hw[i, t], lo[min(t, T - 1), i],
                                wlo[min(t, T - 1), i], names) for t in range(T + 1)]
            for name in ("consumption", "income"):
                ref = ref_stack(np.stack([p[name] for p in per]), hm[:, i])
                one = types.SimpleNamespace(**{k: getattr(stats[name], k)[i] for k in FIELDS})
                compare(one, ref, f"path S={S} n_a={n_a} T={T} cal {i} {name}")
            for t in range(T + 1):
                sw, mean, cov = VR.moments([per[t]["saving"]], hm[t, i])
                assert abs(moments["saving"]["mean"][i, t] - mean[0]) <= RTOL * np.sqrt(cov[0, 0])
                assert rel_err(moments["saving"]["std"][i, t], np.sqrt(cov[0, 0])) <= RTOL
        c = stats["consumption"]
        e = np.max(np.abs(c.mean[:, :T] * c.total[:, :T] - C1) / C1)
        print(f"  mean(c) x total against the sweep's C: {e:.1e}")
        assert e <= RTOL

    # refusal: a decreasing lottery row leaves mass_path, mass, Ks and C untouched
    batch, _, K = pick(ss120, [0, 2, 3])
    T = 5
    buf = path_problem(batch, K, T)
    lo = buf.lo.clone()
    row = lo[2, 1, 3]
    j = int(torch.nonzero(row >= 1)[0]) + 1
    row[j] = row[j - 1] - 1
    n_cal, n_a = len(batch.cals), batch.n_a
    mass = batch.mass.clone()
    masses = torch.full((T + 1, n_cal, batch.S, n_a), -7.0, dtype=torch.float64, device=batch.device)
    Ks = np.full((n_cal, T + 1), -7.0)
    Cc = np.full((n_cal, T), -7.0)
    h = _lib.handle(batch.device.index)

    def call(lottery):
        return h.lib.aiy_transition_forward_masses(
            h.h, n_cal, batch.S, n_a, T, _lib.ptr(lottery), _lib.ptr(buf.wlo), _lib.ptr(batch.d_P),
            _lib.ptr(batch.d_a), _lib.ptr(buf.R), _lib.ptr(buf.w), _lib.ptr(batch.d_lab), _lib.ptr(buf.work),
            _lib.ptr(mass), Ks.ctypes.data_as(_lib.c_double_p), Cc.ctypes.data_as(_lib.c_double_p), _lib.ptr(masses),
            _lib.stream_ptr())

    rc = call(lo)
    torch.cuda.synchronize()
    assert rc == -4
    assert np.all(Ks == -7.0) and np.all(Cc == -7.0) and torch.equal(mass, batch.mass)
    assert bool(torch.all(masses == -7.0))
    with pytest.raises(_lib.AiyagariLibError):
        transition_forward(batch, lo, buf.wlo, mass, T, buf.work, buf.R, buf.w, mass_path=masses)
    assert bool(torch.all(masses == -7.0)) and torch.equal(mass, batch.mass)
    with pytest.raises(ValueError):
        transition_forward(batch, buf.lo, buf.wlo, mass, T, buf.work, buf.R, buf.w, mass_path=masses, rows="any")
    assert call(buf.lo) == 0
    assert np.all(Ks > 0) and np.all(Cc > 0) and bool(torch.all(masses >= 0.0))


def test_solve_transition_with_variables(ss120):
    """5, the solver: [A, B], T = 5, Newton: the path is the one solved without variables bit for
    bit and var_stats of wealth in period 0 has the bits of batch_inequality.  (Period 0 of a path
    after a shock has the path's own prices and lottery, so only wealth, which depends on neither,
    can share the steady state's bits; consumption and income are held to the reference above.)"""
    from aiyagari_hark_amd.stats import batch_inequality
    from aiyagari_hark_amd.transition import household_jacobian, solve_transition
    batch, r, _ = pick(ss120, [0, 1])
    T = 5
    Z = TR.shock_path(T)
    jac = household_jacobian(batch, r, T)
    plain = solve_transition(batch, Z, T, method="newton", jacobian=jac, percentiles=PCT)
    names = ("wealth", "consumption", "income", "saving")
    res = solve_transition(batch, Z, T, method="newton", jacobian=jac, percentiles=PCT, variables=names)
    assert plain.var_stats is None and plain.var_moments is None
    for k in ("K", "r", "w", "C", "iterations", "residual", "status"):
        assert np.array_equal(getattr(plain, k), getattr(res, k)), k
    assert all(np.array_equal(getattr(plain.stats, k), getattr(res.stats, k), equal_nan=True)
               for k in ("lorenz", "percentile_values", "gini", "mean", "total", "bottom_share"))
    assert set(res.var_stats) == {"wealth", "consumption", "income"} and set(res.var_moments) == set(names)
    assert res.var_stats["consumption"].gini.shape == (2, T + 1)
    assert res.var_stats["consumption"].lorenz.shape == (2, T + 1, PCT.size)
    ineq = batch_inequality(batch, PCT, ("wealth", "consumption"))
    assert all(np.array_equal(getattr(res.var_stats["wealth"], k)[:, 0], getattr(ineq.stats["wealth"], k), equal_nan=True)
               for k in FIELDS)
    # wealth along the path: the merged statistics against the marginal ones of percentiles=
    for k in ("lorenz", "gini", "mean", "total"):
        assert rel_err(getattr(res.var_stats["wealth"], k), getattr(res.stats, k)) <= RTOL, k
    c = res.var_stats["consumption"]
    e = np.max(np.abs(c.mean[:, :T] * c.total[:, :T] - res.C) / res.C)
    print(f"mean(c) x total against the solved path's C: {e:.1e}; gini of consumption, A {np.round(c.gini[0], 5)}")
    assert e <= RTOL
    with pytest.raises(ValueError):
        solve_transition(batch, Z, T, method="newton", jacobian=jac, variables=names)


def test_worst_errors_are_reported():
    """Prints the worst error of every field over the cases above (DESIGN.md §4t quotes them)."""
    print("worst errors: " + "  ".join(f"{k} {v:.1e}" for k, v in sorted(WORST.items())))
    assert all(np.isfinite(v) for v in WORST.values())
