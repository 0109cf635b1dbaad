"""GPU tests of one EGM step (csrc/egm.hip: egm_cycle_kernel through aiy_egm_step, and
aiy_policy_eval) against the references of tests/egm_ref.py: every state-count instantiation and
both sides of every dispatch edge, idle waves (S < 4), grid sizes around the tile and the window,
hints that are cold, fresh, stale or useless, two rows per state at a generic S, and the
stationary branch of the policy evaluation.

Every stationary case runs CRRA 1, 3, 5 and 2.5 as four calibrations of one launch, each fed its
own tables, so a calibration that read another's inputs would miss its reference.  CRRA = 1 is
held bit for bit to the float64 oracle step (the kernels follow NumPy's operation order,
csrc/common.h).  The other kinds are held to the long-double step: the references agree with each
other to 7e-16 (tests/test_egm_ref.py), so what is left is the kernel's closed power forms
(rcbrt; the refined powf; the device pow).  Largest relative gaps on m and c measured on the
MI355X on the first run, over all cases of this module: CRRA 3: 4.41e-16 (S = 7, n_a = 1437),
CRRA 5: 4.47e-16 (S = 9, n_a = 700), CRRA 2.5: 6.14e-16 (S = 17, n_a = 200), two to three ulp;
the bounds are ten times those (drift of the device math library and the compiler), far below
the 1e-12 of test_egm_single_steps.  CRRA = 1 was bit-equal at every state count, S < 4 included.
"""
import functools

import numpy as np
import pytest

from oracle import hark_ks as H
from tests import egm_ref as ER
from tests.test_egm_ref import BETA, problem

pytestmark = pytest.mark.gpu

CRRAS = (1.0, 3.0, 5.0, 2.5)
# CRRA 1: bit for bit; the others: the gaps measured on the MI355X (docstring above), times 10
TOL = {1.0: 0.0, 3.0: 10 * 4.41e-16, 5.0: 10 * 4.47e-16, 2.5: 10 * 6.14e-16}
assert max(TOL.values()) <= 1e-12
N_FED = 3    # steps after the terminal one


def frozen(*arrays):
    for x in arrays:
        x.setflags(write=False)
    return arrays


def reference(rho):
    return ER.step64 if rho == 1.0 else ER.step_ld


def args_of(p, rho):
    return (BETA, rho, p["aGrid"], p["R"], p["w"], p["lab"], p["P"])


@functools.lru_cache(maxsize=None)
def chain(S, n_a, steps=N_FED):
    """Per CRRA kind the reference's own tables: [0] the terminal step, [k] the step fed [k - 1]."""
    p = problem(S, n_a)
    out = {}
    for rho in CRRAS:
        tabs = [frozen(*reference(rho)(None, None, *args_of(p, rho)))]
        for _ in range(steps):
            tabs.append(frozen(*reference(rho)(*tabs[-1], *args_of(p, rho))))
        out[rho] = tabs
    return p, out


def batch_of(p, dev):
    """The four calibrations as one stationary EgmBatch (n_M = 1), as test_gpu_transition.chained."""
    import torch

    from aiyagari_hark_amd.egm import EgmBatch
    n, S = len(CRRAS), p["lab"].size
    rep = lambda x: torch.as_tensor(np.ascontiguousarray(np.broadcast_to(x, (n,) + np.shape(x)))).to(dev)  # noqa: E731
    zM = torch.zeros((n, 1, S), dtype=torch.float64, device=dev)
    return EgmBatch(rep(p["aGrid"]), torch.zeros((n, 1), dtype=torch.float64, device=dev), rep(p["P"]),
                    torch.full_like(zM, p["R"]), torch.full_like(zM, p["w"]), zM, rep(p["lab"]),
                    torch.full((n,), BETA, dtype=torch.float64, device=dev),
                    torch.as_tensor(np.array(CRRAS)).to(dev))


def up(dev, tabs):
    """Per-calibration host tables [S][n_a + 1] -> the device tables [n_cal][S][1][n_a + 1]."""
    import torch
    return tuple(torch.as_tensor(np.stack([t[i] for t in tabs])[:, :, None, :].copy()).to(dev) for i in (0, 1))


def down(tabs):
    return tuple(t.cpu().numpy()[:, :, 0, :] for t in tabs)


def forget_hints(dev):
    """A step of a shape no test uses: the handle resets its row hints at the next other shape."""
    from aiyagari_hark_amd.egm import egm_step
    egm_step(batch_of(problem(4, 3), dev))


def check(got, want, what, worst):
    """got: host (m, c) [n_cal][S][n_a + 1]; want: per CRRA kind the reference's (m, c)."""
    for i, rho in enumerate(CRRAS):
        for g, x, name in zip((got[0][i], got[1][i]), want[rho], "mc"):
            assert not np.isnan(x).any() and not np.isnan(g).any(), (what, rho, name)
            gap = ER.rel_gap(g, x)
            worst[rho] = max(worst[rho], gap)
            print(f"{what} CRRA {rho} {name}: rel gap {gap:.3e}")
            if rho == 1.0:
                assert np.array_equal(g, x), (what, name, gap)
            else:
                assert gap <= TOL[rho], (what, rho, name, gap)


def run_sequence(dev, S, n_a):
    """The terminal step, then N_FED steps each fed the reference's tables of the step before:
    the first on cold hints, the next ones on the hints of the cycle before."""
    from aiyagari_hark_amd.egm import egm_step
    p, ref = chain(S, n_a)
    b = batch_of(p, dev)
    worst = dict.fromkeys(CRRAS, 0.0)
    forget_hints(dev)
    check(down(egm_step(b)), {rho: ref[rho][0] for rho in CRRAS}, f"S={S} n_a={n_a} terminal", worst)
    for k in range(1, N_FED + 1):
        fed = up(dev, [ref[rho][k - 1] for rho in CRRAS])
        check(down(egm_step(b, *fed)), {rho: ref[rho][k] for rho in CRRAS}, f"S={S} n_a={n_a} step {k}", worst)
    print(f"S={S} n_a={n_a} worst: " + "  ".join(f"CRRA {rho}: {worst[rho]:.3e}" for rho in CRRAS))


@pytest.mark.parametrize("S", (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 25, 32, 33, 64))
def test_state_counts(gpu, S):
    """a: every instantiation (<8,7> <32,25> <8,0> <16,0> <32,0> <64,0>; <32,28> is the KS
    tests'), both sides of every dispatch edge, waves without a next state (S < 4), S no multiple
    of 4 or 8; n_a = 200 = 3 x 64 + 8 moves the window base and leaves a ragged last tile."""
    run_sequence(gpu, S, 200)


@pytest.mark.parametrize("n_a", (2, 63, 64, 65, 127, 128, 1437))
@pytest.mark.parametrize("S", (7, 9))
def test_grid_sizes(gpu, S, n_a):
    """b: the ABI minimum, the tile edges, n_a + 1 - 128 at <= 0, 0 and 1, an odd many-tile size."""
    run_sequence(gpu, S, n_a)


@pytest.mark.parametrize("S", (7, 9))
def test_hints_never_change_a_bit(gpu, S):
    """c: 'a stale or foreign hint costs a global search, never a different result' (egm.hip).
    T_a, the reference's tables after two steps, fits the window in every tile; tile 3 of T_b
    (egm_ref.dense_tables) spans more than 128 nodes in every row, so its window never holds the
    brackets and the rows are redone from global memory every time."""
    import torch

    from aiyagari_hark_amd.egm import egm_step
    n_a = 700
    p, ref = chain(S, n_a, 2)
    geo = (p["aGrid"], p["R"], p["w"], p["lab"])
    Ta = [ref[rho][1] for rho in CRRAS]
    Tb = frozen(*ER.dense_tables(S, n_a, *geo))
    for t in Ta:
        assert np.all(ER.tile_spans(t[0], *geo) < ER.WINDOW)
    sp = ER.tile_spans(Tb[0], *geo)
    assert np.all(sp[:, 3] > ER.WINDOW) and np.all(np.delete(sp, 3, axis=1) < ER.WINDOW)
    want_a = {rho: ref[rho][2] for rho in CRRAS}
    want_b = {rho: reference(rho)(*Tb, *args_of(p, rho)) for rho in CRRAS}
    b = batch_of(p, gpu)
    da, db = up(gpu, Ta), up(gpu, [Tb] * len(CRRAS))
    egm_step(batch_of(problem(S, n_a + 1), gpu))   # another shape: the hints reset
    runs = [("T_a cold", da), ("T_a own hints", da), ("T_b stale hints", db), ("T_b own hints", db),
            ("T_a stale hints", da)]
    outs = [egm_step(b, *fed) for _, fed in runs]
    worst = dict.fromkeys(CRRAS, 0.0)
    for (what, fed), out in zip(runs, outs):
        check(down(out), want_a if fed is da else want_b, f"S={S} {what}", worst)
    for k in (1, 4):
        assert torch.equal(outs[k][0], outs[0][0]) and torch.equal(outs[k][1], outs[0][1]), runs[k][0]
    assert torch.equal(outs[3][0], outs[2][0]) and torch.equal(outs[3][1], outs[2][1])


def test_two_rows_per_state_generic_state_count(gpu):
    """d: the Krusell-Smith form (n_M = 15, two M' rows per next state) with 5 labour states:
    S = 20, the generic <32,0> instantiation.  CRRA = 1, a cold and a hinted step, bit for bit."""
    import torch

    from aiyagari_hark_amd.egm import egm_step
    from tests.test_gpu_parity import batch_from_fixture
    m = H.KSModel(dict(LaborStatesNo=5), dict(aCount=200, LaborStatesNo=5))
    Rk, Wk, Mk = H.next_prices(m.AFunc, m.Mgrid, 5, m.e)
    assert m.MrkvIndArray.shape == (20, 20)
    args = (0.96, 1.0, m.aGrid, m.Mgrid, Rk, Wk, Mk, m.LSStates, m.MrkvIndArray)
    tabs = [H.egm_step(None, None, *args)]
    for _ in range(2):
        tabs.append(H.egm_step(*tabs[-1], *args))
    b = batch_from_fixture(dict(aGrid=m.aGrid, Mgrid=m.Mgrid, P=m.MrkvIndArray, LSStates=m.LSStates, Rk=Rk, Wk=Wk,
                                Mk=Mk, DiscFac=0.96, CRRA=1.0), gpu)
    forget_hints(gpu)
    for k in (1, 2):
        om, oc = egm_step(b, *(torch.as_tensor(t[None]).to(gpu) for t in tabs[k - 1]))
        assert not np.isnan(tabs[k][0]).any()
        assert np.array_equal(om[0].cpu().numpy(), tabs[k][0]), k
        assert np.array_equal(oc[0].cpu().numpy(), tabs[k][1]), k


def test_policy_eval_stationary_branch(gpu):
    """e: aiy_policy_eval with n_M = 1 (one row per state) against HARK's LinearInterp: every
    node and its two neighbouring doubles, uniform queries, queries below the first node (NaN)
    and above the last (extrapolated), states outside [0, S) (NaN).  Bit for bit."""
    import torch

    from aiyagari_hark_amd.egm import policy_eval
    S, n_a = 7, 700
    _, ref = chain(S, n_a, 2)
    mt, ct = ref[1.0][1]
    rng = np.random.default_rng(7)
    st, q, want = [], [], []
    for s in range(S):
        x = mt[s]
        qs = np.concatenate((x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf),
                             rng.uniform(x[0], x[-1], 1000), [-1.0, 0.0, 0.5e-7],
                             [1.5 * x[-1], x[-1] + 100.0]))
        st.append(np.full(qs.size, s))
        q.append(qs)
        want.append(H.LinearInterp(x, ct[s])(qs))
    for s in (-1, S):
        qs = rng.uniform(0.1, 10.0, 50)
        st.append(np.full(qs.size, s))
        q.append(qs)
        want.append(np.full(qs.size, np.nan))
    st, q, want = (np.concatenate(v) for v in (st, q, want))
    dm, dc = (torch.as_tensor(t[:, None, :].copy()).to(gpu) for t in (mt, ct))
    got = policy_eval(dm, dc, None, st, q).cpu().numpy()
    nan = np.isnan(want)
    assert nan.sum() == S * 4 + 100   # per state: three below x[0] and the double below node 0
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan], want[~nan])
