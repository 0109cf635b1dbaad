"""GPU tests of every form of the stationary-distribution solve behind aiy_hist_solve, each held to
the dense-matrix reference of tests/hist_ref.py (the conditions its cases rely on are pinned on
the CPU by tests/test_hist_ref.py).

The driver calls aiy_hist_solve directly on synthetic lotteries, selects the form with the
handle's options and proves which path ran: the launch count of aiy_hist_launch_stats (zero
for push/mix and the fused step, ceil(n_cal / calibrations per launch) of the mirrored plan for a
resident form) and the caller's work space: a resident solve leaves it alone, push/mix leaves
its accumulator zero, the fused step leaves its source ranges there (so a resident or fused solve
that fell back to push/mix shows).

Which case runs which kernel instantiation (cap = AIY_OPT_HIST_CLUSTER, 0 the default):
  hist_push_kernel + hist_mix_kernel<8>   pushmix f1x255 f2x2 f8x256      <16> f9x257 f16x257
                                          <32> f17x120 f32x100            <64> f33x100 f64x64
  hist_step_kernel<8>  fused f7x256 f7x257          <64> fused f64x64 (S kHistTile 8 = 128 KB)
  hist_cluster_kernel<8,1,512>   cluster f1x1024/0 f3x200/2,3 f8x512/1 s7x300/0
  hist_cluster_kernel<8,2,512>   cluster f1x1024/1 f4x1024/1 (G = 1, nj = 1024: every thread two
                                 columns) f2x1025/1 (g_min = 2: G = 2, nj = 513) f8x513/1 s3x600/1
  hist_cluster_kernel<16,1,512>  cluster f9x200/3 f16x257/0, aitken s12x150
  hist_cluster_kernel<32,1,512>  cluster f17x120/2 f32x100/0      (f33x100: falls back, push/mix)
  Aitken mode (accel 8)          aitken s7x300 (<8,1>) s12x150 (<16,1>)
  hist_bicg_kernel<8,1,512,false>  bicg f1x1024/0 f6x513/2 f7x300/0,3 f8x512/1 s7x300/0 s3x600/0
  hist_bicg_kernel<8,2,512,false>  bicg f1x1024/1 f4x1024/1 f2x1025/1 f8x513/1 s3x600/1
  hist_bicg_kernel<7,2,512,false>  bicg f7x520/1
  hist_bicg_kernel<7,1,512,true>   pull f7x300/0,3 s7x300/0       <7,2,512,true>  pull f7x520/1
  hist_bicg_kernel<8,1,512,true>   pull f1x1024/0 f6x513/2 f8x512/1 s3x600/0
  hist_bicg_kernel<8,2,512,true>   pull f1x1024/1 f4x1024/1 f2x1025/1 f8x513/1 s3x600/1
  hist_pull_kernel<32,512>  pullmany f9x200 f10x150 f11x130 f15x100 f16x200 f25x100 f26x100
                            f32x100 s12x150 (groups of kHpGrp = 5 states, full and ragged)
  hist_pull_kernel<64,512>  pullmany f33x100 f64x64
  (not covered: at every shape a dense matrix allows, N <= 4200, hist_pull_plan puts a workgroup's
  columns into ONE chunk, cw = n_own; the many-state form's multi-chunk matvec needs thousands of
  columns per workgroup and is reached only by tests/test_gpu_hist_resident.py at 25 x 50 000)
  the c0 += per_launch loop of hist_solve_resident: test_more_cells_than_one_launch

Largest observed ratio of a residual to its bound, per form, over every case of this module
(first GPU run, MI355X; test_zz_report_ratios prints them again):
                sum|T m - m| / bound    max|T m - m| / bound
  pushmix             0.620                   0.549
  fused               0.114                   0.044
  cluster             0.212                   0.271
  aitken              0.006                   0.026
  bicg                0.178                   0.288
  pull                0.178                   0.288
  pullmany            0.211                   0.253
(pushmix: the two-node grid of f2x2, where N tol is 4e-12; elsewhere below 0.3.)
"""
import ctypes

import numpy as np
import pytest

from tests import hist_ref as HR

pytestmark = pytest.mark.gpu

EPS = HR.EPS
TOL = HR.TOL
# (sum ratio, max ratio) per form of the cases run so far in this process
RATIOS = {}

PLAIN = ("pushmix", "fused", "cluster")
KRYLOV = ("bicg", "pull", "pullmany")
NO_ATOMICS = ("pull", "pullmany")
RESIDENT = ("cluster", "aitken") + KRYLOV


def _options(form, cap):
    from aiyagari_hark_amd import _lib as L
    o = {L.AIY_OPT_HIST_RESIDENT: int(form in RESIDENT), L.AIY_OPT_HIST_FUSED: int(form == "fused"),
         L.AIY_OPT_HIST_KRYLOV: int(form in KRYLOV), L.AIY_OPT_HIST_PULL: int(form == "pull"),
         L.AIY_OPT_HIST_ACCEL: 8 if form == "aitken" else 0, L.AIY_OPT_HIST_CLUSTER: int(cap)}
    return o


def _launches(h, reset=True):
    ms, n = ctypes.c_double(), ctypes.c_int64()
    h.check(h.lib.aiy_hist_launch_stats(h.h, ctypes.byref(ms), ctypes.byref(n), int(reset)), "stats")
    return n.value


def solve(gpu, form, cap, aGrid, lo, wlo, P, mass0, tol=TOL, max_iter=100000):
    """One aiy_hist_solve in the given form.  Returns (mass, K, iters, resident launches, who wrote
    the caller's work space).  A resident solve leaves it alone (""); the push/mix pair keeps its
    accumulator T = work[0] zero between iterations ("pushmix"); the fused step keeps the tile
    source ranges there, integers that are not all zero ("fused"), and a fused solve that fell
    back to push/mix has zeroed them."""
    import torch
    from aiyagari_hark_amd import _lib
    h = _lib.handle(gpu.index)
    n_cal, S, n_a = lo.shape
    up = lambda x, dt: torch.as_tensor(np.array(x, dtype=dt, order="C")).to(gpu)   # noqa: E731
    d_lo, d_w, d_P = up(lo, np.int32), up(wlo, np.float64), up(P, np.float64)
    d_a = up(np.broadcast_to(aGrid, (n_cal, n_a)), np.float64)
    d_m = up(mass0, np.float64)
    work = torch.full((2, n_cal, S, n_a), float("nan"), dtype=torch.float64, device=gpu)
    K = (ctypes.c_double * n_cal)()
    iters = (ctypes.c_int32 * n_cal)()
    prev = h.set_options(_options(form, cap))
    try:
        _launches(h)
        h.check(h.lib.aiy_hist_solve(h.h, n_cal, S, n_a, _lib.ptr(d_lo), _lib.ptr(d_w), _lib.ptr(d_P), _lib.ptr(d_a),
                                     float(tol), int(max_iter), 64, _lib.ptr(d_m), _lib.ptr(work), K, iters,
                                     _lib.stream_ptr()), "aiy_hist_solve")
        n = _launches(h)
    finally:
        h.set_options(prev)
    if bool(torch.isnan(work).all().item()):
        touched = ""
    else:
        touched = "pushmix" if bool((work[0].view(torch.int64) == 0).all().item()) else "fused"
    return d_m.cpu().numpy(), np.array(K[:]), np.array(iters[:]), n, touched


def plan(gpu, form, cap, n_cal, S, n_a):
    """(G, columns per workgroup, calibrations per launch) of a resident form: hc_make_plan and
    hc_cluster_split of csrc/hist_resident.hip / hist_cluster.h restated (at these grid sizes the
    many-state pull form's LDS holds every column of a workgroup, so its least G is 1)."""
    import torch
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    if form == "pullmany":
        g_min, g_cap = 1, cap if cap > 0 else 128
    else:
        kc_max = 2 if S <= 8 else 1
        g_min, g_cap = -(-n_a // (512 * kc_max)), cap if cap > 0 else 32
    g = min(max(g_min, min(g_cap, 128, cus // max(1, n_cal))), n_a)
    nj = -(-n_a // g)
    G = -(-n_a // nj)
    return G, nj, max(1, cus // G)


# ------------------------------------------------------------------------------------------
# references, cached per case and calibration
# ------------------------------------------------------------------------------------------
_REF = {}


def ref(key, c, lo, wlo, P, want_pi=False):
    """(csr of T, norm_inf(T), pi or None) of calibration c of the batch named by key."""
    r = _REF.get((key, c))
    if r is None or (want_pi and r[2] is None):
        T = HR.dense_T(lo[c], wlo[c], P[c])
        pi = HR.stationary(T) if want_pi else None
        r = (HR.csr(T), HR.norm_inf(T), pi)
        _REF[(key, c)] = r
    return r


def check(form, key, lo, wlo, P, aGrid, m0, m, K, iters, max_iter=100000, cals=None, label="", pi_of=(0,)):
    """The assertions of every form and case, per solved calibration; bounds from the reference
    matrix.  lo, wlo, P: the batch named by key; cals: which of its calibrations were solved, in
    the order of m0, m, K and iters (None: all of them, in order)."""
    S, n_a = lo.shape[1:]
    N = S * n_a
    worst = RATIOS.setdefault(form, [0.0, 0.0])
    for c in range(m.shape[0]):
        rc = c if cals is None else int(cals[c])
        total = float(np.sum(m0[c].astype(HR.LD)))
        A, ninf, pi = ref(key, rc, lo, wlo, P, want_pi=rc in pi_of)
        b1, bmax = HR.residual_bounds(N, ninf, TOL, total)
        s1, smax = HR.residuals(A, m[c])
        worst[0], worst[1] = max(worst[0], s1 / b1), max(worst[1], smax / bmax)
        msg = f"{form} {key}{label} cal {rc}: sum {s1:.3e} / {b1:.3e}, max {smax:.3e} / {bmax:.3e}, iters {iters[c]}"
        if pi is not None:
            print(f"\n{msg}, sum|m - pi| {np.abs(m[c].ravel() / total - pi).sum():.3e}", end="")
        assert s1 <= b1 and smax <= bmax, msg
        assert 1 <= iters[c] <= max_iter, msg
        got = float(np.sum(m[c].astype(HR.LD)))
        assert abs(got - total) <= (S + 4) * EPS * (int(iters[c]) + 1) * total, (msg, got, total)
        Kref = float(np.sum(m[c].astype(HR.LD) * aGrid.astype(HR.LD)[None, :]))
        assert abs(K[c] - Kref) <= N * EPS * abs(Kref), (msg, K[c], Kref)


def uniform(lo):
    n_cal, S, n_a = lo.shape
    return np.full((n_cal, S, n_a), 1.0 / (S * n_a))


def check_path(gpu, form, cap, lo, n, touched, no_plan=False):
    n_cal, S, n_a = lo.shape
    if form not in RESIDENT or no_plan:   # (no plan for the shape: push/mix without a launch)
        assert n == 0, f"{n} resident launches in the {form} form"
        assert touched == ("fused" if form == "fused" else "pushmix"), touched
        return
    assert n >= 1, "the resident path did not run"
    assert not touched, "the resident form fell back to push/mix"
    G, nj, per = plan(gpu, form, cap, n_cal, S, n_a)
    assert n == -(-n_cal // per), (n, n_cal, per)


# ------------------------------------------------------------------------------------------
# every form at its smallest shapes
# ------------------------------------------------------------------------------------------
MAIN = (
    [("pushmix", k, 0) for k in ("f1x255", "f2x2", "f8x256", "f9x257", "f16x257", "f17x120", "f32x100", "f33x100",
                                 "f64x64")]
    + [("fused", k, 0) for k in ("f7x256", "f7x257", "f64x64")]
    + [("cluster", "f1x1024", 0), ("cluster", "f1x1024", 1), ("cluster", "f4x1024", 1), ("cluster", "f2x1025", 1), ("cluster", "f3x200", 2), ("cluster", "f3x200", 3),
       ("cluster", "f8x512", 1), ("cluster", "f8x513", 1), ("cluster", "f9x200", 3), ("cluster", "f16x257", 0),
       ("cluster", "f17x120", 2), ("cluster", "f32x100", 0), ("cluster", "f33x100", 0), ("cluster", "s7x300", 0),
       ("cluster", "s3x600", 1)]
    + [("aitken", "s7x300", 0), ("aitken", "s12x150", 0)]
    + [(f, k, cap) for f in ("bicg", "pull") for k, cap in
       (("f1x1024", 0), ("f1x1024", 1), ("f4x1024", 1), ("f2x1025", 1), ("f6x513", 2), ("f7x300", 3), ("f7x300", 0), ("f7x520", 1), ("f8x512", 1),
        ("f8x513", 1), ("s7x300", 0), ("s3x600", 1), ("s3x600", 0))]
    + [("pullmany", k, cap) for k, cap in
       (("f9x200", 1), ("f10x150", 3), ("f11x130", 0), ("f15x100", 1), ("f16x200", 3), ("f25x100", 0), ("f26x100", 1),
        ("f32x100", 3), ("f33x100", 0), ("f64x64", 1), ("s12x150", 0), ("s12x150", 3))]
)


@pytest.mark.parametrize("form,key,cap", MAIN, ids=[f"{f}-{k}-cap{c}" for f, k, c in MAIN])
def test_form_meets_the_matrix_bounds(gpu, form, key, cap):
    family, S, n_a, n_cal, _ = HR.CASES[key]
    aGrid, lo, wlo, P = HR.batch(key)
    m0 = uniform(lo)
    m, K, it, n, touched = solve(gpu, form, cap, aGrid, lo, wlo, P, m0)
    no_plan = form == "cluster" and S > 32           # the push forms hold up to 32 states
    check_path(gpu, form, cap, lo, n, touched, no_plan)
    if n_a == 1024 and cap == 1:     # the lower side of the g_min edge: one workgroup, every thread two columns
        assert plan(gpu, form, cap, n_cal, S, n_a)[:2] == (1, 1024)
    if n_a == 1025 and cap == 1:     # the upper side: g_min = 2 overrides the cap
        assert plan(gpu, form, cap, n_cal, S, n_a)[:2] == (2, 513)
    check(form, key, lo, wlo, P, aGrid, m0, m, K, it)
    if form in PLAIN:
        mref, itref = HR.plain(key)
        assert np.max(np.abs(it - itref)) <= 1, (it, itref)
        if family == "fast":
            assert np.max(np.abs(m - mref)) < 1e-13
    if form in NO_ATOMICS:
        m2, K2, it2, _, _ = solve(gpu, form, cap, aGrid, lo, wlo, P, m0)
        assert np.array_equal(m, m2) and np.array_equal(it, it2) and np.array_equal(K, K2), "repeat differs"


# alone / inside the batch / inside the reversed batch, the cluster cap fixed so that G does not
# depend on the batch
ORDER = [("cluster", "f7x300", 3), ("cluster", "f9x200", 3), ("bicg", "f7x300", 3), ("bicg", "s7x300", 2),
         ("pull", "f7x300", 3), ("pull", "s7x300", 2), ("pull", "f8x513", 1), ("pullmany", "f10x150", 3),
         ("pullmany", "s12x150", 1), ("pullmany", "f33x100", 3)]


@pytest.mark.parametrize("form,key,cap", ORDER, ids=[f"{f}-{k}-cap{c}" for f, k, c in ORDER])
def test_alone_batch_reversed(gpu, form, key, cap):
    aGrid, lo, wlo, P = HR.batch(key)
    n_cal = lo.shape[0]
    m0 = uniform(lo)
    mb, Kb, itb, n, touched = solve(gpu, form, cap, aGrid, lo, wlo, P, m0)
    check_path(gpu, form, cap, lo, n, touched)
    rev = np.arange(n_cal)[::-1]
    mr, Kr, itr, n, touched = solve(gpu, form, cap, aGrid, lo[rev], wlo[rev], P[rev], m0)
    check_path(gpu, form, cap, lo, n, touched)
    check(form, key, lo, wlo, P, aGrid, m0, mr, Kr, itr, cals=list(rev), label=" reversed", pi_of=())
    c = n_cal - 1   # the slowest calibration, alone
    ma, Ka, ita, n, touched = solve(gpu, form, cap, aGrid, lo[c:], wlo[c:], P[c:], m0[c:])
    check_path(gpu, form, cap, lo[c:], n, touched)
    check(form, key, lo, wlo, P, aGrid, m0, ma, Ka, ita, cals=[c], label=" alone", pi_of=())
    if form in NO_ATOMICS:
        assert np.array_equal(mr[rev], mb) and np.array_equal(itr[rev], itb), "order in the batch changes a solve"
        assert np.array_equal(ma[0], mb[c]) and ita[0] == itb[c], "the batch changes a solve"


# ------------------------------------------------------------------------------------------
# edge cases of the four resident families
# ------------------------------------------------------------------------------------------
CELLS = [("cluster", "t2x16"), ("cluster", "t3x16"), ("cluster", "t9x16"), ("bicg", "t2x16"), ("bicg", "t3x16"),
         ("pull", "t2x16"), ("pull", "t3x16"), ("pullmany", "t9x16")]


@pytest.mark.parametrize("form,key", CELLS, ids=[f"{f}-{k}" for f, k in CELLS])
def test_more_cells_than_one_launch(gpu, form, key):
    """multi_processor_count + 3 tiny cells: the c0 += per_launch loop of hist_solve_resident, its
    cal0 / lc indexing of slabs, granules and v blocks."""
    import torch
    n_cal = torch.cuda.get_device_properties(gpu).multi_processor_count + 3
    assert n_cal <= HR.CASES[key][3], "the case table holds fewer cells than this device needs"
    aGrid, lo, wlo, P = HR.batch(key)
    lo, wlo, P = lo[:n_cal], wlo[:n_cal], P[:n_cal]
    m0 = uniform(lo)
    m, K, it, n, touched = solve(gpu, form, 0, aGrid, lo, wlo, P, m0)
    G, nj, per = plan(gpu, form, 0, n_cal, lo.shape[1], lo.shape[2])
    assert per < n_cal and n == -(-n_cal // per) and n >= 2, (n, per)
    assert not touched
    check(form, key, lo, wlo, P, aGrid, m0, m, K, it, pi_of=())
    if form == "cluster":
        mref, itref = HR.plain(key)
        assert np.max(np.abs(it - itref[:n_cal])) <= 1
        assert np.max(np.abs(m - mref[:n_cal])) < 1e-13


EDGE = [("cluster", "f7x300", 3), ("bicg", "f7x300", 3), ("pull", "f7x300", 3), ("pullmany", "f10x150", 3)]
EDGE_IDS = [f"{f}-{k}" for f, k, _ in EDGE]


@pytest.mark.parametrize("total", [0.5, 3.0])
@pytest.mark.parametrize("form,key,cap", EDGE, ids=EDGE_IDS)
def test_start_total_is_kept(gpu, form, key, cap, total):
    """A start whose total is not 1: the result keeps it (the BiCGSTAB forms rescale to the start's
    total) and meets the bounds scaled by it."""
    aGrid, lo, wlo, P = HR.batch(key)
    m0 = uniform(lo) * total
    m, K, it, n, touched = solve(gpu, form, cap, aGrid, lo, wlo, P, m0)
    check_path(gpu, form, cap, lo, n, touched)
    check(form, key, lo, wlo, P, aGrid, m0, m, K, it, label=f" total {total}", pi_of=())


@pytest.mark.parametrize("form,key,cap", EDGE, ids=EDGE_IDS)
def test_converged_start_stops_at_once(gpu, form, key, cap):
    """The device's own result fed back.  A plain form stops at iteration 1 (the first change is
    below tol).  A BiCGSTAB form (hk_solve / hp_solve) forms the true residual of the start with one
    matvec, finds max|T x - x| < tol at mv == 1 and returns T x unscaled: exactly 1 matvec."""
    aGrid, lo, wlo, P = HR.batch(key)
    m1, _, _, _, _ = solve(gpu, form, cap, aGrid, lo, wlo, P, uniform(lo))
    m, K, it, n, touched = solve(gpu, form, cap, aGrid, lo, wlo, P, m1)
    check_path(gpu, form, cap, lo, n, touched)
    assert np.all(it == 1), it
    check(form, key, lo, wlo, P, aGrid, m1, m, K, it, label=" converged start", pi_of=())


CAPPED = [("cluster", "s7x300", 3), ("bicg", "s7x300", 3), ("pull", "s7x300", 3), ("pullmany", "s12x150", 3)]


@pytest.mark.parametrize("form,key,cap", CAPPED, ids=[f"{f}-{k}" for f, k, _ in CAPPED])
def test_solve_that_ends_at_max_iter(gpu, form, key, cap):
    """max_iter = 5 on the slow family (the plain iterate needs over a thousand).
    A plain form returns iters_out == 5 and the fifth iterate: the reference's fifth iterate to
    5 x 8 eps per unit mass, the bound tests/test_hist_ref.py holds one oracle step to.
    A BiCGSTAB form tests mv >= max_iter after the first matvec of an iteration (two matvecs each)
    and then forms the true residual once more, so it returns T x of its last iterate x, rescaled
    to the start's total, after 5 .. 7 matvecs."""
    aGrid, lo, wlo, P = HR.batch(key)
    n_cal, S, n_a = lo.shape
    m0 = uniform(lo)
    m, K, it, n, touched = solve(gpu, form, cap, aGrid, lo, wlo, P, m0, max_iter=5)
    check_path(gpu, form, cap, lo, n, touched)
    if form in PLAIN:
        assert np.all(it == 5), it
        for c in range(n_cal):
            mref, _ = HR.iterate(lo[c], wlo[c], P[c], max_iter=5)
            assert np.max(np.abs(m[c] - mref)) <= 5 * 8 * EPS
    else:
        assert np.all((it >= 5) & (it <= 7)), it
    for c in range(n_cal):
        assert abs(float(np.sum(m[c].astype(HR.LD))) - 1.0) <= (S + 4) * EPS * (int(it[c]) + 1)
        assert np.all(np.isfinite(m[c]))


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("form,key,cap", EDGE, ids=EDGE_IDS)
def test_error_confined_to_one_workgroup(gpu, form, key, cap, where):
    """The converged mass with 1e-6 moved between two neighbouring nodes inside one workgroup's
    columns: a convergence reduction that dropped that workgroup's partial would return at once
    and miss the bounds by six orders of magnitude."""
    aGrid, lo, wlo, P = HR.batch(key)
    n_cal, S, n_a = lo.shape
    G, nj, _ = plan(gpu, form, cap, n_cal, S, n_a)
    assert G >= 3
    w = {"first": 0, "middle": G // 2, "last": G - 1}[where]
    j0, j1 = w * nj, min((w + 1) * nj, n_a)
    m1, _, _, _, _ = solve(gpu, form, cap, aGrid, lo, wlo, P, uniform(lo))
    m0 = m1.copy()
    for c in range(n_cal):
        s, j = np.unravel_index(np.argmax(m0[c][:, j0:j1 - 1]), (S, j1 - 1 - j0))
        m0[c, s, j0 + j] -= 1e-6
        m0[c, s, j0 + j + 1] += 1e-6
    m, K, it, n, touched = solve(gpu, form, cap, aGrid, lo, wlo, P, m0)
    check_path(gpu, form, cap, lo, n, touched)
    assert np.all(it > 1), it
    check(form, key, lo, wlo, P, aGrid, m0, m, K, it, label=f" moved in workgroup {w}", pi_of=())


# ------------------------------------------------------------------------------------------
# rows that are not monotone
# ------------------------------------------------------------------------------------------
ALL_FORMS = [("pushmix", "f7x300"), ("fused", "f7x300"), ("cluster", "f7x300"), ("bicg", "f7x300"),
             ("pull", "f7x300"), ("pullmany", "f10x150")]


def _spiked(key, nj):
    """One interior entry of the middle workgroup's columns (3 workgroups of nj columns) 40 nodes
    above its neighbours, inside the grid and beyond the lottery of the workgroup's last column."""
    aGrid, lo, wlo, P = HR.batch(key)
    lo = lo.copy()
    n_cal, S, n_a = lo.shape
    j, s = 2 * nj - 10, S // 2
    for c in range(n_cal):
        lo[c, s, j] += 40
        assert lo[c, s, 2 * nj - 1] < lo[c, s, j] <= n_a - 2
    return aGrid, lo, wlo, P


def _swapped(key):
    """Neighbouring entries of three rows swapped where they differ: rows whose neighbours are out
    of order, every entry still between its workgroup's end columns."""
    aGrid, lo, wlo, P = HR.batch(key)
    lo, wlo = lo.copy(), wlo.copy()
    n_cal, S, n_a = lo.shape
    for c in range(n_cal):
        for s in (0, S // 2, S - 1):
            n = 0
            for j in range(n_a // 3 + 5, 2 * n_a // 3 - 5):
                if lo[c, s, j] < lo[c, s, j + 1] and n < 4 and j % 7 == 0:
                    lo[c, s, [j, j + 1]] = lo[c, s, [j + 1, j]]
                    wlo[c, s, [j, j + 1]] = wlo[c, s, [j + 1, j]]
                    n += 1
    assert np.any(np.diff(lo, axis=2) < 0)
    return aGrid, lo, wlo, P


@pytest.mark.parametrize("kind", ["spike", "swaps"])
@pytest.mark.parametrize("form,key", ALL_FORMS, ids=[f"{f}-{k}" for f, k in ALL_FORMS])
def test_rows_that_are_not_monotone(gpu, form, key, kind):
    """Any lottery inside the grid through aiy_hist_solve, three workgroups per calibration.  A spike
    beyond the bracket of its workgroup's end columns is refused by every resident form (error 2
    before the first iteration) and by the fused step, and push/mix gives the answer; swapped
    neighbours inside the bracket are harmless to the push forms and refused by the pull forms.
    Either way the result meets the bounds of the matrix of these rows."""
    n_a = HR.CASES[key][2]
    aGrid, lo, wlo, P = _spiked(key, -(-n_a // 3)) if kind == "spike" else _swapped(key)
    m0 = uniform(lo)
    m, K, it, n, touched = solve(gpu, form, 3, aGrid, lo, wlo, P, m0)
    if form in RESIDENT:
        assert n >= 1
        if kind == "spike" or form in NO_ATOMICS:
            assert touched == "pushmix", "a resident form kept rows it must refuse"
        else:
            assert not touched, "a push form refused swapped neighbours inside its bracket"
    else:   # (the fused step's range kernel refuses both kinds: push/mix)
        assert n == 0 and touched == "pushmix", touched
    ref_key = f"{key}-{kind}"
    check(form, ref_key, lo, wlo, P, aGrid, m0, m, K, it, pi_of=())


def test_zz_report_ratios():
    """Prints the largest ratio of each residual to its bound per form (the figures of the module
    docstring); holds each below 1, which the cases above already assert one by one."""
    for form, (a, b) in sorted(RATIOS.items()):
        print(f"\n{form}: sum|T m - m| / bound {a:.3f}, max|T m - m| / bound {b:.3f}", end="")
        assert a <= 1.0 and b <= 1.0
