"""The two references of tests/egm_ref.py agree with each other (CPU): the float64 oracle step
against its long-double restatement at every state count and CRRA kind the GPU tests use, on
policy tables and on the synthetic dense tables; the span helper on both; and the reduction
order np.sum uses over the next states, which the kernels' pairwise sums restate."""
import numpy as np
import pytest

from oracle import stationary as ST
from tests import egm_ref as ER

S_LIST = (1, 2, 3, 4, 7, 9, 17, 33, 64)
CRRAS = (1.0, 3.0, 5.0, 2.5)
BETA, RATE, ALPHA, DELTA = 0.96, 0.03, 0.36, 0.08
# measured: at most 6.6e-16 on every case (the float64 step's own roundings)
REF_RTOL = 1e-14


def problem(S, n_a):
    """Rouwenhorst(0.9, 0.4) income with S states (S = 1: lab = [1], P = [[1]]), the stationary
    asset grid, prices at r = 3 %."""
    lab, P = ST.income_process(S, 0.9, 0.4, "rouwenhorst")
    w, _ = ST.prices(RATE, ALPHA, DELTA)
    return dict(aGrid=ST.make_stationary_grid(0.001, 50.0, n_a, 2), R=1.0 + RATE, w=w, lab=lab, P=P)


def both(m, c, rho, p):
    args = (BETA, rho, p["aGrid"], p["R"], p["w"], p["lab"], p["P"])
    return ER.step64(m, c, *args), ER.step_ld(m, c, *args)


def check(got, want, what):
    for g, x, name in zip(got, want, "mc"):
        assert np.array_equal(np.isnan(g), np.isnan(x)) and not np.isnan(x).any(), (what, name)
        gap = ER.rel_gap(g, x)
        assert gap <= REF_RTOL, (what, name, gap)


@pytest.mark.parametrize("S", S_LIST)
def test_step64_matches_long_double(S):
    """Four steps from the terminal guess, both references fed the float64 tables."""
    p = problem(S, 200)
    assert p["lab"].shape == (S,) and p["P"].shape == (S, S)
    for rho in CRRAS:
        m = c = None
        for k in range(4):
            (m, c), ld = both(m, c, rho, p)
            check((m, c), ld, (S, rho, k))


@pytest.mark.parametrize("S", (1, 7, 9))
def test_references_agree_on_dense_tables(S):
    p = problem(S, 700)
    m, c = ER.dense_tables(S, 700, p["aGrid"], p["R"], p["w"], p["lab"])
    assert m.shape == (S, 701) and np.all(np.diff(m, axis=1) > 0.0)
    for rho in CRRAS:
        f64, ld = both(m, c, rho, p)
        check(f64, ld, (S, rho))


@pytest.mark.parametrize("S", (7, 9))
def test_spans_tell_dense_tables_from_policies(S):
    """Tile 3 of the dense tables spans more nodes than a window holds, every other tile and
    every tile of a policy table fewer."""
    p = problem(S, 700)
    geo = (p["aGrid"], p["R"], p["w"], p["lab"])
    sp = ER.tile_spans(ER.dense_tables(S, 700, *geo)[0], *geo)
    assert sp.shape == (S, 11)
    assert np.all(sp[:, 3] > ER.WINDOW) and np.all(np.delete(sp, 3, axis=1) < ER.WINDOW)
    m = c = None
    for _ in range(3):
        m, c = ER.step64(m, c, BETA, 3.0, *geo, p["P"])
        assert np.all(ER.tile_spans(m, *geo) < ER.WINDOW)


def kernel_order_sum(v):
    """np_pairwise_sum of csrc/common.h: below 8 terms in order from 0.0; else 8 running
    partials over the first n - n % 8 terms, combined pairwise, then the tail in order."""
    n = v.size
    if n < 8:
        res = 0.0
        for t in range(n):
            res += v[t]
        return res
    nfull = n - n % 8
    r = [v[t] for t in range(8)]
    for t in range(8, nfull):
        r[t % 8] += v[t]
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for t in range(nfull, n):
        res += v[t]
    return res


@pytest.mark.parametrize("S", (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 20, 25, 28, 32, 33, 64))
def test_numpy_sums_next_states_in_the_kernels_order(S):
    """The bit-for-bit contract at CRRA = 1 rests on np.sum over the last axis adding the S
    terms in the order the kernels restate."""
    rng = np.random.default_rng(S)
    V = rng.uniform(0.1, 50.0, (37, S))
    P = rng.dirichlet(np.ones(S), S)
    want = np.sum(V[:, None, :] * P[None, :, :], axis=2)
    for i in range(V.shape[0]):
        for s in range(S):
            assert kernel_order_sum(V[i] * P[s]) == want[i, s], (S, i, s)
