"""CPU tests of the NumPy model of the windowed forward step (tests/forward_any_ref.py): it is
np.add.at bit for bit on disordered rows, it is the monotone pull on sorted rows, and its cost
is what DESIGN.md §4r says."""
import numpy as np
import pytest

from oracle import stationary as ST
from tests import forward_any_ref as FR


def sorted_row(rng, n):
    return np.sort(rng.integers(0, n - 1, size=n))


def reversed_row(n):
    return np.minimum(np.arange(n - 1, -1, -1), n - 2)


def moved(rng, n):
    return FR.disorder(rng, sorted_row(rng, n))


def cases(rng):
    out = {"two": np.array([0, 0]), "three-turned": np.array([1, 0, 1]), "reversed-130": reversed_row(130)}
    for n in (3, 64, 65, 70, 130):
        out[f"moved-{n}"] = moved(rng, n)
    wild = sorted_row(rng, 130)
    idx = rng.choice(130, size=40, replace=False)
    wild[idx] = np.clip(wild[idx] + rng.integers(-19, 20, size=40), 0, 128)
    out["wild-130"] = wild
    first = sorted_row(rng, 70) + 0
    first[0], first[1] = max(first[0], first[1], 1), 0
    out["first-pair"] = first
    last = sorted_row(rng, 70)
    last[-2], last[-1] = 68, 60
    out["last-pair"] = last
    return out


def test_windows_hold_every_source_and_are_tight_at_both_ends():
    rng = np.random.default_rng(0)
    for name, L in cases(rng).items():
        n = len(L)
        jlo, jhi = FR.windows(L)
        assert jlo.shape == jhi.shape == (n + 1,)
        assert np.all(np.diff(jlo) >= 0) and np.all(np.diff(jhi) >= 0), name
        assert jlo[n] == n and jhi[n - 1] == n and jhi[n] == n, name
        for d in range(n):
            src = np.flatnonzero(L == d)
            if len(src):
                assert jlo[d] <= src[0] and src[-1] < jhi[d], name
        # the definition, by brute force
        M = np.maximum.accumulate(L)
        m = np.minimum.accumulate(L[::-1])[::-1]
        for d in range(n + 1):
            a = np.flatnonzero(M >= d)
            b = np.flatnonzero(m > d)
            assert jlo[d] == (a[0] if len(a) else n) and jhi[d] == (b[0] if len(b) else n), name


def test_windowed_pull_is_add_at_bit_for_bit():
    rng = np.random.default_rng(1)
    for name, L in cases(rng).items():
        n = len(L)
        wl, q = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
        assert np.array_equal(FR.pull_row(L, wl, q), FR.push_row(L, wl, q)), name


def test_sorted_rows_give_the_inverse_index():
    rng = np.random.default_rng(2)
    for n in (2, 3, 64, 65, 130, 1000):
        L = sorted_row(rng, n)
        jb = FR.inverse_index(L)
        jlo, jhi = FR.windows(L)
        assert np.array_equal(jlo, jb) and np.array_equal(jhi[:n], jb[1:]) and jhi[n] == n
        assert FR.window_sum(L) == n and not FR.is_turned(L) and FR.within_cap(L)
    head = sorted_row(rng, 1000)
    head[:500] = 0
    assert np.array_equal(FR.windows(head)[0], FR.inverse_index(head))


def test_window_cost_and_the_cap():
    rng = np.random.default_rng(3)
    ratios = [FR.window_ratio(moved(rng, 70)) for _ in range(50)]
    assert 1.0 < min(ratios) and max(ratios) <= 3.0          # the disorder of the GPU tests stays inside the cap
    assert all(FR.within_cap(moved(rng, n)) for n in (3, 64, 65, 1000))
    rev = reversed_row(130)
    assert FR.window_ratio(rev) > 100.0 and not FR.within_cap(rev) and FR.is_turned(rev)
    one = sorted_row(rng, 130)
    j = int(np.flatnonzero(one >= 1)[0]) + 1
    one[j] = one[j - 1] - 1
    assert FR.is_turned(one) and FR.window_ratio(one) < 1.1


def test_rows_turned_counts_rows_not_pairs():
    rng = np.random.default_rng(4)
    lo = np.sort(rng.integers(0, 69, size=(3, 2, 5, 70)), axis=-1)
    assert FR.rows_turned(lo) == 0
    lo[1, 0, 2, 10], lo[1, 0, 2, 11] = 40, 3
    lo[1, 0, 2, 30], lo[1, 0, 2, 31] = 60, 5
    lo[2, 1, 4, 68], lo[2, 1, 4, 69] = 68, 0
    assert FR.rows_turned(lo) == 2


def test_chained_step_equals_hist_step_on_disordered_lotteries():
    """One whole step (every state, mixed by P) of the model against oracle.stationary.hist_step."""
    rng = np.random.default_rng(5)
    S, n = 3, 65
    lo = FR.disorder(rng, np.sort(rng.integers(0, n - 1, size=(S, n)), axis=-1))
    wl = rng.uniform(0, 1, (S, n))
    mass = rng.uniform(0, 1, (S, n))
    P = rng.dirichlet(np.ones(S), size=S)
    T = np.stack([FR.pull_row(lo[s], wl[s], mass[s]) for s in range(S)])
    assert np.array_equal(P.T @ T, ST.hist_step(mass, lo, wl, P))


def test_out_of_range_rows_are_refused():
    with pytest.raises(ValueError):
        FR.windows(np.array([0, 1, 2, 3]))
    with pytest.raises(ValueError):
        FR.windows(np.array([0, -1, 2, 2]))
