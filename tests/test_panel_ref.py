"""CPU tests of tests/panel_ref.py: the scalar period against the oracle's vectorised period and
against the committed panel fixture, the vectorised forms against the scalar one, and the
condition that the table family and the query set reach every path of the bracket index."""
import collections
import functools
import os

import numpy as np

from oracle import hark_ks as H
from tests import panel_ref as PR

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def same(x, y):
    return np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(x[~np.isnan(x)], y[~np.isnan(y)])


def test_scalar_period_equals_oracle_on_fixture_tables():
    fx = np.load(os.path.join(GOLD, "egm_cfg1.npz"))
    rng = np.random.default_rng(1)
    N = 3000
    a = np.exp(rng.uniform(np.log(1e-3), np.log(300.0), N))
    lab, emp, u = rng.integers(0, 7, N), rng.integers(0, 2, N), rng.random(N)
    for Mrkv, Mnow in ((0, float(fx["MSS"])), (1, 0.9 * float(fx["Mgrid"][0])), (0, 1.2 * float(fx["Mgrid"][-1]))):
        args = (a, lab, emp, u, 1.031, 1.17, Mnow, Mrkv, fx["LSStates"], fx["cdf"], fx["m"], fx["c"], fx["Mgrid"])
        got, want = PR.period(*args), H.sim_one_period(*args)
        assert np.array_equal(got[1], want[1])
        for g, w in zip((got[0], got[2], got[3]), (want[0], want[2], want[3])):
            assert not np.isnan(w).any() and np.array_equal(g, w)


def test_scalar_period_equals_oracle_on_family():
    fam, Mnow, (a0, lab0, u, tgt) = PR.lookup_case(32, 14, 3, 7, 1)
    rng = np.random.default_rng(2)
    a0 = np.concatenate([a0, PR.queries_below()])
    lab0 = np.concatenate([lab0, rng.integers(0, 7, 7)])
    u = np.concatenate([u, rng.random(7)])
    emp = rng.integers(0, 2, a0.size)
    for R, W in ((1.0, 0.0), (1.03, 1.2)):
        args = (a0, lab0, emp, u, R, W, Mnow, 1, fam.lvl, fam.cdf, fam.m, fam.c, fam.Mgrid)
        got, want = PR.period(*args), PR.period_fast(*args)
        assert np.array_equal(got[1], want[1])
        assert 0 < np.isnan(want[0]).sum() < 10
        for g, w in zip((got[0], got[2], got[3]), (want[0], want[2], want[3])):
            assert same(g, w)
    assert np.array_equal(got[1][:tgt.size], tgt)


def test_one_row_forms_agree():
    fam, Mnow, (a0, lab0, u, tgt) = PR.lookup_case(33, 6, 1, 7, 0)
    rng = np.random.default_rng(3)
    a0 = np.concatenate([a0, PR.queries_below()])
    lab0 = np.concatenate([lab0, rng.integers(0, 7, 7)])
    u = np.concatenate([u, rng.random(7)])
    emp = rng.integers(0, 2, a0.size)
    for R, W in ((1.0, 0.0), (1.03, 1.2)):
        args = (a0, lab0, emp, u, R, W, Mnow, 0, fam.lvl, fam.cdf, fam.m, fam.c, fam.Mgrid)
        got, want = PR.period(*args), PR.period_fast(*args)
        assert np.array_equal(got[1], want[1])
        assert np.isnan(want[0]).sum() == (want[2] < PR.FIRST).sum() >= 3   # 6 at W = 0; W l lifts the employed
        for g, w in zip((got[0], got[2], got[3]), (want[0], want[2], want[3])):
            assert same(g, w)
    # at R = 1, W = 0 the agent sits on the query: m == a0 bit for bit
    args = (a0, lab0, emp, u, 1.0, 0.0, Mnow, 0, fam.lvl, fam.cdf, fam.m, fam.c, fam.Mgrid)
    assert same(PR.period(*args)[2], a0)


def test_first_period_of_panel_fixture():
    """hist_A[0] of the committed 350-agent history; the sum's order differs: 350 x 2^-53."""
    fx = np.load(os.path.join(GOLD, "egm_cfg1.npz"))
    pf = np.load(os.path.join(GOLD, "panel_cfg1.npz"))
    N = 350
    u = np.random.RandomState(int(pf["u_seed"])).random_sample((int(pf["T"]), N))[0]
    a1, lab1, _, _ = PR.period(np.full(N, float(fx["KSS"])), pf["lab0"], np.ones(N, dtype=np.int64), u,
                               float(fx["RSS"]), float(fx["WSS"]), float(fx["MSS"]), 0, fx["LSStates"], fx["cdf"],
                               fx["m"], fx["c"], fx["Mgrid"])
    assert np.array_equal(lab1, H.draw_labor(pf["lab0"], u, fx["cdf"]))
    got, want = PR.mean_fsum(a1), float(pf["hist_A"][0])
    assert abs(got - want) <= 350 * 2.0 ** -53 * abs(want), (got, want)


def test_prices_long_double_close_to_oracle():
    e = dict(ProdB=0.99, ProdG=1.01, UrateB=0.07, UrateG=0.04, LbrInd=1.0, CapShare=0.36, DeprFac=0.08)
    for Mrkv in (0, 1):
        want = H.calc_R_and_W(np.array([4.7, 5.1]), np.ones(2), Mrkv, e)
        got = PR.prices_ld(4.9, Mrkv)
        for g, w in zip(got, (want[0], want[3], want[4])):
            assert abs(float(g) - w) <= 8 * 2.0 ** -53 * abs(w)


@functools.lru_cache(maxsize=None)
def coverage():
    """Agents per (instantiation, class) over the lookup-path and the index-width cases."""
    hits = {False: collections.Counter(), True: collections.Counter()}
    for n_a, octaves, n_M in PR.LOOKUP:
        for n_lab in (2, 7):
            for Mrkv in (0, 1):
                fam, Mnow, (a0, _, _, tgt) = PR.lookup_case(n_a, octaves, n_M, n_lab, Mrkv)
                hits[n_M > 1].update(PR.classes_of(fam, Mnow, Mrkv, a0, tgt))
    for n_a, n_M in PR.WIDTHS:
        fam, Mnow, Mrkv, (a0, _, _, tgt) = PR.width_case(n_a, n_M)
        hits[n_M > 1].update(PR.classes_of(fam, Mnow, Mrkv, a0, tgt))
    return hits


def test_every_index_path_is_reached():
    hits = coverage()
    print({k: dict(v) for k, v in hits.items()})
    total = hits[False] + hits[True]
    for cls in PR.CLASSES:
        assert total[cls] >= 8, (cls, total[cls])
    assert set(total) <= set(PR.CLASSES)
    for blend in (False, True):
        assert hits[blend]["cnt4_6"] >= 8 and hits[blend]["cnt7"] >= 8, blend
        assert sum(hits[blend][c] for c in ("cnt1_tie", "cnt2_tie", "cnt3_tie")) >= 8, blend


def test_classifier_on_a_hand_made_list():
    """n_a = 16: 16 buckets per octave of width 2^48 ulp, base at z[2] = 1.0."""
    z = np.array([1e-7, 1e-7, 1.0, 1.0 + 2.0 ** -30, 1.07, 1.08, 1.09, 1.26, 1.27, 1.28, 1.29, 1.32, 1.33, 1.34,
                  1.35, 2.0] + [2.0 + 0.01 * k for k in range(1, 17)])
    q = [0.5, 1.0, 1.03, 1.0 + 2.0 ** -29, 1.0625, 1.1, 1.2, 1.27, 1.3, 2.05, 3.0, 5000.0, 1.08]
    want = ["below", "cnt2_tie", "cnt2_fields", "cnt2_tie", "cnt3_fields", "cnt3_fields", "cnt0", "cnt4_6", "cnt4_6",
            "cnt7", "above_last", "beyond_span", "cnt3_tie"]
    assert PR.classify(z, 16, q) == want
