"""Reference of ONE period of the agent panel, the synthetic policy family the panel tests run
it on, and a classifier of the path a query takes through the merged-table bracket index.

The period (csrc/panel.hip, panel_block.hip, panel_resident.hip; per agent: csrc/panel_common.h
tab_policy_t) restated as plain scalar float64 Python, agent by agent, `bisect` for every search,
in the reference's operation order:

    l' = searchsorted(cdf[l], u, 'right')                      get_shocks
    m  = R a + W (lvl[l'] emp)                                 get_states
    c  = (1 - aM) f_{j-1}(m) + aM f_j(m), s = 4 l' + 2 Mrkv + emp,
         f = HARK LinearInterp: i = max(bisect_left(x[:-1], m), 1),
         alpha = (m - x[i-1]) / (x[i] - x[i-1]), y = (1 - alpha) y[i-1] + alpha y[i], NaN below x[0];
         j = clip(searchsorted(Mgrid, Mnow), 1, n_M - 1); n_M == 1: c = f_0(m), one row
    a' = m - c                                                 get_poststates

No index, no merged list, no records: nothing of the device's lookup is restated here.  The
vectorised forms (`period_fast`) are for the multi-million-agent cases; tests/test_panel_ref.py
holds them to the scalar form bit for bit.
"""
import math
from bisect import bisect_left, bisect_right

import numpy as np

from oracle import hark_ks as H

NAN = float("nan")
MARKET = dict(CapShare=0.36, DeprFac=0.08, prod=(0.99, 1.01), agg_L=(0.93, 0.96))


# --------------------------------------------------------------------------------------
# The period
# --------------------------------------------------------------------------------------
def lerp_row(x, y, q):
    """HARK LinearInterp of one row (Python lists) at the scalar q."""
    i = max(bisect_left(x, q, 0, len(x) - 1), 1)
    alpha = (q - x[i - 1]) / (x[i] - x[i - 1])
    v = (1.0 - alpha) * y[i - 1] + alpha * y[i]
    return NAN if q < x[0] else v


def m_bracket(Mgrid, Mnow):
    """(j, aM) of LinearInterpOnInterp1D; (0, 0.0) for one row."""
    n_M = len(Mgrid)
    if n_M == 1:
        return 0, 0.0
    j = min(max(bisect_left(list(Mgrid), Mnow), 1), n_M - 1)
    return j, (Mnow - Mgrid[j - 1]) / (Mgrid[j] - Mgrid[j - 1])


def period(a, lab, emp, u, R, W, Mnow, Mrkv, lvl, cdf, m_tab, c_tab, Mgrid):
    """One period, scalar.  Returns (a', l', m, c) as arrays."""
    R, W, Mnow = float(R), float(W), float(Mnow)
    Mg = [float(v) for v in Mgrid]
    n_M = len(Mg)
    j, aM = m_bracket(Mg, Mnow)
    rows = {}
    cdf_l = [r.tolist() for r in np.asarray(cdf)]
    lv = np.asarray(lvl, dtype=np.float64).tolist()
    N = len(a)
    a_out, l_out, m_out, c_out = np.empty(N), np.empty(N, dtype=np.int64), np.empty(N), np.empty(N)
    al, ll, el, ul = np.asarray(a, dtype=np.float64).tolist(), np.asarray(lab).tolist(), np.asarray(emp).tolist(), \
        np.asarray(u, dtype=np.float64).tolist()
    for i in range(N):
        ln = bisect_right(cdf_l[ll[i]], ul[i])
        e = int(el[i])
        m = R * al[i] + W * (lv[ln] * float(e))
        s = 4 * ln + 2 * int(Mrkv) + e
        if s not in rows:
            ks = (0,) if n_M == 1 else (j - 1, j)
            rows[s] = [(m_tab[s, k].tolist(), c_tab[s, k].tolist()) for k in ks]
        r = rows[s]
        if n_M == 1:
            c = lerp_row(r[0][0], r[0][1], m)
        else:
            c = (1 - aM) * lerp_row(r[0][0], r[0][1], m) + aM * lerp_row(r[1][0], r[1][1], m)
        a_out[i], l_out[i], m_out[i], c_out[i] = m - c, ln, m, c
    return a_out, l_out, m_out, c_out


def period_one_row(a, lab, emp, u, R, W, Mrkv, lvl, cdf, m_tab, c_tab):
    """Vectorised twin of `period` for n_M == 1 (oracle.hark_ks.eval_policy_2d divides 0 by 0
    there)."""
    a, u = np.asarray(a, dtype=np.float64), np.asarray(u, dtype=np.float64)
    lab, emp = np.asarray(lab), np.asarray(emp)
    ln = np.empty(a.size, dtype=np.int64)
    for l in range(cdf.shape[0]):
        sel = lab == l
        ln[sel] = np.searchsorted(cdf[l], u[sel], side="right")
    m = R * a + W * np.multiply(np.asarray(lvl)[ln], emp.astype(np.float64))
    c = np.zeros(a.size)
    state = 4 * ln + 2 * int(Mrkv) + emp.astype(np.int64)
    with np.errstate(all="ignore"):
        for s in np.unique(state):
            sel = state == s
            x, y, q = m_tab[s, 0], c_tab[s, 0], m[sel]
            i = np.maximum(np.searchsorted(x[:-1], q), 1)
            alpha = (q - x[i - 1]) / (x[i] - x[i - 1])
            v = (1.0 - alpha) * y[i - 1] + alpha * y[i]
            v[q < x[0]] = np.nan
            c[sel] = v
    return m - c, ln, m, c


def period_fast(a, lab, emp, u, R, W, Mnow, Mrkv, lvl, cdf, m_tab, c_tab, Mgrid):
    """Vectorised period for large N: the oracle's sim_one_period, or the one-row twin."""
    if len(Mgrid) == 1:
        return period_one_row(a, lab, emp, u, R, W, Mrkv, lvl, cdf, m_tab, c_tab)
    return H.sim_one_period(np.asarray(a, dtype=np.float64), np.asarray(lab), np.asarray(emp),
                            np.asarray(u, dtype=np.float64), R, W, Mnow, Mrkv, np.asarray(lvl), cdf, m_tab, c_tab,
                            np.asarray(Mgrid))


def mean_fsum(a):
    """np.mean(aNow) with an exactly rounded sum (NaN if any asset is NaN)."""
    a = np.asarray(a)
    if np.isnan(a).any():
        return NAN
    return math.fsum(a.tolist()) / a.size


def sum_bound(a):
    """Largest distance of a float64 mean of `a`, summed in any order, from the exact mean:
    each of the N - 1 additions rounds a partial sum no larger than sum |a|."""
    a = np.asarray(a)
    return (a.size - 1) * 2.0 ** -53 * math.fsum(np.abs(a).tolist()) / a.size


def prices_ld(K, Mrkv, market=MARKET):
    """calc_R_and_W (oracle.hark_ks.calc_R_and_W, AS:1839-1894) in np.longdouble at aggregate
    capital K: (Mnow, Rnow, Wnow)."""
    L = np.longdouble
    K, al, depr = L(K), L(market["CapShare"]), L(market["DeprFac"])
    Prod, AggL = L(market["prod"][1 if Mrkv else 0]), L(market["agg_L"][1 if Mrkv else 0])
    KtoL = K / AggL
    Rnow = L(1.0) + Prod * (al * KtoL ** (al - L(1.0))) - depr
    Wnow = Prod * ((L(1.0) - al) * KtoL ** al)
    return Rnow * K + Wnow * AggL, Rnow, Wnow


def rel_gap_ld(got, want):
    return float(abs(np.longdouble(got) - want) / abs(want))


# --------------------------------------------------------------------------------------
# The table family
# --------------------------------------------------------------------------------------
FIRST = 1e-7
# (first node index, nodes, relative spacing): runs of a row overwritten with tight clusters
CLUSTERS = ((5, 9, 1e-6), (16, 5, 1e-5), (22, 3, 1e-4), (26, 2, 1e-4))
SHARED = (1, 3, 15, 29)      # node indices (outside the clusters) an M row shares with the row before


class Family:
    """Policies m, c [4 n_lab][n_M][n_a + 1], an M grid, a labour process and a Markov history."""

    def __init__(self, n_lab, n_M, n_a, octaves, seed=0, first=None, M_scale=1.0, hist_roll=0):
        rng = np.random.default_rng([seed, n_lab, n_M, n_a, octaves])
        S = 4 * n_lab
        self.n_lab, self.n_M, self.n_a, self.octaves = n_lab, n_M, n_a, octaves
        base = 0.05 * 2.0 ** (octaves * np.arange(n_a) / max(n_a - 1, 1))
        if n_a >= 32:
            for p, cnt, rel in CLUSTERS:
                base[p - 1:p - 1 + cnt] = base[p - 1] * (1.0 + rel * np.arange(cnt))
        m = np.empty((S, n_M, n_a + 1))
        for s in range(S):
            for k in range(n_M):
                m[s, k, 0] = FIRST if first is None else first[k]
                m[s, k, 1:] = base * (1.0 + 0.013 * k + 0.001 * s)
                if k > 0:   # a few nodes exactly equal to a node of the row before: ties inside z
                    for i in sorted({i for i in SHARED + (n_a - 2,) if 1 <= i <= n_a - 1}):
                        if n_a >= 32 and any(p <= i < p + cnt for p, cnt, _ in CLUSTERS):
                            continue
                        prev = m[s, k - 1]
                        ok = prev[(prev > m[s, k, i - 1]) & (prev < m[s, k, i + 1])]
                        if ok.size:   # (none where the row's top lies beyond the last node of the row before)
                            m[s, k, i] = ok[np.argmin(np.abs(ok - m[s, k, i]))]
        assert np.all(np.diff(m, axis=-1) > 0)
        coef = 0.5 + 0.01 * np.arange(n_M)[None, :, None] + 0.003 * np.arange(S)[:, None, None]
        self.m, self.c = m, coef * np.log1p(m)     # smooth, strictly concave, positive, 0 < c < m
        self.Mgrid = M_scale * (3.0 + 1.7 * np.arange(n_M) + 0.3 * np.arange(n_M) ** 2)
        P = rng.uniform(0.2, 1.0, (n_lab, n_lab))
        self.cdf = np.stack([H.choice_cdf(r) for r in P])
        self.lvl = (1.0 + 0.05 * seed) * (np.linspace(0.4, 1.9, n_lab) if n_lab > 1 else np.array([1.1]))
        self.mrkv_hist = np.roll(np.array([1, 0, 1, 0], dtype=np.int32), hist_roll)
        for x in (self.m, self.c, self.Mgrid, self.cdf, self.lvl, self.mrkv_hist):
            x.setflags(write=False)

    def M_inside(self, j=1):
        """An M strictly inside bracket j (rows j - 1, j); any value for one row."""
        if self.n_M == 1:
            return 5.0
        return float(0.37 * self.Mgrid[j - 1] + 0.63 * self.Mgrid[j])

    def rows(self, l, Mrkv, emp, Mnow):
        """The searched nodes x[:-1] of the two rows an agent of (l, emp) reads at (Mrkv, Mnow)."""
        s = 4 * l + 2 * Mrkv + emp
        j, _ = m_bracket(self.Mgrid.tolist(), Mnow)
        return (self.m[s, 0, :-1],) * 2 if self.n_M == 1 else (self.m[s, j - 1, :-1], self.m[s, j, :-1])


def tab_shift(n_a):
    """(shift, buckets) of the bracket index over z (panel_tab_geom, csrc/panel_common.h)."""
    lg = 4
    while lg < 13 and (1 << lg) < n_a:
        lg += 1
    return 52 - lg, 12 << lg


def ulps(x, k):
    """The doubles k ulp away from the positive doubles x."""
    return (np.asarray(x, dtype=np.float64).view(np.int64) + k).view(np.float64)


def queries(x0, x1, rng, steps=(1, 3, 100, 5000), n_rand=400, extra=40):
    """The query set of one cell (rows' searched nodes x0, x1): every node above the first and its
    neighbours `steps` ulp away on both sides, the doubles just above the first node, log-uniform
    values, a few dozen values inside the bucket of the three-node cluster, far values.  Nothing
    at or below the first node (those are `queries_below`)."""
    nodes = np.concatenate([x0[1:], x1[1:]])
    last = max(x0[-1], x1[-1])
    out = [nodes] + [ulps(nodes, sg * k) for k in steps for sg in (1, -1)]
    out.append(ulps(np.array([max(x0[0], x1[0])]), np.array(steps)))
    out.append(np.exp(rng.uniform(np.log(0.03), np.log(3.0 * last), n_rand)))
    if x0.size >= 32 and extra:
        shift, _ = tab_shift(x0.size)
        key = int(np.float64(x0[CLUSTERS[2][0]]).view(np.int64)) >> shift
        out.append(rng.integers(key << shift, (key + 1) << shift, extra).view(np.float64))
    out.append(np.array([2e-7, 1e-3, 4.0 * last, 1e6, 1e12]))
    q = np.concatenate(out)
    return q[q > max(x0[0], x1[0])]


def queries_below(first=FIRST):
    """At and below the grid: NaN in the reference, except the first node itself."""
    return np.array([-1.0, -0.0, 0.0, 1e-9, 5e-8, float(ulps(first, -1)), first])


CLASSES = ("below", "cnt0", "cnt1_fields", "cnt1_tie", "cnt2_fields", "cnt2_tie", "cnt3_fields", "cnt3_tie",
           "cnt4_6", "cnt7", "capped", "above_last", "beyond_span", "cnt1_exact")


def classify(z, n_a, q):
    """The path each query q takes through the bracket index of the merged node list z (sorted,
    2 n_a nodes), from z alone: per bucket the key (bits >> shift) - key(z[2]), the nodes in it
    and the field width min(40 // cnt, shift)."""
    shift, buckets = tab_shift(n_a)
    z = np.asarray(z, dtype=np.float64)
    base = int(z[2].view(np.int64)) >> shift
    zk = np.clip((z.view(np.int64) >> shift) - base, -1, buckets - 1)
    zk[~(z > 0)] = -1
    last = int(zk[-1])
    out = []
    for v in np.asarray(q, dtype=np.float64):
        raw = (int(v.view(np.int64)) >> shift) - base if v > 0 else -1
        if raw < 0:
            out.append("below")
        elif raw >= buckets - 1:
            out.append("capped" if last == buckets - 1 else "beyond_span")
        elif raw > last:
            out.append("above_last")
        else:
            inb = z[zk == raw]
            cnt = inb.size
            if cnt == 0:
                out.append("cnt0")
            elif cnt <= 3:
                w = min(40 // cnt, shift)
                if w == shift:
                    out.append(f"cnt{cnt}_exact")
                    continue
                mask = (1 << w) - 1
                qf = (int(v.view(np.int64)) >> (shift - w)) & mask
                tie = any(((int(x.view(np.int64)) >> (shift - w)) & mask) == qf for x in inb)
                out.append(f"cnt{cnt}_{'tie' if tie else 'fields'}")
            else:
                out.append("cnt4_6" if cnt < 7 else "cnt7")
    return out


# --------------------------------------------------------------------------------------
# Agents
# --------------------------------------------------------------------------------------
def place(fam, per_state, rng, emp=None):
    """Agents that land on chosen labour states: per_state[l] = the assets (= m at R = 1, W = 0)
    wanted in state l.  The previous state is random and the uniform lies inside the CDF interval
    of the target, so the draw is generic.  Returns (a0, lab0, u, target l')."""
    tgt = np.concatenate([np.full(len(q), l) for l, q in enumerate(per_state)])
    a0 = np.concatenate([np.asarray(q, dtype=np.float64) for q in per_state])
    perm = rng.permutation(tgt.size)
    tgt, a0 = tgt[perm], a0[perm]
    lab0 = rng.integers(0, fam.n_lab, tgt.size)
    hi = fam.cdf[lab0, tgt]
    lo = np.where(tgt > 0, fam.cdf[lab0, np.maximum(tgt - 1, 0)], 0.0)
    u = lo + (hi - lo) * rng.uniform(0.1, 0.9, tgt.size)
    return a0, lab0, u, tgt


def fill(fam, N, per_state, rng):
    """N agents with random labour draws; the agents landing in state l tile per_state[l]."""
    lab0 = rng.integers(0, fam.n_lab, N)
    u = rng.random(N)
    tgt = H.draw_labor(lab0, u, fam.cdf)
    a0 = np.empty(N)
    for l in range(fam.n_lab):
        sel = np.flatnonzero(tgt == l)
        a0[sel] = np.resize(rng.permutation(np.asarray(per_state[l], dtype=np.float64)), sel.size)
    return a0, lab0, u, tgt


# (n_a, octaves, n_M): the lookup-path cases; every one runs at both Mrkv and n_lab in {2, 7}
LOOKUP = ((32, 14, 1), (32, 14, 3), (33, 6, 1), (33, 6, 2))
WIDTHS = tuple((n_a, n_M) for n_a in (2, 3, 16, 17, 257, 4097) for n_M in (1, 2))


def lookup_case(n_a, octaves, n_M, n_lab, Mrkv):
    """One lookup-path case: the family member, the market state and one agent per query."""
    fam = Family(n_lab, n_M, n_a, octaves)
    rng = np.random.default_rng([11, n_a, octaves, n_M, n_lab, Mrkv])
    Mnow = fam.M_inside(min(1 + Mrkv, max(n_M - 1, 1)))
    # (380 random values per cell: two cells stay within the 2048 agents of the block engine's <2>)
    per = [queries(*fam.rows(l, Mrkv, 1, Mnow), rng, n_rand=380) for l in range(n_lab)]
    return fam, Mnow, place(fam, per, rng)


def width_case(n_a, n_M):
    """One index-width case: nodes, their +-1 ulp neighbours and randoms; 6 octaves, n_lab = 2
    from n_a = 257 on (small tables), 7 below."""
    n_lab = 2 if n_a >= 257 else 7
    fam = Family(n_lab, n_M, n_a, 6)
    rng = np.random.default_rng([13, n_a, n_M])
    Mnow, Mrkv = fam.M_inside(1), n_a % 2
    per = [queries(*fam.rows(l, Mrkv, 1, Mnow), rng, steps=(1,), n_rand=200, extra=0) for l in range(n_lab)]
    return fam, Mnow, Mrkv, place(fam, per, rng)


def classes_of(fam, Mnow, Mrkv, a0, tgt, emp=1):
    """Class of every agent sitting at m = a0 in labour state tgt."""
    out = np.empty(a0.size, dtype=object)
    for l in range(fam.n_lab):
        x0, x1 = fam.rows(l, Mrkv, emp, Mnow)
        z = np.sort(np.concatenate([x0, x1]), kind="stable")
        sel = tgt == l
        out[sel] = classify(z, fam.n_a, a0[sel])
    return out
