#!/usr/bin/env python3
"""Timing of the statistics of household variables (csrc/var_stats.hip, the masses entry of
csrc/transition.hip) at the Table II size: 24 calibrations, n_a = 10 000, S = 7.

  python tools/var_stats_time.py [--n-a N --T T --reps R --out FILE]
      (a) the steady state: 24 distributions x 4 variables (wealth, consumption, income, earnings);
      (b) the consumption of a path with T = 300: (T + 1) x 24 distributions;
      each by aiy_var_merge, aiy_dist_stats and aiy_var_moments, one call each on the whole stack,
      timed separately (HIP events, medians of R after a warm run) with the GB/s of the bytes each
      must move, and by the Python layer (stats.variable_stats, the 256 MB slab loop), against the
      only route there was: a loop of stats.get_lorenz_shares (aiy_wealth_stats, a radix sort per
      distribution) over the same distributions in the same process, alternating with the new
      path.  In (b) the loop runs on every --stride-th period when the full loop would exceed a
      minute, and is scaled to the T + 1 periods;
      (c) the forward sweep by aiy_transition_forward and by aiy_transition_forward_masses on the
      same lotteries, alternating (and a check that Ks, C and mass_T have the same bits).
One JSON document, written to --out (default profiles/var_stats_time.json)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-a", type=int, default=10000)
    ap.add_argument("--T", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stride", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "var_stats_time.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from aiyagari_hark_amd import _lib, build
    from aiyagari_hark_amd.stationary import table2_calibrations
    from aiyagari_hark_amd.stats import (SLAB_BYTES, batch_inequality, get_lorenz_shares, household_variables,
                                         variable_stats)
    from aiyagari_hark_amd.transition import (TransitionBuffers, path_prices, steady_lottery, steady_state,
                                              transition_backward, transition_forward)
    if not torch.cuda.is_available():
        raise SystemExit("var_stats_time.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    T, n_a = args.T, args.n_a
    cals = table2_calibrations()
    batch, r_star, K_star = steady_state(cals, n_a, device=dev)
    n_cal, S = len(cals), batch.S
    N = S * n_a
    med = statistics.median
    h = _lib.handle(dev.index)
    pct = np.linspace(0.01, 0.999, 15)
    dp = _lib.c_double_p

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def phases(values, mass, n_v_list):
        """Merge, aiy_dist_stats and moments of a stack [n][S][n_a], one call each on full-size
        buffers: medians and all repetitions in ms, and the bytes each must move."""
        n = values.shape[0]
        work = _lib.work_space(dev, "var", "", n_dist=n, S=S, n_a=n_a)
        ds_work = _lib.work_space(dev, "dist_stats", "", n_dist=n, n_a=N)
        ks = torch.empty((n, N), dtype=torch.float64, device=dev)
        ws = torch.empty((n, N), dtype=torch.float64, device=dev)
        lor, pcl, summ = np.empty((n, pct.size)), np.empty((n, pct.size)), np.empty((n, 4))
        ptrs = (_lib.vp * len(n_v_list))(*[_lib.ptr(v) for v in n_v_list])
        mom = np.empty((n, 1 + len(n_v_list) + len(n_v_list) ** 2))

        def merge():
            h.check(h.lib.aiy_var_merge(h.h, n, S, n_a, _lib.ptr(values), _lib.ptr(mass), _lib.ptr(work), _lib.ptr(ks),
                                        _lib.ptr(ws), None, _lib.stream_ptr()), "aiy_var_merge")

        def dist():
            h.check(h.lib.aiy_dist_stats(h.h, n, n, N, _lib.ptr(ws), _lib.ptr(ks), pct.ctypes.data_as(dp), pct.size,
                                         _lib.ptr(ds_work), lor.ctypes.data_as(dp), pcl.ctypes.data_as(dp),
                                         summ.ctypes.data_as(dp), _lib.stream_ptr()), "aiy_dist_stats")

        def moments():
            h.check(h.lib.aiy_var_moments(h.h, n, S, n_a, len(n_v_list), ptrs, _lib.ptr(mass), _lib.ptr(work),
                                          mom.ctypes.data_as(dp), _lib.stream_ptr()), "aiy_var_moments")

        out = {}
        nodes = n * N
        for name, fn, nbytes in (("merge", merge, 40 * nodes),          # key twice (check, merge), weight, both out
                                 ("dist_stats", dist, 16 * nodes),       # weight_sorted and key_sorted
                                 ("moments", moments, 16 * (1 + len(n_v_list)) * nodes)):   # two passes
            fn()
            ts = [timed(fn)[0] for _ in range(args.reps)]
            out[name] = dict(ms=med(ts), all_ms=ts, bytes=nbytes, GBps=nbytes / (med(ts) * 1e-3) / 1e9)
        out["gini"] = summ[:, 2].copy()
        return out

    def old_route(values, mass):
        """The loop of get_lorenz_shares over the distributions of [n][S][n_a] stacks."""
        for i in range(values.shape[0]):
            get_lorenz_shares(values[i].reshape(-1), weights=mass[i].reshape(-1), percentiles=pct)

    # (a) the steady state
    names = ("wealth", "consumption", "income", "earnings")
    lo_s, wlo_s, dR_s, dw_s = steady_lottery(batch)
    val = household_variables(batch, lo_s, wlo_s, dR_s, dw_s, names)
    mass = batch.mass.reshape(n_cal, S, n_a)
    stack = torch.stack([val[n] for n in names]).reshape(4 * n_cal, S, n_a).contiguous()
    mass4 = mass.repeat(4, 1, 1).contiguous()
    a_ph = phases(stack, mass4, [stack])
    a_gini = a_ph.pop("gini").reshape(4, n_cal)

    def new_a():
        return {n: variable_stats(val[n], mass, pct) for n in names}

    new_a()
    old_route(stack, mass4)
    t_new_a, t_old_a = [], []
    for _ in range(args.reps):
        t_new_a.append(timed(new_a)[0])
        t_old_a.append(timed(lambda: old_route(stack, mass4))[0])
    ineq = batch_inequality(batch, pct, names)
    t_ineq = [timed(lambda: batch_inequality(batch, pct, names))[0] for _ in range(args.reps)]
    lor_new = variable_stats(val["consumption"], mass, pct).lorenz
    lor_old = np.stack([get_lorenz_shares(val["consumption"][i].reshape(-1), weights=mass[i].reshape(-1), percentiles=pct)
                        for i in range(n_cal)])
    a_agree = float(np.max(np.abs(lor_new - lor_old)))
    iB = next(i for i, c in enumerate(cals) if (c.LaborAR, c.LaborSD, c.CRRA) == (0.6, 0.2, 3.0))
    del stack, mass4

    # the path: lotteries of a TFP shock at the steady capital, masses by the new sweep
    Z = 1.0 + 0.01 * 0.8 ** np.arange(T + 1)
    Z[T] = 1.0
    r, w = path_prices(np.repeat(K_star[:, None], T + 1, axis=1), Z[None, :], batch.alpha, batch.delta)
    dR, dw = torch.as_tensor(1.0 + r).to(dev), torch.as_tensor(w).to(dev)
    m_term, c_term = (t.reshape(n_cal, S, n_a + 1).contiguous() for t in batch.last_tables)
    buf = TransitionBuffers(batch, T)
    transition_backward(batch, dR, dw, m_term, c_term, buf, export_policy=False)
    masses = torch.empty((T + 1, n_cal, S, n_a), dtype=torch.float64, device=dev)

    def forward(mp):
        buf.mass.copy_(batch.mass)
        return transition_forward(batch, buf.lo, buf.wlo, buf.mass, T, buf.work, dR, dw, want_c=True, mass_path=mp)

    # (c) the two sweeps, alternating
    Ks0, C0 = forward(None)
    mT0 = buf.mass.clone()
    Ks1, C1 = forward(masses)
    same = bool(np.array_equal(Ks0, Ks1) and np.array_equal(C0, C1) and torch.equal(mT0, buf.mass))
    del mT0
    t_plain, t_mass = [], []
    for _ in range(args.reps):
        t_plain.append(timed(lambda: forward(None))[0])
        t_mass.append(timed(lambda: forward(masses))[0])
    points = n_cal * N * T

    # (b) the consumption of the path; period T on the lottery of T - 1
    from aiyagari_hark_amd.stats import _variables_into
    cons = torch.empty((T + 1, n_cal, S, n_a), dtype=torch.float64, device=dev)
    _variables_into(batch, buf.lo, buf.wlo, _lib.ptr(dR), _lib.ptr(dw), T + 1, T, 1, cons[:T])
    _variables_into(batch, buf.lo[T - 1], buf.wlo[T - 1], dR.data_ptr() + 8 * T, dw.data_ptr() + 8 * T, T + 1, 1, 1,
                    cons[T:])
    n_dist = (T + 1) * n_cal
    flat_c, flat_m = cons.reshape(n_dist, S, n_a), masses.reshape(n_dist, S, n_a)
    b_ph = phases(flat_c, flat_m, [flat_c])
    b_gini = b_ph.pop("gini").reshape(T + 1, n_cal)
    torch.cuda.empty_cache()

    def new_b():
        return variable_stats(cons, masses, pct)

    vs = new_b()
    t0 = time.perf_counter()
    old_route(cons[0], masses[0])          # one period: 24 calls (also the warm run)
    torch.cuda.synchronize()
    one_period_s = time.perf_counter() - t0
    stride = 1 if one_period_s * (T + 1) <= 60.0 else args.stride
    periods = list(range(0, T + 1, stride))
    sub_c = cons[periods].reshape(len(periods) * n_cal, S, n_a)
    sub_m = masses[periods].reshape(len(periods) * n_cal, S, n_a)
    scale = (T + 1) / len(periods)
    t_new_b, t_old_b = [], []
    for _ in range(args.reps):
        t_new_b.append(timed(new_b)[0])
        t_old_b.append(timed(lambda: old_route(sub_c, sub_m))[0] * scale)
    slab_same = bool(np.array_equal(vs.gini.reshape(-1), b_gini.reshape(-1)))

    def spread(ts):
        return max(ts) - min(ts)

    out = dict(
        shape=dict(n_cal=n_cal, S=S, n_a=n_a, T=T), reps=args.reps, source_digest=build.source_digest(),
        merge_form="a thread owns 16 consecutive nodes of one run: one binary search per other run at the chunk's "
                   "first key, then one pointer per run that only advances (the LDS-staged form was not built)",
        steady=dict(n_dist=4 * n_cal, variables=list(names), phases=a_ph,
                    variable_stats_ms=med(t_new_a), variable_stats_all_ms=t_new_a,
                    batch_inequality_ms=med(t_ineq), batch_inequality_all_ms=t_ineq,
                    lorenz_loop_ms=med(t_old_a), lorenz_loop_all_ms=t_old_a, lorenz_loop_spread_ms=spread(t_old_a),
                    ratio=med(t_new_a) / med(t_old_a), not_slower=bool(med(t_new_a) <= med(t_old_a) + spread(t_old_a)),
                    lorenz_max_abs_diff_consumption=a_agree),
        path=dict(n_dist=n_dist, variable="consumption", phases=b_ph, variable_stats_ms=med(t_new_b),
                  variable_stats_all_ms=t_new_b, slab_distributions=max(1, SLAB_BYTES // (32 * N)),
                  slab_equals_one_call=slab_same, lorenz_loop_stride=stride, lorenz_loop_periods=len(periods),
                  lorenz_loop_scaled=bool(stride != 1), lorenz_loop_one_period_s=one_period_s,
                  lorenz_loop_ms=med(t_old_b), lorenz_loop_all_ms=t_old_b, lorenz_loop_spread_ms=spread(t_old_b),
                  ratio=med(t_new_b) / med(t_old_b), not_slower=bool(med(t_new_b) <= med(t_old_b) + spread(t_old_b)),
                  gini_consumption_B=[float(b_gini[0, iB]), float(b_gini[:, iB].max()), float(b_gini[T, iB])]),
        sweep=dict(forward_ms=med(t_plain), forward_all_ms=t_plain, forward_masses_ms=med(t_mass),
                   forward_masses_all_ms=t_mass, masses_overhead=med(t_mass) / med(t_plain) - 1.0,
                   masses_same_bits=same, forward_algorithmic_bytes=28 * points,
                   masses_copy_bytes=16 * n_cal * N * (T + 1), masses_GB=masses.numel() * 8 / 1e9),
        calibration_B=dict(index=iB, r_star=float(r_star[iB]),
                           gini={n: float(ineq.stats[n].gini[iB]) for n in names},
                           cv={n: float(ineq.moments[n]["cv"][iB]) for n in names},
                           corr_wealth_consumption=float(ineq.corr[iB, 0, 1]),
                           corr_wealth_income=float(ineq.corr[iB, 0, 2]),
                           gini_from_phases={n: float(a_gini[u, iB]) for u, n in enumerate(names)}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
