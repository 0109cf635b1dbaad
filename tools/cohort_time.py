#!/usr/bin/env python3
"""Timing of the cohort sweep (csrc/cohort.hip) at the Table II size: 24 calibrations, S = 7,
n_a = 10 000, T = 300.

  python tools/cohort_time.py [--n-a N --T T --reps R --out FILE]
      for the steady lottery (n_lot = 1) and a path's lotteries (n_lot = T), G = 5 and G = 10:
      ms of one aiy_cohort_forward (no prices: K, occ and inc) against G separate
      aiy_transition_forward calls (no prices: K) on the same lotteries and the same cohorts, in
      the same process, alternating, HIP events around the calls, medians of R >= 10 repetitions
      after a warm run of each.  The separate sweeps take [T][...] lotteries only, so on the steady
      lottery they read T copies of it.  The time condition of §4s: cohort median <= separate
      median + (max - min of the separate repetitions).  Bytes the sweep must move per point and
      period: 12 + 16 G (index, weight, G masses read and written) against 28 G; over the time.
      Also the mobility tables of calibration B (LaborAR 0.6, LaborSD 0.2, CRRA 3) at this grid.
The path is priced at K* with the default TFP shock (not an equilibrium path: the timing does
not depend on it).  One JSON document, written to --out (default profiles/cohort_time.json)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-a", type=int, default=10000)
    ap.add_argument("--T", type=int, default=300)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cohort_time.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from aiyagari_hark_amd import _lib, build
    from aiyagari_hark_amd import mobility as M
    from aiyagari_hark_amd.stationary import table2_calibrations
    from aiyagari_hark_amd.transition import (TransitionBuffers, path_prices, steady_state, transition_backward,
                                              transition_forward)
    if not torch.cuda.is_available():
        raise SystemExit("cohort_time.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    T, n_a = args.T, args.n_a
    cals = table2_calibrations()
    batch, r_star, K_star = steady_state(cals, n_a, device=dev)
    n_cal, S = len(cals), batch.S
    Z = 1.0 + 0.01 * 0.8 ** np.arange(T + 1)
    Z[T] = 1.0
    r, w = path_prices(np.repeat(K_star[:, None], T + 1, axis=1), Z[None, :], batch.alpha, batch.delta)
    dR, dw = torch.as_tensor(1.0 + r).to(dev), torch.as_tensor(w).to(dev)
    m_term, c_term = (t.reshape(n_cal, S, n_a + 1).contiguous() for t in batch.last_tables)
    buf = TransitionBuffers(batch, T)
    med = statistics.median

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # the mobility tables quoted in the README
    res = M.mobility(batch, horizons=(1, 5, 20))
    q = next(i for i, c in enumerate(cals) if (c.LaborAR, c.LaborSD, c.CRRA) == (0.6, 0.2, 3.0))   # calibration B
    quote = dict(calibration=q, cal=dict(LaborAR=cals[q].LaborAR, LaborSD=cals[q].LaborSD, CRRA=cals[q].CRRA),
                 r_star=float(r_star[q]), horizons=res.horizons.tolist(), shares=res.shares[q].tolist(),
                 thresholds=res.thresholds[q].tolist(), matrix=res.matrix[q].tolist(),
                 shorrocks=res.shorrocks[q].tolist(), mean_wealth_h=res.mean_wealth[q][:, [0, 1, 5, 20]].tolist())

    points = n_cal * S * n_a * T
    out = dict(shape=dict(n_cal=n_cal, S=S, n_a=n_a, T=T), reps=args.reps, source_digest=build.source_digest(),
               mobility=quote, cases=[])
    for lottery in ("steady", "path"):
        if lottery == "path":
            transition_backward(batch, dR, dw, m_term, c_term, buf, export_policy=False)
        else:   # the steady lottery in every period of the separate sweeps' [T][...] arrays
            buf.lo[:] = batch.lo[None]
            buf.wlo[:] = batch.wlo[None]
        lo_c = buf.lo if lottery == "path" else batch.lo[None]
        wlo_c = buf.wlo if lottery == "path" else batch.wlo[None]
        for G in (5, 10):
            pct = tuple(np.arange(1, G) / G)
            edges = M.wealth_classes(batch, pct)
            start = M.cohorts_by_class(batch, edges)
            cohorts = start.clone()

            def cohort_sweep():
                cohorts.copy_(start)
                return M.cohort_forward(batch, lo_c, wlo_c, cohorts, T, edges)

            def separate_sweeps():
                Ks = []
                for g in range(G):
                    buf.mass.copy_(start[g])
                    Ks.append(transition_forward(batch, buf.lo, buf.wlo, buf.mass, T, buf.work, want_c=False)[0])
                return np.stack(Ks, axis=1)

            paths = cohort_sweep()
            same = bool(np.array_equal(paths.K, separate_sweeps()))
            t_co, t_sep = [], []
            for _ in range(args.reps):
                t_co.append(timed(cohort_sweep))
                t_sep.append(timed(separate_sweeps))
            spread = max(t_sep) - min(t_sep)
            case = dict(lottery=lottery, n_lot=int(lo_c.shape[0]), G=G, cohort_ms=med(t_co), cohort_all_ms=t_co,
                        separate_ms=med(t_sep), separate_all_ms=t_sep, separate_spread_ms=spread,
                        ratio=med(t_co) / med(t_sep), not_slower=bool(med(t_co) <= med(t_sep) + spread),
                        K_same_bits=same, cohort_bytes=(12 + 16 * G) * points, separate_bytes=28 * G * points,
                        cohort_GBps=(12 + 16 * G) * points / (med(t_co) * 1e-3) / 1e9,
                        separate_GBps=28 * G * points / (med(t_sep) * 1e-3) / 1e9)
            out["cases"].append(case)
            print(json.dumps({k: case[k] for k in ("lottery", "G", "cohort_ms", "separate_ms", "separate_spread_ms",
                                                   "ratio", "not_slower", "K_same_bits", "cohort_GBps",
                                                   "separate_GBps")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(quote, indent=1))


if __name__ == "__main__":
    main()
