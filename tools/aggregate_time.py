#!/usr/bin/env python3
"""Timing of the simulation with aggregate risk (csrc/aggregate.hip, aiyagari_hark_amd/aggregate.py)
at the Table II size: 24 calibrations, n_a = 10 000, T = 300, 1 000 simulated periods in
chunks of 64.

  python tools/aggregate_time.py [--n-a N --T T --periods N --chunk C --reps R --sigmas LIST --launch-only
                                  --rows {monotone,any} --out FILE]
      (a) ms of policy_jacobian (three backward sweeps, the lottery means, the differences),
          median of R builds after a warm one;
      (b) ms of one simulation by stage (synthesis launches, forward sweeps, statistics), each
          stage synchronised, and the synthesis launches' FP64 TFLOP/s
          (2 x 2(T+1) x S n_a flop per calibration and period).  The innovations have the first
          standard deviation of --sigmas at which every lottery row of every period passes the
          forward sweep's monotone check (the attempts are recorded; 0 is the steady lottery in
          every period, which costs the launches the same);
      (c) one synthesis launch by HIP events for several numbers of periods per launch, and in
          the same run aiy_jacobian_contract at the same shape (on the same operands: only the
          time matters) and its TFLOP/s, for comparison.
--rows any: the simulation of (b) moves the mass with the forward sweep that takes rows which are
not monotone, so the first sigma runs unless a row passes that sweep's work cap;
the document then also holds rows_turned and
      (d) the forward sweep of T periods of the steady lottery (monotone, so both forms run it)
          by the default form and by rows="any", alternating, HIP events, with the same bits
          checked; and each form's index pass alone (the host clock around a call whose lottery
          has one entry out of range: it builds the index, reads the flag and returns).
--launch-only: (c)'s synthesis launches alone (a library built with another period tile is
measured through AIYAGARI_LIB).  One JSON document, written to --out (default
profiles/aggregate_time.json)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write(path, out):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def synthesis_launches(args, batch, pol, timed, flop_period):
    """One aiy_aggregate_lotteries launch by HIP events for several numbers of periods."""
    import numpy as np
    import torch

    from aiyagari_hark_amd.aggregate import aggregate_lotteries
    n_cal, S, n_a, T, dev = len(batch.cals), batch.S, batch.n_a, args.T, batch.device
    med = statistics.median
    launch = {}
    for n_p in sorted({min(args.chunk, args.periods), 64, 128, 256}):
        X = torch.as_tensor(1e-3 * np.random.default_rng(n_p).standard_normal((n_cal, n_p, 2 * (T + 1)))).to(dev)
        lo = torch.empty((n_p, n_cal, S, n_a), dtype=torch.int32, device=dev)
        wlo = torch.empty((n_p, n_cal, S, n_a), dtype=torch.float64, device=dev)
        ts = [timed(lambda: aggregate_lotteries(batch, pol, X, lo, wlo)) for _ in range(args.reps + 1)][1:]
        launch[str(n_p)] = dict(ms=med(ts), all_ms=ts, TFLOPs=flop_period * n_p / (med(ts) * 1e-3) / 1e12,
                                written_GBs=12.0 * n_p * n_cal * S * n_a / (med(ts) * 1e-3) / 1e9)
        del X, lo, wlo
    return launch


def forward_forms(args, batch, pol, model, timed):
    """(d): the forward sweep over T periods of the steady lottery by both forms, and their index
    passes alone."""
    import numpy as np
    import torch

    from aiyagari_hark_amd import _lib
    from aiyagari_hark_amd._lib import AiyagariLibError
    from aiyagari_hark_amd.aggregate import aggregate_lotteries
    from aiyagari_hark_amd.transition import transition_forward
    n_cal, S, n_a, T, dev = len(batch.cals), batch.S, batch.n_a, args.T, batch.device
    med = statistics.median
    lo = torch.empty((T, n_cal, S, n_a), dtype=torch.int32, device=dev)
    wlo = torch.empty((T, n_cal, S, n_a), dtype=torch.float64, device=dev)
    for t0 in range(0, T, args.chunk):   # zero expected deviations: the steady lottery in every period
        L = min(args.chunk, T - t0)
        X = torch.zeros((n_cal, L, 2 * (pol.dA_R.shape[0])), dtype=torch.float64, device=dev)
        aggregate_lotteries(batch, pol, X, lo[t0:t0 + L], wlo[t0:t0 + L])
    R = torch.as_tensor(np.repeat((1.0 + model.r)[:, None], T + 1, axis=1)).to(dev)
    w = torch.as_tensor(np.repeat(model.w[:, None], T + 1, axis=1)).to(dev)
    works = {rows: _lib.work_space(dev, what, what, n_cal=n_cal, S=S, n_a=n_a, T=T)
             for rows, what in (("monotone", "transition"), ("any", "transition_any"))}
    mass = torch.empty_like(batch.mass)
    results = {}

    def sweep(rows):
        mass.copy_(batch.mass)
        results[rows] = transition_forward(batch, lo, wlo, mass, T, works[rows], R, w, want_c=True, rows=rows)

    ends = {}
    for rows in works:   # warm, and the bits
        sweep(rows)
        ends[rows] = mass.clone()
    same = bool(torch.equal(ends["monotone"], ends["any"]) and np.array_equal(results["monotone"][0], results["any"][0])
                and np.array_equal(results["monotone"][1], results["any"][1]))
    ms = {rows: [] for rows in works}
    for _ in range(args.reps):
        for rows in works:
            ms[rows].append(timed(lambda: sweep(rows)))
    # the index pass alone: one entry out of range, so the call stops behind its check
    keep = lo[0, 0, 0, 0].clone()
    lo[0, 0, 0, 0] = n_a - 1
    index_ms = {rows: [] for rows in works}
    for _ in range(args.reps + 1):
        for rows in works:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            try:
                sweep(rows)
                raise SystemExit("an out-of-range lottery was not refused")
            except AiyagariLibError:
                pass
            index_ms[rows].append((time.perf_counter() - t0) * 1e3)
    lo[0, 0, 0, 0] = keep
    index_ms = {rows: v[1:] for rows, v in index_ms.items()}
    m, a = med(ms["monotone"]), med(ms["any"])
    return dict(periods=T, rows_turned=results["any"][2], same_bits=same, monotone_ms=m, any_ms=a,
                monotone_all_ms=ms["monotone"], any_all_ms=ms["any"], any_over_monotone=a / m,
                monotone_ms_per_period=m / T, any_ms_per_period=a / T,
                index_monotone_ms=med(index_ms["monotone"]), index_any_ms=med(index_ms["any"]),
                index_monotone_all_ms=index_ms["monotone"], index_any_all_ms=index_ms["any"],
                index_any_over_monotone=med(index_ms["any"]) / med(index_ms["monotone"]),
                work_GB={rows: wk.numel() / 1e9 for rows, wk in works.items()},
                note="the index pass times hold the mass copy, the flag's read-back and the host's return")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-a", type=int, default=10000)
    ap.add_argument("--T", type=int, default=300)
    ap.add_argument("--periods", type=int, default=1000)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sigmas", default="0.007,0.002,0.0007,0.0002,0")
    ap.add_argument("--launch-only", action="store_true")
    ap.add_argument("--rows", choices=("monotone", "any"), default="monotone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aggregate_time.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from aiyagari_hark_amd import _lib, build
    from aiyagari_hark_amd._lib import AiyagariLibError
    from aiyagari_hark_amd.aggregate import PolicyBuffers, ar1, linear_model, policy_jacobian, saving_rule, simulate
    from aiyagari_hark_amd.stationary import table2_calibrations
    from aiyagari_hark_amd.transition import household_jacobian, jacobian_contract, steady_state
    if not torch.cuda.is_available():
        raise SystemExit("aggregate_time.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    T, n_a, n = args.T, args.n_a, args.periods
    cals = table2_calibrations()
    batch, r_star, _ = steady_state(cals, n_a, device=dev)
    n_cal, S = len(cals), batch.S
    med = statistics.median

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # the linear model first: its buffers are released before the policy derivatives are built
    jac = household_jacobian(batch, r_star, T)
    model = linear_model(batch, jac, ar1(0.8, T))
    torch.cuda.empty_cache()

    flop_period = 2.0 * 2 * (T + 1) * S * n_a * n_cal

    # (a) the policy derivatives
    buf = PolicyBuffers(batch, T)
    policy_jacobian(batch, r_star, T, buffers=buf)
    t_pol = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pol = policy_jacobian(batch, r_star, T, buffers=buf)
        torch.cuda.synchronize()
        t_pol.append((time.perf_counter() - t0) * 1e3)

    launch = synthesis_launches(args, batch, pol, timed, flop_period)
    if args.launch_only:
        out = dict(shape=dict(n_cal=n_cal, S=S, n_a=n_a, T=T), reps=args.reps, source_digest=build.source_digest(),
                   library=_lib.LIB_PATH.replace(ROOT + os.sep, ""), library_digest=build.library_digest(_lib.LIB_PATH),
                   synthesis_launch=launch)
        write(args.out, out)
        print(json.dumps(out, indent=1))
        return

    # (b) one simulation by stage, at the first sigma whose lotteries pass the row check
    draw = np.random.default_rng(0).standard_normal(n)
    attempts = []
    for sigma in (float(x) for x in args.sigmas.split(",")):
        try:
            simulate(batch, model, pol, sigma * draw, chunk=args.chunk, percentiles=[0.5, 0.9],
                     rows=args.rows)   # also the warm run
            attempts.append(dict(sigma=sigma, ok=True))
            break
        except AiyagariLibError as e:
            attempts.append(dict(sigma=sigma, ok=False, error=str(e)))
    else:
        raise SystemExit(f"no sigma of {args.sigmas} gives lottery rows that rows={args.rows!r} takes")
    eps = sigma * draw
    runs, wall = [], []
    for _ in range(args.reps):
        tm = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sim = simulate(batch, model, pol, eps, chunk=args.chunk, percentiles=[0.5, 0.9], timings=tm, rows=args.rows)
        wall.append((time.perf_counter() - t0) * 1e3)
        runs.append(tm)
    stage_ms = {k: med([q[k] for q in runs]) for k in runs[0]}
    rule = saving_rule(sim, burn=min(100, n // 4)) if sigma > 0.0 else None   # no rule to fit without shocks

    # (c) the contraction on the same arrays (the synthesis launches were timed above)
    work = _lib.work_space(dev, "jacobian", "Jacobian", n_cal=n_cal, S=S, n_a=n_a, T=T)
    F = torch.empty((n_cal, T, 2 * (T + 1)), dtype=torch.float64, device=dev)
    t_con = [timed(lambda: jacobian_contract(dev, buf.ghost[:T], pol.dA_R, pol.dA_w, work, F=F))
             for _ in range(args.reps + 1)][1:]
    con_flop = 2.0 * T * 2 * (T + 1) * S * n_a * n_cal
    con_TF = con_flop / (med(t_con) * 1e-3) / 1e12

    syn_TF = flop_period * n / (stage_ms["synthesis"] * 1e-3) / 1e12
    forward_ab = forward_forms(args, batch, pol, model, timed) if args.rows == "any" else None
    out = dict(shape=dict(n_cal=n_cal, S=S, n_a=n_a, T=T, periods=n, chunk=args.chunk), reps=args.reps,
               rows=args.rows, rows_turned=sim.rows_turned, forward_forms=forward_ab,
               sigma=sigma, sigma_attempts=attempts, source_digest=build.source_digest(), library=_lib.LIB_PATH.replace(ROOT + os.sep, ""),
               policy_jacobian_ms=med(t_pol), policy_jacobian_all_ms=t_pol,
               simulate_wall_ms=med(wall), simulate_wall_all_ms=wall, stage_ms=stage_ms, stage_all_ms=runs,
               synthesis_flop=flop_period * n, synthesis_TFLOPs=syn_TF, synthesis_share_of_simulation=stage_ms["synthesis"] / med(wall),
               synthesis_launch=launch, contraction_ms=med(t_con), contraction_all_ms=t_con, contraction_TFLOPs=con_TF,
               synthesis_over_contraction=syn_TF / con_TF,
               arrays_GB=dict(dA_per_input=pol.dA_R.numel() * 8 / 1e9,
                              chunk_lottery=args.chunk * n_cal * S * n_a * 12 / 1e9),
               simulation=dict(gap=sim.gap.tolist(), sd_K_over_K=(np.std(sim.K, axis=1) / model.K).tolist(),
                               saving_rule_slope=None if rule is None else rule[:, 1].tolist(),
                               saving_rule_R2=None if rule is None else rule[:, 3].tolist(),
                               gini_min=sim.stats.gini.min(axis=1).tolist(), gini_max=sim.stats.gini.max(axis=1).tolist()))
    write(args.out, out)
    print(json.dumps({k: out[k] for k in ("shape", "rows", "rows_turned", "forward_forms", "simulation", "sigma", "sigma_attempts", "policy_jacobian_ms", "simulate_wall_ms", "stage_ms", "synthesis_TFLOPs",
                                          "synthesis_launch", "contraction_ms", "contraction_TFLOPs",
                                          "synthesis_over_contraction")}, indent=1))


if __name__ == "__main__":
    main()
