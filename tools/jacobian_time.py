#!/usr/bin/env python3
"""Timing of the sequence-space Jacobian of the household block (csrc/transition_jac.hip) at
the Table II size: 24 calibrations, n_a = 10 000, T = 300.

  python tools/jacobian_time.py [--n-a N --T T --reps R --out FILE]
      (a) ms per stage of household_jacobian (backward sweeps, fan-out steps, differences,
          expectation recursion, contraction, host accumulation), each stage synchronised,
          median of R builds after a warm one;
      (b) the contraction alone by HIP events and its achieved FP64 TFLOP/s
          (2 T 2(T+1) S n_a flop per calibration);
      (c) the whole Jacobian against 2(T+1) evaluations of household_block, the cost of the
          same matrices by one perturbed block evaluation per column;
      (d) block evaluations of solve_transition by method, Newton (Jacobian reused) against
          the damped loop, on the TFP shock of the tests.
One JSON document, written to --out (default profiles/jacobian_time.json)."""
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jacobian_time.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from aiyagari_hark_amd import _lib, build
    from aiyagari_hark_amd.stationary import table2_calibrations
    from aiyagari_hark_amd.transition import (JacobianBuffers, TransitionBuffers, household_block, household_jacobian,
                                              jacobian_contract, path_prices, solve_transition, steady_state)
    if not torch.cuda.is_available():
        raise SystemExit("jacobian_time.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    T, n_a = args.T, args.n_a
    cals = table2_calibrations()
    batch, r_star, K_star = steady_state(cals, n_a, device=dev)
    n_cal, S = len(cals), batch.S
    med = statistics.median
    h = _lib.handle(dev.index)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # (a) the stages
    buf = JacobianBuffers(batch, T)
    household_jacobian(batch, r_star, T, buffers=buf)
    stages, wall = [], []
    for _ in range(args.reps):
        tm = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        jac = household_jacobian(batch, r_star, T, buffers=buf, timings=tm)
        wall.append((time.perf_counter() - t0) * 1e3)
        stages.append(tm)
    stage_ms = {k: med([s[k] for s in stages]) for k in stages[0]}

    # (b) the contraction alone
    t_con = [timed(lambda: jacobian_contract(dev, buf.E, buf.dD[0], buf.dD[1], buf.work, F=buf.F))
             for _ in range(args.reps + 1)][1:]
    flop = 2.0 * T * 2 * (T + 1) * S * n_a * n_cal
    arrays_GB = dict(E=buf.E.numel() * 8 / 1e9, dD_per_input=buf.dD[0].numel() * 8 / 1e9,
                     ghost=buf.ghost.numel() * 8 / 1e9,
                     lotteries=(buf.sweep.lo.numel() * 4 + buf.sweep.wlo.numel() * 8) / 1e9,
                     jacobian_work=h.lib.aiy_jacobian_work_bytes(n_cal, S, n_a, T) / 1e9,
                     sweep_work=h.lib.aiy_transition_work_bytes(n_cal, S, n_a, T + 1) / 1e9)
    del buf
    torch.cuda.empty_cache()

    # (c) one block evaluation on the steady prices
    r, w = path_prices(np.repeat(K_star[:, None], T + 1, axis=1), np.ones((1, T + 1)), batch.alpha, batch.delta)
    dR, dw = torch.as_tensor(1.0 + r).to(dev), torch.as_tensor(w).to(dev)
    tb = TransitionBuffers(batch, T)
    m_term, c_term = batch.last_tables

    def block():
        household_block(batch, dR, dw, m_term, c_term, batch.mass, want_c=False, export_policy=False, buffers=tb)

    block()
    t_blk = [timed(block) for _ in range(args.reps)]
    del tb
    torch.cuda.empty_cache()

    # (d) evaluations by method
    Z = 1.0 + 0.01 * 0.8 ** np.arange(T + 1)
    Z[T] = 1.0
    t0 = time.perf_counter()
    newton = solve_transition(batch, Z, T, tol=1e-9, max_iter=args.max_iter, method="newton", jacobian=jac)
    t_newton = time.perf_counter() - t0
    t0 = time.perf_counter()
    damped = solve_transition(batch, Z, T, damping=0.5, tol=1e-9, max_iter=args.max_iter)
    t_damped = time.perf_counter() - t0

    out = dict(shape=dict(n_cal=n_cal, S=S, n_a=n_a, T=T), reps=args.reps, h=jac.h,
               source_digest=build.source_digest(), stage_ms=stage_ms, stage_all_ms=stages,
               jacobian_wall_ms=med(wall), jacobian_wall_all_ms=wall,
               contraction_ms=med(t_con), contraction_all_ms=t_con, contraction_flop=flop,
               contraction_TFLOPs=flop / (med(t_con) * 1e-3) / 1e12, arrays_GB=arrays_GB,
               block_ms=med(t_blk), block_all_ms=t_blk, brute_force_blocks=2 * (T + 1),
               brute_force_ms=2 * (T + 1) * med(t_blk), jacobian_over_brute_force=med(wall) / (2 * (T + 1) * med(t_blk)),
               jacobian_in_blocks=med(wall) / med(t_blk),
               newton=dict(iterations=newton.iterations.tolist(), status=newton.status.tolist(),
                           max_residual=float(np.max(newton.residual)), seconds=t_newton),
               damped=dict(iterations=damped.iterations.tolist(), status=damped.status.tolist(),
                           converged=int(np.sum(damped.status == 0)), seconds=t_damped, max_iter=args.max_iter))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("shape", "stage_ms", "jacobian_wall_ms", "contraction_ms", "contraction_TFLOPs",
                                          "block_ms", "jacobian_over_brute_force", "newton", "damped")}, indent=1))


if __name__ == "__main__":
    main()
