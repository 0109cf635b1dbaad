#!/usr/bin/env python3
"""Timing of the welfare entry points (csrc/welfare.hip) at the Table II size: 24 calibrations,
n_a = 10 000, T = 300.

  python tools/welfare_time.py [--n-a N --T T --reps R --out FILE]
      (a) ms per backward value sweep by aiy_value_backward, without and with V_path_out, and per
          forward sweep by aiy_transition_forward (with C) on the same lotteries, alternating,
          HIP events, medians of R after a warm run of each; the bytes the value sweep must
          move (lo, wlo, two gathered G, one G written: 36 B per point and period at most, 28 B
          when both gathered neighbours come from one line; + 8 B with V_path_out) over the time;
      (b) ms and steps of the steady value solve aiy_value_stationary at tol = 1e-10 (blocking:
          host clock around the call, which ends in a synchronise), and ms per step;
      (c) ms of aiy_value_reduce and of aiy_consumption_equivalent;
      (d) a check of the run: 5 periods at the steady lottery from V* leave sum mass* V unchanged
          (mass* is invariant and V* a fixed point), relative difference recorded.
The path is priced at K* with the default TFP shock (not an equilibrium path: the timing does
not depend on it).  One JSON document, written to --out (default profiles/welfare_time.json)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "welfare_time.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from aiyagari_hark_amd import _lib, build
    from aiyagari_hark_amd import welfare as W
    from aiyagari_hark_amd.stationary import table2_calibrations
    from aiyagari_hark_amd.transition import (TransitionBuffers, path_prices, steady_state, transition_backward,
                                              transition_forward)
    if not torch.cuda.is_available():
        raise SystemExit("welfare_time.py measures on the GPU; none found")
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
    transition_backward(batch, dR, dw, m_term, c_term, buf, export_policy=False)
    med = statistics.median
    h = _lib.handle(dev.index)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    # (b) the steady value: blocking, so a host clock around it is a device time + the polls
    info = {}
    W.stationary_value(batch, info=info)   # warm
    t_steady = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        V_star = W.stationary_value(batch, info=info)
        torch.cuda.synchronize()
        t_steady.append((time.perf_counter() - t0) * 1e3)
    steps = int(np.max(info["iterations"]))

    # (a) the sweeps, alternating
    work = torch.empty(int(h.lib.aiy_value_work_bytes(n_cal, S, n_a)), dtype=torch.uint8, device=dev)
    V0 = torch.empty((n_cal, S, n_a), dtype=torch.float64, device=dev)
    V_path = torch.empty((T, n_cal, S, n_a), dtype=torch.float64, device=dev)

    def value(path):
        h.check(h.lib.aiy_value_backward(h.h, n_cal, S, n_a, T, _lib.ptr(buf.lo), _lib.ptr(buf.wlo),
                                         _lib.ptr(batch.d_P), _lib.ptr(batch.d_a), _lib.ptr(dR), _lib.ptr(dw),
                                         _lib.ptr(batch.d_lab), _lib.ptr(batch.d_beta), _lib.ptr(batch.d_crra),
                                         _lib.ptr(V_star), _lib.ptr(work), _lib.ptr(V0),
                                         _lib.ptr(V_path) if path else None, _lib.stream_ptr()), "aiy_value_backward")

    def forward():
        buf.mass.copy_(batch.mass)
        return transition_forward(batch, buf.lo, buf.wlo, buf.mass, T, buf.work, dR, dw, want_c=True)

    value(False)
    V0_plain = V0.clone()
    value(True)
    same = bool(torch.equal(V0_plain, V0) and torch.equal(V_path[0], V0))
    forward()
    t_val, t_path, t_fwd = [], [], []
    for _ in range(args.reps):
        t_val.append(timed(lambda: value(False))[0])
        t_path.append(timed(lambda: value(True))[0])
        t_fwd.append(timed(forward)[0])
    points = n_cal * S * n_a * T

    # (c) reduce and consumption equivalents
    W.value_reduce(batch, batch.mass, V0)
    t_red = [timed(lambda: W.value_reduce(batch, batch.mass, V0))[0] for _ in range(args.reps)]
    W.consumption_equivalent(batch, V0, V_star)
    t_ce = [timed(lambda: W.consumption_equivalent(batch, V0, V_star))[0] for _ in range(args.reps)]
    res = W.welfare(batch, V0, V_star, batch.mass)

    # (d) T periods at the steady lottery from V*: mass* is invariant, so sum mass* V_0 = sum mass* V*
    lo_s, wlo_s, sR, sw = W.steady_lottery(batch)
    Tc = 5
    V_again = W.path_value(batch, lo_s[None].repeat(Tc, 1, 1, 1), wlo_s[None].repeat(Tc, 1, 1, 1),
                           sR[:, None].repeat(1, Tc + 1), sw[:, None].repeat(1, Tc + 1), V_star)
    Wa = W.value_reduce(batch, batch.mass, V_again).sum(axis=1)
    Wb = W.value_reduce(batch, batch.mass, V_star).sum(axis=1)

    out = dict(shape=dict(n_cal=n_cal, S=S, n_a=n_a, T=T), reps=args.reps, source_digest=build.source_digest(),
               value_sweep_ms=med(t_val), value_sweep_all_ms=t_val, value_sweep_path_ms=med(t_path),
               value_sweep_path_all_ms=t_path, forward_ms=med(t_fwd), forward_all_ms=t_fwd,
               value_over_forward=med(t_val) / med(t_fwd), path_same_bits=same,
               value_bytes_low=28 * points, value_bytes_high=36 * points,
               value_GBps_low=28 * points / (med(t_val) * 1e-3) / 1e9,
               value_GBps_high=36 * points / (med(t_val) * 1e-3) / 1e9,
               value_path_GBps_low=36 * points / (med(t_path) * 1e-3) / 1e9,
               steady=dict(tol=1e-10, ms=med(t_steady), all_ms=t_steady, steps_max=steps,
                           steps=[int(x) for x in info["iterations"]], ms_per_step=med(t_steady) / steps,
                           dist=[float(x) for x in info["dist"]],
                           max_abs_V=[float(x) for x in V_star.abs().amax(dim=(1, 2)).cpu()]),
               reduce_ms=med(t_red), reduce_all_ms=t_red, ce_ms=med(t_ce), ce_all_ms=t_ce,
               priced_at_K_star=dict(ce_aggregate=res.ce_aggregate.tolist(), ce_node_min=float(res.ce.min()),
                                     ce_node_max=float(res.ce.max())),
               steady_invariance_rel=float(np.max(np.abs(Wa - Wb) / np.abs(Wb))))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("shape", "value_sweep_ms", "value_sweep_path_ms", "forward_ms",
                                          "value_GBps_low", "value_GBps_high", "path_same_bits", "reduce_ms", "ce_ms",
                                          "steady_invariance_rel")}, indent=1))
    print(json.dumps({k: out["steady"][k] for k in ("ms", "steps_max", "ms_per_step")}))


if __name__ == "__main__":
    main()
