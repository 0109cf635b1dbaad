#!/usr/bin/env python3
"""Timing of one household-block evaluation of the transition path (csrc/transition.hip) at
the Table II size: 24 calibrations, n_a = 10 000, T = 300.

  python tools/transition_time.py [--n-a N --T T --reps R --cpu-cals C] > times.json
      (a) ms per fused backward sweep (aiy_transition_backward) against the same sweep chained
          from aiy_egm_step + aiy_hist_lottery, alternating, HIP events, after a warm run of each
          (and a check that the two give the same bits);
      (b) ms per forward sweep (aiy_transition_forward, its index / check pass included) and the
          achieved bytes/s against the algorithmic 28 B per (state, node, period);
      (d) seconds of the NumPy reference block (tests/transition_ref.py) for --cpu-cals of the
          calibrations at the same shape, scaled to all of them.
  rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- \
      python tools/transition_time.py --profile
      the sweeps alone (1 warm + R of each), for the kernel-time sums;
  python tools/transition_time.py --combine times.json DIR/.../run_kernel_stats.csv
      (c) the launch-gap share of each sweep: event time minus the kernels' summed time.
One JSON document on stdout per mode."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def combine(times_path, stats_path):
    times = json.load(open(times_path))
    rows = list(csv.DictReader(open(stats_path)))

    def total(sub):
        sel = [r for r in rows if sub in r["Name"]]
        return sum(int(r["TotalDurationNs"]) for r in sel) / 1e6, sum(int(r["Calls"]) for r in sel)

    # sweeps in the profiled run: one lottery-only launch per backward sweep, one K0 launch per forward sweep
    n_back = sum(int(r["Calls"]) for r in rows if "tr_backward_kernel" in r["Name"] and "false" in r["Name"])
    n_fwd = total("tr_K0_kernel")[1]
    back_ms, back_calls = total("tr_backward_kernel")
    fwd_ms = sum(total(k)[0] for k in ("tr_forward_kernel", "tr_range_kernel", "tr_K0_kernel", "tr_sum_kernel"))
    fwd_calls = sum(total(k)[1] for k in ("tr_forward_kernel", "tr_range_kernel", "tr_K0_kernel", "tr_sum_kernel"))
    out = dict(shape=times["shape"])
    for name, ev, ker, n, calls in (("backward", times["backward_fused_ms"], back_ms, n_back, back_calls),
                                    ("forward", times["forward_ms"], fwd_ms, n_fwd, fwd_calls)):
        per = ker / max(1, n)
        out[name] = dict(event_ms=ev, kernel_ms_per_sweep=per, launches_per_sweep=calls / max(1, n),
                         profiled_sweeps=n, launch_gap_ms=ev - per, launch_gap_share=(ev - per) / ev)
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-a", type=int, default=10000)
    ap.add_argument("--T", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-cals", type=int, default=1)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--combine", nargs=2, metavar=("TIMES_JSON", "KERNEL_STATS_CSV"))
    args = ap.parse_args()
    if args.combine:
        return combine(*args.combine)

    import numpy as np
    import torch

    from aiyagari_hark_amd import _lib, build
    from aiyagari_hark_amd.egm import EgmBatch, egm_step
    from aiyagari_hark_amd.stationary import table2_calibrations
    from aiyagari_hark_amd.transition import (TransitionBuffers, path_prices, steady_state, transition_backward,
                                              transition_forward)
    if not torch.cuda.is_available():
        raise SystemExit("transition_time.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    T, n_a = args.T, args.n_a
    cals = table2_calibrations()
    batch, r_star, K_star = steady_state(cals, n_a, device=dev)
    n_cal, S = len(cals), batch.S
    Z = 1.0 + 0.01 * 0.8 ** np.arange(T + 1)
    Z[T] = 1.0
    r, w = path_prices(np.repeat(K_star[:, None], T + 1, axis=1), Z[None, :], batch.alpha, batch.delta)
    R = 1.0 + r
    dR, dw = torch.as_tensor(R).to(dev), torch.as_tensor(w).to(dev)
    m_term, c_term = (t.reshape(n_cal, S, n_a + 1).contiguous() for t in batch.last_tables)
    buf = TransitionBuffers(batch, T)
    h = _lib.handle(dev.index)
    sp = _lib.stream_ptr()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def fused():
        transition_backward(batch, dR, dw, m_term, c_term, buf, export_policy=False)

    def forward():
        buf.mass.copy_(batch.mass)
        return transition_forward(batch, buf.lo, buf.wlo, buf.mass, T, buf.work, dR, dw, want_c=True)

    if args.profile:
        for _ in range(1 + args.reps):
            fused()
            forward()
        torch.cuda.synchronize()
        print(json.dumps(dict(mode="profile", sweeps=1 + args.reps)))
        return

    # the chained sweep: every per-period input on device before the clock starts
    zeros = torch.zeros((n_cal, 1), dtype=torch.float64, device=dev)
    eb, dRt, dwt = [], [], []
    for t in range(T + 1):
        Rn = torch.as_tensor(np.repeat(R[:, t, None, None], S, axis=2)).to(dev)
        Wn = torch.as_tensor(np.repeat(w[:, t, None, None], S, axis=2)).to(dev)
        eb.append(EgmBatch(batch.d_a, zeros, batch.d_P, Rn, Wn, torch.zeros_like(Rn), batch.d_lab, batch.d_beta,
                           batch.d_crra))
        dRt.append(torch.as_tensor(np.ascontiguousarray(R[:, t])).to(dev))
        dwt.append(torch.as_tensor(np.ascontiguousarray(w[:, t])).to(dev))
    shp = (n_cal, S, 1, n_a + 1)
    pp = [(torch.empty(shp, dtype=torch.float64, device=dev), torch.empty(shp, dtype=torch.float64, device=dev))
          for _ in range(2)]
    lo2, wlo2 = torch.empty_like(buf.lo), torch.empty_like(buf.wlo)
    term = (m_term.reshape(shp), c_term.reshape(shp))

    def lottery(t, tab):
        h.check(h.lib.aiy_hist_lottery(h.h, n_cal, S, n_a, _lib.ptr(tab[0]), _lib.ptr(tab[1]), _lib.ptr(batch.d_a),
                                       _lib.ptr(dRt[t]), _lib.ptr(dwt[t]), _lib.ptr(batch.d_lab), _lib.ptr(lo2[t]),
                                       _lib.ptr(wlo2[t]), sp), "aiy_hist_lottery")

    def chained():
        cur = term
        for u in range(T, 0, -1):
            if u < T:
                lottery(u, cur)
            cur = egm_step(eb[u], cur[0], cur[1], out=pp[u & 1])
        lottery(0, cur)

    fused()
    chained()
    torch.cuda.synchronize()
    same = bool(torch.equal(buf.lo, lo2) and torch.equal(buf.wlo, wlo2))
    t_f, t_c = [], []
    for _ in range(args.reps):
        t_f.append(timed(fused))
        t_c.append(timed(chained))
    del lo2, wlo2
    forward()
    t_w = [timed(forward) for _ in range(args.reps)]
    points = n_cal * S * n_a * T
    med = statistics.median
    out = dict(shape=dict(n_cal=n_cal, S=S, n_a=n_a, T=T), reps=args.reps, source_digest=build.source_digest(),
               backward_fused_ms=med(t_f), backward_fused_all_ms=t_f, backward_chained_ms=med(t_c),
               backward_chained_all_ms=t_c, fused_equals_chained=same, fused_over_chained=med(t_f) / med(t_c),
               forward_ms=med(t_w), forward_all_ms=t_w, forward_algorithmic_bytes=28 * points,
               forward_GBps=28 * points / (med(t_w) * 1e-3) / 1e9,
               lottery_GB=12 * points / 1e9, work_GB=h.lib.aiy_transition_work_bytes(n_cal, S, n_a, T) / 1e9)
    if args.cpu_cals > 0:
        from tests import transition_ref as TR
        m_h, c_h, mass_h = m_term.cpu().numpy(), c_term.cpu().numpy(), batch.mass.cpu().numpy()
        t0 = time.perf_counter()
        for i in range(min(args.cpu_cals, n_cal)):
            with np.errstate(all="ignore"):
                TR.block(batch.aGrid[i], batch.levels[i], batch.P[i], cals[i].DiscFac, cals[i].CRRA, R[i], w[i], m_h[i],
                         c_h[i], mass_h[i])
        el = time.perf_counter() - t0
        out.update(numpy_block_s_per_cal=el / min(args.cpu_cals, n_cal),
                   numpy_block_s_all_cals=el / min(args.cpu_cals, n_cal) * n_cal, numpy_cals_timed=min(args.cpu_cals, n_cal))
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
