#!/usr/bin/env python3
"""Timing of the period marginals and of the histogram wealth statistics (csrc/transition.hip,
csrc/dist_stats.hip) at the Table II size: 24 calibrations, n_a = 10 000, T = 300.

  python tools/dist_stats_time.py [--n-a N --T T --reps R --out FILE]
      (a) ms per forward sweep by aiy_transition_forward and by aiy_transition_forward_marginals
          on the same lotteries, alternating, HIP events, medians of R after a warm run of each:
          the overhead of the T + 1 marginal launches against the unchanged entry (and a check
          that Ks, C and mass_T have the same bits);
      (b) ms of aiy_dist_stats over the (T + 1) x 24 marginals at the notebook's 15 percentiles,
          one call on the full work space, and of stats.histogram_stats (the 256 MB slab loop of
          the Python layer), with the GB/s of the 8 B per node the statistics must read.
One JSON document, written to --out (default profiles/dist_stats_time.json)."""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dist_stats_time.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from aiyagari_hark_amd import _lib, build
    from aiyagari_hark_amd.stationary import table2_calibrations
    from aiyagari_hark_amd.stats import SLAB_BYTES, histogram_stats
    from aiyagari_hark_amd.transition import (TransitionBuffers, path_prices, path_wealth_stats, steady_state,
                                              transition_backward, transition_forward)
    if not torch.cuda.is_available():
        raise SystemExit("dist_stats_time.py measures on the GPU; none found")
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
    buf = TransitionBuffers(batch, T, marginals=True)
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

    def forward(marg):
        buf.mass.copy_(batch.mass)
        return transition_forward(batch, buf.lo, buf.wlo, buf.mass, T, buf.work, dR, dw, want_c=True, marg=marg)

    # (a) the two entries, alternating
    Ks0, C0 = forward(None)
    mT0 = buf.mass.clone()
    Ks1, C1 = forward(buf.marg)
    same = bool(np.array_equal(Ks0, Ks1) and np.array_equal(C0, C1) and torch.equal(mT0, buf.mass))
    del mT0
    t_plain, t_marg = [], []
    for _ in range(args.reps):
        t_plain.append(timed(lambda: forward(None))[0])
        t_marg.append(timed(lambda: forward(buf.marg))[0])
    points = n_cal * S * n_a * T
    marg_bytes = 8 * (S + 1) * n_cal * n_a * (T + 1)

    # (b) the statistics of the (T + 1) x n_cal marginals
    pct = np.linspace(0.01, 0.999, 15)
    n_dist = (T + 1) * n_cal
    marg = buf.marg
    work_bytes = int(h.lib.aiy_dist_stats_work_bytes(n_dist, n_a))
    work = torch.empty(work_bytes, dtype=torch.uint8, device=dev)
    lor, pcl, summ = np.empty((n_dist, pct.size)), np.empty((n_dist, pct.size)), np.empty((n_dist, 4))
    dp = _lib.c_double_p

    def one_call():
        h.check(h.lib.aiy_dist_stats(h.h, n_dist, n_cal, n_a, _lib.ptr(marg), _lib.ptr(batch.d_a),
                                     pct.ctypes.data_as(dp), pct.size, _lib.ptr(work), lor.ctypes.data_as(dp),
                                     pcl.ctypes.data_as(dp), summ.ctypes.data_as(dp), _lib.stream_ptr()),
                "aiy_dist_stats")

    one_call()
    t_one = [timed(one_call)[0] for _ in range(args.reps)]
    del work
    torch.cuda.empty_cache()
    ws = histogram_stats(marg, batch.d_a, pct, marginal=True)
    t_slab = [timed(lambda: histogram_stats(marg, batch.d_a, pct, marginal=True))[0] for _ in range(args.reps)]
    slab_same = bool(np.array_equal(ws.gini.reshape(-1), summ[:, 2]) and
                     np.array_equal(ws.lorenz.reshape(n_dist, -1), lor) and
                     np.array_equal(ws.percentile_values.reshape(n_dist, -1), pcl, equal_nan=True))
    path = path_wealth_stats(batch, marg, pct)
    read_bytes = 8 * n_dist * n_a

    out = dict(shape=dict(n_cal=n_cal, S=S, n_a=n_a, T=T), reps=args.reps, source_digest=build.source_digest(),
               forward_ms=med(t_plain), forward_all_ms=t_plain, forward_marginals_ms=med(t_marg),
               forward_marginals_all_ms=t_marg, marginals_overhead=med(t_marg) / med(t_plain) - 1.0,
               marginals_same_bits=same, forward_algorithmic_bytes=28 * points, marginal_bytes=marg_bytes,
               marginal_bytes_share=marg_bytes / (28 * points), marg_GB=marg.numel() * 8 / 1e9,
               masses_GB=marg.numel() * 8 * S / 1e9,
               dist_stats=dict(n_dist=n_dist, n_p=int(pct.size), one_call_ms=med(t_one), one_call_all_ms=t_one,
                               one_call_GBps=read_bytes / (med(t_one) * 1e-3) / 1e9, work_GB=work_bytes / 1e9,
                               slab_loop_ms=med(t_slab), slab_loop_all_ms=t_slab,
                               slab_loop_GBps=read_bytes / (med(t_slab) * 1e-3) / 1e9,
                               slab_distributions=max(1, SLAB_BYTES // (16 * n_a)), slab_equals_one_call=slab_same,
                               read_bytes=read_bytes),
               gini=dict(steady=path.gini[:, 0].tolist(), largest_move=float(np.max(np.abs(path.gini - path.gini[:, :1]))),
                         nan_percentiles=int(np.isnan(path.percentile_values).sum())))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("shape", "forward_ms", "forward_marginals_ms", "marginals_overhead",
                                          "marginals_same_bits", "dist_stats")}, indent=1))


if __name__ == "__main__":
    main()
