"""Bit fixture of the lottery-step kernels: the forward pull and mix (csrc/transition.hip,
csrc/transition_jac.hip), the adjoint step (jac_expect_kernel, value_step_kernel) and the
256-thread row reductions (value_reduce_kernel, dist_stats_kernel).

Every case is a synthetic problem of tests.test_gpu_transition.synthetic_problem (n_cal = 4 with
CRRA 1, 3, 5, 2.5 and the betas of tests/test_gpu_welfare.py, T = 3) with prices as
test_synthetic_recursion builds them (w min(lab) > a_max, so c > 0 at every node).  The
fixture holds the sha256 of the raw bytes of every output: the kernels promise the same bits
whichever entry point walks the lottery, and a change of a summation order anywhere shows
here, where the NumPy comparisons (1e-12) would let it pass.

Run by hand on the GPU, at the commit whose bits are to be kept:

    python tests/golden/make_lottery_bits.py --commit $(git rev-parse --short HEAD)

Output: tests/golden/lottery_step_bits.json.  tests/test_gpu_lottery_bits.py imports CASES,
build_case and run_case from here, so the inputs have one definition.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lottery_step_bits.json")

N_CAL, T = 4, 3
CRRAS = np.array([1.0, 3.0, 5.0, 2.5])
BETAS = np.array([0.96, 0.95, 0.96, 0.9])
N_EXPECT = 4                       # expectation steps
PERCENTILES = [0.1, 0.5, 0.9]
# S = 2: two waves without a state; S = 7: the last wave has one; S = 25: several rounds per wave.
# n_a = 120: a last tile of 56 live lanes; 128: none idle.  tail: a whole row on node n_a - 2.
CASES = [(2, 120, "head"), (7, 120, "tail"), (7, 128, "head"), (25, 1000, "head"), (25, 1000, "tail")]


def case_name(S, n_a, variant):
    return f"S{S}_na{n_a}_{variant}"


def build_case(S, n_a, variant):
    """The inputs of one case (NumPy), from the seed 1000 S + n_a + (variant == "tail")."""
    from tests.test_gpu_transition import synthetic_problem
    rng = np.random.default_rng(1000 * S + n_a + (variant == "tail"))
    lo, wlo, P, mass, aGrid = synthetic_problem(rng, N_CAL, S, n_a, T, variant)
    lab = rng.uniform(0.5, 1.5, size=(N_CAL, S))
    R = 1.0 + rng.uniform(0.01, 0.05, size=(N_CAL, T + 1))
    w = (1.2 * aGrid[:, -1:] / lab.min(axis=1, keepdims=True)) * rng.uniform(1.0, 1.1, size=(N_CAL, T + 1))
    assert np.all(w * lab.min(axis=1, keepdims=True) > aGrid[:, -1:])   # so c > 0 at every node
    V_term = rng.normal(size=(N_CAL, S, n_a))
    return dict(S=S, n_a=n_a, lo=lo.astype(np.int32), wlo=wlo, P=P, mass=mass, aGrid=aGrid, lab=lab, R=R, w=w,
                V_term=V_term)


def run_case(dev, case):
    """Every digested output of one case, as {name: NumPy array}, in a fixed order."""
    import torch

    from aiyagari_hark_amd import _lib, stats
    from aiyagari_hark_amd.transition import jacobian_expectation, jacobian_fanout, transition_forward
    from aiyagari_hark_amd.welfare import path_value, value_reduce
    S, n_a = case["S"], case["n_a"]
    F64 = torch.float64

    def up(x, dt=F64):
        return torch.as_tensor(np.ascontiguousarray(x)).to(dt).to(dev)

    fb = types.SimpleNamespace(cals=[None] * N_CAL, S=S, n_a=n_a, device=dev, d_P=up(case["P"]), d_a=up(case["aGrid"]),
                               d_lab=up(case["lab"]), d_beta=up(BETAS), d_crra=up(CRRAS))
    lo, wlo, dR, dw = up(case["lo"], torch.int32), up(case["wlo"]), up(case["R"]), up(case["w"])
    h = _lib.handle(dev.index)
    out = {}
    # forward sweeps
    work = torch.empty(int(h.lib.aiy_transition_work_bytes(N_CAL, S, n_a, T)), dtype=torch.uint8, device=dev)
    mass = up(case["mass"])
    marg = torch.empty((T + 1, N_CAL, n_a), dtype=F64, device=dev)
    Ks, C = transition_forward(fb, lo, wlo, mass, T, work, dR, dw, want_c=True, marg=marg)
    out.update(fwdm_Ks=Ks, fwdm_C=C, fwdm_mass=mass.cpu().numpy(), fwdm_marg=marg.cpu().numpy())
    mass = up(case["mass"])
    Ks, _ = transition_forward(fb, lo, wlo, mass, T, work, want_c=False)
    out.update(fwd_Ks=Ks, fwd_mass=mass.cpu().numpy())
    # fan-out of the three periods and the expectation steps on period 0's lottery
    jwork = torch.empty(int(h.lib.aiy_jacobian_work_bytes(N_CAL, S, n_a, N_EXPECT)), dtype=torch.uint8, device=dev)
    fan = torch.empty((T, N_CAL, S, n_a), dtype=F64, device=dev)
    jacobian_fanout(fb, lo, wlo, up(case["mass"]), fan, jwork, N_EXPECT)
    out["fanout"] = fan.cpu().numpy()
    E = torch.empty((N_EXPECT, N_CAL, S, n_a), dtype=F64, device=dev)
    jacobian_expectation(fb, lo[0].contiguous(), wlo[0].contiguous(), E, jwork)
    out["expectation"] = E.cpu().numpy()
    # values
    V_term = up(case["V_term"])
    V0, V_path = path_value(fb, lo, wlo, dR, dw, V_term, keep_path=True)
    out.update(V0=V0.cpu().numpy(), V_path=V_path.cpu().numpy())
    vwork = torch.empty(int(h.lib.aiy_value_work_bytes(N_CAL, S, n_a)), dtype=torch.uint8, device=dev)
    V = V_term.clone()
    iters, dist = np.zeros(N_CAL, dtype=np.int32), np.zeros(N_CAL)
    beta = np.ascontiguousarray(BETAS)
    R0, w0 = dR[:, 0].contiguous(), dw[:, 0].contiguous()
    h.check(h.lib.aiy_value_stationary(h.h, N_CAL, S, n_a, _lib.ptr(lo[0].contiguous()), _lib.ptr(wlo[0].contiguous()),
                                       _lib.ptr(fb.d_P), _lib.ptr(fb.d_a), _lib.ptr(R0), _lib.ptr(w0),
                                       _lib.ptr(fb.d_lab), _lib.ptr(fb.d_beta), _lib.ptr(fb.d_crra),
                                       beta.ctypes.data_as(_lib.c_double_p), 1e-8, 48, 16, _lib.ptr(V), _lib.ptr(vwork),
                                       iters.ctypes.data_as(_lib.c_int32_p), dist.ctypes.data_as(_lib.c_double_p),
                                       _lib.stream_ptr()), "aiy_value_stationary")
    out.update(steady_V=V.cpu().numpy(), steady_iterations=iters, steady_dist=dist)
    out["reduce"] = value_reduce(fb, up(case["mass"]), V0)
    ws = stats.histogram_stats(marg, fb.d_a, marginal=True, percentiles=PERCENTILES)
    for f in ("lorenz", "percentile_values", "gini", "mean", "total", "bottom_share"):
        out["stats_" + f] = getattr(ws, f)
    return out


def digests(outputs):
    return {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in outputs.items()}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cases = {case_name(*c): digests(run_case(dev, build_case(*c))) for c in CASES}
    json.dump(dict(generator="tests/golden/make_lottery_bits.py", commit=args.commit, hip=torch.version.hip,
                   cases=cases), open(args.out, "w"), indent=1)
    print("wrote", args.out, flush=True)


if __name__ == "__main__":
    main()
