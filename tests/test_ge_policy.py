"""CPU tests of the GE search policy and the EGM acceleration helpers of csrc/ge_search.h
(GeEval, aa_*, egm_extrap_factor): the scalar decisions the host-driven search (ge.hip, egm.hip)
and the device-resident kernel (ge_resident.hip) share.  tests/cpu/ge_policy_main.hip drives them
on the host, built with the library's floating-point flags and the host sanitizers; every
double crosses the pipe as a hex float, so sequences are compared bit for bit."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA, DELTA, DISC = 0.36, 0.08, 0.96
LO0, HI0 = -0.5 * DELTA, 1.0 / DISC - 1.0 - 1e-9
EGM_TOL, HIST_TOL = 1e-8, 1e-12
hexf = float.fromhex


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    from aiyagari_hark_amd import build
    exe = str(tmp_path_factory.mktemp("ge_policy") / "ge_policy_main")
    subprocess.run([build.hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-Xarch_host",
                    "-fsanitize=address,undefined", os.path.join(ROOT, "tests", "cpu", "ge_policy_main.hip"), "-o", exe],
                   check=True)

    def run(*args):
        # (a sanitizer report fails the run: ASan exits non-zero, UBSan is told to)
        env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1")
        out = subprocess.run([exe] + [a.hex() if isinstance(a, float) else str(a) for a in args], check=True, env=env,
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert out.stderr == "", out.stderr
        return [ln.split() for ln in out.stdout.splitlines()]
    return run


def supply(r, A):
    """The driver's synthetic K_s(r), + - * / only."""
    return A * (r + 0.06) / (0.0417 - r)


def demand(r):
    return (ALPHA / (r + DELTA)) ** (1.0 / (1.0 - ALPHA))


def search(driver, method, loose, logsec, r_tol, A, pert, max_steps=60):
    lines = driver("search", method, loose, logsec, float(r_tol), max_steps, float(A), float(pert))
    keys = ("r", "Kd", "loose", "adapt", "etol", "htol", "theta", "refine", "final", "lo", "hi", "xcur", "xblk")
    evs = []
    for t in lines[:-1]:
        assert t[0] == "E" and len(t) == 1 + len(keys)
        evs.append({k: (int(v) if k in ("loose", "adapt", "refine", "final") else hexf(v)) for k, v in zip(keys, t[1:])})
    assert lines[-1][0] == "END"
    return evs, dict(done=int(lines[-1][1]), steps=int(lines[-1][2]), x=hexf(lines[-1][3]))


def test_prices_and_bracket_defaults(driver):
    from aiyagari_hark_amd.stationary import firm_prices
    evs, _ = search(driver, 0, 0, 0, 1e-7, 0.5, 0.0)
    assert evs[0]["r"] == 0.5 * (LO0 + HI0) and evs[0]["lo"] == LO0 and evs[0]["hi"] == HI0
    for e in evs:
        Kd = firm_prices(e["r"], ALPHA, DELTA)[-1]
        assert abs(e["Kd"] - Kd) <= 4 * np.finfo(float).eps * Kd


@pytest.mark.parametrize("A", [0.3, 0.55, 0.9])
def test_bisection_is_the_oracle_rule(driver, A):
    """Method 0: oracle/stationary.py ge_bisect's rule, written out here."""
    r_tol = 1e-7
    evs, end = search(driver, 0, 0, 0, r_tol, A, 0.0)
    lo, hi, k = LO0, HI0, 0
    while hi - lo > r_tol and k < 60:
        mid = 0.5 * (lo + hi)
        assert evs[k]["r"] == mid
        e = evs[k]
        assert (e["loose"], e["adapt"], e["refine"], e["final"], e["etol"], e["htol"]) == (0, 0, 0, 0, EGM_TOL, HIST_TOL)
        if supply(mid, A) > e["Kd"]:
            hi = mid
        else:
            lo = mid
        k += 1
    assert k == len(evs) == end["steps"] and end["done"] == 1 and end["x"] == 0.5 * (lo + hi)


@pytest.mark.parametrize("A", [0.3, 0.55, 0.9])
def test_brent_is_the_python_mirror(driver, A):
    """Method 1 without loose bracketing: aiyagari_hark_amd.stationary._Brent fed the same f."""
    from aiyagari_hark_amd.stationary import _Brent
    r_tol = 1e-7
    evs, end = search(driver, 1, 0, 0, r_tol, A, 0.0)
    b = _Brent(LO0, HI0, r_tol)
    for e in evs:
        assert not b.done and e["r"] == b.propose()
        assert (e["loose"], e["adapt"], e["refine"], e["final"], e["etol"], e["htol"]) == (0, 0, 0, 0, EGM_TOL, HIST_TOL)
        b.update(supply(e["r"], A) - e["Kd"])
    assert b.done and end["done"] == 1 and end["x"] == b.x and end["steps"] == len(evs)


def test_loose_searches_refine_and_final_pass(driver):
    """Loose bracketing with the log-secant levels 0 / 1 / 2; K_s is off by 4e5 htol K_d (the
    BiCGSTAB stopping rule's error), so evaluations near the root are refined."""
    refined = finals = full_ends = 0
    for logsec in (0, 1, 2):
        for A in (0.3, 0.55, 0.7, 0.9):
            for r_tol in (1e-7, 3e-4):
                evs, end = search(driver, 1, 1, logsec, r_tol, A, 4e5)
                assert end["done"] == 1 and end["steps"] <= 60
                for k, e in enumerate(evs):
                    assert -1.0 <= e["theta"] <= 1.0
                    if k < 2 or e["final"]:
                        assert e["theta"] == 0.0
                    assert not (e["loose"] and e["adapt"])
                    if e["loose"]:
                        assert (e["etol"], e["htol"]) == (1e-6, 1e-8)
                    else:
                        assert e["etol"] == EGM_TOL and HIST_TOL <= e["htol"] <= 1e-8
                        assert e["adapt"] == (e["htol"] > HIST_TOL)
                    if e["refine"]:   # the same r again at the full tolerances, the bracket untouched
                        p = evs[k - 1]
                        refined += 1
                        assert p["loose"] or p["adapt"]
                        assert (e["loose"], e["adapt"], e["etol"], e["htol"]) == (0, 0, EGM_TOL, HIST_TOL)
                        assert all(e[q] == p[q] for q in ("r", "lo", "hi", "xcur", "xblk"))
                # the evaluation the search ended on: evs[-1], or evs[-2] before a final pass
                n_final = sum(e["final"] for e in evs)
                last = evs[-2] if n_final else evs[-1]
                assert n_final == (1 if last["loose"] or last["adapt"] else 0)
                assert all(not e["final"] for e in evs[:-1])
                if n_final:
                    f = evs[-1]
                    finals += 1
                    assert f["r"] == last["r"] and (f["loose"], f["adapt"], f["etol"], f["htol"]) == (0, 0, EGM_TOL, HIST_TOL)
                    assert end["steps"] == len(evs) - 1
                else:
                    full_ends += 1
                    assert end["steps"] == len(evs)
                # the root of K_s + its error, bracketed to r_tol (5 % / 5e6 tol sign margins)
                g = lambda r: supply(r, A) - demand(r)   # noqa: E731
                assert g(end["x"] - 2 * r_tol) < 0 < g(end["x"] + 2 * r_tol)
    assert refined > 0, "no input reached the refine branch"
    assert finals > 0, "no input reached the final-pass branch"
    assert full_ends > 0, "no search ended on a full-tolerance evaluation"


def test_anderson_recovers_a_linear_fixed_point(driver):
    """w_k = x* + sum_i c_i lam_i^k v_i (three modes on disjoint points): the type-II mix of
    w0 .. w4 is x*; an all-equal chain has a zero Gram matrix: no mix."""
    xs = np.array([1.0, 1.5, 0.75, 2.0, 1.25, 0.5])
    lam = np.array([0.8, 0.8, 0.3, 0.3, -0.4, -0.4])
    amp = np.array([0.10, -0.05, 0.08, 0.12, -0.09, 0.06])
    w = [xs + amp * lam ** k for k in range(5)]
    out = driver("aa", 6, *[float(v) for v in np.concatenate(w)])
    assert out[0][:2] == ["MIX", "1"]
    mixed = np.array([hexf(v) for v in out[0][2:]])
    assert np.max(np.abs(mixed - xs) / np.abs(xs)) <= 1e-9
    assert np.max(np.abs(w[4] - xs) / np.abs(xs)) > 1e-4   # (the plain chain is still far)
    same = driver("aa", 6, *[float(v) for v in np.concatenate([xs] * 5)])
    assert same == [["MIX", "0"]]


def test_extrapolation_rule(driver):
    """factor = lam / (1 - lam) only if n >= 4, d1 > 100 tol, 0.5 < lam < 0.999, a previous
    rate, and |lam - lam_prev| < 0.2 (1 - lam); lam_prev always moves to lam."""
    def ext(d1, d0, etol, n, lam_prev):
        (tag, f, lp), = driver("ext", float(d1), float(d0), float(etol), n, float(lam_prev))
        assert tag == "EXT" and hexf(lp) == d1 / d0
        return hexf(f)
    lam = 0.9e-3 / 1e-3
    assert ext(0.9e-3, 1e-3, 1e-8, 32, 0.91) == lam / (1.0 - lam)
    assert ext(0.9e-3, 1e-3, 1e-8, 3, 0.91) == 0.0        # n < 4
    assert ext(0.9e-3, 1e-3, 1e-5, 32, 0.91) == 0.0       # d1 <= 100 tol
    assert ext(0.4e-3, 1e-3, 1e-8, 32, 0.41) == 0.0       # lam <= 0.5
    assert ext(0.9995e-3, 1e-3, 1e-8, 32, 0.9995) == 0.0  # lam >= 0.999
    assert ext(0.9e-3, 1e-3, 1e-8, 32, -1.0) == 0.0       # no previous rate
    assert ext(0.9e-3, 1e-3, 1e-8, 32, 0.95) == 0.0       # the rate is not steady
