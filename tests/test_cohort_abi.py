"""CPU tests of the C ABI of the cohort sweep: header / exports / ctypes
agreement, the host-only work-space size, and the argument checks of the Python interface that
run before any device is touched."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aiyagari.h")
NAMES = ("aiy_cohort_work_bytes", "aiy_cohort_forward")
SHAPES = ((3, 7, 120, 5, 5, 5), (24, 7, 10000, 1, 10, 10), (2, 64, 65, 5, 16, 32))   # n_cal, S, n_a, n_lot, G, Q


@pytest.fixture(scope="module")
def lib():
    from aiyagari_hark_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_header_exports_and_ctypes_agree(lib):
    from aiyagari_hark_amd import _lib, build
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(aiy_\w+)\s*\(", src, re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (aiy_\w+)", out))
    for name in NAMES:
        assert name in declared and name in exported and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.SIGNATURES["aiy_cohort_work_bytes"][0] is ctypes.c_int64
    assert len(_lib.SIGNATURES["aiy_cohort_work_bytes"][1]) == 6
    decl = re.search(r"int32_t aiy_cohort_forward\(([^)]*)\)", src).group(1)
    args = [a.strip() for a in decl.split(",")]
    assert len(args) == len(_lib.SIGNATURES["aiy_cohort_forward"][1]) == 23
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "h", "n_cal", "S", "n_a", "T", "n_lot", "G", "Q", "lo", "wlo", "P", "a_grid", "R", "w", "lab", "edges", "work",
        "mass", "K_out", "C_out", "occ_out", "inc_out", "stream"]
    assert "#define AIY_MAX_COHORTS 16" in src and "#define AIY_MAX_CLASSES 32" in src
    assert _lib.AIY_MAX_COHORTS == 16 and _lib.AIY_MAX_CLASSES == 32
    assert "cohort.hip" in build.SOURCES


def test_work_bytes_host_only(lib):
    for n_cal, S, n_a, n_lot, G, Q in SHAPES:
        b = lib.aiy_cohort_work_bytes(n_cal, S, n_a, n_lot, G, Q)
        assert b > 0 and b % 256 == 0
        # the inverse index and the partner of the cohorts are in it
        assert b >= 4 * n_lot * n_cal * S * (n_a + 1) + 8 * G * n_cal * S * n_a
        if G > 1:
            assert lib.aiy_cohort_work_bytes(n_cal, S, n_a, n_lot, G - 1, Q) < b
        assert lib.aiy_cohort_work_bytes(n_cal, S, n_a, n_lot, 1, Q) < b
        one, five = (lib.aiy_cohort_work_bytes(n_cal, S, n_a, n, G, Q) for n in (1, 5))
        assert five - one >= 4 * 5 * n_cal * S * (n_a + 1)
    n_cal, S, n_a, n_lot, G, Q = SHAPES[0]
    for bad in (dict(G=0), dict(G=17), dict(Q=0), dict(Q=33), dict(S=65), dict(n_a=1), dict(n_lot=0)):
        a = dict(n_cal=n_cal, S=S, n_a=n_a, n_lot=n_lot, G=G, Q=Q)
        a.update(bad)
        assert lib.aiy_cohort_work_bytes(a["n_cal"], a["S"], a["n_a"], a["n_lot"], a["G"], a["Q"]) == -1, bad


def test_null_handle_is_refused_and_version_stays(lib):
    assert lib.aiy_cohort_forward(None, 3, 7, 120, 5, 5, 5, 5, *([None] * 15)) == -1
    assert lib.aiy_version() == 210


def test_package_names_are_lazy():
    import aiyagari_hark_amd as pkg
    from aiyagari_hark_amd import mobility
    assert pkg.mobility is mobility and pkg.cohort_forward is mobility.cohort_forward
    assert pkg.wealth_classes is mobility.wealth_classes and pkg.MobilityResult is mobility.MobilityResult
    assert pkg.cohorts_by_class is mobility.cohorts_by_class and pkg.cohorts_by_state is mobility.cohorts_by_state
    assert pkg.CohortPaths is mobility.CohortPaths
    assert "cohorts" in pkg.TransitionResult.__dataclass_fields__


def test_arguments_are_checked_before_any_device_work():
    """``mobility`` refuses bad horizons, by and percentiles, and ``cohort_forward`` a lottery of
    neither 1 nor T periods, with ValueError: batch = None would fail otherwise."""
    from aiyagari_hark_amd import mobility as M
    for horizons in ((), (0, 1), (-1,), (5, 1), (1, 1), (1.5,), (1, 2.0), 3, (True,)):
        with pytest.raises(ValueError, match="horizons"):
            M.mobility(None, horizons=horizons)
    for by in ("rank", "Wealth", None, 0):
        with pytest.raises(ValueError, match="by must be"):
            M.mobility(None, by=by)
    for pct in ((0.0, 0.5), (0.5, 1.0), (0.5, 0.2), (0.2, 0.2), (), tuple(np.linspace(0.05, 0.95, 16)), 0.5, None):
        with pytest.raises(ValueError, match="[Pp]ercentiles"):
            M.mobility(None, percentiles=pct)
        with pytest.raises(ValueError, match="[Pp]ercentiles"):
            M.wealth_classes(None, percentiles=pct)
    assert M._check_class_percentiles(tuple(np.linspace(0.05, 0.95, 15))).size == 15
    assert M._check_class_percentiles([0.5]).tolist() == [0.5]
    lot = types.SimpleNamespace(shape=(3, 2, 7, 120))
    for T in (2, 4, 0):
        with pytest.raises(ValueError, match="lottery periods"):
            M.cohort_forward(None, lot, lot, None, T, None)
    from aiyagari_hark_amd import transition
    with pytest.raises(ValueError, match="[Pp]ercentiles"):
        transition.solve_transition(types.SimpleNamespace(cals=[None], S=7, n_a=120), [1.0, 1.0], 1, cohorts=(0.5, 0.2))


def test_class_rule_is_the_reference_rule():
    from aiyagari_hark_amd import mobility as M
    from tests import mobility_ref as MR
    rng = np.random.default_rng(11)
    p = np.array([0.2, 0.4, 0.6, 0.8])
    for g in (rng.uniform(size=40), np.array([0.25, 0.25, 0.25, 0.25]), np.eye(9)[4], rng.uniform(size=7) ** 8):
        e = M.class_edges(g, p)
        assert e.dtype == np.int32 and np.array_equal(e, MR.class_edges(g, p))
