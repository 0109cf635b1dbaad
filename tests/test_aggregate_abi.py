"""CPU tests of the aggregate-risk entry points of the C ABI (csrc/aggregate.hip): argument
validation before any device work, and header / exports / ctypes agreement.  The entry points
need no work space, so there is no aiy_aggregate_work_bytes to test."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aiyagari.h")
NAMES = ("aiy_lottery_mean", "aiy_aggregate_lotteries")


@pytest.fixture(scope="module")
def lib():
    from aiyagari_hark_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_null_handle_is_refused(lib):
    assert lib.aiy_lottery_mean(None, 2, 7, 120, 5, None, None, None, None, None) == -1
    assert lib.aiy_aggregate_lotteries(None, 2, 7, 120, 5, 3, None, None, None, None, None, None, None, None) == -1
    assert lib.aiy_version() == 210


def test_header_exports_and_ctypes_agree(lib):
    from aiyagari_hark_amd import _lib
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(aiy_\w+)\s*\(", src, re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (aiy_\w+)", out))
    for name in NAMES:
        assert name in declared and name in exported and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert _lib.SIGNATURES[name][0] is ctypes.c_int32
        decl = re.search(name + r"\s*\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1])
        # the handle first, the caller's stream last
        assert decl.split(",")[0].strip() == "aiy_handle* h" and decl.split(",")[-1].strip() == "aiy_stream stream"
    assert set(_lib.SIGNATURES) <= exported
    assert "aiy_aggregate_work_bytes" not in declared and "aiy_aggregate_work_bytes" not in exported


def test_package_exports_aggregate_api():
    import aiyagari_hark_amd as pkg
    for name in ("policy_jacobian", "PolicyJacobian", "ar1", "linear_model", "AggregateModel", "moments",
                 "expectations", "simulate", "AggregateSimulation", "saving_rule"):
        assert callable(getattr(pkg, name))
    assert list(pkg.ar1(0.5, 3)) == [1.0, 0.5, 0.25, 0.125]
    # the earlier API is still there
    assert callable(pkg.household_jacobian) and callable(pkg.path_wealth_stats)
