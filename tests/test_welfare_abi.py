"""CPU tests of the welfare entry points of the C ABI: the host-only work-space size, the null
handle, header / exports / ctypes agreement and the Python surface."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aiyagari.h")
NAMES = {"aiy_value_work_bytes": 3, "aiy_value_backward": 19, "aiy_value_stationary": 22, "aiy_value_reduce": 8,
         "aiy_consumption_equivalent": 9}


@pytest.fixture(scope="module")
def lib():
    from aiyagari_hark_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_work_bytes_host_only(lib):
    wb = lib.aiy_value_work_bytes
    assert 0 < wb(1, 1, 2) <= wb(1, 7, 2) < wb(1, 7, 120)   # (regions are rounded up to 256 bytes) < wb(4, 7, 120) < wb(4, 25, 120) < wb(4, 25, 1000)
    for n_cal, S, n_a in ((1, 1, 2), (4, 7, 120), (2, 25, 1000), (24, 7, 10000)):
        assert wb(n_cal, S, n_a) >= 16 * n_cal * S * n_a + 64 * n_cal        # two G buffers + the slots
        assert wb(n_cal, S, n_a) <= 16 * n_cal * S * n_a + 64 * n_cal + 512  # and nothing else
    assert wb(4, 7, 1) == -1 and wb(4, 0, 120) == -1 and wb(4, 65, 120) == -1 and wb(0, 7, 120) == -1
    assert wb(4, 64, 120) > 0


def test_null_handle_is_refused(lib):
    assert lib.aiy_value_backward(None, 4, 7, 120, 5, *([None] * 14)) == -1
    assert lib.aiy_value_stationary(None, 4, 7, 120, *([None] * 10), 1e-10, 100, 0, *([None] * 5)) == -1
    assert lib.aiy_value_reduce(None, 4, 7, 120, None, None, None, None) == -1
    assert lib.aiy_consumption_equivalent(None, 4, 840, None, None, None, None, None, None) == -1
    assert lib.aiy_version() == 210


def test_header_exports_and_ctypes_agree(lib):
    from aiyagari_hark_amd import _lib
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(aiy_\w+)\s*\(", src, re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (aiy_\w+)", out))
    for name, n_args in NAMES.items():
        assert name in declared and name in exported and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert len(_lib.SIGNATURES[name][1]) == n_args
        decl = re.search(r"^int\d+_t " + name + r"\s*\(([^;]*)\)\s*;", src, re.M).group(1)
        assert len(decl.split(",")) == n_args
    assert _lib.SIGNATURES["aiy_value_work_bytes"][0] is ctypes.c_int64
    # the two blocking calls hand their results to host arrays
    assert _lib.SIGNATURES["aiy_value_reduce"][1][6] is _lib.c_double_p
    assert _lib.SIGNATURES["aiy_value_stationary"][1][19:21] == [_lib.c_int32_p, _lib.c_double_p]
    assert "welfare.hip" in __import__("aiyagari_hark_amd.build", fromlist=["SOURCES"]).SOURCES


def test_package_exports_welfare():
    import dataclasses
    import inspect
    import types

    import aiyagari_hark_amd as pkg
    for name in ("stationary_value", "path_value", "consumption_equivalent", "WelfareResult"):
        assert callable(getattr(pkg, name))
    assert isinstance(pkg.welfare, types.ModuleType) and callable(pkg.welfare.welfare)
    assert [f.name for f in dataclasses.fields(pkg.WelfareResult)] == [
        "V", "V_base", "ce", "W", "W_base", "W_by_state", "W_base_by_state", "ce_aggregate", "ce_by_state"]
    from aiyagari_hark_amd.transition import TransitionResult, solve_transition
    assert {f.name: f.default for f in dataclasses.fields(TransitionResult)}["welfare"] is None
    assert inspect.signature(solve_transition).parameters["welfare"].default is False
    sig = inspect.signature(pkg.stationary_value).parameters
    assert sig["r"].default is None and sig["tol"].default == 1e-10 and sig["max_iter"].default == 5000
    assert inspect.signature(pkg.path_value).parameters["keep_path"].default is False
