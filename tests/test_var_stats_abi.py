"""CPU tests of the household-variable entry points of the C ABI (csrc/var_stats.hip and the
masses entry of csrc/transition.hip): the host-only work-space size, argument validation before
any device work, header / exports / ctypes agreement and the package's names."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aiyagari.h")
NAMES = {"aiy_transition_forward_masses": 18, "aiy_var_work_bytes": 3, "aiy_household_variables": 15,
         "aiy_var_merge": 11, "aiy_var_moments": 10}


@pytest.fixture(scope="module")
def lib():
    from aiyagari_hark_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_work_bytes_host_only(lib):
    wb = lib.aiy_var_work_bytes
    assert 0 < wb(1, 1, 2) < wb(2, 1, 2) < wb(24, 7, 120) < wb(7224, 7, 10000)
    # monotone (not necessarily strictly) in S and n_a
    assert wb(5, 1, 120) <= wb(5, 7, 120) <= wb(5, 64, 120) and wb(5, 7, 2) <= wb(5, 7, 120) <= wb(5, 7, 10000)
    # the moments of 8 variables: 73 doubles per distribution, and the flag
    assert wb(7224, 7, 10000) >= 7224 * 73 * 8 + 4
    for bad in ((0, 7, 120), (-1, 7, 120), (3, 0, 120), (3, 65, 120), (3, 7, 1), (3, 64, 2 ** 26)):
        assert wb(*bad) == -1, bad


def test_null_handle_and_bad_arguments_are_refused(lib):
    assert lib.aiy_transition_forward_masses(None, 3, 7, 120, 5, None, None, None, None, None, None, None, None, None,
                                             None, None, None, None) == -1
    assert lib.aiy_household_variables(None, 3, 7, 120, 1, None, None, None, None, 1, None, None, 1, None, None) == -1
    assert lib.aiy_var_merge(None, 3, 7, 120, None, None, None, None, None, None, None) == -1
    assert lib.aiy_var_moments(None, 3, 7, 120, 1, None, None, None, None, None) == -1
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
    assert _lib.SIGNATURES["aiy_var_work_bytes"][0] is ctypes.c_int64
    assert "var_stats.hip" in __import__("aiyagari_hark_amd.build", fromlist=["SOURCES"]).SOURCES
    # the masses entry is aiy_transition_forward's arguments with mass_path_out before the stream
    fwd = _lib.SIGNATURES["aiy_transition_forward"][1]
    assert _lib.SIGNATURES["aiy_transition_forward_masses"][1] == fwd[:-1] + [_lib.vp] + fwd[-1:]
    # the variables' bits in the header are the binding's
    for name, bit in _lib.AIY_VARIABLES.items():
        assert re.search(rf"#define AIY_VAR_{name.upper()} {bit}\b", src), name
    assert re.search(rf"#define AIY_VAR_MAX_MOMENTS {_lib.AIY_VAR_MAX_MOMENTS}\b", src)


def test_package_exports_variable_statistics():
    import dataclasses

    import aiyagari_hark_amd as pkg
    for name in ("variable_stats", "household_variables", "batch_inequality", "path_variable_stats", "VariableStats",
                 "Inequality"):
        assert callable(getattr(pkg, name))
    wealth = [f.name for f in dataclasses.fields(pkg.WealthStats)]
    assert [f.name for f in dataclasses.fields(pkg.VariableStats)] == wealth + ["std", "cv"]
    assert [f.name for f in dataclasses.fields(pkg.Inequality)] == ["stats", "moments", "corr", "variables"]
    from aiyagari_hark_amd.stats import VARIABLES
    assert VARIABLES == ("consumption", "income", "earnings", "cash", "saving", "wealth")
    from aiyagari_hark_amd.transition import BlockResult, TransitionResult
    assert {f.name: f.default for f in dataclasses.fields(BlockResult)}["masses"] is None
    defaults = {f.name: f.default for f in dataclasses.fields(TransitionResult)}
    assert defaults["var_stats"] is None and defaults["var_moments"] is None
