"""CPU tests of the histogram-statistics entry points of the C ABI: the host-only work-space
size, argument validation before any device work, and header / exports / ctypes agreement."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aiyagari.h")
NAMES = {"aiy_transition_forward_marginals": 18, "aiy_dist_stats_work_bytes": 2, "aiy_dist_marginal": 7,
         "aiy_dist_stats": 13}


@pytest.fixture(scope="module")
def lib():
    from aiyagari_hark_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_work_bytes_host_only(lib):
    wb = lib.aiy_dist_stats_work_bytes
    assert 0 < wb(1, 2) < wb(2, 2) < wb(2, 120) < wb(5, 120) < wb(5, 1000)
    for n_dist, n_a in ((1, 2), (24, 120), (7224, 10000), (1677, 10000)):
        assert wb(n_dist, n_a) >= 16 * n_dist * n_a
    # the cw / cd space dominates: the results of 256 percentiles add 4 KB per distribution
    assert wb(7224, 10000) < 16 * 7224 * 10000 + 7224 * 4200 + 4096
    assert wb(0, 120) == -1 and wb(3, 1) == -1 and wb(-1, 120) == -1


def test_null_handle_is_refused(lib):
    assert lib.aiy_transition_forward_marginals(None, 3, 7, 120, 5, None, None, None, None, None, None, None, None,
                                                None, None, None, None, None) == -1
    assert lib.aiy_dist_marginal(None, 3, 7, 120, None, None, None) == -1
    assert lib.aiy_dist_stats(None, 3, 1, 120, None, None, None, 0, None, None, None, None, None) == -1
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
        # the header's parameter list has as many entries
        decl = re.search(name + r"\s*\(([^;]*)\)\s*;", src).group(1)
        assert len(decl.split(",")) == n_args
    assert _lib.SIGNATURES["aiy_dist_stats_work_bytes"][0] is ctypes.c_int64
    # the marginals entry is aiy_transition_forward's arguments with marg_out before the stream
    fwd = _lib.SIGNATURES["aiy_transition_forward"][1]
    assert _lib.SIGNATURES["aiy_transition_forward_marginals"][1] == fwd[:-1] + [_lib.vp] + fwd[-1:]


def test_package_exports_wealth_statistics():
    import dataclasses

    import aiyagari_hark_amd as pkg
    for name in ("histogram_stats", "batch_wealth_stats", "path_wealth_stats", "WealthStats"):
        assert callable(getattr(pkg, name))
    assert [f.name for f in dataclasses.fields(pkg.WealthStats)] == [
        "lorenz", "percentile_values", "gini", "mean", "total", "bottom_share", "percentiles"]
    from aiyagari_hark_amd.transition import BlockResult, TransitionResult
    assert {f.name: f.default for f in dataclasses.fields(BlockResult)}["marg"] is None
    assert {f.name: f.default for f in dataclasses.fields(TransitionResult)}["stats"] is None
