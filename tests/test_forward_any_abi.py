"""CPU tests of the C ABI of the forward sweep for lotteries whose rows need not be monotone
(DESIGN.md §4r): header / exports / ctypes agreement, the host-only work-space size and the
argument checks that need no device."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aiyagari.h")
NAMES = ("aiy_transition_any_work_bytes", "aiy_transition_forward_any")


@pytest.fixture(scope="module")
def lib():
    from aiyagari_hark_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_header_exports_and_ctypes_agree(lib):
    from aiyagari_hark_amd import _lib
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(aiy_\w+)\s*\(", src, re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (aiy_\w+)", out))
    for name in NAMES:
        assert name in declared and name in exported and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.SIGNATURES["aiy_transition_any_work_bytes"][0] is ctypes.c_int64
    # the arguments of aiy_transition_forward_marginals, then rows_turned_out before the stream
    marg = _lib.SIGNATURES["aiy_transition_forward_marginals"][1]
    any_ = _lib.SIGNATURES["aiy_transition_forward_any"][1]
    assert len(any_) == len(marg) + 1 == 19
    assert any_[:-2] == marg[:-1] and any_[-2] is _lib.c_int32_p and any_[-1] is marg[-1]
    decl = re.search(r"int32_t aiy_transition_forward_any\(([^)]*)\)", src).group(1)
    assert len(decl.split(",")) == 19 and "rows_turned_out" in decl and "marg_out" in decl


def test_work_bytes_host_only(lib):
    for sizes in ((3, 7, 120, 5), (1, 1, 2, 1), (2, 25, 1000, 5), (24, 7, 10000, 300), (3, 64, 120, 5)):
        base = lib.aiy_transition_work_bytes(*sizes)
        more = lib.aiy_transition_any_work_bytes(*sizes)
        n_cal, S, n_a, T = sizes
        # the second index array ([T][n_cal][S][n_a + 1] int32) and the counters
        assert 0 < base < more
        assert more - base >= 4 * T * n_cal * S * (n_a + 1) + 8
        assert more - base <= 4 * T * n_cal * S * (n_a + 1) + 2 * 256
        assert more % 256 == 0
    for bad in ((3, 7, 120, 0), (3, 7, 1, 5), (3, 65, 120, 5), (3, 0, 120, 5), (0, 7, 120, 5), (3, 7, 120, -1)):
        assert lib.aiy_transition_any_work_bytes(*bad) == -1
        assert lib.aiy_transition_work_bytes(*bad) == -1


def test_null_handle_is_refused_and_version_stays(lib):
    assert lib.aiy_transition_forward_any(None, 3, 7, 120, 5, None, None, None, None, None, None, None, None, None,
                                          None, None, None, None, None) == -1
    assert lib.aiy_version() == 210


def test_rows_argument_is_checked_before_anything_else():
    """An unknown ``rows`` raises ValueError from both wrappers before they touch a device, and
    both default to "monotone"."""
    from aiyagari_hark_amd import aggregate, transition
    assert inspect.signature(transition.transition_forward).parameters["rows"].default == "monotone"
    assert inspect.signature(aggregate.simulate).parameters["rows"].default == "monotone"
    with pytest.raises(ValueError, match="rows"):
        transition.transition_forward(None, None, None, None, 5, None, rows="sorted")
    with pytest.raises(ValueError, match="rows"):
        aggregate.simulate(None, None, None, [0.0], rows="sorted")
    assert "rows_turned" in aggregate.AggregateSimulation.__dataclass_fields__
    assert aggregate.AggregateSimulation.__dataclass_fields__["rows_turned"].default is None
