"""CPU tests of the transition-path entry points of the C ABI: the host-only work-space
size, argument validation before any device work, and header / exports / ctypes agreement."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aiyagari.h")
NAMES = ("aiy_transition_work_bytes", "aiy_transition_backward", "aiy_transition_forward")


@pytest.fixture(scope="module")
def lib():
    from aiyagari_hark_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_work_bytes_host_only(lib):
    small = lib.aiy_transition_work_bytes(3, 7, 120, 5)
    longer = lib.aiy_transition_work_bytes(3, 7, 120, 40)
    assert 0 < small < longer
    assert lib.aiy_transition_work_bytes(3, 7, 120, 1) < small
    # Table II size: the per-period inverse index alone passes 2^31 bytes' worth of entries
    assert lib.aiy_transition_work_bytes(24, 7, 10000, 300) > 24 * 300 * 7 * 10001 * 4
    assert lib.aiy_transition_work_bytes(3, 7, 120, 0) == -1
    assert lib.aiy_transition_work_bytes(3, 7, 1, 5) == -1
    assert lib.aiy_transition_work_bytes(3, 65, 120, 5) == -1
    assert lib.aiy_transition_work_bytes(3, 0, 120, 5) == -1
    assert lib.aiy_transition_work_bytes(0, 7, 120, 5) == -1
    assert lib.aiy_transition_work_bytes(3, 64, 120, 5) > 0


def test_null_handle_is_refused(lib):
    from aiyagari_hark_amd import _lib
    model = _lib.TransitionModel(3, 7, 120, 5)
    assert lib.aiy_transition_backward(None, ctypes.byref(model), None, None, None, None, None, None) == -1
    assert lib.aiy_transition_forward(None, 3, 7, 120, 5, None, None, None, None, None, None, None, None, None,
                                      None, None, None) == -1
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
    assert _lib.SIGNATURES["aiy_transition_work_bytes"][0] is ctypes.c_int64
    assert len(_lib.SIGNATURES["aiy_transition_backward"][1]) == 8
    assert len(_lib.SIGNATURES["aiy_transition_forward"][1]) == 17
    # aiy_transition_model: 4 int32, then 9 pointers
    assert ctypes.sizeof(_lib.TransitionModel) == 16 + 9 * 8
    fields = re.search(r"typedef struct \{([^}]*)\} aiy_transition_model;", src).group(1)
    names = re.findall(r"(\w+)\s*[;,]", fields)
    assert names == [n for n, _ in _lib.TransitionModel._fields_]


def test_package_exports_transition_api():
    import aiyagari_hark_amd as pkg
    for name in ("steady_state", "household_block", "solve_transition", "TransitionResult"):
        assert callable(getattr(pkg, name))


def test_path_prices_match_steady_state_firm():
    """On Z = 1 the path prices are stationary.firm_prices read backwards."""
    import numpy as np

    from aiyagari_hark_amd.stationary import firm_prices
    from aiyagari_hark_amd.transition import path_prices
    r0 = np.array([0.02, 0.035])
    w0, K0 = firm_prices(r0, 0.36, 0.08)
    r, w = path_prices(np.repeat(K0[:, None], 4, axis=1), np.ones(4), np.full(2, 0.36), np.full(2, 0.08))
    assert np.allclose(r, r0[:, None], rtol=0, atol=1e-14) and np.allclose(w, w0[:, None], rtol=1e-14, atol=0)
