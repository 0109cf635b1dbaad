"""CPU tests of the sequence-space Jacobian entry points of the C ABI: the host-only work-space
size, argument validation before any device work, and header / exports / ctypes agreement."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aiyagari.h")
NAMES = ("aiy_jacobian_work_bytes", "aiy_jacobian_fanout", "aiy_jacobian_diff", "aiy_jacobian_expectation",
         "aiy_jacobian_contract")


@pytest.fixture(scope="module")
def lib():
    from aiyagari_hark_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_work_bytes_host_only(lib):
    small = lib.aiy_jacobian_work_bytes(3, 7, 120, 5)
    longer = lib.aiy_jacobian_work_bytes(3, 7, 120, 40)
    assert 0 < small < longer
    assert lib.aiy_jacobian_work_bytes(3, 7, 120, 1) < small
    # the inverse index of T + 1 periods, two mixed vectors and one chunk of partials at least
    assert small >= 6 * 3 * 7 * 121 * 4 + 2 * 3 * 7 * 120 * 8 + 3 * 5 * 12 * 8
    # Table II size with T = 300: the inverse index passes 2^31 bytes; 18 chunks of 4096 (7 x 10 000 / 4096)
    big = lib.aiy_jacobian_work_bytes(24, 7, 10000, 300)
    assert big > 24 * 301 * 7 * 10001 * 4 + 24 * 18 * 300 * 602 * 8
    assert big < 24 * 301 * 7 * 10001 * 4 + 24 * 19 * 300 * 602 * 8 + 2 * 24 * 7 * 10000 * 8 + 4096
    for bad in ((3, 7, 120, 0), (3, 7, 1, 5), (3, 65, 120, 5), (3, 0, 120, 5), (0, 7, 120, 5)):
        assert lib.aiy_jacobian_work_bytes(*bad) == -1
    assert lib.aiy_jacobian_work_bytes(3, 64, 120, 5) > 0


def test_null_handle_is_refused(lib):
    assert lib.aiy_jacobian_fanout(None, 3, 7, 120, 5, 6, None, None, None, None, None, None, None) == -1
    assert lib.aiy_jacobian_diff(None, 10, None, None, 1e-5, None) == -1
    assert lib.aiy_jacobian_expectation(None, 3, 7, 120, 5, None, None, None, None, None, None, None) == -1
    assert lib.aiy_jacobian_contract(None, 3, 7, 120, 5, None, None, None, None, None, None) == -1
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
        # the header's parameter count is the binding's
        decl = re.search(name + r"\s*\(([^;]*)\);", src).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1])
    assert _lib.SIGNATURES["aiy_jacobian_work_bytes"][0] is ctypes.c_int64
    assert _lib.SIGNATURES["aiy_jacobian_diff"][1][1] is ctypes.c_int64
    assert _lib.SIGNATURES["aiy_jacobian_diff"][1][4] is ctypes.c_double
    # every symbol the binding names is exported, the new ones included
    assert set(_lib.SIGNATURES) <= exported


def test_package_exports_jacobian_api():
    import aiyagari_hark_amd as pkg
    for name in ("household_jacobian", "HouseholdJacobian", "impulse_response", "solve_transition"):
        assert callable(getattr(pkg, name))


def test_jacobian_from_fake_news_and_capital_map():
    """The host side of the Jacobian: the diagonal accumulation and H against their definitions."""
    import numpy as np

    from aiyagari_hark_amd.transition import HouseholdJacobian, jacobian_from_fake_news
    rng = np.random.default_rng(5)
    T = 6
    F = rng.normal(size=(2, T, T + 1))
    J = jacobian_from_fake_news(F)
    for t in range(T):
        for u in range(T + 1):
            ref = sum(F[:, t - k, u - k] for k in range(min(t, u) + 1))
            assert np.allclose(J[:, t, u], ref, rtol=1e-15, atol=1e-15)
    alpha, K = np.array([0.36, 0.3]), np.array([5.0, 7.0])
    jac = HouseholdJacobian(JR=J, Jw=2.0 * J, FR=F, Fw=2.0 * F, h=1e-5, K=K, alpha=alpha)
    H = jac.capital_map()
    assert H.shape == (2, T, T)
    for c in range(2):
        dR = alpha[c] * (alpha[c] - 1.0) * K[c] ** (alpha[c] - 2.0)
        dw = alpha[c] * (1.0 - alpha[c]) * K[c] ** (alpha[c] - 1.0)
        assert np.allclose(H[c], J[c][:, 1:] * dR + 2.0 * J[c][:, 1:] * dw - np.eye(T), rtol=1e-14, atol=0)
    b = rng.normal(size=T)
    assert np.allclose(H[1] @ jac.solver()(1, b), b, rtol=0, atol=1e-12)
