"""Handle options (aiy_set_option / aiy_get_option): every default, every range end, the values
just outside, the flags' normalisation and the unknown ids, on a fresh handle.  Written from the
documented table of options (name, id, default, range), not from the library's code."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

# name: (id, default)
FLAGS = {"USE_GRAPHS": (1, 1), "RESIDENT": (2, 1), "HIST_FUSED": (4, 0), "RESIDENT_STREAM": (5, 0),
         "HIST_RESIDENT": (6, 1), "HIST_KRYLOV": (9, 0), "GE_RESIDENT": (10, 0), "HIST_PULL": (15, 0),
         "HIST_IID": (24, 1)}
# name: (id, low, high, default)
RANGES = {"RESIDENT_SHAPE": (3, 0, 2, 0), "HIST_CLUSTER": (7, 0, 128, 0), "HIST_ACCEL": (8, 0, 1 << 20, 0),
          "CU_LIMIT": (11, 0, 65536, 0), "GE_REBALANCE": (12, 0, 100, 55), "GE_EXTRAP_PERIOD": (13, 4, 1024, 32),
          "GE_LOGSEC": (14, 0, 2, 2), "GE_LOOSE_HIST": (17, 6, 14, 8), "RESIDENT_SHAPE_STREAM": (18, -1, 2, 1),
          "GE_ANDERSON": (23, 5, 1024, 12)}   # GE_ANDERSON: 0 (off) or [5, 1024]
UNKNOWN = (0, 16, 19, 20, 21, 22, 25, -1, 1000)
AIY_ERR_ARG = -1


@pytest.fixture()
def fresh(gpu):
    from aiyagari_hark_amd import _lib
    h = _lib.Handle(0)
    try:
        yield h
    finally:
        h.close()


def put(h, opt, value):
    return h.lib.aiy_set_option(h.h, opt, value)


def defaults_hold(h):
    for name, (opt, d) in FLAGS.items():
        assert h.get_option(opt) == d, name
    for name, (opt, _, _, d) in RANGES.items():
        assert h.get_option(opt) == d, name


def test_ids_match_the_python_constants():
    from aiyagari_hark_amd import _lib
    table = {"AIY_OPT_" + k: v[0] for k, v in {**FLAGS, **RANGES}.items()}
    assert table == {k: getattr(_lib, k) for k in dir(_lib) if k.startswith("AIY_OPT_")}
    assert _lib.ERRORS[AIY_ERR_ARG] == "AIY_ERR_ARG"


def test_defaults(fresh):
    defaults_hold(fresh)


def test_flags_normalise(fresh):
    for name, (opt, _) in FLAGS.items():
        for v, want in ((0, 0), (1, 1), (7, 1), (-3, 1), (1 << 40, 1), (0, 0)):
            assert put(fresh, opt, v) == 0, (name, v)
            assert fresh.get_option(opt) == want, (name, v)


def test_range_ends_and_beyond(fresh):
    for name, (opt, lo, hi, _) in RANGES.items():
        for v in (lo, hi):
            assert put(fresh, opt, v) == 0, (name, v)
            assert fresh.get_option(opt) == v, (name, v)
        outside = [lo - 1, hi + 1, -(1 << 40), 1 << 40]
        if name == "GE_ANDERSON":
            outside = [-1, 1, 4, hi + 1, -(1 << 40), 1 << 40]
        for keep in (hi, lo):
            assert put(fresh, opt, keep) == 0
            for v in outside:
                assert put(fresh, opt, v) == AIY_ERR_ARG, (name, v)
                assert name in fresh.lib.aiy_last_error(fresh.h).decode(), name
                assert fresh.get_option(opt) == keep, (name, v)
    opt = RANGES["GE_ANDERSON"][0]
    assert put(fresh, opt, 0) == 0 and fresh.get_option(opt) == 0


def test_unknown_ids(fresh):
    v = ctypes.c_int64(-77)
    for opt in UNKNOWN:
        assert put(fresh, opt, 1) == AIY_ERR_ARG, opt
        assert fresh.lib.aiy_get_option(fresh.h, opt, ctypes.byref(v)) == AIY_ERR_ARG, opt
        assert v.value == -77
    defaults_hold(fresh)   # nothing was disturbed
