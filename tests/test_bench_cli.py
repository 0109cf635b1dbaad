"""bench.py's command line off the GPU: what a plain run refuses, and the --dump-outputs files."""
import importlib.util
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_cli_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("argv, message", [
    (["--legs", "table2,configs3"], "needs --full"),
    (["--full", "--legs", "configs9"], "unknown leg"),
    (["--steps", "0"], "--steps must be at least 1"),
])
def test_refused_arguments(argv, message):
    """Secondary legs without --full, unknown legs and zero timed steps end with a usage
    error before anything touches the GPU."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True,
                         timeout=60, cwd=ROOT)
    assert out.returncode == 2
    assert message in out.stderr
    assert out.stdout == ""


def test_dump_outputs_writes_every_field_in_cell_order(tmp_path):
    """One float64 array per StationaryResult field, in Table II cell order whichever cells
    the rank solved."""
    bench = _bench()
    mine = [5, 1, 3, 0, 4, 2]
    vals = {f: np.arange(6.0) * (k + 1) for k, f in enumerate(bench.DUMP_FIELDS)}
    vals["status"] = np.array([0, 1, 2, 4, 0, 0], dtype=np.int32)
    res = types.SimpleNamespace(**vals)
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), res, mine, 6, 1, 0)
    assert sorted(os.listdir(out)) == sorted(f + ".npy" for f in bench.DUMP_FIELDS)
    for f in bench.DUMP_FIELDS:
        a = np.load(out / (f + ".npy"))
        assert a.dtype == np.float64 and a.shape == (6,)
        assert np.array_equal(a[mine], np.asarray(vals[f], dtype=np.float64))
