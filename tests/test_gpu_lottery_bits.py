"""The lottery-step kernels keep their bits: every output of tests/golden/make_lottery_bits.py's
cases (forward sweeps with and without C, fan-out, expectation steps, values on a path and at the
steady state, the row reduction and the wealth statistics) has the sha256 recorded in
tests/golden/lottery_step_bits.json.  No tolerance: the shared pull, mix, adjoint step and row
reduction must add in the order the recorded kernels added."""
import json
import os

import pytest

from tests.golden.make_lottery_bits import CASES, build_case, case_name, digests, run_case

pytestmark = pytest.mark.gpu

FIXTURE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lottery_step_bits.json")))


@pytest.mark.parametrize("S,n_a,variant", CASES)
def test_lottery_step_bits(gpu, S, n_a, variant):
    want = FIXTURE["cases"][case_name(S, n_a, variant)]
    got = digests(run_case(gpu, build_case(S, n_a, variant)))
    assert sorted(got) == sorted(want)
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, f"outputs whose bits differ from commit {FIXTURE['commit']} (HIP {FIXTURE['hip']}): {bad}"
