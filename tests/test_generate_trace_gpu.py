"""Whole `generate()` calls return what they returned when tests/golden/generate_traces.json was recorded: for every case of
tests/generate_trace_cases.py - greedy, EOS, both samplers, the penalty, returned logits, left padding, the e4m3 cache, fp8 and int8 weights,
merged and live adapters, a constraint, a prefix cache over two calls, streamer and stopping criteria, beams; batch 1 and 2 on the session,
batch 17 on the GEMM step - the token ids must equal the recorded lists and every other returned tensor (logits, beam scores, choice
scores) must have the recorded SHA-256.  No tolerance: the file pins host-side changes of the decode path, which hand the kernels the same
operands in the same order.

The golden file comes from tools/record_generate_traces.py, run before the change it guards (two recordings of that commit agreed in every
case, the host multinomial included)."""
import json
import os

import pytest

import generate_trace_cases as gc

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate_traces.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def models():
    return gc.model_cache()


def test_the_golden_file_holds_exactly_the_cases():
    assert sorted(GOLDEN) == sorted(gc.CASES)


@pytest.mark.parametrize("name", list(gc.CASES))
def test_generate_returns_the_recorded_values(name, models):
    got, want = gc.run_case(name, models), GOLDEN[name]
    assert len(got) == len(want)
    for call, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"call {call}: {g}  -  recorded: {w}"
