"""The training path of the LLaMA decoder launches what it launched when tests/golden/decoder_traces.json was recorded: for every frozen
base (bf16, e4m3, LLM.int8, 4-bit nf4) x adapter setting (fp8_base_cases.SETTINGS) x {every row, compact last layer}, and the operator path
of the bf16 base (LHRS_NATIVE_LAYER=0), one decode + backward of the one-layer model of fp8_base_cases.MODEL on the batch of
decoder_trace_cases.batch runs under a recorder over every public function of lhrs_bot_amd/kernels.py; the log (name, dtype and shape of
every tensor argument, the optional arguments given) must equal the recorded one line for line.  Every entry point takes the widths of
MODEL (dim 512, ff 512, 4 heads), so all four bases run at the same size.

The golden file comes from tools/record_decoder_traces.py, run before the change it guards; what the calls compute is held per element by
test_fp8_base_paths_gpu.py, test_lora_gpu.py, test_int8_gpu.py and test_nf4_gpu.py."""
import json
import os

import pytest

import decoder_trace_cases as dc

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_traces.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def models():
    return dc.model_cache()


def test_the_golden_file_holds_exactly_the_cells():
    assert sorted(GOLDEN["cells"]) == sorted(map(dc.cell_id, dc.CELLS)) and len(dc.CELLS) == 26


@pytest.mark.parametrize("cell", dc.CELLS, ids=dc.cell_id)
def test_decode_and_backward_make_the_recorded_calls(cell, models):
    log, out = dc.run_cell(cell, models)
    want = [GOLDEN["calls"][i] for i in GOLDEN["cells"][dc.cell_id(cell)]]
    for i, (got, exp) in enumerate(zip(log, want)):
        assert got == exp, f"call {i}: {got}  -  recorded: {exp}  (after {log[max(0, i - 3):i]})"
    assert len(log) == len(want), f"{len(log)} calls, {len(want)} recorded; first surplus: {(log + want)[min(len(log), len(want))]}"
    assert bool(out["loss"].isfinite())
