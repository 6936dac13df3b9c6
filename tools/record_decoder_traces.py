"""Record the kernel-call traces that tests/test_decoder_trace_gpu.py compares against: for every cell of
tests/decoder_trace_cases.py::CELLS, the calls into lhrs_bot_amd/kernels.py of one decode + backward of the one-layer model.

    python tools/record_decoder_traces.py [--out tests/golden/decoder_traces.json]

Run it on a GPU on the commit whose launch sequence is the reference - BEFORE a change to the training path, never after it: the file pins
a refactor to what the code did, and regenerating it from the changed code compares that code with itself.

The file holds every distinct log line once ("calls") and per cell the indices of its lines in order ("cells")."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import decoder_trace_cases as dc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "decoder_traces.json"))
    a = ap.parse_args()
    models, index, cells = dc.model_cache(), {}, {}
    for cell in dc.CELLS:
        log, _ = dc.run_cell(cell, models)
        cells[dc.cell_id(cell)] = [index.setdefault(line, len(index)) for line in log]
        print(f"{dc.cell_id(cell)}: {len(log)} calls")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"calls": list(index), "cells": cells}, f, indent=0)
        f.write("\n")
    print(f"{len(cells)} cells, {len(index)} distinct calls -> {a.out}")


if __name__ == "__main__":
    main()
