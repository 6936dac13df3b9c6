"""Record what tests/test_generate_trace_gpu.py compares against: for every case of tests/generate_trace_cases.py::CASES, the values its
`generate()` calls return on the tiny decoder - token ids as lists, every other tensor (logits, beam scores, choice scores) as the SHA-256
of its bytes.

    python tools/record_generate_traces.py [--out tests/golden/generate_traces.json] [--only PREFIX]

Run it on a GPU on the commit whose results are the reference - BEFORE a change to the decode path, never after it: the file pins a
refactor to what the code computed, and regenerating it from the changed code compares that code with itself."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import generate_trace_cases as gc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "generate_traces.json"))
    ap.add_argument("--only", default="", help="record the cases whose name starts with this")
    a = ap.parse_args()
    models, cases = gc.model_cache(), {}
    for name in gc.CASES:
        if name.startswith(a.only):
            cases[name] = gc.run_case(name, models)
            print(f"{name}: {len(cases[name])} calls, first ids {cases[name][0][0]}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(cases, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases -> {a.out}")


if __name__ == "__main__":
    main()
