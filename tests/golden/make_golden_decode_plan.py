"""tests/golden/decode_plan.json: per case of tests/decode_plan_cases.py the names of the kernel wrappers that single-token decoding calls, in
order, and the SHA-256 of the canonical trace (names, scalar arguments, tensor labels); for a rejected case the exception's type, its
message and the number of wrapper calls made before it.  No GPU - the wrappers are recorders - but the built liblhrs_hip.so: the slice
count of `lora_down` is asked from it.

The file pins the host side of decoding across refactors: it is written from the commit BEFORE such a change and must come out byte for
byte the same after it.  Regenerate it only with a change that is meant to alter what is launched.  (The `generate/` entries were recorded
before the token loops became one; four `reject/generate/` counts - `sampler/unmerged-adapters`, `beam-rows`, `beam-width`,
`beam-rows/unmerged-adapters` - were 4, 1, 1 and 5 then and are 0 since those checks moved in front of every launch.)

    python tests/golden/make_golden_decode_plan.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import decode_plan_cases as dp  # noqa: E402


def main():
    out = dp.record_all()
    with open(os.path.join(HERE, "decode_plan.json"), "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in out.items()) + "\n}\n")
    n_err = sum("error" in v for v in out.values())
    print(f"{len(out)} cases ({n_err} rejections), {sum(len(v.get('calls', ())) for v in out.values())} calls")


if __name__ == "__main__":
    main()
