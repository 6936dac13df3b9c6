"""What single-token decoding launches, per weight format, batch, cache format, context length, adapter store and head size, and what every
rejected call raises before anything is launched: recorded on the CPU (tests/decode_plan_cases.py) and compared with
tests/golden/decode_plan.json.  The names are compared first, so a difference reads as a list of wrappers; the digest then pins every scalar
argument and every tensor operand (which buffer, offset, shape, strides, dtype) of every call."""
import json
import os

import pytest

import decode_plan_cases as dp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_plan.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_exactly_the_cases_of_the_table(golden):
    assert list(golden) == list(dp.CASES)


def test_the_table_covers_every_format_boundary_and_rejection(golden):
    names = set(golden)
    for w in dp.WEIGHTS:
        for B in (1, 2, 3, 4, 16):       # <= 2 fused, >= 2 re-tiled bf16, > 2 quantising producers, >= 4 staged activations
            for kv in ("bf16", "fp8"):
                for ctx in (32, 256):    # nsplit 1 and 2
                    assert f"session/{w}/B{B}/kv-{kv}/ctx{ctx}" in names
    assert sum("error" in v for k, v in golden.items() if k.startswith("reject/")) == sum(k.startswith("reject/") for k in golden) >= 9
    assert all("error" not in v for k, v in golden.items() if k.startswith("session/"))


def test_the_table_holds_a_whole_generate_call_for_every_arm(golden):
    whole = {k: v for k, v in golden.items() if k.startswith("generate/")}
    assert whole and all("error" not in v for v in whole.values())
    for arm in dp.ARMS:
        assert any(k.startswith(f"generate/{arm}/") for k in whole), arm
    for arm in ("greedy", "sampler-device", "constraint"):   # the session at batch 1 and 2, the GEMM step at batch 17
        assert {f"generate/{arm}/B{B}" for B in (1, 2, 17)} <= set(whole)
    assert all("HipGraph.launch" in whole[f"generate/greedy/B{B}"]["calls"] for B in (1, 2)) and "HipGraph.launch" not in whole["generate/greedy/B17"]["calls"]
    rejected = {k[len("reject/generate/"):] for k in golden if k.startswith("reject/generate/")}
    assert golden["generate/adapters-merged/B2/stray-live-lora"] == golden["generate/adapters-merged/B2"]
    assert {"adapters", "adapters-none", "adapters-none/unmerged-adapters", "constraint", "prefix-cache-batch", "kv-cache", "int8-without-base", "sampler", "sampler/unmerged-adapters", "beam-count", "beam-sample",
            "beam-streamer", "beam-criteria", "beam-sequences", "beam-early", "beam-rows", "4bit-merged", "int8-merged"} <= rejected
    # a rejected call has made no wrapper call - but for `weights` outside the table, which the session itself rejects, behind the prefill
    assert all(golden["reject/generate/" + k]["error"][2] == 0 for k in rejected - {"unknown-weights"})


def test_every_public_wrapper_is_a_recorder():
    import lhrs_bot_amd.kernels as hk
    real = {n: getattr(hk, n) for n in dp.PUBLIC}
    rec = dp.Recorder()
    with rec.installed():
        assert all(getattr(hk, n) is not real[n] for n in dp.PUBLIC)
        assert {n: getattr(hk, n) for n in dp.REAL} == dp.REAL_FNS
        hk.rope_kv_append(None, None, None, None, None, None, 1, 2, 64, 32)
    assert [n for n, _ in rec.calls] == ["rope_kv_append"]
    assert all(getattr(hk, n) is real[n] for n in dp.PUBLIC)    # and the real wrappers are back afterwards
    assert {"gemv_fused", "gemv4", "gemv_mx4", "gemv_int8", "gemv_fp8_mfma", "lora_down", "lora_up", "decode_attn_kv8", "copy_2d"} <= set(dp.PUBLIC)


@pytest.mark.parametrize("name", list(dp.CASES))
def test_launch_plan(name, golden):
    got, want = dp.run(dp.CASES[name]), golden[name]
    assert got.get("error") == want.get("error")
    assert got.get("calls") == want.get("calls")
    assert got.get("sha256") == want.get("sha256")


def test_the_digest_sees_an_operand_and_a_scalar():
    """the canonical trace tells two buffers of one shape apart, and two values of a scalar"""
    import torch
    import lhrs_bot_amd.kernels as hk

    def plan(swap, eps):
        def fn(rec):
            m = dp.model()
            rec.reset()
            a, b = torch.empty((2, 256), dtype=torch.bfloat16), torch.empty((2, 256), dtype=torch.bfloat16)
            hk.rmsnorm_fwd(a, m.p["norm_w"], eps, out=b)
            hk.rmsnorm_fwd(*((b, m.p["norm_w"], eps) if swap else (a, m.p["norm_w"], eps)), out=a[:1])
            return m
        return dp.run(fn)["sha256"]
    assert plan(False, 1e-5) == plan(False, 1e-5)
    assert len({plan(False, 1e-5), plan(True, 1e-5), plan(False, 1e-6)}) == 3
