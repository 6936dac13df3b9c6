"""generate(weights="int8") on an MI355X: a 2-layer model on the LLM.int8 base (quantize_base(8, "int8")), built once per module.

The mode exists only on that base; graph replay equals eager launches for batch 1 and 3, beams, the e4m3 KV cache and live adapters; equal
prompts give equal logit rows; and the arithmetic is LLM.int8, not bf16: against row 0 of the same prompt at batch 17 - which takes the
multi-row hk.int8_linear step that tests/test_int8_paths_gpu.py checks per element - the batch-1 int8 step is closer than the bf16 and the
fp8 steps are (an ordering of one run's own yardsticks; the three gaps and the ratios are printed)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from lhrs_bot_amd import kernels as hk  # noqa: E402
from lhrs_bot_amd.engine import LHRSEngine  # noqa: E402
from lhrs_bot_amd.text import TextModal  # noqa: E402
from lhrs_bot_amd.unibind import UniBind  # noqa: E402
from oracle import params as OP  # noqa: E402

DEV = "cuda"
NL = 2
_M = {}
NAMES = ("qkv_w", "o_w", "gu_w", "down_w")


def _model():
    if "m" not in _M:
        m = UniBind(("rgb", "text"), None, device=DEV, llama_layers=NL).init_random(seed=1).eval()
        m.text.quantize_base(8, "int8")
        assert m.text.base_int8
        _M["m"] = m
    return _M["m"]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _inputs(B, seed=5, same=False):
    g = torch.Generator().manual_seed(seed)
    ids_ = torch.tensor([[1, -200, 9, 8, 7, 6]]).repeat(B, 1)
    if B > 1 and not same:
        ids_[1:, 2:] = torch.randint(3, 32000, (B - 1, 4), generator=g)
    rgb = torch.randn(1 if same else B, 3, 224, 224, generator=g)
    return ids_, rgb.repeat(B, 1, 1, 1) if same else rgb


KW = dict(do_sample=False, max_new_tokens=5, return_logits=True, eos_token_id=None, weights="int8")


def test_int8_needs_the_int8_base_and_unmerged_adapters_need_live():
    m = UniBind(("rgb", "text"), None, device=DEV, llama_layers=NL).init_random(seed=1).eval()
    ids_, rgb = _inputs(1)
    kw = dict(KW, max_new_tokens=3)
    with pytest.raises(ValueError, match="quantize_base"):
        m.generate(ids_, images=rgb, **kw)
    with pytest.raises(ValueError, match="quantize_base"):
        m.text.pack_int8_decode()
    m.text.quantize_base(8, "e4m3")
    with pytest.raises(ValueError, match="quantize_base"):
        m.generate(ids_, images=rgb, **kw)
    m.text.quantize_base(8, "int8")
    targets = ("q", "k", "v", "o", "gate", "up", "down")
    lora_p = OP.make_lora_params(seed=4, layers=NL, r=16, alpha=32, targets=targets)
    lora = m.enable_lora(r=16, alpha=32, targets=targets, seed=0)
    for l in range(NL):
        for pr in targets:
            lora.set_adapter(l, pr, *lora_p[l][pr])
    lora.refresh()
    with pytest.raises(ValueError, match="merge_lora"):
        m.generate(ids_, images=rgb, **kw)
    # adapters="live": graph replay equals eager launches, and the adapters move the logits
    a_ids, a_lg = m.generate(ids_, images=rgb, adapters="live", **kw)
    b_ids, b_lg = m.generate(ids_, images=rgb, adapters="live", use_graph=False, **kw)
    assert torch.equal(a_ids, b_ids) and torch.equal(a_lg, b_lg) and bool(torch.isfinite(a_lg).all())
    m.text.lora, saved = None, m.text.lora
    _, base_lg = m.generate(ids_, images=rgb, **kw)
    m.text.lora = saved
    assert rel(a_lg[:, 1], base_lg[:, 1]) > 1e-4
    # merge_lora re-quantises the rows: the tiled copies are dropped and rebuilt from the new codes
    L = m.text.p["layers"][0]
    old = L["o_wi8p"]
    old_data = old.data.clone()
    m.text.merge_lora()
    assert m.text.lora is None and m.text.base_int8 and "o_wi8p" not in L
    _, lg = m.generate(ids_, images=rgb, **kw)
    new = L["o_wi8p"]
    assert new is not old and not torch.equal(new.data, old_data) and bool(torch.isfinite(lg).all())
    assert torch.equal(new.data, hk.repack_int8_mfma(L["o_wi8"]).data)


@pytest.mark.parametrize("B", [1, 3])
def test_int8_runs_and_graph_replay_equals_eager_launches(B):
    m = _model()
    ids_, rgb = _inputs(B)
    a_ids, a_lg = m.generate(ids_, images=rgb, **KW)
    b_ids, b_lg = m.generate(ids_, images=rgb, use_graph=False, **KW)
    assert bool(torch.isfinite(a_lg).all()) and a_ids.shape == (B, 5)
    assert torch.equal(a_ids, b_ids) and torch.equal(a_lg, b_lg)
    L = m.text.p["layers"][0]
    assert isinstance(L["qkv_wi8p"], hk.PackedI8) and L["qkv_wi8p"].shape == tuple(L["qkv_w"].shape)
    assert "qkv_wp" not in L and "qkv_w8p" not in L          # lm_head alone is re-tiled for the bf16 MFMA GEMV, as in the 4-bit mode


def test_int8_beam_search_graph_equals_eager():
    m = _model()
    ids_, rgb = _inputs(1)
    kw = dict(do_sample=False, max_new_tokens=5, eos_token_id=None, weights="int8", num_beams=2, return_beam_scores=True)
    a_ids, a_sc = m.generate(ids_, images=rgb, **kw)
    b_ids, b_sc = m.generate(ids_, images=rgb, use_graph=False, **kw)
    assert torch.equal(a_ids, b_ids) and torch.equal(a_sc, b_sc) and bool(torch.isfinite(a_sc).all())


def test_int8_with_the_e4m3_kv_cache_graph_equals_eager():
    m = _model()
    ids_, rgb = _inputs(2)
    a_ids, a_lg = m.generate(ids_, images=rgb, kv_cache="fp8", **KW)
    b_ids, b_lg = m.generate(ids_, images=rgb, kv_cache="fp8", use_graph=False, **KW)
    assert torch.equal(a_ids, b_ids) and torch.equal(a_lg, b_lg) and bool(torch.isfinite(a_lg).all())


def test_equal_prompts_give_equal_rows():
    m = _model()
    ids_, rgb = _inputs(4, same=True)
    _, lg = m.generate(ids_, images=rgb, **KW)
    for b in range(1, 4):
        assert torch.equal(lg[b], lg[0]), b


def test_the_arithmetic_is_llm_int8_not_bf16():
    m = _model()
    ids1, rgb1 = _inputs(1)
    ids17, rgb17 = _inputs(17, same=True)
    kw = dict(KW, max_new_tokens=2)
    _, ref = m.generate(ids17, images=rgb17, **kw)          # batch 17: prefill and step on hk.int8_linear
    ref = ref[:1]
    gaps = {}
    for w in ("int8", "bf16", "fp8"):
        _, lg = m.generate(ids1, images=rgb1, **dict(kw, weights=w))
        gaps[w] = rel(lg[:, 1], ref[:, 1])
    print(f"step-1 logits of batch 1, rel-L2 against the batch-17 LLM.int8 step: int8 {gaps['int8']:.3e}, bf16 {gaps['bf16']:.3e}, fp8 {gaps['fp8']:.3e}; "
          f"bf16 / int8 {gaps['bf16'] / max(gaps['int8'], 1e-30):.2f}, fp8 / int8 {gaps['fp8'] / max(gaps['int8'], 1e-30):.2f}")
    assert gaps["int8"] < gaps["bf16"] and gaps["int8"] < gaps["fp8"], gaps


def test_tiled_int8_copies_are_derived_keys(tmp_path):
    m = _model()
    ids_, rgb = _inputs(1)
    m.generate(ids_, images=rgb, **dict(KW, max_new_tokens=2))
    L = m.text.p["layers"][0]
    names = {k + "i8p" for k in NAMES}
    assert names <= set(L) and "i8p" in TextModal.DERIVED_SUFFIXES and names <= LHRSEngine.DERIVED_KEYS

    def keys(o, pre=""):
        if isinstance(o, dict):
            for k, v in o.items():
                yield from keys(v, f"{pre}{k}.")
        else:
            assert torch.is_tensor(o), (pre, type(o))
            yield pre
    ckpt = m.custom_save_checkpoint(str(tmp_path / "ckpt"))
    assert not any("i8p" in k for k in keys(ckpt))
    probe = dict(L)
    m.text._drop_derived(probe)
    assert not names & set(probe) and names <= set(L)


def test_cli_qa_decode_weights_int8(capsys):
    import json

    import cli_qa
    args = ["--synthetic-prompt", "24", "--max-new-tokens", "6", "--llama-layers", "2"]
    out = cli_qa.main(cli_qa.parse_option(args + ["--opts", "bits", "8", "--decode-weights", "int8"]))
    assert tuple(out.shape) == (1, 6)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["weights"] == "int8"
    with pytest.raises(ValueError, match="bits: 8"):
        cli_qa.main(cli_qa.parse_option(args + ["--decode-weights", "int8"]))
