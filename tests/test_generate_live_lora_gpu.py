"""generate(adapters="live"): un-merged LoRA adapters run next to the base weights of whatever format - `hk.lora_down` / `hk.lora_up` around the
decode GEMVs (TextModal._decode_session), the training forward in prefill - and no merged copy of a weight is made.

2-layer models on the oracle's parameters with adapters from `OP.make_lora_params` (non-zero B), built once per module.  Bounds:
  - against the oracle: what tests/test_lora_gpu.py::test_generate_with_unmerged_adapters_uses_them_and_leaves_the_base_untouched gives the
    merged path (rel-L2 < 3e-2 teacher-forced, the adapter-free base at least 3x further away);
  - a decode step against the prefill path of the same position (one longer prefill), on the NF4 model as tests/test_gemv4_gpu.py builds it, for every
    `weights`: "bf16" and "4bit" get that file's bound, 4 g with g as it defines it there (the existing code's two bf16 summation orders on this model
    and step: batch 1 against row 0 of the same prompt at batch 2, default merged mode); "fp8" gets the 1.5e-1 that
    tests/test_generate_gpu.py::test_fp8_weight_decode_and_fused_prologues gives the first e4m3 step against bf16.  "4bit" additionally gets
    test_gemv4_gpu's own assertion in live mode: its first decode step is within 4 g of the live bf16 one.
    Measured on an MI355X on that model (batch 1 / 2 / 5): g = 6.1e-3; live decode against live prefill 1.0e-2 / 9.4e-3 / 9.1e-3 (bf16), 9.9e-3 / 9.3e-3 /
    9.1e-3 (4bit), 1.0e-1 / 9.7e-2 / 1.0e-1 (fp8); 4bit against bf16, both live, 4.0e-3 / 2.3e-3 / 4.5e-3.  (The default merged mode's own decode-against-prefill gap there: 7.1e-3 - 7.5e-3.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from lhrs_bot_amd import kernels as hk  # noqa: E402
from lhrs_bot_amd.unibind import UniBind  # noqa: E402
from oracle import lhrs_oracle as O  # noqa: E402
from oracle import params as OP  # noqa: E402

DEV = "cuda"
NL = 2
ALL = ("q", "k", "v", "o", "gate", "up", "down")
KW = dict(do_sample=False, return_logits=True, eos_token_id=None)
_P, _LORA, _MODELS = {}, {}, {}


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _params():
    if not _P:
        _P.update(vit=OP.make_vit_params(seed=2), pooler=OP.make_pooler_params(seed=1), llama=OP.make_llama_params(seed=3, layers=NL))
    return _P


def _lora_params(r, targets, seed=4):
    key = (r, targets, seed)
    if key not in _LORA:
        _LORA[key] = OP.make_lora_params(seed=seed, layers=NL, r=r, alpha=2 * r, targets=targets)
    return _LORA[key]


def _build(r=16, targets=ALL, quant4=False, seed=4):
    m = UniBind(("rgb", "text"), None, device=DEV, llama_layers=NL).load_params(_params()).eval()
    if quant4:
        m.text.quantize_base(4, quant_type="nf4", double_quant=True)
    lora = m.enable_lora(r=r, alpha=2 * r, targets=targets, seed=0)
    for l, lp in enumerate(_lora_params(r, targets, seed)):
        for pr in targets:
            lora.set_adapter(l, pr, *lp[pr])
    lora.refresh()
    return m


def _model(quant4=False):
    """r = 16 on all seven projections, on the bf16 base or on the NF4 base; built once per module"""
    if quant4 not in _MODELS:
        _MODELS[quant4] = _build(quant4=quant4)
    return _MODELS[quant4]


def _inputs(B, seed=5):
    g = torch.Generator().manual_seed(seed)
    ids_ = torch.tensor([[1, -200, 9, 8, 7, 6]]).repeat(B, 1)
    if B > 1:
        ids_[1:, 2:] = torch.randint(3, 32000, (B - 1, 4), generator=g)
    return ids_, torch.randn(B, 3, 224, 224, generator=g)


def test_live_matches_the_oracle_and_merges_nothing():
    m = _model()
    ids_, rgb = _inputs(1)
    m.text._merged_cache = None
    layers = m.text.p["layers"]
    before = {k: v.clone() for k, v in layers[1].items() if k in ("qkv_w", "down_w")}
    new_ids, logits = m.generate(ids_, images=rgb, max_new_tokens=4, adapters="live", **KW)
    assert m.text._merged_cache is None and m.text.p["layers"] is layers          # no merged copies, nothing swapped
    assert all(torch.equal(layers[1][k], v) for k, v in before.items())
    assert m.text.lora.train_mode is True and not m.text.base8
    P = _params()
    Pl = dict(P, llama=dict(P["llama"], layers=[dict(L, lora=lp) for L, lp in zip(P["llama"]["layers"], _lora_params(16, ALL))]))
    with torch.no_grad():
        want = O.generate_logits(Pl, rgb, ids_, new_ids.cpu())
        base = O.generate_logits(P, rgb, ids_, new_ids.cpu())
    print(f"live vs oracle rel-L2 {rel(logits, want):.3e}; adapter-free base vs oracle {rel(base, want):.3e}")
    assert rel(logits, want) < 3e-2 and rel(base, want) > 3 * rel(logits, want)


_G = {}


def _step_vs_prefill(m, ids_, rgb, **kw):
    """-> (rel-L2 of the first decode step's logits against the prefill-path logits of the same position, ids, logits of the 3-token run)"""
    new_ids, lg = m.generate(ids_, images=rgb, max_new_tokens=3, **kw, **KW)
    longer = torch.cat([ids_, new_ids[:, :1].cpu()], 1)                            # the first new token joins the prompt: its position is prefilled
    _, lg_p = m.generate(longer, images=rgb, max_new_tokens=1, **{**kw, "weights": "bf16"}, **KW)
    return rel(lg[:, 1], lg_p[:, 0]), new_ids, lg


def _g(quant4):
    """g of tests/test_gemv4_gpu.py: the existing code's two bf16 summation orders on this model's first decode step - batch 1 against row 0 of the
    same prompt twice (default merged mode: bf16 on the merged copies of the dequantised weights)"""
    if quant4 not in _G:
        m = _model(quant4)
        ids_, rgb = _inputs(1)
        _, a = m.generate(ids_, images=rgb, max_new_tokens=2, **KW)
        _, b = m.generate(ids_.repeat(2, 1), images=rgb.repeat(2, 1, 1, 1), max_new_tokens=2, **KW)
        _G[quant4] = rel(b[:1, 1], a[:, 1])
        m.text._merged_cache = None
    return _G[quant4]


@pytest.mark.parametrize("weights", ["bf16", "fp8", "4bit"])
@pytest.mark.parametrize("B", [1, 2, 5])
def test_every_branch_of_lin_decode_step_against_the_prefill_path(B, weights):
    m = _model(True)
    ids_, rgb = _inputs(B)
    gap, new_ids, lg = _step_vs_prefill(m, ids_, rgb, weights=weights, adapters="live")
    assert new_ids.shape == (B, 3) and lg.shape[:2] == (B, 3) and bool(torch.isfinite(lg).all())
    assert m.text._merged_cache is None
    if weights == "fp8":
        print(f"B={B} fp8: decode step 1 vs prefill path rel-L2 {gap:.3e} (bound 1.5e-1)")
        assert gap < 1.5e-1, gap
        return
    g = _g(True)
    print(f"B={B} {weights}: decode step 1 vs prefill path rel-L2 {gap:.3e}; g {g:.3e}; ratio {gap / max(g, 1e-30):.2f}")
    assert g > 0 and gap <= 4 * g, (gap, g)
    if weights == "4bit":
        _, lg_bf = m.generate(ids_, images=rgb, max_new_tokens=3, weights="bf16", adapters="live", **KW)
        gap4 = rel(lg[:, 1], lg_bf[:, 1])
        print(f"B={B} 4bit vs bf16, both live, step 1: {gap4:.3e}; g {g:.3e}; ratio {gap4 / max(g, 1e-30):.2f}")
        assert torch.equal(lg[:, 0], lg_bf[:, 0])                                  # the prefill is the bf16 GEMM path in both
        assert gap4 <= 4 * g, (gap4, g)


@pytest.mark.parametrize("B", [1, 5])
def test_live_graph_replay_equals_eager_launches(B):
    m = _model()
    ids_, rgb = _inputs(B)
    a_ids, a_lg = m.generate(ids_, images=rgb, max_new_tokens=4, adapters="live", **KW)
    b_ids, b_lg = m.generate(ids_, images=rgb, max_new_tokens=4, adapters="live", use_graph=False, **KW)
    assert torch.equal(a_ids, b_ids) and torch.equal(a_lg, b_lg)


def test_adapter_update_is_seen_without_a_rebuild():
    m = _build()
    ids_, rgb = _inputs(1)
    _, lg0 = m.generate(ids_, images=rgb, max_new_tokens=3, adapters="live", **KW)
    A2, B2 = _lora_params(16, ALL, seed=11)[1]["o"]
    m.text.lora.set_adapter(1, "o", A2, B2)
    m.text.lora.refresh()
    _, lg1 = m.generate(ids_, images=rgb, max_new_tokens=3, adapters="live", **KW)
    assert not torch.equal(lg1, lg0)
    fresh = _build()
    fresh.text.lora.set_adapter(1, "o", A2, B2)
    fresh.text.lora.refresh()
    _, lg2 = fresh.generate(ids_, images=rgb, max_new_tokens=3, adapters="live", **KW)
    assert torch.equal(lg1, lg2)


def test_default_is_the_merged_path_and_4bit_without_the_opt_in_still_raises():
    m = _model()
    ids_, rgb = _inputs(1)
    a_ids, a_lg = m.generate(ids_, images=rgb, max_new_tokens=3, **KW)
    assert m.text._merged_cache is not None
    b_ids, b_lg = m.generate(ids_, images=rgb, max_new_tokens=3, adapters="merged", **KW)
    assert torch.equal(a_ids, b_ids) and torch.equal(a_lg, b_lg)
    m.text._merged_cache = None
    with pytest.raises(ValueError, match="adapters"):
        m.generate(ids_, images=rgb, max_new_tokens=3, adapters="both", **KW)
    m4 = _model(True)
    with pytest.raises(ValueError, match="merge_lora") as e:
        m4.generate(ids_, images=rgb, max_new_tokens=3, weights="4bit", **KW)
    assert 'adapters="live"' in str(e.value)
    saved, m.text.lora = m.text.lora, None                                         # without adapters "live" is the plain path
    try:
        c_ids, c_lg = m.generate(ids_, images=rgb, max_new_tokens=3, **KW)
        d_ids, d_lg = m.generate(ids_, images=rgb, max_new_tokens=3, adapters="live", **KW)
    finally:
        m.text.lora = saved
    assert torch.equal(c_ids, d_ids) and torch.equal(c_lg, d_lg)


def test_beam_search_live_on_the_4bit_base():
    m = _model(True)
    ids_, rgb = _inputs(1)
    ids, lg, sc = m.generate(ids_, images=rgb, max_new_tokens=4, weights="4bit", adapters="live", num_beams=2, return_beam_scores=True, **KW)
    assert ids.shape == (1, 4) and lg.shape[:2] == (2, 4) and sc.shape == (1,)
    assert bool(torch.isfinite(sc).all()) and bool(torch.isfinite(lg).all())
    assert m.text._merged_cache is None


def test_stage3_groups_only_the_adapted_linears_change(monkeypatch):
    """r = 8 on q, k, v, o: the gate|up and down launches are exactly today's - one eager step calls hk.lora_down twice per layer"""
    m = _build(r=8, targets=("q", "k", "v", "o"))
    ids_, rgb = _inputs(1)
    calls = []
    real_down, real_up = hk.lora_down, hk.lora_up

    def down(x, A, tpart, K, R=None, **kw):
        calls.append(("down", K, R))
        return real_down(x, A, tpart, K, R, **kw)

    def up(acc, tpart, nsl, s, Bw, r, fout, out, **kw):
        calls.append(("up", r, fout))
        return real_up(acc, tpart, nsl, s, Bw, r, fout, out, **kw)

    monkeypatch.setattr(hk, "lora_down", down)
    monkeypatch.setattr(hk, "lora_up", up)
    _, lg = m.generate(ids_, images=rgb, max_new_tokens=2, adapters="live", use_graph=False, **KW)   # prefill + ONE eager step
    assert bool(torch.isfinite(lg).all())
    assert [c for c in calls if c[0] == "down"] == [("down", 4096, 24), ("down", 4096, 8)] * NL
    assert [c for c in calls if c[0] == "up"] == [("up", 8, 4096), ("up", 8, 4096)] * NL
