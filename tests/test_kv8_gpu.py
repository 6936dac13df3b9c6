"""Decode from an e4m3 KV cache (csrc/decode_attn.hip behind hk.kv8_quant_rows / hk.decode_attn_kv8, generate(kv_cache="fp8")) on an MI355X,
against the restatement of tests/kv8_cases.py.

Format: codes and scale bytes byte for byte, read from a strided qkv buffer with a NaN surround, written at a non-zero cache row of a
sentinel-filled cache whose other rows must come back untouched.
Attention: every case of kv8_cases.CASES against float64 per element inside the derived bound of that module (ratio <= 1, printed), the
appended codes and scale bytes exact (exact-rotation cases) or within one e4m3 spacing (model tables), every other cache byte unchanged -
the caches are NaN codes and 0xFF scale bytes wherever the kernel must not read - tickets back at zero.
Model: generate(kv_cache="fp8") computes the prompt on the exact bf16 K / V (step-0 logits and first token torch.equal to the bf16-cache
run) and reads the rounded cache from step 1 on: those logits differ from the bf16-cache ones, and by no more (rel-L2) than those of
weights="fp8" do - kv8 rounds two activations per layer at e4m3 precision with a per-head scale, the fp8 weight mode every decoder weight
and activation at the same element precision.  Seen on an MI355X (DESIGN.md "Decode from an e4m3 KV cache"): worst error / bound 0.9032
(the bf16 store; the float32 emulation of kv8_cases gives the same nine figures), step-1 gaps 1.56e-2 against 9.86e-2 (batch 1, ratio
0.16) and 1.39e-2 against 9.81e-2 (batch 3, 0.14)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from lhrs_bot_amd import kernels as hk  # noqa: E402
from lhrs_bot_amd.text import TextModal  # noqa: E402
from lhrs_bot_amd.unibind import UniBind  # noqa: E402

import kv8_cases as kv  # noqa: E402

DEV = "cuda"
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
CASE_IDS = [c.name.replace(" ", "_") for c in kv.CASES]


# ------------------------------------------------------------------------------------------------------------------------- 1. kv8_quant_rows
def _quant_rows_roundtrip(rows, H, row0, block, name):
    """rows: host bf16 [n, H * 128], placed as column block `block` (1: K, 2: V) of a [n, 3 H 128] buffer that is NaN elsewhere"""
    n, d = rows.shape
    qkv = torch.full((n, 3 * d), float("nan"), dtype=BF)
    qkv[:, block * d:(block + 1) * d] = rows
    qkv = qkv.to(DEV)
    total = row0 + n + 7
    codes = torch.full((total, d), 0xA5, dtype=U8, device=DEV)
    scales = torch.full((total, H), 0xA5, dtype=U8, device=DEV)
    hk.kv8_quant_rows(qkv[:, block * d:(block + 1) * d], codes, scales, row0, H)
    want_c, want_s = kv.quant(rows.reshape(n, H, kv.D))
    codes, scales = codes.cpu(), scales.cpu()
    assert torch.equal(scales[row0:row0 + n], want_s), name
    assert torch.equal(codes[row0:row0 + n], want_c.reshape(n, d)), name
    for t in (codes, scales):
        assert bool((t[:row0] == 0xA5).all()) and bool((t[row0 + n:] == 0xA5).all()), f"{name}: a neighbouring cache row was written"


def test_kv8_quant_rows_planted_and_random_rows_byte_for_byte():
    g = torch.Generator().manual_seed(5)
    rnd = (torch.randn(74, kv.D, generator=g).double() * torch.exp2(torch.randint(-30, 31, (74, 1), generator=g).double())).to(BF)
    rows = torch.cat((kv.planted(), rnd)).reshape(41, 2 * kv.D)             # H = 2: 82 head rows, three workgroups
    _quant_rows_roundtrip(rows, 2, 5, 1, "K block")
    _quant_rows_roundtrip(rows, 2, 0, 2, "V block")


def test_kv8_quant_rows_model_width():
    g = torch.Generator().manual_seed(6)
    rows = torch.randn(37, 32 * kv.D, generator=g).to(BF)                  # H = 32: 1184 head rows, 37 workgroups
    _quant_rows_roundtrip(rows, 32, 11, 1, "H 32")


# ------------------------------------------------------------------------------------------------------------------------- 2. decode_attn_kv8
def _run(c, nsplit=None, use_cs=False):
    """-> (out bf16 [B, H D] on the host, dict of the four cache arrays on the host after the call)"""
    i = kv.inputs(c)
    NS = c.nsplit if nsplit is None else nsplit
    B, H, D = kv.B, kv.H, kv.D
    qbuf = torch.full((B + 1, 3 * H * D + 8), float("nan"), dtype=BF)        # NaN columns past the row and a NaN row after the last
    qbuf[:B, :3 * H * D] = i["qkv"]
    qkv = qbuf.to(DEV)[:B, :3 * H * D]
    caches = {k: i[k].to(DEV) for k in ("kc", "vc", "ks", "vs")}
    cos, sin = i["cos"].to(DEV), i["sin"].to(DEV)
    pos = torch.tensor(c.pos, dtype=torch.int32, device=DEV)
    obuf = torch.full((B + 2, H * D + 8), -1, dtype=torch.int16, device=DEV).view(BF)
    out = obuf[:B, :H * D]
    part = torch.full((B, H, NS, 132), float("nan"), device=DEV, dtype=F32)
    tickets = torch.zeros((B, H), device=DEV, dtype=torch.int32)
    km = None if i["kmask"] is None else i["kmask"].to(DEV)
    cs = torch.cat((i["cos"][list(c.pos)], i["sin"][list(c.pos)]), 1).contiguous().to(DEV) if use_cs else None
    hk.decode_attn_kv8(qkv, caches["kc"], caches["vc"], caches["ks"], caches["vs"], cos, sin, pos, out, B, H, D, kv.MAX_CTX, kv.SCALE, NS,
                       part, tickets, key_mask=km, cs=cs)
    torch.cuda.synchronize()
    assert not bool(tickets.any()), f"{c.name}: a ticket was left non-zero"
    ob = obuf.view(torch.int16)
    assert bool((ob[B:] == -1).all()) and bool((ob[:, H * D:] == -1).all()), f"{c.name}: an element outside the output was written"
    assert bool(torch.isfinite(out.float()).all()), f"{c.name}: non-finite output"
    return out.cpu(), {k: v.cpu() for k, v in caches.items()}


def _check_caches(c, got):
    """exact-rotation cases: every byte; model tables: V and every row but the appended K rows exact, those within one spacing"""
    if not c.real:
        want = kv.expected_caches(c)
        for k in want:
            assert torch.equal(got[k], want[k]), f"{c.name}: {k} differs from the expected cache bytes"
        return kv.case_reference(c)
    want = kv.expected_caches(c)
    keep = torch.ones(kv.B * kv.MAX_CTX, dtype=torch.bool)
    keep[[b * kv.MAX_CTX + p for b, p in enumerate(c.pos)]] = False
    assert torch.equal(got["vc"], want["vc"]) and torch.equal(got["vs"], want["vs"]), c.name
    assert torch.equal(got["kc"][keep], want["kc"][keep]) and torch.equal(got["ks"][keep], want["ks"][keep]), c.name
    kv.check_real_append(c, got["kc"], got["ks"])
    return kv.reference(c, got)


@pytest.mark.parametrize("c", kv.CASES, ids=CASE_IDS)
def test_decode_attn_kv8_case_vs_fp64(c):
    out, caches = _run(c)
    ref = _check_caches(c, caches)
    r = kv.ratio(out, ref, "decode_attn_kv8")
    print(f"{c.name}: {r:.4f} x the bound")
    assert r <= 1.0, (c.name, r)


@pytest.mark.parametrize("c", [kv.CASES[5], kv.CASES[6], kv.CASES[8]], ids=[CASE_IDS[5], CASE_IDS[6], CASE_IDS[8]])
def test_decode_attn_kv8_split_counts_agree(c):
    """nsplit 1, 2 and 3 on the same inputs: identical appended bytes, outputs within twice the bound of each other"""
    runs = [_run(c, ns) for ns in (1, 2, 3)]
    ref = _check_caches(c, runs[0][1])
    for out, caches in runs[1:]:
        assert all(torch.equal(caches[k], runs[0][1][k]) for k in caches), c.name
        assert bool(((out.double() - runs[0][0].double()).abs() <= 2 * ref.bound).all()), c.name
    for ns, (out, _) in zip((1, 2, 3), runs):
        assert kv.ratio(out, ref, "decode_attn_kv8") <= 1.0, (c.name, ns)


@pytest.mark.parametrize("c", [kv.CASES[0], kv.CASES[2], kv.CASES[6], kv.CASES[8]], ids=[CASE_IDS[0], CASE_IDS[2], CASE_IDS[6], CASE_IDS[8]])
def test_decode_attn_kv8_cs_rows_change_nothing(c):
    """with the cos | sin rows of the new position handed in (what decode_advance leaves) the output and the cache are bit-identical"""
    a, ca = _run(c)
    b, cb = _run(c, use_cs=True)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and all(torch.equal(ca[k], cb[k]) for k in ca), c.name


# ------------------------------------------------------------------------------------------------------------------------- 3. generate
NL = 2
_M = {}
KW = dict(do_sample=False, max_new_tokens=5, return_logits=True, eos_token_id=None)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _model():
    if not _M:
        _M["m"] = UniBind(("rgb", "text"), None, device=DEV, llama_layers=NL).init_random(seed=1).eval()
    return _M["m"]


def _inputs(B, seed=5):
    g = torch.Generator().manual_seed(seed)
    ids_ = torch.tensor([[1, -200, 9, 8, 7, 6]]).repeat(B, 1)
    if B > 1:
        ids_[1:, 2:] = torch.randint(3, 32000, (B - 1, 4), generator=g)
    return ids_, torch.randn(B, 3, 224, 224, generator=g)


def _pair(m, B, **extra):
    """-> (tokens, logits) of the bf16-cache run and of the fp8-cache run; the step-0 assertions every mode shares"""
    ids_, rgb = _inputs(B)
    tok_bf, lg_bf = m.generate(ids_, images=rgb, **KW, **extra)
    tok_8, lg_8 = m.generate(ids_, images=rgb, kv_cache="fp8", **KW, **extra)
    assert torch.equal(lg_8[:, 0], lg_bf[:, 0]) and torch.equal(tok_8[:, 0], tok_bf[:, 0])      # the prompt attends over the exact bf16 K / V
    assert tok_8.shape == (B, 5) and bool(torch.isfinite(lg_8).all())
    gap = rel(lg_8[:, 1], lg_bf[:, 1])
    assert gap > 0, "step 1 of kv_cache='fp8' equals the bf16-cache step bit for bit: the new path did not run"
    return (tok_bf, lg_bf), (tok_8, lg_8), gap


@pytest.mark.parametrize("B", [1, 3])
def test_fp8_cache_first_step_is_no_further_from_bf16_than_fp8_weights(B):
    m = _model()
    (_, lg_bf), _, gap_kv = _pair(m, B)
    ids_, rgb = _inputs(B)
    _, lg_w8 = m.generate(ids_, images=rgb, weights="fp8", **KW)
    gap_w8 = rel(lg_w8[:, 1], lg_bf[:, 1])
    print(f"batch {B}, step-1 logits, rel-L2 against the bf16 cache and weights: kv_cache fp8 {gap_kv:.3e}, weights fp8 {gap_w8:.3e}, "
          f"ratio {gap_kv / max(gap_w8, 1e-30):.3f}")
    assert gap_w8 > 0 and gap_kv <= gap_w8, (gap_kv, gap_w8)


def test_fp8_cache_with_mxfp4_weights():
    """the kv8 rounding moves the mxfp4 step no further than the MXFP4 rounding of the weights moves the bf16 step (both e4m3-or-coarser
    roundings of every decoder linear against two e4m3 roundings per layer): a condition, printed with both figures"""
    m = _model()
    (_, lg_mx), _, gap = _pair(m, 3, weights="mxfp4")
    ids_, rgb = _inputs(3)
    _, lg_bf = m.generate(ids_, images=rgb, **KW)
    gap_w = rel(lg_mx[:, 1], lg_bf[:, 1])
    print(f"weights mxfp4: kv_cache fp8 against the bf16 cache, step-1 rel-L2 {gap:.3e}; mxfp4 against bf16 weights {gap_w:.3e}")
    assert gap <= gap_w


def test_fp8_cache_with_live_adapters():
    m = _model()
    targets = ("q", "k", "v", "o")
    lora = m.enable_lora(r=8, alpha=16, targets=targets, seed=0)
    try:
        g = torch.Generator(device=DEV).manual_seed(1)
        for l in range(NL):
            for pr in targets:
                A, Bm = lora.get_adapter(l, pr)
                lora.set_adapter(l, pr, A, torch.randn(Bm.shape, device=DEV, generator=g) * 0.02)
        lora.refresh()
        m.eval()
        for B in (1, 3):
            _, _, gap = _pair(m, B, adapters="live")
            print(f"live adapters, batch {B}: kv_cache fp8 against bf16, step-1 rel-L2 {gap:.3e}")
    finally:
        m.text.lora, m.text._merged_cache = None, None


def test_fp8_cache_with_a_left_padded_batch():
    m = _model()
    pad = int(m.text.tokenizer.pad_token_id)
    ids_ = torch.tensor([[1, -200, 9, 8, 7, 6, 5, 4], [pad, pad, 1, -200, 11, 12, 13, 14], [pad, pad, pad, pad, 1, -200, 21, 22]])
    mask = ids_.ne(pad)
    rgb = torch.randn(3, 3, 224, 224, generator=torch.Generator().manual_seed(7))
    tok_bf, lg_bf = m.generate(ids_, images=rgb, attention_mask=mask, **KW)
    tok_8, lg_8 = m.generate(ids_, images=rgb, attention_mask=mask, kv_cache="fp8", **KW)
    assert torch.equal(lg_8[:, 0], lg_bf[:, 0]) and torch.equal(tok_8[:, 0], tok_bf[:, 0]) and bool(torch.isfinite(lg_8).all())
    gap = rel(lg_8[:, 1], lg_bf[:, 1])
    print(f"left-padded batch: kv_cache fp8 against bf16, step-1 rel-L2 {gap:.3e}")
    assert gap > 0
    # the mask reaches the kv8 kernel: without it the padded rows change, the unpadded row does not
    _, lg_nomask = m.generate(ids_, images=rgb, kv_cache="fp8", **KW)
    assert rel(lg_nomask[0], lg_8[0]) < 1e-6 and rel(lg_nomask[2, 1], lg_8[2, 1]) > 1e-3


def test_fp8_cache_is_reproducible_graph_or_not_split_or_not(monkeypatch):
    m = _model()
    ids_, rgb = _inputs(3)
    a_ids, a_lg = m.generate(ids_, images=rgb, kv_cache="fp8", **KW)
    b_ids, b_lg = m.generate(ids_, images=rgb, kv_cache="fp8", **KW)                      # graph replay: tickets back at zero
    assert torch.equal(a_ids, b_ids) and torch.equal(a_lg, b_lg)
    c_ids, c_lg = m.generate(ids_, images=rgb, kv_cache="fp8", use_graph=False, **KW)
    assert torch.equal(a_ids, c_ids) and torch.equal(a_lg, c_lg)
    # one workgroup per head: the same bytes in the cache, sums in another order
    monkeypatch.setenv("LHRS_DECODE_SPLIT", "0")
    d_ids, d_lg = m.generate(ids_, images=rgb, kv_cache="fp8", **KW)
    assert torch.equal(d_lg[:, 0], a_lg[:, 0]) and rel(d_lg, a_lg) < 1e-2 and bool(torch.isfinite(d_lg).all())
    monkeypatch.delenv("LHRS_DECODE_SPLIT")
    # the device sampler draws from the kv8 logits like from any others
    kw = dict(do_sample=True, sampler="device", seed=3, max_new_tokens=5, eos_token_id=None, kv_cache="fp8")
    assert torch.equal(m.generate(ids_, images=rgb, **kw), m.generate(ids_, images=rgb, **kw))


# ------------------------------------------------------------------------------------------------------------------------- 4. beam
def test_fp8_cache_beam_search_replicates_and_reorders_codes_and_scales(monkeypatch):
    m = _model()
    ids_, rgb = _inputs(1)
    held = []
    alloc = m.text._alloc_kv
    monkeypatch.setattr(m.text, "_alloc_kv", lambda rows, kind: held.append(alloc(rows, kind)) or held[-1])
    kw = dict(do_sample=False, num_beams=3, max_new_tokens=6, eos_token_id=None, return_beam_scores=True, kv_cache="fp8")
    a_ids, a_sc = m.generate(ids_, images=rgb, **kw)
    b_ids, b_sc = m.generate(ids_, images=rgb, **kw)
    assert torch.equal(a_ids, b_ids) and torch.equal(a_sc, b_sc) and bool(torch.isfinite(a_sc).all()) and a_ids.shape[0] == 1
    caches = held[0]
    assert len(caches) == NL and len(caches[0]) == 4 and all(t.dtype == U8 for t in caches[0])
    max_ctx = caches[0][0].shape[0] // 3
    S0 = max_ctx - 6
    for layer in caches:
        for t in layer:                                                                    # codes [3 max_ctx, d] and scales [3 max_ctx, H]
            v = t.view(3, max_ctx, -1)[:, :S0].cpu()
            assert torch.equal(v[1], v[0]) and torch.equal(v[2], v[0])                     # the prompt was replicated, scales included


def test_kv_beam_reorder_moves_kv8_codes_and_scales_together():
    H, nb, max_ctx, t0, t1 = 16, 3, 16, 2, 9
    d = H * kv.D
    g = torch.Generator().manual_seed(9)
    codes = torch.randint(0, 256, (nb * max_ctx, d), generator=g).to(U8)
    scales = torch.randint(0, 256, (nb * max_ctx, H), generator=g).to(U8)
    parent = torch.tensor([2, 0, 0], dtype=torch.int32)
    cd, sd = codes.to(DEV), scales.to(DEV)
    hk.kv_beam_reorder(hk.kv_cache_table([(cd,)], DEV), 1, nb, max_ctx, d // 2, parent.to(DEV), t0, t1, max_ctx - t0)
    hk.kv_beam_reorder(hk.kv_cache_table([(sd,)], DEV), 1, nb, max_ctx, H // 2, parent.to(DEV), t0, t1, max_ctx - t0)
    for got, old in ((cd.cpu(), codes), (sd.cpu(), scales)):
        want = old.clone().view(nb, max_ctx, -1)
        want[:, t0:t1] = old.view(nb, max_ctx, -1)[parent.long(), t0:t1]
        assert torch.equal(got.view(nb, max_ctx, -1), want)


# ------------------------------------------------------------------------------------------------------------------------- 5. rejections
def test_rejections_leave_the_bf16_path_working():
    m = _model()
    ids_, rgb = _inputs(1)
    kw = dict(do_sample=False, max_new_tokens=2, eos_token_id=None)
    want = m.generate(ids_, images=rgb, **kw)
    with pytest.raises(ValueError, match="kv_cache"):
        m.generate(ids_, images=rgb, kv_cache="int8", **kw)
    assert torch.equal(m.generate(ids_, images=rgb, **kw), want)
    ids17 = ids_.repeat(17, 1)
    with pytest.raises(ValueError, match="17"):
        m.generate(ids17, images=rgb.repeat(17, 1, 1, 1), kv_cache="fp8", **kw)
    assert torch.equal(m.generate(ids_, images=rgb, **kw), want)
    with pytest.raises(ValueError, match="16"):
        m.generate(ids_.repeat(6, 1), images=rgb.repeat(6, 1, 1, 1), kv_cache="fp8", num_beams=3, **kw)
    tm = TextModal(device=DEV, layers=0, dim=2048, heads=32)                               # head_dim 64
    with pytest.raises(ValueError, match="head_dim"):
        tm.generate(torch.tensor([[1, 5, 6, 7]]), kv_cache="fp8", **kw)
    assert torch.equal(m.generate(ids_, images=rgb, **kw), want)


def test_worst_ratio_seen_on_the_device():
    """last in the file: the largest error / bound the comparisons above saw (allowed: 1)"""
    for k in sorted(kv.WORST):
        print(f"WORST {k:18s} {kv.WORST[k]:.4f}")
