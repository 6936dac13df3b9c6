"""Keeping the KV cache across chat turns on an MI355X: hk.kv8_dequant_rows (csrc/decode_attn.hip) bit for bit against the restatement of
tests/kv8_cases.py, and generate(prefix_cache=...) on the two-layer, dim-4096 random UniBind: what is reused, that the reused rows are read
(and only the live ones), rollback, the image encoder's call count, the e4m3 cache behind a context (exact by construction: the same
attention kernel over the same values as a bf16 cache holding the dequantised rows), reproducibility and the rejections.

Tolerances: 1e-2 (rel-L2) of a cached decode against the engine's own uncached computation and 3e-2 against the fp32 oracle are those of
tests/test_generate_gpu.py; everything else is bit equality."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from lhrs_bot_amd import generation  # noqa: E402
from lhrs_bot_amd import kernels as hk  # noqa: E402
from lhrs_bot_amd.text import TextModal  # noqa: E402
from lhrs_bot_amd.unibind import UniBind  # noqa: E402
from oracle import lhrs_oracle as O  # noqa: E402
from oracle import params as OP  # noqa: E402

import kv8_cases as kv  # noqa: E402

DEV = "cuda"
BF, U8, I16 = torch.bfloat16, torch.uint8, torch.int16
NL, NI, MAXP = 2, 144, 256
KW = dict(do_sample=False, return_logits=True, eos_token_id=None)
_M = {}


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# ------------------------------------------------------------------------------------------------------------------------- 1. kv8_dequant_rows
def _head_rows(n_rows, seed):
    """codes uint8 [n_rows, 128] and bytes uint8 [n_rows]: the quantised planted rows of kv8_cases first, then random non-NaN codes under
    scale bytes from [10, 240]"""
    g = torch.Generator().manual_seed(seed)
    pc, pb = kv.quant(kv.planted())
    codes = torch.randint(0, 256, (n_rows, kv.D), generator=g).to(U8)
    codes = torch.where((codes & 0x7F) == 0x7F, codes & 0xF0, codes)              # no NaN code
    byte = torch.randint(10, 241, (n_rows,), generator=g).to(U8)
    codes[:8], byte[:8] = pc, pb
    return codes, byte


@pytest.mark.parametrize("H,n,row0,pad", [(2, 5, 0, 0), (2, 17, 3, 0), (32, 3, 2, 64)], ids=["partial_workgroup", "two_workgroups_row0", "model_width_strided"])
def test_kv8_dequant_rows_bit_exact(H, n, row0, pad):
    d = H * kv.D
    c, b = _head_rows(n * H, seed=H + n)
    total = row0 + n + 2
    codes = torch.full((total, d), 0x7F, dtype=U8)                                # NaN codes and byte 255 wherever the kernel must not read
    scales = torch.full((total, H), 0xFF, dtype=U8)
    codes[row0:row0 + n], scales[row0:row0 + n] = c.reshape(n, d), b.reshape(n, H)
    buf = torch.full((n + 2, d + pad), -1, dtype=I16, device=DEV)
    out = buf.view(BF)[1:1 + n, :d]
    assert hk.kv8_dequant_rows(codes.to(DEV), scales.to(DEV), row0, n, H, out) is out
    want = kv.dequant(c.reshape(n, H, kv.D), b.reshape(n, H)).to(BF).reshape(n, d)
    got = buf.cpu()
    assert torch.equal(got[1:1 + n, :d], want.view(I16))
    assert bool((got[0] == -1).all()) and bool((got[1 + n] == -1).all()) and bool((got[:, d:] == -1).all())


def test_kv8_quantise_dequantise_quantise_returns_the_same_bytes():
    """rows whose head maximum is a power of two (256 * 2^e: no rounding of the maximum, so the second quantisation finds the same scale);
    every dequantised value is then on the e4m3 grid of that scale.  The planted rows are left out: the maximum of planted row 2 rounds DOWN
    to 224 * 2^e, where the format's rule picks the next smaller scale for the rounded row - the same values, other bytes."""
    H, n, row0 = 2, 17, 3
    g = torch.Generator().manual_seed(21)
    mag = torch.exp2(torch.randint(-30, 31, (n, H, 1), generator=g).double())
    rows = (torch.randn(n, H, kv.D, generator=g).double().clamp(-3.5, 3.5) * mag).to(BF)
    rows[:, :, 7] = (4.0 * mag[:, :, 0]).to(BF)
    rows = rows.reshape(n, H * kv.D).to(DEV)
    c1, s1 = torch.zeros((row0 + n, H * kv.D), dtype=U8, device=DEV), torch.zeros((row0 + n, H), dtype=U8, device=DEV)
    hk.kv8_quant_rows(rows, c1, s1, row0, H)
    back = torch.empty_like(rows)
    hk.kv8_dequant_rows(c1, s1, row0, n, H, back)
    c2, s2 = torch.zeros_like(c1), torch.zeros_like(s1)
    hk.kv8_quant_rows(back, c2, s2, row0, H)
    assert torch.equal(c1, c2) and torch.equal(s1, s2)
    want_c, want_s = kv.quant(rows.cpu().reshape(n, H, kv.D))
    assert torch.equal(c1[row0:].cpu(), want_c.reshape(n, -1)) and torch.equal(s1[row0:].cpu(), want_s)


def test_kv8_dequant_rows_rejects_bad_shapes_and_strides():
    H, d = 2, 2 * kv.D
    codes, scales = torch.zeros((4, d), dtype=U8, device=DEV), torch.zeros((4, H), dtype=U8, device=DEV)
    with pytest.raises(RuntimeError, match="kv8_dequant_rows: n=2 H=2 row0=0 ld=260"):
        hk.kv8_dequant_rows(codes, scales, 0, 2, H, torch.zeros((2, d + 4), dtype=BF, device=DEV)[:, :d])      # ld % 8 != 0
    with pytest.raises(RuntimeError, match="kv8_dequant_rows: n=0"):
        hk.kv8_dequant_rows(codes, scales, 0, 0, H, torch.zeros((2, d), dtype=BF, device=DEV))
    with pytest.raises(AssertionError):
        hk.kv8_dequant_rows(codes, scales, 3, 2, H, torch.zeros((2, d), dtype=BF, device=DEV))                 # rows 3, 4 of a 4-row cache


# ------------------------------------------------------------------------------------------------------------------------- 2. the model
def _model():
    if not _M:
        P = {"vit": OP.make_vit_params(seed=2), "pooler": OP.make_pooler_params(seed=1), "llama": OP.make_llama_params(seed=3, layers=NL)}
        _M["P"] = P
        _M["m"] = UniBind(("rgb", "text"), None, device=DEV, llama_layers=NL).load_params(P).eval()
        _M["rgb"] = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(5))
    return _M["m"]


IDS1 = torch.tensor([[1, -200, 9, 8, 7, 6, 5, 4, 3]])
TAIL2 = [11, 12, 13, 14, 15]
S1 = 1 + NI + 7


def _turn1(kv_cache="bf16", **kw):
    """-> (cache after the first turn, its 4 tokens)"""
    m = _model()
    pc = m.new_prefix_cache(kv_cache, MAXP)
    tok, _ = m.generate(IDS1, images=_M["rgb"], max_new_tokens=4, prefix_cache=pc, **{**KW, **kw})
    assert pc.ids == IDS1[0].tolist() + tok[0, :3].tolist() and pc.length == S1 + 3 and (pc.last_reused, pc.last_prefilled) == (0, S1)
    return pc, tok


def _ids2(tok1):
    return torch.cat([IDS1, tok1.cpu(), torch.tensor([TAIL2])], 1)


def _reference_turn2():
    """turn 2 on a clean bf16 cache, made once and shared: (ids2, tokens, logits)"""
    if "ref2" not in _M:
        pc, tok1 = _turn1()
        ids2 = _ids2(tok1)
        tok, lg = _model().generate(ids2, max_new_tokens=5, prefix_cache=pc, **KW)
        _M["ref2"] = (ids2, tok, lg, pc)
    return _M["ref2"][:3]


def _uncached(ids):
    if "plain" not in _M:
        _M["plain"] = {}
    key = tuple(ids[0].tolist())
    if key not in _M["plain"]:
        _M["plain"][key] = _model().generate(ids, images=_M["rgb"], max_new_tokens=1, **KW)[1]
    return _M["plain"][key]


def test_second_turn_on_the_bf16_cache():
    m = _model()
    ids2, tok, lg = _reference_turn2()
    pc = _M["ref2"][3]
    S0 = S1 + 4 + 5
    assert pc.last_reused == 144 + 8 + 3 and pc.last_prefilled == S0 - pc.last_reused
    assert pc.length == S0 + 4 and pc.ids == ids2[0].tolist() + tok[0, :4].tolist()
    assert tok.shape == (1, 5) and torch.equal(tok, lg.argmax(-1))
    gap0 = rel(lg[:, 0], _uncached(ids2)[:, 0])
    want = O.generate_logits(_M["P"], _M["rgb"], ids2, tok.cpu())
    gap = rel(lg, want)
    print(f"second turn, bf16 cache: step 0 against the uncached generate {gap0:.3e} (allowed 1e-2), 5 steps against the oracle {gap:.3e} (allowed 3e-2)")
    assert gap0 < 1e-2
    assert gap < 3e-2
    picked = want.gather(-1, tok.cpu()[..., None]).squeeze(-1)
    assert torch.all(want.max(-1).values - picked < 0.15 * want.std(-1))


def test_the_cache_is_read_and_only_its_live_part():
    m = _model()
    ids2, tok, lg = _reference_turn2()
    dirty, _ = _turn1()
    for K, V in dirty.caches:
        K[dirty.length:], V[dirty.length:] = 3e4, 3e4               # finite: masked MFMA lanes still multiply
    tok_d, lg_d = m.generate(ids2, max_new_tokens=5, prefix_cache=dirty, **KW)
    assert torch.equal(lg_d, lg) and torch.equal(tok_d, tok)
    hit, _ = _turn1()
    hit.caches[0][0][NI // 2] = 1.0                                 # one K row of the image block, layer 0
    _, lg_h = m.generate(ids2, max_new_tokens=1, prefix_cache=hit, **KW)
    assert bool(torch.isfinite(lg_h).all()) and not torch.equal(lg_h[:, 0], lg[:, 0])


def test_rollback_to_a_shorter_common_prefix():
    m = _model()
    ids2, _, _ = _reference_turn2()
    pc, _ = _turn1()
    other = torch.cat([IDS1[:, :5], torch.tensor([[21, 22, 23, 24, 25, 26]])], 1)      # shares <s>, the image and 3 tokens
    _, lg = m.generate(other, max_new_tokens=3, prefix_cache=pc, **KW)
    assert pc.last_reused == 1 + 144 + 3 and pc.last_prefilled == 6 and pc.length == 1 + NI + 9 + 2
    gap = rel(lg[:, 0], _uncached(other)[:, 0])
    _, lg2 = m.generate(ids2, max_new_tokens=1, prefix_cache=pc, **KW)
    assert pc.last_reused == 1 + 144 + 3 and pc.length == ids2.shape[1] - 1 + NI
    gap2 = rel(lg2[:, 0], _uncached(ids2)[:, 0])
    print(f"rollback: step 0 against the uncached generate {gap:.3e}, and back on the first conversation {gap2:.3e} (allowed 1e-2)")
    assert gap < 1e-2 and gap2 < 1e-2


def test_the_image_is_encoded_once(monkeypatch):
    m = _model()
    ids2_ref, _, _ = _reference_turn2()
    want = _uncached(ids2_ref)[:, 0]                                              # before the counter is installed
    calls = []
    real = m.encode_image
    monkeypatch.setattr(m, "encode_image", lambda *a, **k: calls.append(1) or real(*a, **k))
    pc, tok1 = _turn1()
    assert len(calls) == 1 and torch.equal(pc.pixels, _M["rgb"]) and pc.image_embedding.shape == (1, NI, 4096)
    ids2 = _ids2(tok1)
    assert torch.equal(ids2, ids2_ref)
    _, lg_none = m.generate(ids2, images=None, max_new_tokens=1, prefix_cache=pc, **KW)
    assert len(calls) == 1 and pc.last_reused == 144 + 8 + 3
    _, lg_same = m.generate(ids2, images=_M["rgb"].clone(), max_new_tokens=1, prefix_cache=pc, **KW)
    assert len(calls) == 1 and pc.last_reused == ids2.shape[1] - 1 + NI - 1       # the same prompt again: all but one position
    assert rel(lg_none[:, 0], want) < 1e-2 and rel(lg_same[:, 0], want) < 1e-2
    rgb2 = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(6))
    m.generate(ids2, images=rgb2, max_new_tokens=1, prefix_cache=pc, **KW)
    assert len(calls) == 2 and pc.last_reused == 1 and torch.equal(pc.pixels, rgb2)


def test_the_e4m3_cache_behind_a_context_is_exact_by_construction():
    m = _model()
    pc8, tok1 = _turn1("fp8")
    ids2 = _ids2(tok1)
    n, H = pc8.length, m.text.heads
    pc16 = m.new_prefix_cache("bf16", MAXP)
    pc16.ids, pc16.length, pc16.image_embedding, pc16.pixels = list(pc8.ids), n, pc8.image_embedding, pc8.pixels
    pc16.caches = generation.alloc_kv(m.text, MAXP, "bf16")
    for (K, V), (kc, vc, ks, vs) in zip(pc16.caches, pc8.caches):
        for dst, codes, sc in ((K, kc, ks), (V, vc, vs)):
            dst.zero_()
            dst[:n] = kv.dequant(codes[:n].cpu().reshape(n, H, kv.D), sc[:n].cpu()).to(BF).reshape(n, -1).to(DEV)
    tok8, lg8 = m.generate(ids2, max_new_tokens=5, prefix_cache=pc8, **KW)
    tok16, lg16 = m.generate(ids2, max_new_tokens=5, prefix_cache=pc16, **KW)
    reuse, S0 = pc8.last_reused, ids2.shape[1] - 1 + NI
    assert reuse == pc16.last_reused == 144 + 8 + 3
    assert torch.equal(lg8[:, 0], lg16[:, 0]) and torch.equal(tok8[:, 0], tok16[:, 0])          # same kernels, same values
    for (K, V), (kc, vc, ks, vs) in zip(pc16.caches, pc8.caches):
        for src, codes, sc in ((K, kc, ks), (V, vc, vs)):
            want_c, want_s = kv.quant(src[reuse:S0].cpu().reshape(S0 - reuse, H, kv.D))
            assert torch.equal(codes[reuse:S0].cpu(), want_c.reshape(S0 - reuse, -1)) and torch.equal(sc[reuse:S0].cpu(), want_s)
    assert bool(torch.isfinite(lg8).all()) and not torch.equal(lg8[:, 1], lg16[:, 1])           # the step reads the codes
    print(f"fp8 cache behind a context: step 1 against the bf16 cache holding the dequantised prefix {rel(lg8[:, 1], lg16[:, 1]):.3e}")


def _two_turns(kv_cache, **kw):
    pc, tok1 = _turn1(kv_cache, **kw)
    out = _model().generate(_ids2(tok1), max_new_tokens=5, prefix_cache=pc, **{**KW, **kw})
    return pc, tok1, out


def test_composition_and_reproducibility():
    _, a1, (a_tok, a_lg) = _two_turns("fp8")
    _, b1, (b_tok, b_lg) = _two_turns("fp8")
    _, c1, (c_tok, c_lg) = _two_turns("fp8", use_graph=False)
    assert torch.equal(a1, b1) and torch.equal(a_tok, b_tok) and torch.equal(a_lg, b_lg)
    assert torch.equal(a1, c1) and torch.equal(a_tok, c_tok) and torch.equal(a_lg, c_lg)
    pc, _, (w_tok, w_lg) = _two_turns("bf16", weights="fp8")
    assert bool(torch.isfinite(w_lg).all()) and w_tok.shape == (1, 5) and pc.last_reused == 144 + 8 + 3
    draw = dict(do_sample=True, sampler="device", seed=3, return_logits=False)
    m = _model()
    runs = []
    for _ in range(2):
        pc = m.new_prefix_cache("fp8", MAXP)
        t1 = m.generate(IDS1, images=_M["rgb"], max_new_tokens=4, prefix_cache=pc, eos_token_id=None, **draw)
        t2 = m.generate(_ids2(t1), max_new_tokens=5, prefix_cache=pc, eos_token_id=None, **draw)
        assert pc.last_reused == 144 + 8 + 3
        runs.append((t1, t2))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_rejections_leave_the_cache_usable():
    m = _model()
    ids2, tok, lg = _reference_turn2()
    pc, _ = _turn1()
    rgb = _M["rgb"]
    state = (list(pc.ids), pc.length, pc.image_embedding, pc.pixels, [t.clone() for layer in pc.caches for t in layer])
    kw = dict(max_new_tokens=5, prefix_cache=pc, **KW)
    mask = torch.ones_like(ids2)
    mask[0, 3] = 0
    two = torch.cat([ids2, torch.tensor([[-200, 5]])], 1)
    foreign = TextModal(device=DEV, layers=0).new_prefix_cache("bf16", MAXP)
    for what, match, call in (
            ("batch 2", r"batch 1, got input_ids of shape \(2, ", lambda: m.generate(ids2.repeat(2, 1), images=rgb.repeat(2, 1, 1, 1), **kw)),
            ("beams", "num_beams=2", lambda: m.generate(ids2, images=rgb, num_beams=2, **kw)),
            ("mask", "hides 1 positions", lambda: m.generate(ids2, images=rgb, attention_mask=mask, **kw)),
            ("placeholders", "2 <image> placeholders", lambda: m.generate(two, images=rgb, **kw)),
            ("kind", "kv_cache='fp8' disagrees .* kv_cache='bf16'", lambda: m.generate(ids2, images=rgb, kv_cache="fp8", **kw)),
            ("model", "another model", lambda: m.generate(ids2, images=rgb, **{**kw, "prefix_cache": foreign})),
            ("length", rf"max_new_tokens \(200\) exceeds the {MAXP} positions", lambda: m.generate(ids2, images=rgb, **{**kw, "max_new_tokens": 200})),
            ("length, text level", r"max_new_tokens \(200\)", lambda: m.text.generate(ids2, **{**kw, "max_new_tokens": 200}))):
        with pytest.raises(ValueError, match=match):
            call()
        now = [t for layer in pc.caches for t in layer]
        assert (pc.ids, pc.length) == state[:2] and pc.image_embedding is state[2] and pc.pixels is state[3], what
        # bit for bit: the rows past `length` are whatever torch.empty found there, NaN patterns included (NaN != NaN under torch.equal)
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(now, state[4])), what
    assert foreign.caches is None and foreign.length == 0
    tok_v, lg_v = m.generate(ids2, images=rgb, **kw)
    assert torch.equal(lg_v, lg) and torch.equal(tok_v, tok)


# ------------------------------------------------------------------------------------------------------------------------- 3. cli_qa.py
def test_cli_qa_prefix_cache_flag(monkeypatch, capsys, tmp_path):
    """two turns of the chat loop with --prefix-cache: one cache object for the conversation, the image encoded once, the second turn
    reuses at least the whole first prompt; with beams the flag is rejected before the model is built"""
    import builtins

    import numpy as np
    import transformers
    from PIL import Image

    import cli_qa
    import lhrs_bot_amd.unibind as U
    from test_cli_qa_gpu import ToyTok

    with pytest.raises(ValueError, match="--prefix-cache with --num-beams"):
        cli_qa.main(cli_qa.parse_option(["--prefix-cache", "--num-beams", "2", "--llama-layers", "2"]))
    img = tmp_path / "tile.png"
    Image.fromarray(np.random.default_rng(0).integers(0, 256, (300, 260, 3), dtype=np.uint8)).save(img)
    tok = ToyTok()
    monkeypatch.setattr(transformers.AutoTokenizer, "from_pretrained", staticmethod(lambda *a, **k: tok))
    turns = iter(["what is in this image ?", "and how many ?", ""])
    monkeypatch.setattr(builtins, "input", lambda prompt="": next(turns))
    seen, encoded = [], []
    orig, enc = U.UniBind.generate, U.UniBind.encode_image

    def spy(self, input_ids, **kw):
        out = orig(self, input_ids, **kw)
        seen.append((input_ids.shape[1], kw["prefix_cache"], kw["prefix_cache"].last_reused, kw["prefix_cache"].last_prefilled))
        return out

    monkeypatch.setattr(U.UniBind, "generate", spy)
    monkeypatch.setattr(U.UniBind, "encode_image", lambda self, *a, **k: encoded.append(1) or enc(self, *a, **k))
    cli_qa.main(cli_qa.parse_option(["--image-file", str(img), "--tokenizer-path", "unused", "--max-new-tokens", "6", "--llama-layers", "2",
                                     "--prefix-cache", "--kv-cache", "fp8"]))
    text = capsys.readouterr().out
    assert text.count("ASSISTANT: ") == 2 and "exit..." in text
    (T1, pc1, reused1, filled1), (T2, pc2, reused2, filled2) = seen
    assert pc1 is pc2 and pc1.kv_cache == "fp8" and len(encoded) == 1
    assert (reused1, filled1) == (0, T1 - 1 + NI)
    assert reused2 >= T1 - 1 + NI and reused2 + filled2 == T2 - 1 + NI
