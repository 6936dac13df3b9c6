"""Decode from MXFP4 weights (csrc/gemv_mx4.hip behind hk.quant_mx4_rows / dequant_mx4_rows / repack_mx4_mfma / gemv_mx4 / gemv_mx4_fused,
TextModal.pack_mx4_decode, generate(weights="mxfp4")) on an MI355X, against the restatement of tests/mx4_cases.py.

Format: codes, scales, dequantised weights and both tiled buffers byte for byte, operands in padded buffers with a NaN / 0xFF surround,
outputs inside sentinel-filled buffers that must come back untouched outside the result.
Operand map: one-hot e4m3 activations make every output a single product plus zeros - exact whatever the instruction truncates - so
y[b][n] == 1.5 * dequant[n][k_b] pins the nibble order, the lane <-> block map, the scale byte and its op_sel, the wave split and the row guard.
Arithmetic: every case of mx4_cases.CASES against float64 inside the derived bound of that module (c = 2); the worst ratios at c = 1 are
printed by the last test and recorded in DESIGN.md "Decode from MXFP4 weights".
Model: on a model whose decoder linears ARE MXFP4 values, weights="mxfp4" multiplies the weights weights="bf16" multiplies; what differs is
the e4m3 activations and the MFMA's truncation, which weights="fp8" has too (plus an e4m3 weight error): the first decode step may be at
most 1.5 x as far from bf16 as fp8 is, measured in the same test."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from lhrs_bot_amd import _lib  # noqa: E402
from lhrs_bot_amd import kernels as hk  # noqa: E402
from lhrs_bot_amd.engine import LHRSEngine  # noqa: E402
from lhrs_bot_amd.text import TextModal  # noqa: E402
from lhrs_bot_amd.unibind import UniBind  # noqa: E402

import mx4_cases as mx  # noqa: E402

DEV = "cuda"
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
_INT = {BF: torch.int16, F32: torch.int32, U8: torch.uint8}
_SENT = {BF: -1, F32: -1, U8: 0xA5}


def padded(t, pad, fill, rows_after=1):
    """[rows, cols] -> the same values as the top-left view of a [rows + rows_after, cols + pad] device buffer that holds `fill` elsewhere"""
    rows, cols = t.shape
    buf = torch.full((rows + rows_after, cols + pad), fill, dtype=t.dtype)
    buf[:rows, :cols] = t
    return buf.to(DEV)[:rows, :cols]


def nanvec(t, pad=8):
    buf = torch.full((t.numel() + pad,), float("nan"), dtype=t.dtype)
    buf[:t.numel()] = t
    return buf.to(DEV)[:t.numel()]


def sent_buf(rows, cols, dtype, pad, extra=3):
    buf = torch.full((rows + extra, cols + pad), _SENT[dtype], dtype=_INT[dtype], device=DEV).view(dtype)
    return buf, buf[:rows, :cols]


def untouched(buf, view, what):
    b = buf.view(_INT[buf.dtype])
    mark = torch.zeros(b.shape, dtype=torch.bool, device=DEV)
    mark[:view.shape[0], :view.shape[1]] = True
    assert bool((b[~mark] == _SENT[buf.dtype]).all()), f"{what}: an element outside the result was written"


def sent_flat(n, lead=64, tail=96):
    """n bytes inside a flat 0xA5 buffer, 16-byte aligned"""
    buf = torch.full((lead + n + tail,), 0xA5, dtype=U8, device=DEV)
    return buf, buf[lead:lead + n]


def flat_untouched(buf, n, what, lead=64):
    assert bool((buf[:lead] == 0xA5).all()) and bool((buf[lead + n:] == 0xA5).all()), f"{what}: a byte outside the result was written"


def packed(codes, scales):
    """host row-major (codes, scales) -> PackedMX4 on the device"""
    return hk.repack_mx4_mfma(codes.to(DEV), scales.to(DEV))


# ------------------------------------------------------------------------------------------------------------------------- 1. format
def _format_roundtrip(W, name):
    """W: host bf16 [N, K].  quantise, dequantise, re-tile on the device; every buffer byte for byte against the restatement"""
    N, K = W.shape
    want_c, want_s = mx.quant(W)
    Wp = padded(W, 8, float("nan"))                               # NaN columns past K and a NaN row after N - 1
    cbuf, codes = sent_buf(N, K // 2, U8, 16)
    sbuf, scales = sent_buf(N, K // 32, U8, 3)
    hk.quant_mx4_rows(Wp, out=(codes, scales))
    untouched(cbuf, codes, name + " codes")
    untouched(sbuf, scales, name + " scales")
    assert torch.equal(scales.cpu(), want_s), name
    assert torch.equal(codes.cpu(), want_c), name
    # dequantise from padded operands (0xFF codes / scale bytes around them)
    cp, sp = padded(want_c, 16, 0xFF), padded(want_s, 5, 0xFF)
    wbuf, Wd = sent_buf(N, K, BF, 8)
    hk.dequant_mx4_rows(cp, sp, out=Wd)
    untouched(wbuf, Wd, name + " dequant")
    want_d = mx.dequant(want_c, want_s)
    assert torch.equal(Wd.cpu().view(torch.int16), want_d.to(BF).view(torch.int16)), name     # bit patterns: signed zeros included
    if K % 128 == 0:
        want_ct, want_st = mx.tile(want_c, want_s, N, K)
        b1, ct = sent_flat(want_ct.numel())
        b2, st = sent_flat(want_st.numel())
        P = hk.repack_mx4_mfma(cp, sp, out=(ct, st))
        flat_untouched(b1, want_ct.numel(), name + " codes_t")
        flat_untouched(b2, want_st.numel(), name + " scales_t")
        assert torch.equal(P.codes_t.cpu().reshape(-1), want_ct.reshape(-1)), name
        assert torch.equal(P.scales_t.cpu().reshape(-1), want_st.reshape(-1)), name
        assert P.shape == (N, K) and P.nbytes() == want_ct.numel() + want_st.numel()


@pytest.mark.parametrize("K", [128, 640, 11008])
@pytest.mark.parametrize("N", [16, 24, 40])
def test_quant_dequant_repack_bit_exact(N, K):
    _format_roundtrip(mx.weight(N, K, seed=N * 7 + K), f"N{N} K{K}")


def test_quant_dequant_repack_bit_exact_on_planted_blocks():
    """a zero block, an outlier 2^10 above the rest, values near 2^-120, exact ties, the saturating range, a negative value that rounds to
    zero, bf16 subnormals (byte 0) and the largest finite bf16 (byte 252): tests/mx4_cases.py `planted`"""
    _format_roundtrip(mx.planted(), "planted")


# ------------------------------------------------------------------------------------------------------------------------- 2. operand map
E4_1P5 = 0x3C                                                      # e4m3 1.5: exponent field 7, mantissa 100


def _one_hot_sweep(K, ks):
    N = 24
    g = torch.Generator().manual_seed(K)
    codes = torch.randint(0, 256, (N, K // 2), generator=g).to(U8)
    scales = torch.randint(120, 135, (N, K // 32), generator=g).to(U8)
    assert bool((scales[:, 1:] != scales[:, :-1]).any(1).all())
    W = packed(codes, scales)
    Wd = mx.dequant(codes, scales)                                  # float64 [N, K]
    assert torch.equal(hk.dequant_mx4_rows(codes.to(DEV), scales.to(DEV)).cpu().double(), Wd)
    ones = torch.ones(16, device=DEV, dtype=F32)
    ks = torch.tensor(ks)
    ks = torch.cat([ks, ks[: (-len(ks)) % 16]])                      # a whole number of batches of 16
    for i in range(0, len(ks), 16):
        kb = ks[i:i + 16]
        x8 = torch.zeros((16, K), dtype=U8)
        x8[torch.arange(16), kb] = E4_1P5
        y = torch.full((16, N), float("nan"), device=DEV, dtype=F32)
        hk.gemv_mx4(W, x8.to(DEV), ones, y, out_f32=True)
        want = 1.5 * Wd[:, kb].t()                                  # a single product plus zeros: exact (compared as values: -0 == +0)
        got = y.cpu().double()
        assert torch.equal(got, want), (K, kb[(got != want).any(1)].tolist())


def test_one_hot_activations_return_the_dequantised_column_exactly_K640():
    """every k of five steps: crosses a scale-dword boundary and leaves a partial dword"""
    _one_hot_sweep(640, list(range(640)))


def test_one_hot_activations_return_the_dequantised_column_exactly_K11008():
    """every 32nd k and its two neighbours: every block boundary of the uneven wave split (7 x 12 + 2 steps)"""
    K = 11008
    _one_hot_sweep(K, sorted({k for b in range(0, K, 32) for k in (b - 1, b, b + 1) if 0 <= k < K}))


# ------------------------------------------------------------------------------------------------------------------------- 3. arithmetic
def _run(c):
    i = mx.inputs(c)
    s = c.K >= 512                                                 # strided operands wherever a row is long enough to matter
    W = packed(i["codes"], i["scales"])
    res = None if i["res"] is None else padded(i["res"], 8 if s else 0, float("nan"))
    buf, y = sent_buf(c.B, c.N, F32 if c.f32 else BF, 24 if s else 0)
    if c.op == "x8":
        x8 = padded(i["x8"], 16 if s else 0, 0xFF)
        hk.gemv_mx4(W, x8, nanvec(i["xscale"]), y, residual=res, out_f32=c.f32)
    else:
        x = padded(i["x"], 16 if s else 0, float("nan"))
        hk.gemv_mx4_fused(W, x, y, c.K, prologue=c.pro, norm_w=nanvec(i["norm_w"]), eps=mx.EPS, residual=res, out_f32=c.f32)
    untouched(buf, y, c.name)
    return y


@pytest.mark.parametrize("c", mx.CASES, ids=[c.name.replace(" ", "_") for c in mx.CASES])
def test_gemv_mx4_case_vs_fp64(c):
    ref, act, _ = mx.case_reference(c)
    if c.op == "fused":
        assert mx.marked_fraction(act) < mx.MARKED_MAX
    y = _run(c)
    what = ("gemv_mx4" if c.op == "x8" else "gemv_mx4_fused") + (" f32" if c.f32 else " bf16")
    r = mx.ratio(y, ref)
    print(f"{c.name}: {r:.4f} x the bound at c = 1")
    mx.check(y, ref, what, c.name)


# ------------------------------------------------------------------------------------------------------------------------- 4. model
NL = 2
_M = {}


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _inputs(B, seed=5):
    g = torch.Generator().manual_seed(seed)
    ids_ = torch.tensor([[1, -200, 9, 8, 7, 6]]).repeat(B, 1)
    if B > 1:
        ids_[1:, 2:] = torch.randint(3, 32000, (B - 1, 4), generator=g)
    return ids_, torch.randn(B, 3, 224, 224, generator=g)


def _to_mx(m):
    """every decoder linear <- dequant(quant(W)): from here on the bf16 weights ARE MXFP4 values"""
    for L in m.text.p["layers"]:
        m.text._drop_derived(L)
        for k in ("qkv_w", "o_w", "gu_w", "down_w"):
            hk.dequant_mx4_rows(*hk.quant_mx4_rows(L[k]), out=L[k])
            L[k + "T"] = hk.transpose(L[k])
    return m


def _models():
    """(the original model, the mx model): the same random parameters, built once per module"""
    if not _M:
        _M["orig"] = UniBind(("rgb", "text"), None, device=DEV, llama_layers=NL).init_random(seed=1).eval()
        _M["mx"] = _to_mx(UniBind(("rgb", "text"), None, device=DEV, llama_layers=NL).init_random(seed=1).eval())
    return _M["orig"], _M["mx"]


KW = dict(do_sample=False, max_new_tokens=5, return_logits=True, eos_token_id=None)


def _first_step_gaps(m, B, **extra):
    ids_, rgb = _inputs(B)
    out = {w: m.generate(ids_, images=rgb, weights=w, **KW, **extra) for w in ("bf16", "fp8", "mxfp4")}
    (tok_bf, lg_bf), (_, lg_8), (tok_mx, lg_mx) = out["bf16"], out["fp8"], out["mxfp4"]
    assert torch.equal(lg_mx[:, 0], lg_bf[:, 0]) and torch.equal(lg_8[:, 0], lg_bf[:, 0])     # the prefill is the bf16 GEMM path in all modes
    assert torch.equal(tok_mx[:, 0], tok_bf[:, 0])
    assert bool(torch.isfinite(lg_mx).all()) and tok_mx.shape == (B, 5)
    return rel(lg_mx[:, 1], lg_bf[:, 1]), rel(lg_8[:, 1], lg_bf[:, 1]), lg_bf


@pytest.mark.parametrize("B", [1, 3])
def test_mxfp4_first_decode_step_is_no_further_from_bf16_than_fp8(B):
    """B 1: the fused kernel; B 3: rmsnorm_fwd_q / swiglu_fwd_q / quant_fp8_rows + the x8 kernel"""
    orig, m = _models()
    gap_mx, gap_8, lg_bf = _first_step_gaps(m, B)
    ids_, rgb = _inputs(B)
    _, lg_orig = orig.generate(ids_, images=rgb, **KW)
    print(f"batch {B}, step-1 logits, rel-L2 against bf16 on the mx model: mxfp4 {gap_mx:.3e}, fp8 {gap_8:.3e}, ratio {gap_mx / max(gap_8, 1e-30):.2f}; "
          f"the format's own loss (mx model against the original model, both bf16): {rel(lg_bf[:, 1], lg_orig[:, 1]):.3e}")
    assert gap_8 > 0 and gap_mx <= 1.5 * gap_8, (gap_mx, gap_8)
    L = m.text.p["layers"][0]
    assert isinstance(L["qkv_wmx4"], hk.PackedMX4) and L["qkv_wmx4"].shape == tuple(L["qkv_w"].shape)


def test_mxfp4_with_live_adapters():
    """r = 8 on q, k, v, o with non-zero B: the base GEMV writes fp32 s.acc without a residual, lora_up adds adapter and residual"""
    _, m = _models()
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
            gap_mx, gap_8, _ = _first_step_gaps(m, B, adapters="live")
            print(f"live adapters, batch {B}, step-1 logits, rel-L2 against bf16: mxfp4 {gap_mx:.3e}, fp8 {gap_8:.3e}, ratio {gap_mx / max(gap_8, 1e-30):.2f}")
            assert gap_8 > 0 and gap_mx <= 1.5 * gap_8, (B, gap_mx, gap_8)
    finally:
        m.text.lora, m.text._merged_cache = None, None


# ------------------------------------------------------------------------------------------------------------------------- 5. surface
def test_mxfp4_is_bit_reproducible_and_packs_once():
    _, m = _models()
    ids_, rgb = _inputs(1)
    a_ids, a_lg = m.generate(ids_, images=rgb, weights="mxfp4", **KW)
    held = [L[k + "mx4"] for L in m.text.p["layers"] for k in ("qkv_w", "o_w", "gu_w", "down_w")]
    b_ids, b_lg = m.generate(ids_, images=rgb, weights="mxfp4", **KW)
    assert torch.equal(a_ids, b_ids) and torch.equal(a_lg, b_lg)
    assert all(h is L[k + "mx4"] for h, (L, k) in zip(held, ((L, k) for L in m.text.p["layers"] for k in ("qkv_w", "o_w", "gu_w", "down_w"))))
    c_ids, c_lg = m.generate(ids_, images=rgb, weights="mxfp4", use_graph=False, **KW)
    assert torch.equal(a_ids, c_ids) and torch.equal(a_lg, c_lg)
    names = {k + "mx4" for k in ("qkv_w", "o_w", "gu_w", "down_w")}
    assert names <= set(m.text.p["layers"][0]) and "mx4" in TextModal.DERIVED_SUFFIXES and names <= LHRSEngine.DERIVED_KEYS
    # lm_head has no MXFP4 form: nothing under an mx4 name at the top level
    assert not any("mx4" in k for k in m.text.p if isinstance(k, str))


def test_quantize_base_drops_the_tiled_copies_and_unknown_modes_raise():
    m = UniBind(("rgb", "text"), None, device=DEV, llama_layers=NL).init_random(seed=1).eval()
    ids_, rgb = _inputs(1)
    kw = dict(do_sample=False, max_new_tokens=2, eos_token_id=None)
    m.generate(ids_, images=rgb, weights="mxfp4", **kw)
    L = m.text.p["layers"][0]
    old = L["o_wmx4"]
    m.text.quantize_base(4)
    assert not any(k.endswith("mx4") for Lr in m.text.p["layers"] for k in Lr)
    m.generate(ids_, images=rgb, weights="mxfp4", **kw)          # rebuilt from the (now NF4-valued) weights
    assert L["o_wmx4"] is not old and not torch.equal(L["o_wmx4"].codes_t, old.codes_t)
    with pytest.raises(ValueError, match="mxfp4"):
        m.generate(ids_, images=rgb, weights="fp4", **kw)


def test_rejections():
    """the operands are complete and of full size: were a call accepted it would run inside its buffers"""
    N, K = 16, 192                                                 # K % 32 == 0 but K % 128 != 0
    codes = torch.zeros((N, 128), device=DEV, dtype=U8)
    scales = torch.full((N, 8), 127, device=DEV, dtype=U8)
    ct = torch.zeros(2 * 1024, device=DEV, dtype=U8)
    st = torch.zeros(256, device=DEV, dtype=U8)
    x8 = torch.zeros((2, 256), device=DEV, dtype=U8)
    x = torch.zeros((2, 512), device=DEV, dtype=BF)
    xs = torch.ones(16, device=DEV, dtype=F32)
    y = torch.zeros((2, N), device=DEV, dtype=BF)
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    calls = {
        "repack_mx4_mfma": lambda: lib.lhrs_repack_mx4_mfma(codes.data_ptr(), 128, scales.data_ptr(), 8, ct.data_ptr(), st.data_ptr(), N, K, s),
        "gemv_mx4": lambda: lib.lhrs_gemv_mx4(ct.data_ptr(), st.data_ptr(), x8.data_ptr(), 256, xs.data_ptr(), None, 0, y.data_ptr(), N, 2, N, K, 0, s),
        "gemv_mx4_fused": lambda: lib.lhrs_gemv_mx4_fused(ct.data_ptr(), st.data_ptr(), x.data_ptr(), 512, 0, None, 1e-5, None, 0, y.data_ptr(), N, 2, N, K, 0, s),
        "gemv_mx4 B17": lambda: lib.lhrs_gemv_mx4(ct.data_ptr(), st.data_ptr(), x8.data_ptr(), 256, xs.data_ptr(), None, 0, y.data_ptr(), N, 17, N, 128, 0, s),
        "gemv_mx4_fused B3": lambda: lib.lhrs_gemv_mx4_fused(ct.data_ptr(), st.data_ptr(), x.data_ptr(), 512, 0, None, 1e-5, None, 0, y.data_ptr(), N, 3, N, 128, 0, s),
        "gemv_mx4 misaligned": lambda: lib.lhrs_gemv_mx4(ct.data_ptr() + 8, st.data_ptr(), x8.data_ptr(), 256, xs.data_ptr(), None, 0, y.data_ptr(), N, 2, N, 128, 0, s),
        "quant_mx4_rows K48": lambda: lib.lhrs_quant_mx4_rows(x.data_ptr(), 512, codes.data_ptr(), 128, scales.data_ptr(), 8, 2, 48, s),
    }
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match="rejected by liblhrs_hip"):
            _lib.check(call(), name)
    with pytest.raises(RuntimeError, match="rejected by liblhrs_hip"):      # the same through the public wrapper
        hk.gemv_mx4(hk.PackedMX4(ct, st, N, K), x8[:, :K], xs, y)
    torch.cuda.synchronize()
    assert not bool(y.any()) and not bool(ct.any())


def test_worst_ratios_seen_on_the_device():
    """last in the file: what the comparisons above saw per entry point and output type, at c = 1 (allowed: c = 2)"""
    for k in sorted(mx.WORST):
        print(f"WORST {k:22s} {mx.WORST[k]:.4f}")
