"""Decode from the 4-bit base (csrc/gemv4.hip behind hk.gemv4, TextModal.pack4_decode, generate(weights="4bit")) on an MI355X.

Kernels: every case of tests/gemv4_cases.py through hk.gemv4 against the float64 reference on the oracle's dequantised bf16 weight, element by
element.  Operands lie in padded buffers: NaN in the activation columns past K and in the row after the batch, NaN block statistics past a row's
K / 64 and in the row after N - 1, a row of 0xFF codes after row N - 1; every output lies inside a larger buffer prefilled with a NaN bit
pattern that must come back unchanged outside [B, N].

Exactness: one-hot activations make every output a single product plus zeros, exact in any summation order - the result must be the column
of hk.dequant4_blocks times the activation value, which pins the nibble order, the absmax index and the bf16 rounding of the weight without
any tolerance.  (Compared as values: a sum of zeros is +0 where the dequantised weight may hold -0.)

Model: generate(weights="4bit") against weights="bf16" on the same 4-bit model.  The decoder linears of both multiply the same bf16 weights, so
the two differ by the order of fp32 sums only; the bound on that gap is measured in the same test on the existing code's own two orders (g:
batch 1 on the VALU kernel against the same prompt at batch 2 on the MFMA kernel), and the 4-bit path may differ from bf16 batch 1 by 4 g (two
reordered kernels in a row instead of one).  Measured on an MI355X: see DESIGN.md "Decode from the 4-bit base"."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from lhrs_bot_amd import _lib  # noqa: E402
from lhrs_bot_amd import kernels as hk  # noqa: E402
from lhrs_bot_amd.engine import LHRSEngine  # noqa: E402
from lhrs_bot_amd.text import TextModal  # noqa: E402
from lhrs_bot_amd.unibind import UniBind  # noqa: E402
from oracle import params as OP  # noqa: E402

import gemv4_cases as g4  # noqa: E402

DEV = "cuda"
SENT = -1
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
_INT = {BF: torch.int16, F32: torch.int32}


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
    buf = torch.full((rows + extra, cols + pad), SENT, dtype=_INT[dtype], device=DEV).view(dtype)
    return buf, buf[:rows, :cols]


def untouched(buf, view, what):
    b = buf.view(_INT[buf.dtype])
    mark = torch.zeros(b.shape, dtype=torch.bool, device=DEV)
    mark[:view.shape[0], :view.shape[1]] = True
    assert bool((b[~mark] == SENT).all()), f"{what}: an element outside the result was written"


class Operands:
    def __init__(self, c):
        i, o = g4.inputs(c), c.opt
        s = o["strided"]
        self.c, self.B, self.N, self.K = c, o["B"], o["N"], o["K"]
        self.W4 = hk.Packed4(padded(i["codes"], 16 if s else 0, 0xFF), padded(i["absmax"], 3 if s else 0, float("nan")), o["fp4"], self.N, self.K)
        self.x = padded(i["x"], 16 if s else 0, float("nan"))
        self.res = None if i["res"] is None else padded(i["res"], 8 if s else 0, float("nan"))
        self.norm_w = nanvec(i["norm_w"])
        self.f32, self.pad = o["f32"], 24 if s else 0

    def run(self):
        buf, y = sent_buf(self.B, self.N, F32 if self.f32 else BF, self.pad)
        hk.gemv4(self.W4, self.x, y, self.K, prologue=self.c.opt["pro"], norm_w=self.norm_w, eps=g4.EPS, residual=self.res, out_f32=self.f32)
        untouched(buf, y, self.c.name)
        return y


def ids(cases):
    return [c.name.replace(" ", "_") for c in cases]


@pytest.mark.parametrize("c", g4.CASES, ids=ids(g4.CASES))
def test_gemv4_case_vs_fp64(c):
    ref, _ = g4.reference(c)
    y = Operands(c).run()
    rep = g4.measure(g4.kind_of(c), y, ref, "gemv4", c.name)
    print(f"{c.name}: {rep.unit:.3g} at c = 1 ({g4.plan(c.opt['B'], c.opt['N'], c.opt['K'], c.opt['pro'])})")
    g4.check(g4.kind_of(c), y, ref, "gemv4", c.name)


@pytest.mark.parametrize("name", sorted(g4.REJECTS))
def test_gemv4_rejections(name):
    """the operands are complete and of full size: were a call accepted it would run inside its buffers"""
    o = g4.REJECTS[name]
    B, N, K = o["B"], o["N"], o["K"]
    Kp = -(-K // 64) * 64
    codes = torch.zeros((N, max(Kp // 2, o.get("ldc", 0))), device=DEV, dtype=U8)
    absmax = torch.ones((N, Kp // 64), device=DEV, dtype=F32)
    x = torch.zeros((B, Kp), device=DEV, dtype=BF)
    y = torch.zeros((B, N), device=DEV, dtype=BF)
    st = _lib.load().lhrs_gemv4(codes.data_ptr(), o.get("ldc", codes.stride(0)), absmax.data_ptr() if o.get("absmax", True) else None, absmax.stride(0), 0,
                                x.data_ptr(), x.stride(0), 0, None, g4.EPS, None, 0, y.data_ptr(), y.stride(0), B, N, K, 0,
                                torch.cuda.current_stream().cuda_stream)
    with pytest.raises(RuntimeError, match="rejected by liblhrs_hip"):
        _lib.check(st, "gemv4")
    with pytest.raises(g4.Rejected):
        g4.plan(B, N, K, 0, o.get("absmax", True), o.get("ldc"))
    assert not bool(y.any())


# ------------------------------------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("quant_type", ["nf4", "fp4"])
@pytest.mark.parametrize("K", [128, 704, 1152])
def test_one_hot_rows_return_the_dequantised_column_exactly(quant_type, K):
    """K 128 and 1152: the 16 rows at once on the MFMA kernel (one and nine steps) and one at a time on the VALU kernel.  K 704 is no multiple
    of 128, so no batch of it reaches the MFMA kernel: there the 16 rows go as two batches of 8 through the VALU kernel, and one at a time."""
    N = 35
    g = torch.Generator().manual_seed(K)
    st = hk.quant4_blocks(g4.weight(N, K, seed=7 + K).to(DEV), quant_type, True)
    Wd = hk.dequant4_blocks(st).float()                                     # [N, K]: the bits every bf16 product of the 4-bit model reads
    W4 = hk.pack4_decode([st], N, K)
    ks = [0, 1, 62, 63, 64, 65, K - 2, K - 1] + torch.randint(0, K, (8,), generator=g).tolist()
    for v in (1.0, 2.0 ** -3):
        x = torch.zeros((16, K), device=DEV, dtype=BF)
        x[torch.arange(16), torch.tensor(ks)] = v
        want = Wd[:, ks].t() * v                                            # a bf16 value times a power of two: exact in fp32 and in bf16
        for out_f32 in (True, False):
            dt = F32 if out_f32 else BF
            groups = [slice(0, 16)] if K % 128 == 0 else [slice(0, 8), slice(8, 16)]
            for sl in groups + [slice(b, b + 1) for b in range(16)]:
                y = torch.full((sl.stop - sl.start, N), float("nan"), device=DEV, dtype=dt)
                hk.gemv4(W4, x[sl], y, K, out_f32=out_f32)
                assert torch.equal(y.float(), want[sl]), (quant_type, K, v, out_f32, sl)


# ------------------------------------------------------------------------------------------------------------------------- packing
def test_pack4_decode_concatenates_the_parts_and_gemv4_reads_them():
    """a qkv-like weight of three reference Linears with double_quant statistics of their own"""
    rows, K = 32, 256
    g = torch.Generator().manual_seed(3)
    parts = [g4.weight(rows, K, seed=20 + i).to(DEV) * s for i, s in enumerate((1.0, 4.0, 0.25))]
    states = [hk.quant4_blocks(p.contiguous(), "nf4", True) for p in parts]
    assert all("qabsmax" in st for st in states) and len({st["offset"] for st in states}) == 3
    W4 = hk.pack4_decode(states, 3 * rows, K)
    assert W4.shape == (3 * rows, K) and not W4.fp4 and W4.codes.dtype == U8 and W4.absmax.dtype == F32
    assert torch.equal(W4.codes.reshape(-1), torch.cat([st["packed"] for st in states]))
    assert torch.equal(W4.absmax.reshape(-1), torch.cat([hk.absmax_of(st) for st in states]))
    Wq = torch.cat([hk.dequant4_blocks(st) for st in states]).cpu()         # the fused dequantised weight
    for B in (1, 3):
        x = torch.randn(B, K, generator=g).to(BF)
        res = torch.randn(B, 3 * rows, generator=g).to(BF)
        ref = g4.gc.ref_gemv(g4.gc.ref_prologue(x, 0), Wq, None, res, True)
        y = torch.full((B, 3 * rows), float("nan"), device=DEV, dtype=F32)
        hk.gemv4(W4, x.to(DEV), y, K, residual=res.to(DEV), out_f32=True)
        g4.check("f32_plain", y, ref, "gemv4", f"three parts B={B}")
    with pytest.raises(ValueError, match="rows"):
        hk.pack4_decode(states[:2], 3 * rows, K)
    with pytest.raises(ValueError, match="K="):
        hk.gemv4(W4, x.to(DEV), y, K // 2)
    with pytest.raises(TypeError, match="gemv4 out"):          # a bf16 buffer must not be written as fp32
        hk.gemv4(W4, x.to(DEV), y.to(BF), K, out_f32=True)
    with pytest.raises(ValueError, match="out"):
        hk.gemv4(W4, x.to(DEV), y[:, :-1], K, out_f32=True)


# ------------------------------------------------------------------------------------------------------------------------- model
NL = 2
_P = {}


def _params():
    if not _P:
        _P.update(vit=OP.make_vit_params(seed=2), pooler=OP.make_pooler_params(seed=1), llama=OP.make_llama_params(seed=3, layers=NL))
    return _P


_MODELS = {}


def _model(quant_type, double_quant):
    """the 4-bit model of a storage format, built once per module"""
    if (quant_type, double_quant) not in _MODELS:
        m = UniBind(("rgb", "text"), None, device=DEV, llama_layers=NL).load_params(_params()).eval()
        m.text.quantize_base(4, quant_type=quant_type, double_quant=double_quant)
        assert m.text.base4 == (quant_type, double_quant)
        _MODELS[(quant_type, double_quant)] = m
    return _MODELS[(quant_type, double_quant)]


@pytest.fixture(params=[("nf4", True), ("fp4", False)], ids=["nf4_dq", "fp4_plain"])
def model4(request):
    return _model(*request.param)


@pytest.fixture
def model_nf4():
    return _model("nf4", True)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _inputs(B, seed=5):
    g = torch.Generator().manual_seed(seed)
    ids_ = torch.tensor([[1, -200, 9, 8, 7, 6]]).repeat(B, 1)
    if B > 1:
        ids_[1:, 2:] = torch.randint(3, 32000, (B - 1, 4), generator=g)
    return ids_, torch.randn(B, 3, 224, 224, generator=g)


def test_4bit_decode_is_the_bf16_decode_up_to_summation_order(model4):
    ids_, rgb = _inputs(1)
    kw = dict(do_sample=False, max_new_tokens=5, return_logits=True, eos_token_id=None)
    tok_bf, lg_bf = model4.generate(ids_, images=rgb, **kw)
    tok_4, lg_4 = model4.generate(ids_, images=rgb, weights="4bit", **kw)
    assert torch.equal(lg_4[:, 0], lg_bf[:, 0])                  # the prefill is the bf16 GEMM path in both
    assert torch.equal(tok_4[:, 0], tok_bf[:, 0])                # so the first decoded step is fed the same token
    # g: the existing code's two bf16 summation orders on this model and step - batch 1 (VALU kernel) against row 0 of the prompt twice (MFMA kernel)
    _, lg_b2 = model4.generate(ids_.repeat(2, 1), images=rgb.repeat(2, 1, 1, 1), **kw)
    g = rel(lg_b2[:1, 1], lg_bf[:, 1])
    gap = rel(lg_4[:, 1], lg_bf[:, 1])
    print(f"step-1 logits, rel-L2: 4bit vs bf16 (both batch 1) {gap:.3e}; bf16 batch 1 vs bf16 batch 2 (g) {g:.3e}; ratio {gap / max(g, 1e-30):.2f}")
    assert g > 0 and gap <= 4 * g, (gap, g)
    L = model4.text.p["layers"][0]
    assert isinstance(L["qkv_w4p"], hk.Packed4) and L["qkv_w4p"].fp4 == (model4.text.base4[0] == "fp4")
    assert "qkv_wp" in L and "lm_headp" in model4.text.p       # the bf16 batch-2 run above made its own tiles; 4bit adds only lm_head's


@pytest.mark.parametrize("B", [1, 3])
def test_4bit_graph_replay_equals_eager_launches(model_nf4, B):
    model4 = model_nf4
    ids_, rgb = _inputs(B)
    kw = dict(do_sample=False, max_new_tokens=6, return_logits=True, eos_token_id=None, weights="4bit")
    a_ids, a_lg = model4.generate(ids_, images=rgb, **kw)
    b_ids, b_lg = model4.generate(ids_, images=rgb, use_graph=False, **kw)
    assert torch.equal(a_ids, b_ids) and torch.equal(a_lg, b_lg)
    assert bool(torch.isfinite(a_lg).all()) and a_ids.shape == (B, 6)


def test_4bit_beam_search_graph_equals_eager(model_nf4):
    model4 = model_nf4
    ids_, rgb = _inputs(1)
    kw = dict(do_sample=False, max_new_tokens=6, eos_token_id=None, weights="4bit", num_beams=2, return_beam_scores=True)
    a_ids, a_sc = model4.generate(ids_, images=rgb, **kw)
    b_ids, b_sc = model4.generate(ids_, images=rgb, use_graph=False, **kw)
    assert torch.equal(a_ids, b_ids) and torch.equal(a_sc, b_sc)


def test_4bit_needs_the_4bit_base_and_merged_adapters():
    m = UniBind(("rgb", "text"), None, device=DEV, llama_layers=NL).init_random(seed=1).eval()
    ids_, rgb = _inputs(1)
    kw = dict(do_sample=False, max_new_tokens=3, return_logits=True, eos_token_id=None)
    with pytest.raises(ValueError, match="quantize_base"):
        m.generate(ids_, images=rgb, weights="4bit", **kw)
    with pytest.raises(ValueError, match="quantize_base"):
        m.text.pack4_decode()
    targets = ("q", "k", "v", "o", "gate", "up", "down")
    lora_p = OP.make_lora_params(seed=4, layers=NL, r=16, alpha=32, targets=targets)
    lora = m.enable_lora(r=16, alpha=32, targets=targets, seed=0)
    for l in range(NL):
        for pr in targets:
            lora.set_adapter(l, pr, *lora_p[l][pr])
    lora.refresh()
    m.text.quantize_base(4, "e4m3", quant_type="nf4", double_quant=True)
    with pytest.raises(ValueError, match="merge_lora"):
        m.generate(ids_, images=rgb, weights="4bit", **kw)
    m.text.lora, saved = None, m.text.lora                      # the base alone decodes from its codes
    m.generate(ids_, images=rgb, weights="4bit", **kw)
    m.text.lora = saved
    L = m.text.p["layers"][0]
    old = L["o_w4p"]
    old_codes = old.codes.clone()
    m.text.merge_lora()                                          # W <- Q4(dequant(W) + s B A): new codes, the packed copies are dropped
    assert m.text.lora is None and m.text.base4 == ("nf4", True) and "o_w4p" not in L
    _, lg_4 = m.generate(ids_, images=rgb, weights="4bit", **kw)
    _, lg_bf = m.generate(ids_, images=rgb, **kw)
    new = L["o_w4p"]
    assert new is not old and new.codes.data_ptr() != old.codes.data_ptr()
    assert torch.equal(new.codes.reshape(-1), torch.cat([st["packed"] for st in L["o_wq4"]]))
    assert torch.equal(new.absmax.reshape(-1), torch.cat([hk.absmax_of(st) for st in L["o_wq4"]]))
    assert not torch.equal(new.codes, old_codes)                 # the merge moved the weights: these are the re-quantised codes
    assert torch.equal(lg_4[:, 0], lg_bf[:, 0]) and bool(torch.isfinite(lg_4).all())


def test_packed_4bit_copies_are_derived_keys(model_nf4, tmp_path):
    model4 = model_nf4
    ids_, rgb = _inputs(1)
    model4.generate(ids_, images=rgb, do_sample=False, max_new_tokens=2, eos_token_id=None, weights="4bit")
    L = model4.text.p["layers"][0]
    names = {k + "4p" for k in ("qkv_w", "o_w", "gu_w", "down_w")}
    assert names <= set(L) and "4p" in TextModal.DERIVED_SUFFIXES and names <= LHRSEngine.DERIVED_KEYS

    def keys(o, pre=""):
        if isinstance(o, dict):
            for k, v in o.items():
                yield from keys(v, f"{pre}{k}.")
        else:
            assert torch.is_tensor(o), (pre, type(o))
            yield pre
    ckpt = model4.custom_save_checkpoint(str(tmp_path / "ckpt"))
    assert not any("4p" in k for k in keys(ckpt))
    probe = dict(L)
    model4.text._drop_derived(probe)                             # what merge_lora, checkpoint loads and quantize_base do to a layer
    assert not names & set(probe) and names <= set(L)


def test_worst_ratios_seen_on_the_device():
    """last in the file: what the comparisons above saw, per kind, next to the emulation's figure; each comparison asserted its own bound"""
    for kind in sorted(g4.BOUNDS):
        print(f"WORST {kind:12s} device {g4.WORST.get(kind, float('nan')):.4g}  emulation {g4.EMU_WORST[kind]:.4g}  c = {g4.BOUNDS[kind]:.4g}")
