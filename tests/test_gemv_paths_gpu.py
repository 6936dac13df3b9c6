"""Every kernel, template instance and branch of the decode weight stream (csrc/decode.hip: gemv_kernel, gemv_mfma_kernel,
gemv_fp8_mfma_kernel with and without its fused prologue, quant_fp8_rows_kernel, the two repack kernels) against the float64 references of
tests/gemv_cases.py, element by element.

The cases are gemv_cases.CASES: the smallest shapes that reach each cell of gemv_cases.paths (not the model's shapes).  Inputs are seeded and
lie in NaN-padded buffers: NaN in the columns past K (past 2K for SwiGLU) where a stride is larger than the width, a NaN row after row N - 1
of W and after row B - 1 of x, NaN past norm_w and past the scales.  Every output lies inside a larger buffer prefilled with a sentinel bit
pattern that must come back unchanged outside [B, N].  Tiled weights must give the bits the row format gives, and all eight (RPW, UNR)
instances of the batch-1 kernel the same bits as each other.  The quantiser's codes are compared with the reference quantiser's, the repacked
tiles with their index restatement (torch.equal).

On an MI355X every case passes, and the worst ratio of every kind equals the emulation's to four digits: the emulation's models of both MFMAs
(gemv_cases docstring) give the device's bits."""
import pytest
import torch

from lhrs_bot_amd import _lib

import gemv_cases as gc

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -1
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
_INT = {BF: torch.int16, F32: torch.int32, U8: torch.int8}


def L():
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def nanbuf(t, pad=0, rows_after=1):
    """[rows, cols] -> the same values as the top-left view of a [rows + rows_after, cols + pad] device buffer that holds NaN elsewhere
    (e4m3 bytes: 0x7F, the format's NaN)"""
    rows, cols = t.shape
    buf = torch.full((rows + rows_after, cols + pad), 0x7F if t.dtype == U8 else float("nan"), dtype=t.dtype)
    buf[:rows, :cols] = t
    return buf.to(DEV)[:rows, :cols]


def nanvec(t, pad=8):
    if t is None:
        return None
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


def bits(t):
    return t.contiguous().view(_INT[t.dtype])


def ok(st, what):
    _lib.check(st, what)


class Operands:
    """the device operands of a gemv / fp8_mfma / fp8_fused case"""

    def __init__(self, c, i=None, B=None):
        o = c.opt
        self.c, self.i = c, i or gc.inputs(c)
        i = self.i
        self.B, self.N, self.K = B or o["B"], o["N"], o["K"]
        s = o.get("strided", False)
        self.W = nanbuf(i["W"], 16 if s else 0)
        self.x = nanbuf(i["x"], 16 if s else 0)
        self.res = None if i.get("res") is None else nanbuf(i["res"], 8 if s else 0)
        self.wscale, self.xscale, self.norm_w = nanvec(i.get("wscale")), nanvec(i.get("xscale")), nanvec(i.get("norm_w"))
        self.f32, self.pad = bool(o.get("f32")), 24 if s else 0
        self.tiles = None

    def out(self):
        return sent_buf(self.B, self.N, F32 if self.f32 else BF, self.pad)

    def ldr(self):
        return 0 if self.res is None else self.res.stride(0)

    def tiled(self):
        """the library's re-tiled copy of W, checked against the index restatement"""
        if self.tiles is None:
            G, fp8 = -(-self.N // 16), self.W.dtype == U8
            t = torch.full((G * 16 * self.K,), SENT, dtype=_INT[self.W.dtype], device=DEV).view(self.W.dtype)
            f = L().lhrs_repack_fp8_mfma if fp8 else L().lhrs_repack_bf16_mfma
            ok(f(self.W.data_ptr(), self.W.stride(0), t.data_ptr(), self.N, self.K, stream()), "repack")
            whole = torch.cat([self.i["W"], torch.full((1, self.K), 0x7F if fp8 else float("nan"), dtype=self.W.dtype)])
            want = (gc.repack_fp8 if fp8 else gc.repack_bf16)(whole, self.N, self.K)
            assert torch.equal(bits(t).cpu(), bits(want).reshape(-1)), "repack: not the permutation of the index restatement"
            self.tiles = t
        return self.tiles


def run_gemv(p, fmt):
    o = p.c.opt
    buf, y = p.out()
    W = p.tiled() if fmt == 2 else p.W
    ok(L().lhrs_gemv(W.data_ptr(), 0 if fmt == 2 else W.stride(0), ptr(p.wscale), fmt, p.x.data_ptr(), p.x.stride(0), o["pro"], ptr(p.norm_w), gc.EPS,
                     ptr(p.res), p.ldr(), y.data_ptr(), y.stride(0), p.B, p.N, p.K, int(p.f32), stream()), "gemv")
    untouched(buf, y, p.c.name)
    return y


def run_fp8(p, packed):
    buf, y = p.out()
    W = p.tiled() if packed else p.W
    if p.c.op == "fp8_mfma":
        ok(L().lhrs_gemv_fp8_mfma(W.data_ptr(), 0 if packed else W.stride(0), p.wscale.data_ptr(), p.x.data_ptr(), p.x.stride(0), p.xscale.data_ptr(),
                                  ptr(p.res), p.ldr(), y.data_ptr(), y.stride(0), p.B, p.N, p.K, int(p.f32), int(packed), stream()), "gemv_fp8_mfma")
    else:
        ok(L().lhrs_gemv_fp8_mfma_fused(W.data_ptr(), 0 if packed else W.stride(0), p.wscale.data_ptr(), p.x.data_ptr(), p.x.stride(0), p.c.opt["pro"],
                                        ptr(p.norm_w), gc.EPS, ptr(p.res), p.ldr(), y.data_ptr(), y.stride(0), p.B, p.N, p.K, int(p.f32), int(packed),
                                        stream()), "gemv_fp8_mfma_fused")
    untouched(buf, y, p.c.name)
    return y


def ids(cases):
    return [c.name.replace(" ", "_") for c in cases]


@pytest.mark.parametrize("c", gc.cases_of("gemv"), ids=ids(gc.cases_of("gemv")))
def test_gemv(c):
    o = c.opt
    p = Operands(c)
    ref, _ = gc.reference(c, p.i)
    try:
        y = run_gemv(p, o["fmt"])
        rep = gc.check(gc.kind_of(c), y, ref, "gemv", c.name)
        print(f"{c.name}: {rep.unit:.3g} at c = 1")
        if o["tiles"]:
            assert torch.equal(bits(run_gemv(p, 2)), bits(y)), "tiled weights: not the bits of the row format"
        if o["tunings"]:
            for rpw, unr in gc.TUNINGS:
                ok(L().lhrs_gemv_set_tuning(rpw, unr), "set_tuning")
                assert torch.equal(bits(run_gemv(p, o["fmt"])), bits(y)), f"(RPW, UNR) = ({rpw}, {unr}): not the bits of the shape rule's instance"
    finally:
        L().lhrs_gemv_set_tuning(0, 0)


@pytest.mark.parametrize("c", gc.cases_of("fp8_mfma") + gc.cases_of("fp8_fused"), ids=ids(gc.cases_of("fp8_mfma") + gc.cases_of("fp8_fused")))
def test_gemv_fp8_mfma(c):
    p = Operands(c)
    ref, _ = gc.reference(c, p.i)
    y = run_fp8(p, False)
    rep = gc.check(gc.kind_of(c), y, ref, c.op, c.name)
    print(f"{c.op} {c.name}: {rep.unit:.3g} at c = 1")
    assert torch.equal(bits(run_fp8(p, True)), bits(y)), "tiled weights: not the bits of the row format"


@pytest.mark.parametrize("c", gc.cases_of("quant"), ids=ids(gc.cases_of("quant")))
def test_quant_fp8_rows(c):
    x = gc.quant_inputs(c)
    N, K = x.shape
    s = c.opt["strided"]
    xd = nanbuf(x, 8 if s else 0)
    buf, out = sent_buf(N, K, U8, 32 if s else 0)
    sbuf = torch.full((N + 8,), SENT, dtype=torch.int32, device=DEV).view(F32)
    ok(L().lhrs_quant_fp8_rows(xd.data_ptr(), xd.stride(0), out.data_ptr(), out.stride(0), sbuf.data_ptr(), N, K, stream()), "quant_fp8_rows")
    untouched(buf, out, c.name)
    assert bool((sbuf[N:].view(torch.int32) == SENT).all()), "a scale past row N - 1 was written"
    ref = gc.ref_quant(x)
    bad_scale, bad_codes = gc.quant_mismatch(sbuf[:N], out, ref)
    other = int((out.cpu() != ref.codes).sum())
    print(f"quant {c.name}: {other} of {ref.border} borderline elements took the neighbouring code")
    assert (bad_scale, bad_codes) == (0, 0), f"{c.name}: {bad_scale} scales off by more than an ulp, {bad_codes} codes that are neither admissible value"
    assert float(sbuf[1]) == 1.0 and not bool(out[1].any())


@pytest.mark.parametrize("c", gc.cases_of("repack_bf16") + gc.cases_of("repack_fp8"), ids=ids(gc.cases_of("repack_bf16") + gc.cases_of("repack_fp8")))
def test_repack(c):
    g, N, K = gc._gen(c), c.opt["N"], c.opt["K"]
    W = torch.randn(N, K, generator=g).to(BF) if c.op == "repack_bf16" else torch.randint(0, 0x7F, (N, K), generator=g, dtype=U8)
    case = gc.Case(c.op, c.name, dict(c.opt, B=1))
    Operands(case, dict(W=W, x=W[:1])).tiled()                  # compares with the restatement


@pytest.mark.parametrize("c", gc.cases_of("reject"), ids=ids(gc.cases_of("reject")))
def test_rejections(c):
    """the operands are complete and of full size: were a call accepted it would run inside its buffers"""
    o = c.opt
    B, N, K = o["B"], o["N"], o["K"]
    g = gc._gen(c)
    x = torch.randn(B, 2 * K if o["pro"] == 2 else K, generator=g).to(BF)
    W = (torch.randn(N, K, generator=g) * 0.05).to(BF)
    i = dict(x=x, W=W, norm_w=torch.ones(K, dtype=BF), wscale=torch.ones(N))
    if o["entry"] == "fp8_fused" or o.get("fmt") == 1:
        i["W"] = gc.ref_quant(W).codes
    p = Operands(gc.Case(o["entry"], c.name, dict(o, f32=False, res=False)), i)
    with pytest.raises(RuntimeError, match="rejected by liblhrs_hip"):
        if o["entry"] == "gemv":
            run_gemv(p, o["fmt"])
        else:
            run_fp8(p, False)
    with pytest.raises(gc.Rejected):
        if o["entry"] == "gemv":
            gc.gemv_plan(o["fmt"], B, N, K, o["pro"])
        else:
            gc.path_of(p.c)


def test_the_table_reaches_every_cell():
    reached = set().union(*(gc.path_of(c) for c in gc.CASES))
    assert reached == gc.paths, (sorted(gc.paths - reached), sorted(reached - gc.paths))


def test_worst_ratios_seen_on_the_device():
    """last in the file: what the comparisons above saw, per kind, next to the emulation's figure (gemv_cases.EMU_WORST); each comparison
    asserted its own bound"""
    for kind in sorted(gc.BOUNDS):
        print(f"WORST {kind:12s} device {gc.WORST.get(kind, float('nan')):.4g}  emulation {gc.EMU_WORST[kind]:.4g}  c = {gc.BOUNDS[kind]:.4g}")
