"""lhrs_lora_down / lhrs_lora_up (csrc/lora_decode.hip, the live-adapter half of a decode linear) against the float64 references of
tests/lora_decode_cases.py, element by element, on the cases of that module: the smallest shapes at which each kernel can still go wrong.

Operands lie in NaN-padded device buffers (a NaN row after the last batch row of x, acc and the residual; NaN past the row width where a stride is
larger); tpart carries one guard slice and one guard batch row, y one guard batch row and a guard column tail, all NaN before the call and NaN
after it.  The off-block columns of Bw hold finite non-zero garbage that the reference never reads."""
import pytest
import torch

from lhrs_bot_amd import _lib
from lhrs_bot_amd import kernels as hk

import lora_decode_cases as lc

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")


def nanbuf(t, pad=0, rows_after=1):
    """[rows, cols] -> the same values as the top-left view of a [rows + rows_after, cols + pad] device buffer that holds NaN elsewhere"""
    rows, cols = t.shape
    buf = torch.full((rows + rows_after, cols + pad), NAN, dtype=t.dtype)
    buf[:rows, :cols] = t
    return buf.to(DEV)[:rows, :cols]


def _ids(cases):
    return [getattr(c, "name", None) or "B{} R{} K{} pro{}".format(*c) for c in cases]


@pytest.mark.parametrize("c", lc.DOWN_CASES, ids=_ids(lc.DOWN_CASES))
def test_lora_down_against_fp64(c):
    i = lc.down_inputs(c)
    ref, nsl = lc.down_reference(c, i)
    assert hk.lora_down_splits(c.K, c.R) == nsl == lc.splits(c.K, c.R)
    x = nanbuf(i["x"], pad=8 if c.pro != 2 else 0)             # SwiGLU: x is the strided [B, 2K] row pair itself
    A = nanbuf(i["A"])
    nw = torch.full((c.K + 8,), NAN, dtype=BF)
    nw[:c.K] = i["norm_w"]
    nw = nw.to(DEV)[:c.K]
    tpart = torch.full(((nsl + 1) * c.B + 1, c.R), NAN, dtype=F32, device=DEV)   # live slices, a guard slice, a guard batch row
    got_nsl = hk.lora_down(x, A, tpart, c.K, c.R, prologue=c.pro, norm_w=nw if c.pro == 1 else None, eps=lc.EPS)
    torch.cuda.synchronize()
    assert got_nsl == nsl
    rep = lc.check(lc.down_kind(c), tpart, ref, op="lora_down", case=str(tuple(c)))
    print(f"lora_down {tuple(c)} nsl={nsl}: {rep.unit:.4g} at c = 1 (c = {lc.BOUNDS[lc.down_kind(c)]:.4g})")


@pytest.mark.parametrize("c", lc.UP_CASES, ids=_ids(lc.UP_CASES))
def test_lora_up_against_fp64(c):
    i = lc.up_inputs(c)
    ref, _ = lc.up_reference(c, i)
    B, N, R = c.B, i["N"], i["R"]
    acc = nanbuf(i["acc"], pad=5)
    res = nanbuf(i["res"], pad=2) if i["res"] is not None else None
    Bw = i["Bw"].to(DEV)
    tpart = i["tpart"].to(DEV).contiguous()
    y = torch.full((B + 1, N + 3), NAN, dtype=BF, device=DEV)
    r, fout = (R, N) if c.dense else (c.r, c.fout)
    hk.lora_up(acc, tpart, c.nsl, c.s, Bw, r, fout, y[:B, :N], residual=res, R=R)
    torch.cuda.synchronize()
    rep = lc.check("up", y, ref, op="lora_up", case=c.name)
    print(f"lora_up {c.name}: {rep.unit:.4g} at c = 1 (c = {lc.BOUNDS['up']:.4g})")
    if c.zero:                                                  # t == 0: exactly the rounded sum of the base product and the residual
        assert torch.equal(y[:B, :N].cpu(), (i["acc"] + i["res"].float()).to(BF))


def test_blocked_and_dense_forms_agree_on_a_block_diagonal_bw():
    """a Bw whose off-block columns ARE zero: the blocked read and the dense read over all R columns differ only in fp32 summation order"""
    c = lc.UP_CASES[3]
    i = lc.up_inputs(c)
    ref, _ = lc.up_reference(c, i)
    B, N, R = c.B, i["N"], i["R"]
    Bw = torch.zeros_like(i["Bw"])
    for p in range(c.parts):
        Bw[p * c.fout:(p + 1) * c.fout, p * c.r:(p + 1) * c.r] = i["Bw"][p * c.fout:(p + 1) * c.fout, p * c.r:(p + 1) * c.r]
    acc, res, tp, Bw = i["acc"].to(DEV), i["res"].to(DEV), i["tpart"].to(DEV), Bw.to(DEV)
    y = torch.full((2, B + 1, N + 3), NAN, dtype=BF, device=DEV)
    hk.lora_up(acc, tp, c.nsl, c.s, Bw, c.r, c.fout, y[0, :B, :N], residual=res, R=R)
    hk.lora_up(acc, tp, c.nsl, c.s, Bw, R, N, y[1, :B, :N], residual=res, R=R)
    torch.cuda.synchronize()
    lc.check("up", y[0], ref, op="lora_up", case="blocked")
    lc.check("up", y[1], ref._replace(n=R), op="lora_up", case="dense over zeros")


def _call_down(o):
    B, R, K = 17, 776, 128                                      # full-size operands: an accepted call would stay inside them
    x = torch.zeros((B, 2 * K), dtype=BF, device=DEV)
    A = torch.zeros((R, K), dtype=BF, device=DEV)
    nw = torch.ones(K, dtype=BF, device=DEV)
    tpart = torch.zeros(lc.MAX_SLICES * B * R, dtype=F32, device=DEV)
    p = dict(x=x.data_ptr(), A=A.data_ptr(), tpart=tpart.data_ptr())
    if o["null"]:
        p[o["null"]] = None
    return _lib.load().lhrs_lora_down(p["x"], x.stride(0), o["pro"], nw.data_ptr(), 1e-5, p["A"], A.stride(0), p["tpart"], o["B"], o["R"], o["K"],
                                      torch.cuda.current_stream().cuda_stream)


def _call_up(o):
    B, R, N = 17, 776, 80
    acc = torch.zeros((B, N), dtype=F32, device=DEV)
    tpart = torch.zeros(17 * B * R, dtype=F32, device=DEV)
    Bw = torch.zeros((N, R), dtype=BF, device=DEV)
    res = torch.zeros((B, N), dtype=BF, device=DEV)
    y = torch.zeros((B, N), dtype=BF, device=DEV)
    p = dict(acc=acc.data_ptr(), tpart=tpart.data_ptr(), Bw=Bw.data_ptr(), y=y.data_ptr())
    if o["null"]:
        p[o["null"]] = None
    return _lib.load().lhrs_lora_up(p["acc"], acc.stride(0), p["tpart"], o["nsl"], 2.0, p["Bw"], Bw.stride(0), o["r"], o["fout"], res.data_ptr(), res.stride(0),
                                    p["y"], y.stride(0), o["B"], o["N"], o["R"], torch.cuda.current_stream().cuda_stream)


def test_base_argument_sets_are_accepted():
    """the argument sets the rejections are one change away from"""
    assert _call_down(lc.REJECT_BASE["down"]) == 0 and _call_up(lc.REJECT_BASE["up"]) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("entry,over", lc.REJECTS, ids=[f"{e}-{'-'.join(f'{k}={v}' for k, v in o.items())}" for e, o in lc.REJECTS])
def test_bad_arguments_are_rejected_before_any_launch(entry, over):
    o = dict(lc.REJECT_BASE[entry], **over)
    rc = _call_down(o) if entry == "down" else _call_up(o)
    assert rc == -1
    msg = _lib.load().lhrs_last_error().decode()
    assert ("lora_down" if entry == "down" else "lora_up") in msg, msg
    torch.cuda.synchronize()


def test_wrapper_rejects_what_the_library_would_misread():
    x = torch.zeros((2, 128), dtype=BF, device=DEV)
    A = torch.zeros((16, 128), dtype=BF, device=DEV)
    with pytest.raises(ValueError, match="tpart"):
        hk.lora_down(x, A, torch.zeros(8, dtype=F32, device=DEV), 128)
    with pytest.raises(TypeError):
        hk.lora_down(x.float(), A, torch.zeros(1024, dtype=F32, device=DEV), 128)
    with pytest.raises(RuntimeError, match="lora_down"):
        hk.lora_down(x[:, :96], A[:, :96].contiguous(), torch.zeros(1024, dtype=F32, device=DEV), 96)


def test_worst_ratios_seen_on_the_device():
    """last in the file: what the comparisons above saw, per kind, next to the emulation's figure; each comparison asserted its own bound"""
    for kind in sorted(lc.BOUNDS):
        print(f"WORST {kind:12s} device {lc.WORST.get(kind, float('nan')):.4g}  emulation {lc.EMU_WORST[kind]:.4g}  c = {lc.BOUNDS[kind]:.4g}")
