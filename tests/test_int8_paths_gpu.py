"""The LLM.int8 base product by product: everything lhrs_quant_int8_rows / lhrs_dequant_int8_rows / lhrs_int8_prepare write is compared
bit for bit with tests/int8_cases.py (exact expected values), hk.int8_linear element by element and 64x64 cell by cell with its float64
reference.  Operands sit in larger buffers: NaN and 1e30 in the padding of x (neither may flag a column or enter an absmax), sentinels
around every output (rows past M / N, the XQ padding, A2 / B2 columns past n_pad and the 64 LoRA columns in front of them, the tails of
flags / idx / meta), which must come back unchanged.  tests/test_int8_cases_cpu.py shows what these comparisons catch."""
import pytest
import torch

from lhrs_bot_amd import _lib
from lhrs_bot_amd import kernels as hk

import gemm_cases as gc
import int8_cases as ic

pytestmark = pytest.mark.gpu

DEV = "cuda"
S8, S16, S32 = 0x5A, 0x5A5A, 0x5A5A5A5A       # sentinel bytes (bf16 0x5A5A = 1.5e16, a value no case computes)
LORA = 64


def sent(shape, dtype):
    if dtype == torch.int8:
        return torch.full(shape, S8, dtype=torch.int8, device=DEV)
    if dtype == torch.bfloat16:
        return torch.full(shape, S16, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    return torch.full(shape, S32, dtype=torch.int32, device=DEV).view(dtype)


def only_written(buf, rows, c0, c1, what):
    """every element of buf outside [0, rows) x [c0, c1) still holds the sentinel"""
    b = buf.view({1: torch.int8, 2: torch.int16, 4: torch.int32}[buf.element_size()])
    b = b.reshape(b.shape[0], -1) if b.dim() > 1 else b.reshape(1, -1)
    inside = torch.zeros_like(b, dtype=torch.bool)
    inside[:rows, c0:c1] = True
    s = {1: S8, 2: S16, 4: S32}[buf.element_size()]
    assert bool((b[~inside] == s).all()), f"{what}: written outside rows [0, {rows}) x columns [{c0}, {c1})"


def padded_x(x, pad):
    """x in the top-left of a [M + 2, K + pad] buffer: NaN / 1e30 alternate in the padding columns, 1e30 fills the rows past M"""
    M, K = x.shape
    buf = torch.full((M + 2, K + pad), 1e30, dtype=torch.bfloat16)
    buf[:M, K::2] = float("nan")
    buf[:M, :K] = x
    return buf.to(DEV)


def run_prepare(x, wq, wscale, strided, state=None):
    """lhrs_int8_prepare through the C ABI on canary buffers -> dict for ic.prepare_mismatches (+ the buffers).  strided: ldx, ldq, ldwq,
    lda2, ldb2 larger than the rows and A2 / B2 handed in offset by the 64 LoRA columns, as hk.int8_linear passes them.  state: the
    (flags, idx, meta) of an earlier call (workspace reuse)."""
    M, K = x.shape
    N = wq.shape[0]
    kpad = ic.ceil64(K)
    px, pq, p2, off = (24, 16, 8, LORA) if strided else (0, 0, 0, 0)
    X = padded_x(x, px)
    WQ = torch.full((N + 2, K + pq), 127, dtype=torch.int8)
    WQ[:N, :K] = wq
    WQ = WQ.to(DEV)
    wsc = torch.full((N + 2,), 1e30, dtype=torch.float32)
    wsc[:N] = wscale
    wsc = wsc.to(DEV)
    XQ, sx = sent((M + 2, K + pq), torch.int8), sent((M + 3,), torch.float32)
    A2, B2 = sent((M + 2, off + kpad + p2), torch.bfloat16), sent((N + 2, off + kpad + p2), torch.bfloat16)
    if state is None:
        state = (sent((K + 4,), torch.int32), sent((kpad + 8,), torch.int32), sent((4,), torch.int32))
    flags, idx, meta = state
    st = _lib.load().lhrs_int8_prepare(X.data_ptr(), X.stride(0), M, K, ic.THR, WQ.data_ptr(), WQ.stride(0), wsc.data_ptr(), N, XQ.data_ptr(),
                                       XQ.stride(0), sx.data_ptr(), flags.data_ptr(), idx.data_ptr(), meta.data_ptr(),
                                       A2.data_ptr() + 2 * off, A2.stride(0), B2.data_ptr() + 2 * off, B2.stride(0), hk._stream())
    _lib.check(st, "int8_prepare")
    torch.cuda.synchronize()
    nb = (K // 8 + 3) // 4 * 4
    got = dict(meta=meta[:2].tolist(), idx=idx, sx=sx[:M], XQ=XQ[:M, :K], A2=A2[:M, off:], B2=B2[:N, off:],
               mask8=flags.view(torch.uint8)[:K // 8])
    return got, dict(XQ=XQ, sx=sx, A2=A2, B2=B2, flags=flags, idx=idx, meta=meta, off=off, nb=nb, state=state)


def check_prepare(x, wq, wscale, strided, what, state=None, fresh_state=True):
    ref = ic.ref_prepare(x, wq, wscale)
    got, b = run_prepare(x, wq, wscale, strided, state)
    M, K = x.shape
    N = wq.shape[0]
    assert ic.prepare_mismatches(got, ref) == [], what
    only_written(b["XQ"], M, 0, K, what + " XQ")
    only_written(b["sx"], 1, 0, M, what + " sx")
    only_written(b["A2"], M, b["off"], b["off"] + ref.n_pad, what + " A2")
    only_written(b["B2"], N, b["off"], b["off"] + ref.n_pad, what + " B2")
    fb = b["flags"].view(torch.uint8)
    assert not bool(fb[K // 8:b["nb"]].any()), what + ": mask bytes past K / 8 are not zero"
    only_written(fb, 1, 0, b["nb"], what + " flags")
    only_written(b["meta"], 1, 0, 2, what + " meta")
    if fresh_state:
        only_written(b["idx"], 1, 0, ref.n_pad, what + " idx")
    return ref, b


@pytest.fixture(scope="module")
def weights():
    """(N, K) -> (wq, wscale) of ic.ref_quant_rows, shared by the prepare cases"""
    cache = {}

    def get(N, K):
        if (N, K) not in cache:
            cache[(N, K)] = ic.ref_quant_rows(ic.make_w(100 + N + K, N, K))[:2]
        return cache[(N, K)]
    return get


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided_lora_offset"])
@pytest.mark.parametrize("case", ic.PREPARE, ids=[c.name for c in ic.PREPARE])
def test_int8_prepare_products_bit_exact(case, strided, weights):
    wq, wscale = weights(case.N, case.K)
    check_prepare(case.build(), wq, wscale, strided, f"{case.name} ({case.edge})")


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided_lora_offset"])
def test_int8_prepare_workspace_reuse(strided, weights):
    """flags / idx / meta of ONE workspace through 130, then 0, then 1 outlier columns: every call's products equal the reference, i.e.
    those of a fresh workspace (which check_prepare's other callers use)."""
    M, N, K = 33, 5, 264
    wq, wscale = weights(N, K)
    state = None
    for i, (x, n) in enumerate(zip(ic.reuse_inputs(M, K), ic.REUSE_N)):
        ref, b = check_prepare(x, wq, wscale, strided, f"reuse call {i} (n = {n})", state=state, fresh_state=state is None)
        assert ref.n == n
        state = b["state"]
    only_written(state[1], 1, 0, ic.ceil64(max(ic.REUSE_N)), "reuse idx")       # nothing past the largest n_pad of the sequence


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("case", ic.WEIGHTS, ids=[c.name for c in ic.WEIGHTS])
def test_int8_weight_side_bit_exact(case, strided):
    w = case.build()
    N, K = w.shape
    q_ref, s_ref, d_ref = ic.ref_quant_rows(w)
    pw, pq = (24, 16) if strided else (0, 0)
    W = padded_x(w, pw)
    Q, sc = sent((N + 2, K + pq), torch.int8), sent((N + 3,), torch.float32)
    L = _lib.load()
    _lib.check(L.lhrs_quant_int8_rows(W.data_ptr(), W.stride(0), Q.data_ptr(), Q.stride(0), sc.data_ptr(), N, K, hk._stream()), "quant_int8_rows")
    torch.cuda.synchronize()
    what = f"{case.name} ({case.edge})"
    assert torch.equal(Q[:N, :K].cpu(), q_ref), what
    assert torch.equal(ic.bits32(sc[:N].cpu()), ic.bits32(s_ref)), what
    only_written(Q, N, 0, K, what + " codes")
    only_written(sc, 1, 0, N, what + " scales")
    D = sent((N + 2, K + pw), torch.bfloat16)
    _lib.check(L.lhrs_dequant_int8_rows(Q.data_ptr(), Q.stride(0), sc.data_ptr(), D.data_ptr(), D.stride(0), N, K, hk._stream()), "dequant_int8_rows")
    torch.cuda.synchronize()
    assert torch.equal(ic.bits16(D[:N, :K].cpu()), ic.bits16(d_ref)), what
    assert bool(torch.isfinite(D[:N, :K].float()).all())
    only_written(D, N, 0, K, what + " dequantised")


# ------------------------------------------------------------------------------------------------------------- hk.int8_linear

def _dev(t):
    return None if t is None else t.to(DEV)


def _linear(x, o, ws, alpha=1.0):
    return hk.int8_linear(x.to(DEV), o["wq"].to(DEV), o["wscale"].to(DEV), ws, residual=_dev(o["residual"]), a2=_dev(o["a2"]), b2=_dev(o["b2"]),
                          alpha=alpha)


@pytest.mark.parametrize("case", ic.LINEAR, ids=[c.name for c in ic.LINEAR])
def test_int8_linear_per_element(case):
    x, o = case.build(), ic.lin_operands(case)
    ws = hk.Int8Workspace(DEV, kmax=case.K)
    y = _linear(x, o, ws, case.alpha)
    torch.cuda.synchronize()
    ref_p = ic.ref_prepare(x, o["wq"], o["wscale"])
    assert ws.last_outlier_columns() == ref_p.cols and ws.meta.tolist() == [case.n, ic.ceil64(case.n)]
    ref = ic.ref_linear(x, o["wq"], o["wscale"], a2=o["a2"], b2=o["b2"], residual=o["residual"], alpha=case.alpha)
    rep = gc.check("bf16", y, ref, what=f"{case.name} ({case.edge})")
    print(f"\nint8_linear {case.name}: element ratio at c = 1 {rep.elem:.4f}, cell rel-L2 {rep.cell:.3g}")
    if case.n == 0 and not case.KP:      # no bf16 stage: one correctly rounded value per element
        emu = ic.emu_linear(x, o["wq"], o["wscale"], ic.EmuWorkspace(case.K), residual=o["residual"], alpha=case.alpha)
        assert torch.equal(ic.bits16(y.cpu()), ic.bits16(emu))


def test_int8_linear_workspace_reuse():
    """One Int8Workspace, its persistent B2 buffer prefilled with NaN, three calls in a row with 130, 0 and 1 outlier columns: a stale
    meta[1], or a column of A2 / B2 past it, would put the NaNs (or the previous call's columns) into the product."""
    M, N, K = ic.REUSE_LINEAR
    o = ic.lin_operands((M, N, K, 0, False))
    ws = hk.Int8Workspace(DEV, kmax=K)
    ws.b2(N, ic.ceil64(K)).fill_(float("nan"))
    for i, (x, n) in enumerate(zip(ic.reuse_inputs(M, K), ic.REUSE_N)):
        y = _linear(x, o, ws)
        torch.cuda.synchronize()
        assert ws.meta.tolist() == [n, ic.ceil64(n)] and ws.last_outlier_columns() == ic.ref_prepare(x, o["wq"], o["wscale"]).cols
        rep = gc.check("bf16", y, ic.ref_linear(x, o["wq"], o["wscale"]), what=f"reuse call {i} (n = {n})")
        print(f"\nint8_linear reuse call {i} (n = {n}): element ratio at c = 1 {rep.elem:.4f}, cell rel-L2 {rep.cell:.3g}")
        y_fresh = _linear(x, o, hk.Int8Workspace(DEV, kmax=K))
        assert torch.equal(ic.bits16(y.cpu()), ic.bits16(y_fresh.cpu())), f"reuse call {i}: differs from a fresh workspace"
