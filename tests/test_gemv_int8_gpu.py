"""Decode from the LLM.int8 base, kernel level (csrc/gemv_int8.hip behind hk.int8_decode_prepare / hk.repack_int8_mfma / hk.gemv_int8) on an
MI355X, against tests/gemv_int8_cases.py.

Operand map: one-hot int8 activation rows over an asymmetric weight make every output f32(WQ[n, k_b]) * fl(sx * sw) exactly - the check of the
i8 MFMA's lane map, the tiled layout, the wave split and the accumulator map with exact integer data.
Prepare: every output bit for bit against int8_cases.ref_prepare of the kernel's own h_out; h_out inside the FLIP window of
gemv_cases.ref_prologue.
GEMV: every case row-major and packed, the output inside a NaN-filled buffer whose guard rows must stay NaN; fp32 / n = 0 / no residual
bit-equal to f32(acc) * fl(sx * sw), with one outlier column bit-equal to hk.int8_linear, bf16 / n = 0 / no residual inside (2^-8 + 2^-21) |want|, everything else inside the measure() bound
whose constant is 4 x the CPU emulation's worst ratio.  The worst ratios at c = 1 are printed by the last test."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from lhrs_bot_amd import _lib  # noqa: E402
from lhrs_bot_amd import kernels as hk  # noqa: E402

import gemv_int8_cases as g8  # noqa: E402
import int8_cases as ic  # noqa: E402

DEV = "cuda"
BF, F32, I8 = torch.bfloat16, torch.float32, torch.int8
NAN = float("nan")


def _weights(wq, packed, ldw=None):
    """-> what hk.gemv_int8 takes: a PackedI8 made by the device repack (checked against the restatement) or int8 rows, strided on request"""
    N, K = wq.shape
    if ldw is None:
        rows = wq.to(DEV)
    else:
        buf = torch.full((N + 1, ldw), 0x55, dtype=I8)
        buf[:N, :K] = wq
        rows = buf.to(DEV)[:N, :K]
    if not packed:
        return rows
    pk = hk.repack_int8_mfma(rows)
    assert torch.equal(pk.data.cpu(), g8.repack(wq)), "repack_int8_mfma differs from its restatement"
    return pk


def _prepare(h, ws, pro=hk.PRO_NONE, norm_w=None, want_h=False):
    B = h.shape[0]
    K = h.shape[1] // 2 if pro == hk.PRO_SWIGLU else h.shape[1]
    h_out = torch.full((B, K), NAN, device=DEV, dtype=BF) if want_h else None
    hk.int8_decode_prepare(h.to(DEV), K, ws, prologue=pro, norm_w=None if norm_w is None else norm_w.to(DEV), eps=g8.gc.EPS, h_out=h_out)
    n = int(ws.meta[0].item())
    return dict(n=n, idx=ws.idx, sx=ws.sx[:B], XQ=ws.xq[:B, :K], xo=ws.xo[:B]), h_out


def _out(B, N, f32, ldy=None, guard=2):
    buf = torch.full((B + guard, N if ldy is None else ldy), NAN, device=DEV, dtype=F32 if f32 else BF)
    return buf, buf[:B, :N]


# ------------------------------------------------------------------------------------------------------------------------- operand map
@pytest.mark.parametrize("packed", [False, True], ids=["rows", "packed"])
@pytest.mark.parametrize("K", g8.PROBE_K)
def test_one_hot_rows_return_single_weights_exactly(K, packed):
    wq = g8.probe_weights(K)
    sx, sw = g8.probe_factors()
    W = _weights(wq, packed)
    ws = hk.Int8DecodeWorkspace(DEV, 16, K)
    ws.sx.copy_(sx)
    ws.meta.zero_()
    sw_d = sw.to(DEV)
    f = sx[:, None] * sw[None, :]
    for k0 in range(0, K, 16):
        ks = [k0 + (5 * b + 3) % 16 for b in range(16)]       # the 16 columns of this block, not in row order: every k is probed once
        xq = torch.zeros(16, K, dtype=I8)
        xq[torch.arange(16), torch.tensor(ks)] = 1
        ws.xq[:, :K].copy_(xq)
        buf, y = _out(16, g8.PROBE_N, True)
        hk.gemv_int8(W, sw_d, ws, y, K, out_f32=True)
        want = wq[:, ks].t().float() * f
        assert torch.equal(ic.bits32(y.cpu()), ic.bits32(want)), (K, packed, k0)
        assert bool(torch.isnan(buf[16:]).all())


# ------------------------------------------------------------------------------------------------------------------------- prepare
@pytest.mark.parametrize("c", g8.PREPARE, ids=[c.name for c in g8.PREPARE])
def test_prepare_bit_for_bit(c):
    h = c.build()
    ws = hk.Int8DecodeWorkspace(DEV, c.B, c.K)
    ws.meta.fill_(-7)
    got, h_out = _prepare(h, ws, want_h=True)
    assert torch.equal(ic.bits16(h_out.cpu()), ic.bits16(h)), "prologue 0 must copy"
    ref = ic.ref_prepare(h_out.cpu(), torch.zeros(1, c.K, dtype=I8), torch.zeros(1))
    assert ref.n == c.n and g8.prepare_mismatches(got, ref) == [], (c.name, g8.prepare_mismatches(got, ref))
    got2, none = _prepare(h, ws)                       # h_out = NULL: the same outputs
    assert none is None and g8.prepare_mismatches(got2, ref) == []


@pytest.mark.parametrize("c", g8.PROLOGUE, ids=[c.name for c in g8.PROLOGUE])
def test_prepare_takes_the_flags_on_the_prologues_output(c):
    x, norm_w = c.build()
    ws = hk.Int8DecodeWorkspace(DEV, c.B, c.K)
    got, h_out = _prepare(x, ws, c.pro, norm_w, want_h=True)
    ok, two = g8.prologue_ok(h_out, x, c.pro, norm_w)
    assert ok, f"{c.name}: h_out outside the FLIP window of ref_prologue ({two} elements have two admissible values)"
    ref = ic.ref_prepare(h_out.cpu(), torch.zeros(1, c.K, dtype=I8), torch.zeros(1))
    assert g8.prepare_mismatches(got, ref) == [], (c.name, g8.prepare_mismatches(got, ref))
    cols = set(ref.cols)
    assert set(c.flagged) <= cols and not (set(c.clear) & cols), (c.name, sorted(cols)[:20])
    xin = x[:, :c.K].float().abs()
    assert float(xin[:, list(c.flagged)].max()) < g8.THR <= float(xin[:, list(c.clear)].max())


# ------------------------------------------------------------------------------------------------------------------------- GEMV
def _run_case(c, packed, strides=None):
    i = g8.inputs(c)
    p, ref = g8.reference(c)
    st = strides or {}
    ws = hk.Int8DecodeWorkspace(DEV, c.B, c.K)
    if strides:                                         # wider operand rows: views into larger buffers
        ws.xq = torch.full((c.B + 1, st["ldq"]), 0x55, device=DEV, dtype=I8)[:c.B, :c.K]
        ws.xo = torch.full((c.B + 1, st["ldo"]), NAN, device=DEV, dtype=BF)[:c.B, :c.K]
        ws.kmax = c.K
    got, _ = _prepare(i["h"], ws)
    assert g8.prepare_mismatches(got, p) == [], (c.name, g8.prepare_mismatches(got, p))
    res = None
    if i["res"] is not None:
        rb = torch.full((c.B + 1, st.get("ldr", c.N)), NAN, dtype=BF)
        rb[:c.B, :c.N] = i["res"]
        res = rb.to(DEV)[:c.B, :c.N]
    W = _weights(i["wq"], packed, st.get("ldw"))
    sw = i["wscale"].to(DEV)
    buf, y = _out(c.B, c.N, c.f32, st.get("ldy"))
    hk.gemv_int8(W, sw, ws, y, c.K, residual=res, out_f32=c.f32)
    again_buf, again = _out(c.B, c.N, c.f32, st.get("ldy"))
    hk.gemv_int8(W, sw, ws, again, c.K, residual=res, out_f32=c.f32)
    full = buf[:, :c.N]
    bad = g8.verdict(c, full, p)
    rep = g8.check(g8.kind_of(c), full, ref, "gemv_int8", c.name + (" packed" if packed else " rows"))
    print(f"{c.name} {'packed' if packed else 'rows'}: {rep.unit:.4g} at c = 1 (c = {g8.BOUNDS[g8.kind_of(c)]:.4g})")
    assert bad == [], bad
    ints = torch.int32 if c.f32 else torch.int16
    assert torch.equal(buf.view(ints), again_buf.view(ints)), "two runs differ"
    if buf.shape[1] > c.N:
        assert bool(torch.isnan(buf[:, c.N:]).all()), "written past N"


@pytest.mark.parametrize("packed", [False, True], ids=["rows", "packed"])
@pytest.mark.parametrize("c", g8.GEMV, ids=[c.name for c in g8.GEMV])
def test_gemv_case(c, packed):
    _run_case(c, packed)


@pytest.mark.parametrize("packed", [False, True], ids=["rows", "packed"])
def test_gemv_with_every_stride_wider_than_its_row(packed):
    _run_case(g8.STRIDED, packed, g8.STRIDES)


@pytest.mark.parametrize("packed", [False, True], ids=["rows", "packed"])
def test_three_calls_on_one_workspace(packed):
    """130, 0, 1 outlier columns in a row: nothing of an earlier call leaks into a later one"""
    B, N, K = g8.REUSE
    xs, wq, wscale = g8.reuse_operands()
    W, sw = _weights(wq, packed), wscale.to(DEV)
    ws = hk.Int8DecodeWorkspace(DEV, B, K)
    for x, n in zip(xs, ic.REUSE_N):
        p, ref = g8.make_ref(x, wq, wscale, None, False)
        got, _ = _prepare(x, ws)
        assert got["n"] == n and g8.prepare_mismatches(got, p) == []
        buf, y = _out(B, N, False)
        hk.gemv_int8(W, sw, ws, y, K)
        g8.check("bf16", buf, ref, "gemv_int8 reuse", f"n={n}")
        if n == 0:
            ok, r = ic.tight_bound_ok(y.cpu(), ref.want)
            assert ok, r


@pytest.mark.parametrize("B,N,K", [(3, 64, 1152), (16, 64, 11008), (1, 264, 4096)], ids=["b3_k1152", "b16_k11008", "b1_k4096"])
def test_decode_pair_equals_int8_linear_bit_for_bit_with_one_outlier_column(B, N, K):
    """With exactly one outlier column both paths compute bf16(f32(acc) * fl(sx * sw) + one exact product): hk.int8_linear adds a 64-column
    bf16 stage that holds one non-zero product (the MFMA's sum of it and 63 zeros is exact, rounded once into the accumulator), the decode
    GEMV adds the same product after a butterfly over zeros.  No residual (int8_linear adds it after its bf16 store), alpha = 1."""
    x = ic.make_x(90 + B, B, K, 1).to(DEV)
    wq, wscale, _ = ic.ref_quant_rows(ic.make_w(91 + N, N, K))
    wq_d, sw = wq.to(DEV), wscale.to(DEV)
    want = hk.int8_linear(x, wq_d, sw, hk.Int8Workspace(DEV, kmax=K))
    ws = hk.Int8DecodeWorkspace(DEV, B, K)
    hk.int8_decode_prepare(x, K, ws)
    assert int(ws.meta[0].item()) == 1
    for packed in (False, True):
        y = torch.full((B, N), NAN, device=DEV, dtype=BF)
        hk.gemv_int8(_weights(wq, packed), sw, ws, y, K)
        assert torch.equal(ic.bits16(y.cpu()), ic.bits16(want.cpu())), (B, N, K, packed)


def test_rejections_through_the_wrappers_enqueue_nothing():
    ws = hk.Int8DecodeWorkspace(DEV, 16, 128)
    wq = torch.zeros((16, 96), device=DEV, dtype=I8)
    y = torch.zeros((1, 16), device=DEV, dtype=BF)
    sw = torch.ones(16, device=DEV)
    with pytest.raises(RuntimeError, match="rejected by liblhrs_hip"):
        hk.gemv_int8(wq, sw, ws, y, 96)
    with pytest.raises(RuntimeError, match="rejected by liblhrs_hip"):
        hk.int8_decode_prepare(torch.zeros((1, 96), device=DEV, dtype=BF), 96, ws)
    with pytest.raises(RuntimeError, match="rejected by liblhrs_hip"):
        hk.repack_int8_mfma(wq)
    with pytest.raises(ValueError):
        hk.int8_decode_prepare(torch.zeros((1, 256), device=DEV, dtype=BF), 256, ws)      # larger than the workspace
    with pytest.raises(ValueError):
        hk.int8_decode_prepare(torch.zeros(128, device=DEV, dtype=BF), 128, ws)              # not a matrix
    with pytest.raises(ValueError):
        hk.gemv_int8(torch.zeros((16, 128), device=DEV, dtype=I8), sw, ws, torch.zeros(16, device=DEV, dtype=BF), 128)
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    assert lib.lhrs_gemv_int8(wq.data_ptr(), 96, 0, sw.data_ptr(), ws.xq.data_ptr(), 128, ws.sx.data_ptr(), ws.idx.data_ptr(), ws.meta.data_ptr(),
                              ws.xo.data_ptr(), 128, None, 0, y.data_ptr(), 16, 17, 16, 128, 0, s) == -1
    torch.cuda.synchronize()
    assert not bool(y.any())


def test_worst_ratios_seen_on_the_device():
    """last in the file: what the comparisons above saw per output type, at c = 1"""
    for k in sorted(g8.WORST):
        print(f"WORST {k:5s} {g8.WORST[k]:.4g} (c = {g8.BOUNDS[k]:.4g})")
