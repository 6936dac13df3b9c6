"""Every dispatch path of the GEMM entry points against the float64 references of tests/gemm_cases.py, element by element and 64x64 cell by
cell.

Each case is a boundary shape of one path (path_of's prediction must equal the kernels the library's profile counted and its launch count).
Inputs are poisoned: NaN in the padding columns [K, lda) of A, B, A2, B2, in the residual's columns [N, ldr), in the bias past N and in the
cos / sin rows past the last position used (e4m3 operands: NaN bytes past K).  Outputs are [M + 3, ldc > N] buffers prefilled with a sentinel bit pattern; everything outside [0, M) x [0, N)
must come back unchanged.  Every term of a result (pair, bias, residual, mask, RoPE, accumulated C) carries at least ~5 % of its RMS.

8-byte aligned operands (column-offset views): lhrs_gemm_bf16_nt accepts them (it checks lda % 8), the four-wave kernel is not planned for them
(gemm_plan.h: u4_nt_ok) and the 16-wave, 144-row and small-tile kernels move their rows with 16-byte global_load_lds_dwordx4 and 16-byte stores.
gfx950 supports unaligned global (buffer) loads and stores - the compiler's own gfx950 target lists unaligned-buffer-access and emits
global_load_dwordx4 / global_store_dwordx4 for 8-byte aligned vectors - and the LDS side of the DMA is the wave's aligned LDS base + 16 x
lane, independent of the global address; so the cases below run such views like any other."""
import pytest
import torch

from lhrs_bot_amd import _lib
from lhrs_bot_amd import kernels as hk

import gemm_cases as gc
import int8_cases as ic

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
SENT = -1          # sentinel bits: bf16 0xFFFF / f32 0xFFFFFFFF, NaNs that no kernel computes


@pytest.fixture(autouse=True)
def _defaults():
    lib = _lib.load()
    hk.ensure_gemm_workspace(DEV)
    hk.gemm_set_u4(True)
    try:
        yield lib
    finally:
        hk.gemm_set_u4(True)
        lib.lhrs_gemm_set_min_tiles(128)
        lib.lhrs_gemm_set_bm144(1)
        lib.lhrs_gemm_set_tail_split(1)
        lib.lhrs_gemm_set_policy(1)


class Gen:
    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def mat(self, rows, cols, scale=1.0, pad=8, off=0):
        """bf16 [rows, cols] view at column off of a [rows, cols + pad] buffer whose other columns hold NaN (off = 4: an 8-byte aligned view)."""
        buf = torch.full((rows, cols + pad), NAN, dtype=torch.bfloat16)
        buf[:, off:off + cols] = (torch.randn(rows, cols, generator=self.g) * scale).to(torch.bfloat16)
        return buf.to(DEV)[:, off:off + cols]

    def vec(self, n, scale=1.0):
        v = torch.full((n + 8,), NAN, dtype=torch.bfloat16)
        v[:n] = (torch.randn(n, generator=self.g) * scale).to(torch.bfloat16)
        return v.to(DEV)[:n]


def out_buf(M, N, f32=False, extra=8, off=0):
    """[M + 3, N + extra] sentinel buffer and its [M, N] view at column off."""
    buf = torch.full((M + 3, N + extra), SENT, dtype=torch.int32 if f32 else torch.int16, device=DEV)
    buf = buf.view(torch.float32 if f32 else torch.bfloat16)
    return buf, buf[:M, off:off + N]


def untouched(buf, M, N, off, what):
    b = buf.view(torch.int32 if buf.dtype == torch.float32 else torch.int16)
    inside = torch.zeros_like(b, dtype=torch.bool)
    inside[:M, off:off + N] = True
    assert bool((b[~inside] == SENT).all()), f"{what}: an element outside [0, M) x [0, N) was written"


def census_of(plan):
    return {hk.GEMM_KIND_NAMES[k]: n for k, n in plan.kinds.items()}


def run_checked(plan, what, fn):
    with hk.gemm_kernel_census() as c:
        fn()
    torch.cuda.synchronize()
    assert c.counts == census_of(plan), (what, c.counts, plan.segments)
    assert c.launches == plan.launches, (what, c.launches, plan.segments)


# ------------------------------------------------------------------------------------------------------------- nt / lora / mask / f32

NT = [
    # name, entry, M, N, K, flags
    ("u4_whole_ragged_strided_res", "nt", 3839, 4104, 4096, dict(res=True, extra=8)),
    ("u4_splitk_tail", "nt", 8736, 4096, 11008, dict()),
    ("u4_small_tile_tail_res", "nt", 8736, 4096, 4096, dict(res=True)),
    ("u4_pair_two_launch_tail", "lora", 8736, 4096, 4096, dict(K2=64, res=True)),
    ("s256_bias_act1_alpha_res", "nt", 4000, 4096, 1024, dict(bias=True, act=1, alpha=0.5, res=True)),
    ("s256_bias_act3_alpha_res", "nt", 4000, 4096, 1024, dict(bias=True, act=3, alpha=0.5, res=True)),
    ("s256_small_tile_tail_bias", "nt", 8736, 4096, 4096, dict(bias=True)),
    ("s256_f32_accumulate_tail", "nt", 8736, 4096, 4096, dict(out_f32=True, accumulate=True)),
    ("b144_cost_model_act2_bias", "nt", 2184, 4096, 4096, dict(bias=True, act=2)),
    ("b144_override_bias_res", "nt", 7710, 1024, 1024, dict(bias=True, res=True)),
    ("b144_long_m_bias", "nt", 8736, 4096, 1024, dict(bias=True)),
    ("t128_act0", "nt", 3000, 2048, 512, dict(bias=True, res=True)),
    ("t128_act1", "nt", 3000, 2048, 512, dict(bias=True, act=1)),
    ("t128_act2", "nt", 3000, 2048, 512, dict(bias=True, act=2, alpha=0.5)),
    ("t128_act3", "nt", 3000, 2048, 512, dict(bias=True, act=3, res=True)),
    ("t64x128_act1_res", "nt", 2000, 1024, 256, dict(bias=True, act=1, res=True)),
    ("t64x128_act2", "nt", 2000, 1024, 256, dict(bias=True, act=2)),
    ("t64x128_act3_f32", "nt", 2000, 1024, 256, dict(bias=True, act=3, out_f32=True)),
    ("t64x64_act0_res", "nt", 300, 264, 320, dict(bias=True, res=True)),
    ("t64x64_act1", "nt", 300, 264, 320, dict(bias=True, act=1)),
    ("t64x64_act2", "nt", 300, 264, 320, dict(bias=True, act=2)),
    ("t64x64_act3_f32_accumulate", "nt", 300, 264, 320, dict(bias=True, act=3, out_f32=True, accumulate=True)),
    ("n_mod8_4", "nt", 8190, 4100, 4096, dict(extra=8)),
    ("views8_s256", "nt", 4000, 4096, 1024, dict(off=4, res=True, bias=True)),
    ("views8_u4_sized", "nt", 8190, 4096, 4096, dict(off=4, res=True)),
    ("s256_pair_bias_alpha", "lora", 4000, 4096, 4096, dict(K2=64, bias=True, alpha=0.5)),
    ("mask_s256_res", "mask", 4096, 4096, 128, dict(res=True, p=0.3)),
    ("mask_small_tile", "mask", 300, 4096, 64, dict(p=0.3, alpha=2.0)),
    ("mask_t128", "mask", 3000, 2048, 512, dict(p=0.3, res=True)),
    ("mask_t64x128", "mask", 2000, 1024, 256, dict(p=0.05)),
    ("pair_two_launch_b144_base", "lora", 7710, 1024, 1024, dict(K2=64, bias=True, res=True)),
    ("pair_two_launch_t128", "lora", 3000, 2048, 512, dict(K2=128, alpha=0.5, res=True)),
    ("pair_two_launch_t64x64_f32", "lora", 300, 264, 320, dict(K2=64, out_f32=True, accumulate=True, bias=True)),
]


def nt_plan(case):
    _, entry, M, N, K, f = case
    return gc.path_of(entry, M, N, K, K2=f.get("K2", 0), bias=f.get("bias", False), res=f.get("res", False), act=f.get("act", 0),
                      out_f32=f.get("out_f32", False), accumulate=f.get("accumulate", False), alpha=f.get("alpha", 1.0), lda=K + 8, ldb=K + 8,
                      ldc=N + f.get("extra", 8), ldr=N + 8, al16_ptrs=f.get("off", 0) == 0)


@pytest.mark.parametrize("case", NT, ids=[c[0] for c in NT])
def test_gemm_nt_path(case):
    name, entry, M, N, K, f = case
    g = Gen(M + N + K + len(name))
    off, extra = f.get("off", 0), f.get("extra", 8)
    K2, alpha, act = f.get("K2", 0), f.get("alpha", 1.0), f.get("act", 0)
    f32, acc = f.get("out_f32", False), f.get("accumulate", False)
    A = g.mat(M, K, 1.0, off=off)
    B = g.mat(N, K, K ** -0.5, off=off)
    A2 = g.mat(M, K2, 1.0) if K2 else None
    B2 = g.mat(N, K2, 0.5 * K2 ** -0.5) if K2 else None
    bias = g.vec(N, 0.5) if f.get("bias") else None
    res = g.mat(M, N, 0.5, off=off) if f.get("res") else None
    buf, C = out_buf(M, N, f32, extra, off)
    old = None
    if acc:
        old = (torch.randn(M, N, generator=g.g) * 0.5).to(DEV)
        C.copy_(old)
    mask = gc.drop_mask(M, N, 1234, f["p"], DEV) if entry == "mask" else None
    ldc, ldr = C.stride(0), res.stride(0) if res is not None else 0
    assert (A.stride(0), B.stride(0), ldc) == (K + 8, K + 8, N + extra) and all(t is None or (t.data_ptr() % 16 == 0) == (off == 0)
                                                                               for t in (A, B, C, res))
    plan = nt_plan(case)
    L = _lib.load()
    s = hk._stream()
    p = hk._p

    def call():
        if entry == "nt":
            st = L.lhrs_gemm_bf16_nt(A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), C.data_ptr(), ldc, M, N, K, p(bias), p(res), ldr, act,
                                     int(f32), int(acc), float(alpha), s)
        elif entry == "lora":
            st = L.lhrs_gemm_bf16_nt_lora(A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), A2.data_ptr(), A2.stride(0), B2.data_ptr(),
                                          B2.stride(0), K2, C.data_ptr(), ldc, M, N, K, p(bias), p(res), ldr, int(f32), int(acc), float(alpha), s)
        else:
            st = L.lhrs_gemm_bf16_nt_dropmask(A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), C.data_ptr(), ldc, M, N, K, p(res), ldr,
                                              float(alpha), float(f["p"]), 1234, s)
        _lib.check(st, entry)

    run_checked(plan, name, call)
    ref = gc.ref_nt(A, B, alpha=alpha, bias=bias, residual=res, act=act, A2=A2, B2=B2, mask=mask, old=old)
    gc.check("f32" if f32 else "bf16", C, ref, plan.segments, what=name)
    untouched(buf, M, N, off, name)


# ------------------------------------------------------------------------------------------------------------- SwiGLU

SWIGLU_FWD = [("u4", 4000, 2048, 4096), ("s256", 4000, 2048, 1024), ("b144", 2184, 2048, 4096), ("u4_main_tail", 2184, 11008, 4096),
              ("unfused", 300, 1000, 256)]


@pytest.mark.parametrize("case", SWIGLU_FWD, ids=[c[0] for c in SWIGLU_FWD])
def test_gemm_swiglu_fwd_path(case):
    name, M, ff, K = case
    g = Gen(M + ff + K)
    X = g.mat(M, K)
    W = g.mat(2 * ff, K, K ** -0.5)
    plan = gc.path_of("swiglu_fwd", M, 0, K, ff=ff, lda=X.stride(0), ldb=W.stride(0))
    gbuf, gu = out_buf(M, 2 * ff, extra=0)   # the unfused fallback needs dense gate|up / act rows
    abuf, act = out_buf(M, ff, extra=0)
    L = _lib.load()
    run_checked(plan, name, lambda: _lib.check(L.lhrs_gemm_swiglu_fwd(X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), None, 0, None, 0, 0,
                                                                       gu.data_ptr(), gu.stride(0), act.data_ptr(), act.stride(0), M, ff, K,
                                                                       hk._stream()), "swiglu_fwd"))
    rgu, ract = gc.ref_swiglu_fwd(X, W, ff)
    gc.check("gu", gu, rgu, plan.segments, what=name + " gate|up")
    gc.check("act", act, ract, plan.segments, what=name + " act")
    untouched(gbuf, M, 2 * ff, 0, name + " gate|up")
    untouched(abuf, M, ff, 0, name + " act")


SWIGLU_BWD = [("u4", 4096, 4096, 4096, True), ("s256", 4096, 4096, 1024, False), ("b144", 2184, 4096, 4096, True),
              ("unfused_in_place", 300, 1000, 256, True), ("unfused_out_of_place", 300, 1000, 256, False)]


@pytest.mark.parametrize("case", SWIGLU_BWD, ids=[c[0] for c in SWIGLU_BWD])
def test_gemm_swiglu_bwd_path(case):
    name, M, ff, K, in_place = case
    g = Gen(M + ff + K + 1)
    dY = g.mat(M, K)
    Wd = g.mat(ff, K, K ** -0.5)
    gu_bits = torch.randn(M, 2 * ff, generator=g.g).to(torch.bfloat16).to(DEV)
    plan = gc.path_of("swiglu_bwd", M, 0, K, ff=ff, lda=dY.stride(0), ldb=Wd.stride(0))
    if in_place:
        buf, dgu = out_buf(M, 2 * ff, extra=0)
        dgu.copy_(gu_bits)
        gu = dgu
    else:
        gu = gu_bits
        buf, dgu = out_buf(M, 2 * ff, extra=0)
    gu_in = gu_bits.clone()
    scratch = torch.empty(M, ff, device=DEV, dtype=torch.bfloat16) if plan.kernels()[0].startswith("t") else None
    L = _lib.load()
    run_checked(plan, name, lambda: _lib.check(L.lhrs_gemm_swiglu_bwd(dY.data_ptr(), dY.stride(0), Wd.data_ptr(), Wd.stride(0), None, 0, None, 0, 0,
                                                                       gu.data_ptr(), dgu.data_ptr(), dgu.stride(0), hk._p(scratch), M, ff, K,
                                                                       hk._stream()), "swiglu_bwd"))
    gc.check("dgu", dgu, gc.ref_swiglu_bwd(dY, Wd, gu_in, ff), plan.segments, what=name)
    untouched(buf, M, 2 * ff, 0, name)
    if not in_place:
        assert torch.equal(gu.view(torch.int16), gu_in.view(torch.int16)), f"{name}: gate|up input was written"


# ------------------------------------------------------------------------------------------------------------- RoPE

ROPE = [("u4", 4000, 4096, 4096, 0, 128), ("u4_pair", 4000, 4096, 4096, 64, 128), ("s256", 4096, 4096, 1024, 0, 128),
        ("b144", 2184, 4096, 4096, 0, 128), ("fallback_head64_ragged_v", 4000, 4104, 1024, 0, 64)]


@pytest.mark.parametrize("case", ROPE, ids=[c[0] for c in ROPE])
def test_gemm_rope_path(case):
    name, M, N, K, K2, hd = case
    g = Gen(M + N + K + K2 + hd)
    X = g.mat(M, K)
    W = g.mat(N, K, K ** -0.5)
    A2 = g.mat(M, K2) if K2 else None
    B2 = g.mat(N, K2, 0.5 * K2 ** -0.5) if K2 else None
    rope_cols = 2048
    pos_mod, pos0 = 1000, 7
    cos_t, sin_t = gc.rope_tables(pos_mod + pos0, hd, DEV)      # exactly the positions used: a read past the last one is out of the table
    cos_t = torch.cat([cos_t, torch.full((4, hd // 2), NAN, device=DEV)])
    sin_t = torch.cat([sin_t, torch.full((4, hd // 2), NAN, device=DEV)])
    buf, C = out_buf(M, N)
    plan = gc.path_of("rope", M, N, K, K2=K2, rope_cols=rope_cols, head_dim=hd, lda=X.stride(0), ldb=W.stride(0), ldc=C.stride(0))
    L = _lib.load()
    run_checked(plan, name, lambda: _lib.check(L.lhrs_gemm_rope_fwd(X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), hk._p(A2),
                                                                     A2.stride(0) if K2 else 0, hk._p(B2), B2.stride(0) if K2 else 0, K2,
                                                                     C.data_ptr(), C.stride(0), M, N, K, cos_t.data_ptr(), sin_t.data_ptr(),
                                                                     pos_mod, pos0, rope_cols, hd, hk._stream()), "rope_fwd"))
    gc.check("rope", C, gc.ref_rope(X, W, cos_t, sin_t, pos_mod, pos0, rope_cols, hd, A2=A2, B2=B2), plan.segments, what=name)
    untouched(buf, M, N, 0, name)


# ------------------------------------------------------------------------------------------------------------- e4m3

FP8 = [("s256_whole", 4096, 4096, 4096, False), ("ragged_small_m", 300, 4096, 4096, False), ("main_small_tail_pair_res_alpha", 8736, 4096, 4096, True)]


def e4m3_rows(g, rows, K, scale):
    x = (torch.randn(rows, K, generator=g.g) * scale).to(torch.bfloat16).to(DEV)
    buf = torch.full((rows, K + 16), 0x7F, dtype=torch.uint8, device=DEV)        # 0x7F: e4m3 NaN in the padding bytes
    q, s = hk.quant_fp8_rows(x)
    buf[:, :K] = q
    return buf[:, :K], s


@pytest.mark.parametrize("case", FP8, ids=[c[0] for c in FP8])
def test_gemm_fp8_path(case):
    name, M, N, K, full = case
    g = Gen(M + N + K + 5)
    A8, sa = e4m3_rows(g, M, K, 1.0)
    B8, sb = e4m3_rows(g, N, K, K ** -0.5)
    A2 = g.mat(M, 64) if full else None
    B2 = g.mat(N, 64, 0.0625) if full else None
    res = g.mat(M, N, 0.5) if full else None
    alpha = 0.5 if full else 1.0
    buf, C = out_buf(M, N)
    plan = gc.path_of("fp8", M, N, K, K2=64 if full else 0)
    L = _lib.load()
    s = hk._stream()
    if full:
        fn = lambda: _lib.check(L.lhrs_gemm_fp8_nt_lora(A8.data_ptr(), A8.stride(0), sa.data_ptr(), B8.data_ptr(), B8.stride(0), sb.data_ptr(),
                                                        A2.data_ptr(), A2.stride(0), B2.data_ptr(), B2.stride(0), 64, C.data_ptr(), C.stride(0),
                                                        M, N, K, res.data_ptr(), res.stride(0), float(alpha), s), "fp8_lora")
    else:
        fn = lambda: _lib.check(L.lhrs_gemm_fp8_nt(A8.data_ptr(), A8.stride(0), sa.data_ptr(), B8.data_ptr(), B8.stride(0), sb.data_ptr(),
                                                   C.data_ptr(), C.stride(0), M, N, K, None, 0, float(alpha), s), "fp8")
    run_checked(plan, name, fn)
    gc.check("bf16", C, gc.ref_fp8(A8, sa, B8, sb, alpha=alpha, residual=res, A2=A2, B2=B2), plan.segments, what=name)
    untouched(buf, M, N, 0, name)


# the kernel body at its small edges: K = 256 (two stages, the minimum), K = 384 (an odd stage count), one and three bf16 stages behind them
FP8_EDGES = [("k256_ragged_no_pair", 257, 264, 256, 0), ("k384_pair64_res_alpha", 300, 520, 384, 64), ("k384_pair192_res_alpha", 70, 264, 384, 192)]


@pytest.mark.parametrize("case", FP8_EDGES, ids=[c[0] for c in FP8_EDGES])
def test_gemm_fp8_edge_shapes(case):
    name, M, N, K, K2 = case
    g = Gen(M + N + K + K2 + 6)
    A8, sa = e4m3_rows(g, M, K, 1.0)
    B8, sb = e4m3_rows(g, N, K, K ** -0.5)
    A2 = g.mat(M, K2, pad=72) if K2 else None                 # NaN in a whole stage past K2
    B2 = g.mat(N, K2, 0.5 * K2 ** -0.5, pad=72) if K2 else None
    res = g.mat(M, N, 0.5) if K2 else None
    alpha = 0.5 if K2 else 1.0
    buf, C = out_buf(M, N)
    plan = gc.path_of("fp8", M, N, K, K2=K2)
    assert plan.kernels() == ("fp8_256",)
    L = _lib.load()
    s = hk._stream()
    if K2:
        fn = lambda: _lib.check(L.lhrs_gemm_fp8_nt_lora(A8.data_ptr(), A8.stride(0), sa.data_ptr(), B8.data_ptr(), B8.stride(0), sb.data_ptr(),
                                                        A2.data_ptr(), A2.stride(0), B2.data_ptr(), B2.stride(0), K2, C.data_ptr(), C.stride(0),
                                                        M, N, K, res.data_ptr(), res.stride(0), float(alpha), s), "fp8_lora")
    else:
        fn = lambda: _lib.check(L.lhrs_gemm_fp8_nt(A8.data_ptr(), A8.stride(0), sa.data_ptr(), B8.data_ptr(), B8.stride(0), sb.data_ptr(),
                                                   C.data_ptr(), C.stride(0), M, N, K, None, 0, float(alpha), s), "fp8")
    run_checked(plan, name, fn)
    gc.check("bf16", C, gc.ref_fp8(A8, sa, B8, sb, alpha=alpha, residual=res, A2=A2, B2=B2), plan.segments, what=name)
    untouched(buf, M, N, 0, name)


# ------------------------------------------------------------------------------------------------------------- LLM.int8

INT8 = [
    # name, M, N, K, host K2, device k2 (None: no k2_dev pointer), flags
    ("min_shape_no_pair", 1, 8, 256, 0, None, dict()),
    ("ragged_device_stage", 257, 264, 256, 0, 64, dict()),
    ("odd_stages_host_pair_device_zero_res_alpha", 300, 520, 384, 64, 0, dict(res=True, alpha=0.5)),
    ("odd_plus_odd_stages_res", 70, 264, 384, 192, 128, dict(res=True)),
    ("long_k_device_stage", 40, 64, 24832, 0, 64, dict()),
    ("device_count_equals_k", 256, 256, 512, 0, 512, dict()),
]


def int8_rows(g, rows, K, scale):
    """int8 codes uniform in +-127 in a [rows, K + 16] buffer (127 in the padding bytes) and positive per-row factors around scale / 127"""
    buf = torch.full((rows, K + 16), 127, dtype=torch.int8)
    buf[:, :K] = torch.randint(-127, 128, (rows, K), generator=g.g).to(torch.int8)
    s = (0.5 + torch.rand(rows, generator=g.g)) * (scale / 127.0)
    return buf.to(DEV)[:, :K], s.to(DEV)


@pytest.mark.parametrize("case", INT8, ids=[c[0] for c in INT8])
def test_gemm_int8_path(case):
    name, M, N, K, K2, k2, f = case
    g = Gen(M + N + K + K2 + 7)
    A8, sa = int8_rows(g, M, K, 1.0)
    B8, sb = int8_rows(g, N, K, 0.02)
    rms = (73.0 / 127.0) ** 2 * 0.02 * K ** 0.5                 # of the 8-bit term: codes uniform in +-127 have RMS ~73
    K2t = K2 + (k2 or 0)
    pair = K2 > 0 or k2 is not None
    A2 = g.mat(M, K2t, 1.0, pad=72) if pair else None          # NaN in a whole stage past K2 + k2
    B2 = g.mat(N, K2t, 0.5 * rms * max(K2t, 1) ** -0.5, pad=72) if pair else None
    k2_dev = torch.tensor([k2], dtype=torch.int32, device=DEV) if k2 is not None else None
    res = g.mat(M, N, 0.5 * rms) if f.get("res") else None
    alpha = f.get("alpha", 1.0)
    buf, C = out_buf(M, N)
    plan = gc.path_of("int8", M, N, K, K2=K2)
    L = _lib.load()
    p = hk._p
    fn = lambda: _lib.check(L.lhrs_gemm_int8_nt(A8.data_ptr(), A8.stride(0), sa.data_ptr(), B8.data_ptr(), B8.stride(0), sb.data_ptr(), p(A2),
                                                A2.stride(0) if pair else 0, p(B2), B2.stride(0) if pair else 0, K2, p(k2_dev), C.data_ptr(),
                                                C.stride(0), M, N, K, p(res), res.stride(0) if res is not None else 0, float(alpha),
                                                hk._stream()), "gemm_int8_nt")
    run_checked(plan, name, fn)
    assert res is None or res.stride(0) > N
    ref = ic.ref_int8(A8, sa, B8, sb, alpha=alpha, residual=res, A2=A2, B2=B2)
    assert bool(torch.isfinite(C).all()), f"{name}: a column of A2 / B2 past K2 + k2 was read"
    rep = gc.check("bf16", C, ref, plan.segments, what=name)
    print(f"\nint8 GEMM {name}: element ratio at c = 1 {rep.elem:.4f}, cell rel-L2 {rep.cell:.3g}")
    if K2t == 0 and res is None:
        ok, ratio = ic.tight_bound_ok(C, ref.want)
        print(f"int8 GEMM {name}: worst |err| / ((2^-8 + 2^-21) |want|) {ratio:.4f}")
        assert ok, f"{name}: {ratio:.4f}x the derived bound"
    if K2t == 0:        # exact integer sums, no bf16 stage: one correctly rounded value per element
        emu = ic.emu_product(A8.cpu(), sa.cpu(), B8.cpu(), sb.cpu(), None, None, 0, alpha=alpha, residual=None if res is None else res.cpu())
        assert torch.equal(ic.bits16(C.cpu()), ic.bits16(emu)), name
    untouched(buf, M, N, 0, name)


def test_gemm_int8_no_pair_residual_is_bit_exact():
    """Without bf16 stages the product has one value per element: int32 sum, f32, (sa * alpha), sb, bf16, and the residual added in bf16 AFTER the
    store (as gemm_fp8 does).  The element bound cannot tell that order from a residual added before the store; bit equality can."""
    M, N, K = 70, 264, 384
    g = Gen(M + N + K + 8)
    A8, sa = int8_rows(g, M, K, 1.0)
    B8, sb = int8_rows(g, N, K, 0.02)
    res = g.mat(M, N, 0.1)
    buf, C = out_buf(M, N)
    L = _lib.load()
    _lib.check(L.lhrs_gemm_int8_nt(A8.data_ptr(), A8.stride(0), sa.data_ptr(), B8.data_ptr(), B8.stride(0), sb.data_ptr(), None, 0, None, 0, 0, None,
                                   C.data_ptr(), C.stride(0), M, N, K, res.data_ptr(), res.stride(0), 0.5, hk._stream()), "gemm_int8_nt")
    torch.cuda.synchronize()
    gc.check("bf16", C, ic.ref_int8(A8, sa, B8, sb, alpha=0.5, residual=res), what="int8 no pair, residual")
    emu = ic.emu_product(A8.cpu(), sa.cpu(), B8.cpu(), sb.cpu(), None, None, 0, alpha=0.5, residual=res.cpu())
    assert torch.equal(ic.bits16(C.cpu()), ic.bits16(emu))
    untouched(buf, M, N, 0, "int8 no pair, residual")


@pytest.mark.parametrize("K", [256, 384])
def test_gemm_int8_k_mapping_probe(K):
    """A8 = I (code 1 on the diagonal), unit factors: the result is B8^T exactly (integers up to 127 are exact in bf16).  Any disagreement
    between the k a byte slot of A holds and the k the same slot of B holds moves or drops an element."""
    N = 264
    g = Gen(K + 9)
    A8 = torch.eye(K, dtype=torch.int8).to(DEV)
    B8, _ = int8_rows(g, N, K, 1.0)
    ones_m, ones_n = torch.ones(K, device=DEV), torch.ones(N, device=DEV)
    buf, C = out_buf(K, N)
    L = _lib.load()
    _lib.check(L.lhrs_gemm_int8_nt(A8.data_ptr(), A8.stride(0), ones_m.data_ptr(), B8.data_ptr(), B8.stride(0), ones_n.data_ptr(), None, 0, None, 0,
                                   0, None, C.data_ptr(), C.stride(0), K, N, K, None, 0, 1.0, hk._stream()), "gemm_int8_nt")
    torch.cuda.synchronize()
    assert torch.equal(C.float(), B8.t().float())
    untouched(buf, K, N, 0, f"int8 k-mapping K={K}")


# ------------------------------------------------------------------------------------------------------------- f32 weight gradients

def test_gemm_f32_weight_gradient_family():
    for M, N, K in ((2048, 1024, 27392), (256, 128, 640)):                     # splitk_f32: 8 splits / one plain launch
        g = Gen(M + N + K)
        A, B = g.mat(M, K, 0.1), g.mat(N, K, 0.1)
        buf, C = out_buf(M, N, f32=True)
        plan = gc.path_of("splitk_f32", M, N, K, lda=A.stride(0), ldb=B.stride(0), ldc=C.stride(0))
        assert (gc.splitk_splits(M, N, K) > 1) == (M == 2048)
        run_checked(plan, f"splitk_f32 {M}", lambda: hk.gemm_nt_splitk_f32(A, B, C))
        gc.check("f32", C, gc.ref_nt(A, B), plan.segments, what=f"splitk_f32 {M}x{N}x{K}")
        untouched(buf, M, N, 0, "splitk_f32")
    for T, Mo, No in ((4320, 1024, 1024), (4321, 1024, 4096), (130, 128, 256)):  # tn_f32: splits > 1, ragged T, one split
        g = Gen(T + Mo + No)
        P, Q = g.mat(T, Mo, 0.1, pad=64), g.mat(T, No)
        buf, C = out_buf(Mo, No, f32=True)
        hk.gemm_tn_f32(P, Q, C)
        gc.check("f32", C, gc.ref_tn(P, Q), what=f"tn_f32 {T}x{Mo}x{No} splits {gc.tn_splits(T, Mo, No)}")
        untouched(buf, Mo, No, 0, "tn_f32")
    assert gc.tn_splits(4320, 1024, 1024) > 1 and gc.tn_splits(130, 128, 256) == 1
    for M, N, K in ((8190, 64, 4096), (4095, 128, 11008), (8190, 256, 4096)):    # nt_skinny: 64 x 64 and 64 x 128 tiles, split-K
        g = Gen(M + N + K)
        A, B = g.mat(M, K), g.mat(N, K, K ** -0.5)
        with hk.gemm_kernel_census() as c:
            y = hk.gemm_nt_skinny(A, B, alpha=2.0)
        assert c.launches == 1 and not c.counts
        gc.check("bf16", y, gc.ref_nt(A, B, alpha=2.0), what=f"nt_skinny {M}x{N}x{K} splits {gc.skinny_splits(K, N)}")
    for M, N, KP in ((8190, 4096, 64), (1000, 12288, 128), (70, 64, 384)):      # tn_skinny, accumulate into a non-zero C
        g = Gen(M + N + KP)
        P, Q = g.mat(M, KP), g.mat(M, N, 0.1)
        buf, C = out_buf(KP, N, f32=True)
        old = (torch.randn(KP, N, generator=g.g) * 0.5).to(DEV)
        C.copy_(old)
        hk.gemm_tn_skinny(P, Q, C, accumulate=True)
        gc.check("f32", C, gc.ref_tn(P, Q, old=old), what=f"tn_skinny {M}x{N}x{KP} splits {gc.tn_skinny_splits(M, N)}")
        untouched(buf, KP, N, 0, "tn_skinny")
    assert gc.tn_skinny_splits(8190, 4096) > 1


def test_gemm_table_reaches_every_cell():
    """The tables above reach every (entry point, segment kernels) cell that default settings can reach; prints the worst measured values
    behind gemm_cases.BOUNDS."""
    print("\nGEMM worst (element ratio at c = 1, cell rel-L2):", {k: (round(e, 4), float(f"{c:.3g}")) for k, (e, c) in sorted(gc.WORST.items())})
    paths = [(c[1], nt_plan(c).kernels()) for c in NT]
    paths += [("swiglu_fwd", gc.path_of("swiglu_fwd", M, 0, K, ff=ff).kernels()) for _, M, ff, K in SWIGLU_FWD]
    paths += [("swiglu_bwd", gc.path_of("swiglu_bwd", M, 0, K, ff=ff).kernels()) for _, M, ff, K, _ in SWIGLU_BWD]
    paths += [("rope", gc.path_of("rope", M, N, K, K2=K2, rope_cols=2048, head_dim=hd).kernels()) for _, M, N, K, K2, hd in ROPE]
    paths += [("fp8", gc.path_of("fp8", M, N, K, K2=64 if full else 0).kernels()) for _, M, N, K, full in FP8]
    paths += [("int8", gc.path_of("int8", M, N, K, K2=K2).kernels()) for _, M, N, K, K2, _, _ in INT8]
    reached = set().union(*(gc.cells_of(e, ks) for e, ks in paths))
    missing = gc.reachable_cells() - reached
    assert not missing, sorted(missing)
