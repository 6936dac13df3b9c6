"""The tools of tests/gemm_cases.py on the CPU: the comparator rejects subtly wrong GEMM results (each mutation of a float64 reference
by at least 3x its bound, while the reference rounded to the output type passes), the old whole-matrix rel-L2 check would not, and
path_of's restated host rules agree with the ones the library exports."""
import ctypes
import math
from collections import Counter

import pytest
import torch

from lhrs_bot_amd import _lib

import gemm_cases as gc

M, N, K = 192, 256, 256


def bf(x):
    return x.to(torch.bfloat16)


@pytest.fixture(scope="module")
def ops():
    g = torch.Generator().manual_seed(3)
    r = lambda *s, sc=1.0: bf(torch.randn(*s, generator=g) * sc)
    d = dict(A=r(M, K), B=r(N, K, sc=0.1), A2=r(M, 64), B2=r(N, 64, sc=0.3), bias=r(N, sc=1.0), res=r(M, N, sc=1.0), old=torch.randn(M, N, generator=g))
    d["gu"] = r(M, 2 * N, sc=2.0)
    d["cos"], d["sin"] = gc.rope_tables(M + 8, 128, "cpu")
    return d


def as_bf16(ref):
    return ref.want.to(torch.bfloat16)


def worst(kind, got, ref):
    return gc.measure(kind, got, ref)


def _nt(o, **kw):
    base = dict(alpha=0.5, bias=o["bias"], residual=o["res"], act=3, A2=o["A2"], B2=o["B2"])
    base.update(kw)
    return gc.ref_nt(o["A"], o["B"], **base)


def _mask(o, seed):
    return gc.ref_nt(o["A"], o["B"], alpha=0.5, residual=o["res"], mask=gc.drop_mask(M, N, seed, 0.3, "cpu"))


def _zero_frag(t, m0=48, n0=96):
    t = t.clone()
    t[m0:m0 + 16, n0:n0 + 16] = 0
    return t


def _transpose_frag(t, m0=48, n0=96):
    t = t.clone()
    t[m0:m0 + 16, n0:n0 + 16] = t[m0:m0 + 16, n0:n0 + 16].t().clone()
    return t


def _short_k(o, rows, cols):
    """rows x cols of the result miss the last 64-k stage of the base product"""
    A = o["A"].clone()
    want = _nt(o).want.clone()
    A[:, K - 64:] = 0
    short = gc.ref_nt(A, o["B"], alpha=0.5, bias=o["bias"], residual=o["res"], act=3, A2=o["A2"], B2=o["B2"]).want
    want[rows, cols] = short[rows, cols]
    return bf(want)


def _residual_shift(o):
    res = o["res"].clone()
    res[M - 64:M - 1] = o["res"][M - 63:M]            # the last tile row reads row m + 1
    return as_bf16(_nt(o, residual=res))


def _alpha_after_residual(o):
    r = gc.ref_nt(o["A"], o["B"], bias=o["bias"], act=3, A2=o["A2"], B2=o["B2"])
    return bf(0.5 * (r.want + o["res"].double()))


def _pair_dropped_in_tile(o):
    want = _nt(o).want.clone()
    nopair = gc.ref_nt(o["A"], o["B"], alpha=0.5, bias=o["bias"], residual=o["res"], act=3).want
    want[128:192, 128:256] = nopair[128:192, 128:256]
    return bf(want)


def _swiglu(o, swap=False):
    W = torch.cat([o["B"], bf(o["B"].float().flip(0))])            # gate rows, then up rows
    gu, act = gc.ref_swiglu_fwd(o["A"], W, N)
    if swap:
        W2 = torch.cat([W[N:], W[:N]])
        gu2, act2 = gc.ref_swiglu_fwd(o["A"], W2, N)
        return bf(act2.want), act
    return bf(act.want), act


def _rope(o, mutate=False):
    ref = gc.ref_rope(o["A"], torch.cat([o["B"], o["B"]]), o["cos"], o["sin"], 100, 5, 256, 128)
    if not mutate:
        return bf(ref.want), ref
    wrong = gc.ref_rope(o["A"], torch.cat([o["B"], o["B"]]), o["cos"], o["sin"], 10 ** 6, 0, 256, 128).want   # position m, not m % 100 + 5
    got = ref.want.clone()
    got[:, 128:256] = wrong[:, 128:256]                                                                       # on one head
    return bf(got), ref


def _accumulate(o, ignore):
    ref = gc.ref_nt(o["A"], o["B"], old=o["old"])
    if ignore:
        return gc.ref_nt(o["A"], o["B"]).want.float(), ref
    return ref.want.float(), ref


MUTATIONS = {
    "fragment_zeroed": lambda o: ("bf16", _zero_frag(as_bf16(_nt(o))), _nt(o)),
    "fragment_transposed": lambda o: ("bf16", _transpose_frag(as_bf16(_nt(o))), _nt(o)),
    "row_missing_last_k_stage": lambda o: ("bf16", _short_k(o, slice(77, 78), slice(0, N)), _nt(o)),
    "fragment_missing_last_k_stage": lambda o: ("bf16", _short_k(o, slice(32, 48), slice(16, 32)), _nt(o)),
    "bias_shifted_4_columns": lambda o: ("bf16", as_bf16(_nt(o, bias=torch.roll(o["bias"], 4))), _nt(o)),
    "residual_from_next_row_in_last_tile_row": lambda o: ("bf16", _residual_shift(o), _nt(o)),
    "alpha_after_residual": lambda o: ("bf16", _alpha_after_residual(o), gc.ref_nt(o["A"], o["B"], alpha=0.5, bias=o["bias"], residual=o["res"],
                                                                               act=3, A2=o["A2"], B2=o["B2"])),
    "pair_dropped_in_one_tile": lambda o: ("bf16", _pair_dropped_in_tile(o), _nt(o)),
    "gate_and_up_swapped": lambda o: ("act",) + _swiglu(o, swap=True),
    "rope_position_m_on_one_head": lambda o: ("rope",) + _rope(o, mutate=True),
    "mask_seed_off_by_one": lambda o: ("bf16", as_bf16(_mask(o, 1235)), _mask(o, 1234)),
    "accumulate_ignores_old_c": lambda o: ("f32",) + _accumulate(o, ignore=True),
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_comparator_rejects_mutation_by_3x(ops, mutation):
    kind, got, ref = MUTATIONS[mutation](ops)
    rep = worst(kind, got, ref)
    assert rep.ratio >= 3.0, (mutation, rep)


@pytest.mark.parametrize("name", ["nt", "mask", "act", "rope", "f32", "swiglu_bwd", "fp8"])
def test_reference_rounded_to_the_output_type_passes(ops, name):
    o = ops
    if name == "nt":
        kind, ref = "bf16", _nt(o)
        got = as_bf16(ref)
    elif name == "mask":
        kind, ref = "bf16", _mask(o, 7)
        got = as_bf16(ref)
    elif name == "act":
        kind, (got, ref) = "act", _swiglu(o)
    elif name == "rope":
        kind, (got, ref) = "rope", _rope(o)
    elif name == "f32":
        kind, (got, ref) = "f32", _accumulate(o, ignore=False)
    elif name == "swiglu_bwd":
        kind, ref = "dgu", gc.ref_swiglu_bwd(o["A"], o["B"], o["gu"], N)
        got = as_bf16(ref)
    else:
        a8 = o["A"].float().clamp(-400, 400).to(torch.float8_e4m3fn).view(torch.uint8)
        b8 = (o["B"].float() * 10).to(torch.float8_e4m3fn).view(torch.uint8)
        sa, sb = torch.full((M,), 0.5), torch.full((N,), 0.1)
        kind, ref = "bf16", gc.ref_fp8(a8, sa, b8, sb, alpha=0.5, residual=o["res"], A2=o["A2"], B2=o["B2"])
        got = as_bf16(ref)
    rep = worst(kind, got, ref)
    assert rep.ratio <= 1.0, rep.where


def test_sentinel_check_sees_one_column_past_n():
    buf = torch.full((M + 3, N + 8), -1, dtype=torch.int16)
    assert bool((buf[:, N:] == -1).all())
    buf[5, N] = 0x3F80                                   # one column past N written
    assert not bool((buf[:, N:] == -1).all()) and not bool((buf[M:] != -1).any())


def test_comparator_names_the_worst_element_and_segment(ops):
    ref = _nt(ops)
    got = as_bf16(ref).clone()
    got[130, 17] = float("nan")
    rep = gc.measure("bf16", got, ref, segments=[(0, 128, "256"), (128, M, "t64x128")])
    assert rep.ratio == float("inf") and "element (130, 17) [t64x128 rows 128..191]" in rep.where, rep.where


def test_old_whole_matrix_check_misses_one_fragment_at_8190x4096():
    """rel_err(out, ref) < 4e-3 (test_kernels_gpu.py) over 8190 x 4096 elements of unit RMS: one zeroed 16 x 16 fragment, or one fragment of
    wrong values at the right scale (error RMS sqrt(2)), moves it by sqrt(256 / (8190 * 4096)) resp. sqrt(2 * 256 / ...): both pass."""
    zeroed = math.sqrt(256 / (8190 * 4096))
    wrong = math.sqrt(2 * 256 / (8190 * 4096))
    assert zeroed < 4e-3 and wrong < 4e-3
    # the per-cell bound sees either of them: a 64 x 64 cell with one of its 16 fragments zeroed has rel-L2 1 / 4
    assert math.sqrt(256 / 4096) / gc.BOUNDS["bf16"][2] > 3


def test_drop_keep_restatement_matches_the_device_rule_on_known_values():
    # lowbias32 of (idx * 0x9E3779B1) ^ seed, computed by hand for idx 0 and 1, seed 0: x = 0 stays 0; x = 0x9E3779B1 ...
    idx = torch.tensor([0, 1, 2 ** 32 + 5], dtype=torch.int64)
    keep = gc.drop_keep(0, idx, 1)
    assert not bool(keep[0])                               # lowbias32(0) == 0 < 1
    x = 0x9E3779B1
    x ^= x >> 16; x = (x * 0x7FEB352D) & gc.M32; x ^= x >> 15; x = (x * 0x846CA68B) & gc.M32; x ^= x >> 16
    assert bool(gc.drop_keep(0, idx[1:2], x)) and not bool(gc.drop_keep(0, idx[1:2], x + 1))
    hi = ((5 * 0x9E3779B1) & gc.M32) ^ (0x85EBCA77 & gc.M32)
    y = hi; y ^= y >> 16; y = (y * 0x7FEB352D) & gc.M32; y ^= y >> 15; y = (y * 0x846CA68B) & gc.M32; y ^= y >> 16
    assert bool(gc.drop_keep(0, idx[2:3], y)) and not bool(gc.drop_keep(0, idx[2:3], y + 1))


# ---------------------------------------------------------------------------------------------------------------------- host rules

SHAPES_M = (1, 300, 1000, 1023, 1024, 2000, 2184, 3000, 3839, 3840, 4000, 4095, 4096, 4368, 7710, 8190, 8192, 8714, 8736, 16380, 27360)
SHAPES_N = (64, 264, 1000, 1024, 2048, 4096, 4100, 11008, 12288, 32000)
SHAPES_K = (64, 256, 1024, 4032, 4096, 4160, 11008, 22016)


def test_path_rules_match_the_exported_host_rules():
    lib = _lib.load()
    lib.lhrs_gemm_set_u4(1)
    for Mv in SHAPES_M:
        for Nv in SHAPES_N:
            assert lib.lhrs_gemm_u4_main_rows(Mv, Nv) == gc.u4_main_rows(Mv, gc.cdiv(Nv, 256)), (Mv, Nv)
            assert lib.lhrs_tn_skinny_splits(Mv, Nv) == gc.tn_skinny_splits(Mv, Nv), (Mv, Nv)
            for Kv in SHAPES_K:
                for ldc in (Nv, Nv + 4, Nv + 8):
                    got = lib.lhrs_gemm_u4_takes(Mv, Nv, Kv, Kv, Kv, ldc, 0, 0, 0, 0, 0, 1.0)
                    assert got == gc.u4_takes(Mv, Nv, Kv, Kv, Kv, ldc), (Mv, Nv, Kv, ldc)
                assert lib.lhrs_gemm_u4_takes(Mv, Nv, Kv, Kv, Kv, Nv, 0, 1, 0, 0, 0, 1.0) == 0
                assert lib.lhrs_gemm_splitk_splits(Mv, Nv, Kv) == gc.splitk_splits(Mv, Nv, Kv), (Mv, Nv, Kv)
                if Nv <= 384:
                    assert lib.lhrs_gemm_skinny_splits(Kv, Nv) == gc.skinny_splits(Kv, Nv), (Kv, Nv)
                for kind in (0, 1, 2):
                    for K2 in (0, 64, 96):
                        tn = gc.cdiv(Nv, 256) if kind != 1 else Nv // 128
                        assert lib.lhrs_gemm_u4_fused_takes(kind, Mv, tn, Kv, K2) == gc.u4_fused_takes(kind, Mv, tn, Kv, K2), (kind, Mv, Nv, Kv, K2)
                for K2 in (0, 64):
                    ff = Nv
                    want = (gc.swiglu_fusable(gc.cdiv(Mv, 256) * (ff // 128), ff, Kv, K2) and
                            gc.swiglu_fusable(gc.cdiv(Mv, 256) * gc.cdiv(ff, 256), ff, Kv, K2))
                    assert lib.lhrs_gemm_swiglu_fusable(Mv, ff, Kv, Kv, K2) == int(want), (Mv, ff, Kv, K2)
    for T in (1, 64, 130, 4320, 4321, 27360):
        for Mo in (128, 1024, 2048, 4096):
            for No in (128, 256, 1024, 4096):
                assert lib.lhrs_gemm_tn_splits(T, Mo, No) == gc.tn_splits(T, Mo, No), (T, Mo, No)


def test_path_of_hand_worked_shapes():
    P = gc.path_of
    # 8736 x 4096: 35 x 16 = 560 tiles -> 2 full rounds of 256 CUs cover 32 tile rows (8192 rows); 544 tail rows
    p = P("nt", 8736, 4096, 11008)
    assert p.segments == [(0, 8192, "u4"), (8192, 8736, "splitk_tail")] and p.kinds == {6: 1} and p.launches == 2
    p = P("nt", 8736, 4096, 4096)
    assert p.segments == [(0, 8192, "u4"), (8192, 8736, "t64x128")] and p.launches == 2
    p = P("lora", 8736, 4096, 4096, K2=64)
    assert p.kernels() == ("u4", "t64x128", "t64x128") and p.launches == 3         # the pair's two-launch tail: base, then the rank-64 update
    assert P("nt", 3839, 4104, 4096, res=True, ldc=4112).kernels() == ("u4",)
    assert P("nt", 4000, 4096, 1024, bias=True, act=1).kernels() == ("256",)
    assert P("nt", 8736, 4096, 4096, bias=True).segments == [(0, 8192, "256"), (8192, 8736, "t64x128")]
    assert P("nt", 2184, 4096, 4096, act=2, bias=True).kernels() == ("144",)
    assert P("nt", 7710, 1024, 1024, bias=True, res=True).kernels() == ("144",)    # the override: 124 tiles of 256 rows, 216 of 144
    assert P("nt", 3000, 2048, 512).kernels() == ("t128",) and P("nt", 2000, 1024, 256).kernels() == ("t64x128",)
    assert P("nt", 300, 264, 320).kernels() == ("t64x64",)
    assert P("nt", 8190, 4100, 4096).kernels() == ("t128",)                        # N % 8 == 4: no 16-B epilogue rows
    assert P("nt", 8190, 4096, 4096, al16_ptrs=False).kernels() == ("256",)        # 8-B aligned operands: not the four-wave kernel
    assert P("mask", 4096, 4096, 128).kernels() == ("256",) and P("mask", 300, 4096, 64).kernels() == ("t64x64",)
    assert P("swiglu_fwd", 4000, 0, 4096, ff=2048).kernels() == ("u4_swiglu_fwd",)
    assert P("swiglu_fwd", 2184, 0, 4096, ff=11008).segments == [(0, 2048, "u4_swiglu_fwd"), (2048, 2184, "t64x128")]
    assert P("swiglu_fwd", 300, 0, 256, ff=1000).kernels() == ("t64x64",)
    assert P("swiglu_bwd", 4096, 0, 4096, ff=4096).kernels() == ("u4_swiglu_bwd",)
    assert P("rope", 4000, 4096, 4096, rope_cols=2048).kernels() == ("u4_rope",)
    assert P("rope", 2184, 4096, 4096, rope_cols=2048).kernels() == ("rope_144",)
    assert P("fp8", 8736, 4096, 4096).segments == [(0, 8192, "fp8_256"), (8192, 8736, "fp8_small")]
    assert P("int8", 8736, 4096, 4096).segments == [(0, 8736, "i8_256")] and P("int8", 1, 8, 256).launches == 1   # no tail split for int8
    assert P("splitk_f32", 2048, 1024, 27392).kernels() == ("splitk_f32",) and P("splitk_f32", 256, 128, 640).kernels() == ("t64x64",)


# ---------------------------------------------------------------------------------------------------------------------- the library's planner
# lhrs_gemm_plan (csrc/gemm_plan.h, the planner every GEMM entry point runs through) against path_of, which stays the reference.

_ENTRY = {"nt": 0, "lora": 0, "mask": 0, "swiglu_fwd": 1, "swiglu_bwd": 2, "rope": 3, "fp8": 4, "int8": 5, "splitk_f32": 6}


def lib_plan(lib, entry, Mv, Nv, Kv, *, K2=0, bias=False, res=False, act=0, out_f32=False, accumulate=False, alpha=1.0, ldc=None, ldr=None, ff=0,
             rope_cols=0, head_dim=128, al16_ptrs=True, cus=256, workspace=True):
    """lhrs_gemm_plan with path_of's arguments (dense operands but ldc and ldr) -> (segments, Counter of profile kinds, launches)"""
    flags = 1 * bias | 2 * res | 4 * out_f32 | 8 * accumulate | 16 * (entry == "mask")
    quads = (ctypes.c_int * 32)()
    n = lib.lhrs_gemm_plan(_ENTRY[entry], Mv, Nv, Kv, K2, flags, act, alpha, Kv, Kv, Nv if ldc is None else ldc, Nv if ldr is None else ldr, ff, 2 * ff, ff, rope_cols, head_dim,
                           16 if al16_ptrs else 8, cus, int(workspace), quads, 8)
    assert 0 < n <= 8, (entry, Mv, Nv, Kv, n)
    segments = [(quads[4 * i], quads[4 * i + 1], lib.lhrs_gemm_kernel_name(quads[4 * i + 2]).decode()) for i in range(n)]
    return segments, Counter(quads[4 * i + 3] for i in range(n) if quads[4 * i + 3] >= 0), n


def _same_plan(lib, entry, Mv, Nv, Kv, **kw):
    want = gc.path_of(entry, Mv, Nv, Kv, **kw)
    got = lib_plan(lib, entry, Mv, Nv, Kv, **kw)
    assert got == (want.segments, want.kinds, want.launches), (entry, Mv, Nv, Kv, kw, got, want.segments, want.kinds)


_NT_FLAGS = (("nt", {}), ("nt", dict(bias=True)), ("nt", dict(bias=True, act=1)), ("nt", dict(act=3)), ("nt", dict(res=True)), ("nt", dict(alpha=0.5)),
             ("nt", dict(out_f32=True)), ("nt", dict(out_f32=True, accumulate=True)), ("lora", dict(K2=64)), ("lora", dict(K2=64, res=True)),
             ("lora", dict(K2=64, out_f32=True)), ("mask", {}), ("mask", dict(res=True)))
_FFS = (1000, 2048, 4096, 11008)


@pytest.mark.parametrize("cus", [256, 304])
@pytest.mark.parametrize("workspace", [True, False])
def test_library_plan_equals_path_of(cus, workspace):
    """Segments, profile kinds and launch count of lhrs_gemm_plan == path_of over SHAPES_M x SHAPES_N x SHAPES_K and every entry / flag combination
    reachable_paths sweeps, on 256 and 304 CUs (where the CU-count and the 256-round copies of the tail-row rule differ), with and without a workspace."""
    lib = _lib.load()
    lib.lhrs_gemm_set_u4(1)
    kw = dict(cus=cus, workspace=workspace)
    for Mv in SHAPES_M:
        for Nv in SHAPES_N:
            for Kv in SHAPES_K:
                for entry, f in _NT_FLAGS:
                    _same_plan(lib, entry, Mv, Nv, Kv, **f, **kw)
                _same_plan(lib, "nt", Mv, Nv, Kv, ldc=Nv + 8, **kw)                  # strided output (16-B rows when N % 8 == 0)
                _same_plan(lib, "nt", Mv, Nv, Kv, res=True, ldc=Nv + 8, **kw)
                for ldr in (Nv + 4, Nv + 8):                                         # residual rows that are / are not 16-B multiples
                    _same_plan(lib, "nt", Mv, Nv, Kv, res=True, ldr=ldr, **kw)
                    _same_plan(lib, "lora", Mv, Nv, Kv, K2=64, res=True, ldr=ldr, **kw)
                for entry in ("fp8", "int8", "splitk_f32"):
                    _same_plan(lib, entry, Mv, Nv, Kv, **kw)
                for K2 in (0, 64):
                    _same_plan(lib, "rope", Mv, Nv, Kv, K2=K2, rope_cols=Nv // 512 * 256, **kw)
        for ff in _FFS:
            for Kv in SHAPES_K:
                for K2 in (0, 64):
                    _same_plan(lib, "swiglu_fwd", Mv, 0, Kv, K2=K2, ff=ff, **kw)
                    _same_plan(lib, "swiglu_bwd", Mv, 0, Kv, K2=K2, ff=ff, **kw)


def test_library_plan_with_8_byte_aligned_operands(monkeypatch):
    """Operands that are only 8-byte aligned never reach the four-wave kernel.  The plain entry points: path_of(al16_ptrs=False).  The fused ones
    (path_of's flag covers the plain entries only): the plan the declining wrappers of gemm_u4.hip used to leave - path_of at the same shape with
    its u4_fused_takes branch never taken."""
    lib = _lib.load()
    lib.lhrs_gemm_set_u4(1)
    for Mv in SHAPES_M:
        for Nv in SHAPES_N:
            for Kv in SHAPES_K:
                for entry, f in _NT_FLAGS:
                    _same_plan(lib, entry, Mv, Nv, Kv, al16_ptrs=False, **f)
    monkeypatch.setattr(gc, "u4_fused_takes", lambda *a, **k: False)
    for Mv in SHAPES_M:
        for Nv in SHAPES_N:
            for Kv in SHAPES_K:
                for K2 in (0, 64):
                    _same_plan(lib, "rope", Mv, Nv, Kv, K2=K2, rope_cols=Nv // 512 * 256, al16_ptrs=False)
        for ff in _FFS:
            for Kv in SHAPES_K:
                for entry in ("swiglu_fwd", "swiglu_bwd"):
                    _same_plan(lib, entry, Mv, 0, Kv, ff=ff, al16_ptrs=False)


def test_hand_worked_shapes_come_out_of_the_library():
    """The expectations of test_path_of_hand_worked_shapes, verbatim, asked of lhrs_gemm_plan."""
    lib = _lib.load()
    lib.lhrs_gemm_set_u4(1)

    class L:
        def __init__(self, entry, Mv, Nv, Kv, **kw):
            self.segments, self.kinds, self.launches = lib_plan(lib, entry, Mv, Nv, Kv, **kw)

        def kernels(self):
            return tuple(k for _, _, k in self.segments)

    P = L
    p = P("nt", 8736, 4096, 11008)
    assert p.segments == [(0, 8192, "u4"), (8192, 8736, "splitk_tail")] and p.kinds == {6: 1} and p.launches == 2
    p = P("nt", 8736, 4096, 4096)
    assert p.segments == [(0, 8192, "u4"), (8192, 8736, "t64x128")] and p.launches == 2
    p = P("lora", 8736, 4096, 4096, K2=64)
    assert p.kernels() == ("u4", "t64x128", "t64x128") and p.launches == 3
    assert P("nt", 3839, 4104, 4096, res=True, ldc=4112).kernels() == ("u4",)
    assert P("nt", 4000, 4096, 1024, bias=True, act=1).kernels() == ("256",)
    assert P("nt", 8736, 4096, 4096, bias=True).segments == [(0, 8192, "256"), (8192, 8736, "t64x128")]
    assert P("nt", 2184, 4096, 4096, act=2, bias=True).kernels() == ("144",)
    assert P("nt", 7710, 1024, 1024, bias=True, res=True).kernels() == ("144",)
    assert P("nt", 3000, 2048, 512).kernels() == ("t128",) and P("nt", 2000, 1024, 256).kernels() == ("t64x128",)
    assert P("nt", 300, 264, 320).kernels() == ("t64x64",)
    assert P("nt", 8190, 4100, 4096).kernels() == ("t128",)
    assert P("nt", 8190, 4096, 4096, al16_ptrs=False).kernels() == ("256",)
    assert P("mask", 4096, 4096, 128).kernels() == ("256",) and P("mask", 300, 4096, 64).kernels() == ("t64x64",)
    assert P("swiglu_fwd", 4000, 0, 4096, ff=2048).kernels() == ("u4_swiglu_fwd",)
    assert P("swiglu_fwd", 2184, 0, 4096, ff=11008).segments == [(0, 2048, "u4_swiglu_fwd"), (2048, 2184, "t64x128")]
    assert P("swiglu_fwd", 300, 0, 256, ff=1000).kernels() == ("t64x64",)
    assert P("swiglu_bwd", 4096, 0, 4096, ff=4096).kernels() == ("u4_swiglu_bwd",)
    assert P("rope", 4000, 4096, 4096, rope_cols=2048).kernels() == ("u4_rope",)
    assert P("rope", 2184, 4096, 4096, rope_cols=2048).kernels() == ("rope_144",)
    assert P("fp8", 8736, 4096, 4096).segments == [(0, 8192, "fp8_256"), (8192, 8736, "fp8_small")]
    assert P("int8", 8736, 4096, 4096).segments == [(0, 8736, "i8_256")] and P("int8", 1, 8, 256).launches == 1
    assert P("splitk_f32", 2048, 1024, 27392).kernels() == ("splitk_f32",) and P("splitk_f32", 256, 128, 640).kernels() == ("t64x64",)


def test_reachable_cells():
    cells = gc.reachable_cells()
    kernels = {k for _, ks in gc.reachable_paths() for k in ks}
    assert {k for _, k in cells} <= kernels | {"unfused"} and ("rope", "unfused") in cells and ("lora", "144") in cells
    assert ("int8", "i8_256") in cells and {k for e, k in cells if e == "int8"} == {"i8_256"}
    assert kernels >= {"u4", "splitk_tail", "256", "144", "t128", "t64x128", "t64x64", "u4_swiglu_fwd", "swiglu_fwd_256", "swiglu_fwd_144",
                       "u4_swiglu_bwd", "swiglu_bwd_256", "swiglu_bwd_144", "u4_rope", "rope_256", "rope_144", "fp8_256", "fp8_small", "i8_256"}, kernels
