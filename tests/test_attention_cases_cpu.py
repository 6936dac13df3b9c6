"""The tools of tests/attention_cases.py on the CPU: the comparator rejects subtly wrong attention results (each mutation of the float64
reference by at least 3x its bound while the reference rounded to bf16 passes), and path_of restates the host dispatch of
csrc/attention.hip on hand-worked shapes and agrees with the plan the library exports."""
import ctypes

import pytest
import torch

from lhrs_bot_amd import _lib

from attention_cases import BOUNDS, Path, Seq, measure, path_of, reachable_cells, ref_attention64, rope_tables, self_entries

D, H = 64, 2
# a compact-tail layout (causal_off = p0 > 0, q_len < kv_rows, padded keys) with a half last query tile (81 = 64 + 17) next to a plain one
SEQS = [Seq(120, 95, 20, 81), Seq(100, 100, 0, 100)]   # key 95 is within the causal reach of the last queries (<= 80 + 20)
SCALE = D ** -0.5
NAMES = ("o", "lse", "delta", "dq", "dk", "dv")


@pytest.fixture(scope="module")
def inputs():
    entries, T = self_entries(SEQS)
    g = torch.Generator().manual_seed(0)
    q, k, v, do = (torch.randn(T, H * D, generator=g).to(torch.bfloat16) for _ in range(4))
    cos_t, sin_t = rope_tables(T + 4, D, "cpu")   # one more position for the shifted-RoPE mutation
    rope = (cos_t, sin_t, T, 3)
    want = ref_attention64(q, k, v, do, entries, H, D, SCALE, True, rope=rope)
    return dict(entries=entries, q=q, k=k, v=v, do=do, rope=rope, want=want)


def as_kernel_output(ref):
    """what a kernel returns: bf16 rows, fp32 statistics"""
    return [{n: (r[n].float() if n in ("lse", "delta") else r[n].to(torch.bfloat16)) for n in NAMES} for r in ref]


def worst(got, want):
    reps = [measure(n, [g[n] for g in got], [w[n] for w in want]) for n in NAMES]
    return max(reps, key=lambda r: r.ratio)


def test_reference_rounded_to_bf16_passes(inputs):
    rep = worst(as_kernel_output(inputs["want"]), inputs["want"])
    assert rep.ratio < 0.5, rep.where


def _mutated_ref(inputs, entries=None, rope=None, do=None):
    return ref_attention64(inputs["q"], inputs["k"], inputs["v"], inputs["do"] if do is None else do, entries or inputs["entries"], H, D,
                           SCALE, True, rope=rope or inputs["rope"])


def _with(entries, seq, field, delta):
    e = [list(x) for x in entries]
    e[seq][field] += delta
    return [tuple(x) for x in e]


def _swap_heads(out):
    return [{n: t[:, [1, 0]] for n, t in r.items()} for r in out]


def _zero_group(out, name, seq, head, row0):
    out = [dict(r) for r in out]
    t = out[seq][name].clone()
    t[row0:row0 + 16, head] = 0
    out[seq][name] = t
    return out


def _drop_last_half_tile(inputs):
    """the 17 queries of sequence 0's last (half) tile contribute nothing: what a dK/dV kernel that skips that tile would return"""
    q_off, q_len = inputs["entries"][0][:2]
    do = inputs["do"].clone()
    do[q_off + 64:q_off + q_len] = 0
    return _mutated_ref(inputs, do=do)


MUTATIONS = {
    "causal_off+1": lambda i: as_kernel_output(_mutated_ref(i, entries=_with(i["entries"], 0, 5, +1))),
    "causal_off-1": lambda i: as_kernel_output(_mutated_ref(i, entries=_with(i["entries"], 0, 5, -1))),
    "kv_len+1": lambda i: as_kernel_output(_mutated_ref(i, entries=_with(i["entries"], 0, 3, +1))),
    "rope_pos+1": lambda i: as_kernel_output(_mutated_ref(i, rope=i["rope"][:3] + (i["rope"][3] + 1,))),
    "heads_swapped": lambda i: _swap_heads(as_kernel_output(i["want"])),
    "row_group_zeroed": lambda i: _zero_group(as_kernel_output(i["want"]), "dq", 1, 1, 48),
    "last_half_tile_dropped": lambda i: as_kernel_output(_drop_last_half_tile(i)),
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_comparator_rejects_mutation_by_3x(inputs, mutation):
    rep = worst(MUTATIONS[mutation](inputs), inputs["want"])
    assert rep.ratio >= 3.0, (mutation, rep)


def test_comparator_names_the_worst_cell():
    want = [torch.randn(40, 3, 8, dtype=torch.float64), torch.randn(20, 3, 8, dtype=torch.float64)]
    got = [w.clone() for w in want]
    got[1][17, 2, 5] += 1.0
    rep = measure("o", got, want)
    assert rep.ratio > 1 and "seq 1 head 2 rows 16..31" in rep.where, rep
    got[1][17, 2, 5] = float("nan")
    assert measure("o", got, want).ratio == float("inf")
    lw = [torch.tensor([[float("-inf"), 1.0]], dtype=torch.float64)]
    assert measure("lse", [lw[0].clone()], lw).ratio == 0.0
    assert measure("lse", [torch.tensor([[0.0, 1.0]], dtype=torch.float64)], lw).ratio == float("inf")


def test_bounds_are_bf16_level():
    for name, (rel, mx) in BOUNDS.items():
        assert 0 < rel <= mx < 0.05, name


def test_path_of_hand_worked_shapes():
    # D = 128: resident rows 320; the dK/dV image of 288 queries + lse | delta of LTq = 320: 288*256 + 8*320 = 76288 <= 81920
    assert path_of(128, 288, 320, 320) == Path("res", "res", "res", "none", "input", 1)
    # 289 queries: 320*256 alone fills the half of the LDS
    assert path_of(128, 289, 320, 320) == Path("res", "res", "tiled", "none", "input", 1)
    assert path_of(128, 320, 320, 320, rope=True, bwd_o=True) == Path("res", "res", "tiled", "separate", "dq_res", 1)
    assert path_of(128, 288, 321, 320, rope=True, bwd_o=True) == Path("tiled", "tiled", "res", "separate", "delta_kernel", 1)
    assert path_of(128, 288, 288, 320, rope=True, bwd_o=True) == Path("res", "res", "res", "fused", "dq_res", 1)
    # D = 64: resident rows 640; 576*128 + 8*576 = 78336 fits, 577 -> 608*128 + 8*640 = 82944 does not
    assert path_of(64, 576, 640, 576) == Path("res", "res", "res", "none", "input", 1)
    assert path_of(64, 577, 640, 640) == Path("res", "res", "tiled", "none", "input", 1)
    assert path_of(64, 576, 641, 576, bwd_o=True) == Path("tiled", "tiled", "res", "none", "delta_kernel", 1)
    # LTq > pad64(max_q) (the compact tail: LTq = pad64(S)): the row statistics take LDS room of their own
    assert path_of(128, 288, 300, 1024).dkv == "res" and path_of(128, 288, 300, 1088).dkv == "tiled"
    assert path_of(64, 576, 600, 1024).dkv == "res" and path_of(64, 576, 600, 1088).dkv == "tiled"
    assert path_of(128, 64, 273, 320, rope=True, bwd_o=True) == Path("res", "res", "res", "fused", "dq_res", 1)   # the product's last layer
    # the key mask lives in the tiled forward only; max_kv 0 never takes the resident forward
    assert path_of(128, 100, 200, 128, key_mask=True).fwd == "tiled" and path_of(128, 100, 0, 128).fwd == "tiled"
    # 16-byte stores need every row stride % 8 == 0 and every pointer 16-byte aligned
    assert path_of(128, 64, 64, 64, strides=[3 * 4096] * 3, ptrs=[0, 8192, 16384]).wide == 1
    assert path_of(128, 64, 64, 64, strides=[3 * 4096] * 3, ptrs=[8, 8200, 16392]).wide == 0
    assert path_of(128, 64, 64, 64, strides=[4100, 4096, 4096], ptrs=[0, 0, 0]).wide == 0


# ---------------------------------------------------------------------------------------------------------------------- the library's planner
# lhrs_attn_plan (csrc/attn_plan.h, the planner every attention entry point runs through) against path_of, which stays the reference.

_ENTRY = {"fwd": 0, "fwd_kmask": 1, "bwd": 2, "bwd_rope": 3, "bwd_o": 4}


def lib_plan(lib, entry, D, max_q, max_kv, LTq, rope=False, out_wide=1):
    """lhrs_attn_plan -> (kernel names in launch order, flags: 1 wide | 2 rope fused | 4 delta written by the resident dQ kernel)"""
    kernels, flags = (ctypes.c_int * 8)(), ctypes.c_int(-1)
    n = lib.lhrs_attn_plan(_ENTRY[entry], D, max_q, max_kv, LTq, int(rope), out_wide, kernels, 8, ctypes.byref(flags))
    assert 1 <= n <= 5, (entry, D, max_q, max_kv, LTq, rope, out_wide, n)
    return [lib.lhrs_attn_kernel_name(kernels[i]).decode() for i in range(n)], flags.value


def plan_of_path(entry, p):
    """The launches, in launch order, and the flags that a Path of path_of stands for."""
    flags = p.wide | 2 * (p.rope == "fused") | 4 * (p.delta == "dq_res")
    if entry in ("fwd", "fwd_kmask"):
        return ["fwd_" + p.fwd], p.wide
    kernels = ["delta"] if p.delta == "delta_kernel" else []
    kernels += [f"{k}_res" for k in ("dq", "dkv") if getattr(p, k) == "res"]        # the resident launches go out first, dQ in front
    kernels += [f"{k}_tiled" for k in ("dq", "dkv") if getattr(p, k) == "tiled"]
    return kernels + (["rope_dq", "rope_dk"] if p.rope == "separate" else []), flags


_LENS = (1, 16, 17, 32, 33, 64, 65, 256, 257, 272, 273, 288, 289, 304, 320, 321, 330, 639, 640, 641, 700, 2048)
_CALLS = (("fwd", False), ("fwd_kmask", False), ("bwd", False), ("bwd_rope", True), ("bwd_o", False), ("bwd_o", True))


def test_library_plan_equals_path_of():
    """Kernels in launch order and the three flags of lhrs_attn_plan == path_of over every entry, both head dims, max_q x max_kv around every
    threshold, three LTq (a large LTq alone flips dkv_fits) and both store widths."""
    lib = _lib.load()
    for D in (64, 128):
        for max_q in _LENS:
            pad = (max_q + 63) // 64 * 64
            for max_kv in _LENS:
                for LTq in (pad, pad + 64, 1024):
                    for entry, rope in _CALLS:
                        for out_wide in (0, 1):
                            p = path_of(D, max_q, max_kv, LTq, rope=rope, bwd_o=entry == "bwd_o", key_mask=entry == "fwd_kmask",
                                        strides=[8 if out_wide else 4])
                            got = lib_plan(lib, entry, D, max_q, max_kv, LTq, rope=rope, out_wide=out_wide)
                            assert got == plan_of_path(entry, p), (entry, D, max_q, max_kv, LTq, rope, out_wide, got, p)


def test_library_plan_hand_worked_cells():
    """Cells worked by hand from the rules, the expected launches spelled out.  Flags: 1 wide, 2 rope fused, 4 delta written by the resident dQ kernel."""
    lib = _lib.load()
    P = lambda *a, **k: lib_plan(lib, *a, **k)
    # the training cell, S = 273 at D = 128: 288 * 256 + 8 * 320 = 76288 <= 81920 - everything resident, rotation and delta inside the kernels
    assert P("fwd", 128, 273, 273, 320) == (["fwd_res"], 1)
    assert P("bwd_o", 128, 273, 273, 320, rope=True) == (["dq_res", "dkv_res"], 7)
    assert P("bwd_o", 128, 273, 273, 320, rope=True, out_wide=0) == (["dq_res", "dkv_res"], 6)
    # ViT, 257 tokens at D = 64
    assert P("fwd", 64, 257, 257, 320) == (["fwd_res"], 1)
    assert P("bwd_o", 64, 257, 257, 320) == (["dq_res", "dkv_res"], 5)
    assert P("bwd", 64, 257, 257, 320) == (["dq_res", "dkv_res"], 1)
    # the pooler's largest group: 64 queries over 320 keys at D = 64
    assert P("fwd", 64, 64, 320, 64) == (["fwd_res"], 1)
    assert P("bwd", 64, 64, 320, 64) == (["dq_res", "dkv_res"], 1)
    # D = 128, 289..320 queries: the Q image alone fills its half of the LDS - resident dQ (which writes delta), tiled dK/dV, separate rotation
    for max_q in (289, 304, 320):
        assert P("bwd_o", 128, max_q, 320, 320) == (["dq_res", "dkv_tiled"], 5)
        assert P("bwd_o", 128, max_q, 320, 320, rope=True) == (["dq_res", "dkv_tiled", "rope_dq", "rope_dk"], 5)
        assert P("bwd_rope", 128, max_q, 320, 320, rope=True) == (["dq_res", "dkv_tiled", "rope_dq", "rope_dk"], 1)
    # 321 keys at D = 128: nothing resident, the delta kernel first
    assert P("fwd", 128, 321, 321, 384) == (["fwd_tiled"], 1)
    assert P("bwd_o", 128, 321, 321, 384) == (["delta", "dq_tiled", "dkv_tiled"], 1)
    assert P("bwd_o", 128, 321, 321, 384, rope=True) == (["delta", "dq_tiled", "dkv_tiled", "rope_dq", "rope_dk"], 1)
    assert P("bwd", 128, 321, 321, 384) == (["dq_tiled", "dkv_tiled"], 1)
    # ... with at most 288 queries the resident dK/dV kernel is launched in front of the tiled dQ kernel
    assert P("bwd_o", 128, 288, 321, 320) == (["delta", "dkv_res", "dq_tiled"], 1)
    # the key mask lives in the tiled forward, whatever max_kv; no keys at all: never the resident forward
    assert P("fwd_kmask", 128, 100, 200, 128) == (["fwd_tiled"], 1) and P("fwd", 128, 100, 200, 128) == (["fwd_res"], 1)
    assert P("fwd", 128, 100, 0, 128) == (["fwd_tiled"], 1) and P("fwd", 64, 100, 0, 128, out_wide=0) == (["fwd_tiled"], 0)
    assert P("bwd", 128, 100, 0, 128) == (["dq_res", "dkv_res"], 1)
    # rejected: head_dim, entry, lhrs_attn_bwd_rope without tables, room for fewer launches than the plan has
    kernels, flags = (ctypes.c_int * 8)(), ctypes.c_int(0)
    for args in ((0, 96, 64, 64, 64, 0, 1, kernels, 8), (5, 128, 64, 64, 64, 0, 1, kernels, 8), (3, 128, 64, 64, 64, 0, 1, kernels, 8),
                 (4, 128, 321, 321, 384, 1, 1, kernels, 4)):
        assert lib.lhrs_attn_plan(*args, ctypes.byref(flags)) == -1, args[:7]


def test_reachable_cells():
    cells = reachable_cells()
    # per D: 4 kernel pairings x 2 entry points x (no rope, rope) x 2 store widths, less the separate RoPE pass on narrow rows (3 x 2)
    assert len(cells) == 2 * (4 * 2 * 2 * 2 - 3 * 2)
    assert all(p.fwd == p.dq for _, p in cells)
