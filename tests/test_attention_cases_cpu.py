"""The tools of tests/attention_cases.py on the CPU: the comparator rejects subtly wrong attention results (each mutation of the float64
reference by at least 3x its bound while the reference rounded to bf16 passes), and path_of restates the host dispatch of
csrc/attention.hip on hand-worked shapes."""
import pytest
import torch

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


def test_reachable_cells():
    cells = reachable_cells()
    # per D: 4 kernel pairings x 2 entry points x (no rope, rope) x 2 store widths, less the separate RoPE pass on narrow rows (3 x 2)
    assert len(cells) == 2 * (4 * 2 * 2 * 2 - 3 * 2)
    assert all(p.fwd == p.dq for _, p in cells)
