"""tests/decode_attn_cases.py against itself and against plain torch, without a GPU: the float64 attention against a torch.softmax
formulation, a float32 emulation of each kernel's order of operations inside the derived bound on EVERY case - so the case table cannot
hide a failure: each case must pass for the reference alone - the NaN filler where the module says it is, and the integer models of the
step bookkeeping on a hand-written example."""
import pytest
import torch

import decode_attn_cases as da
import kv8_cases as kv

F64 = torch.float64
ALL = da.CASES + da.COMPOSED
IDS = [da.ident(c) for c in ALL]
EMU_WORST = {}


def _after(c, kernel):
    """(out, kc, vc, Ref) of the emulation: the reference of a model-table case comes from the K row the emulation left"""
    out, kc, vc = da.emulate(c, kernel)
    da.check_caches(c, kc, vc)
    return out, da.reference(c, kc, vc) if c.real else da.case_reference(c)


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_float64_attention_equals_a_plain_softmax(c):
    kc, vc = da.emulate(c, "composed")[1:] if c.real else da.expected_caches(c)
    ref = da.reference(c, kc, vc)
    q = da.rotated(c)[0]
    for b, p in enumerate(c.pos):
        rows = slice(b * c.max_ctx, b * c.max_ctx + p + 1)
        vis = da.visible(c, b)
        K = torch.nan_to_num(kc[rows].double().reshape(p + 1, c.H, c.D), nan=0.0)
        V = torch.where(vis[:, None, None], torch.nan_to_num(vc[rows].double().reshape(p + 1, c.H, c.D), nan=0.0), torch.zeros((), dtype=F64))
        s = da.scale_of(c) * torch.einsum("nhd,hd->hn", K, q[b])
        s = s.masked_fill(~vis[None], float("-inf"))
        w = torch.softmax(s, -1) if bool(vis.any()) else torch.zeros_like(s)             # no visible key: the kernels return 0
        want = torch.einsum("hn,nhd->hd", w, V).reshape(-1)
        assert torch.allclose(want, ref.want[b], rtol=1e-10, atol=1e-13), (c.name, b)
        assert c.mask is None or not bool(vis.all())


@pytest.mark.parametrize("c", da.CASES, ids=IDS[:len(da.CASES)])
def test_float32_emulation_of_both_decode_kernels_stays_within_the_bound(c):
    for kernel in ("one", "split"):
        out, ref = _after(c, kernel)
        r = da.ratio(out, ref.want, da.bound(c, ref, kernel))
        EMU_WORST[kernel] = max(EMU_WORST.get(kernel, 0.0), r)
        print(f"{c.name}: float32 emulation of the {kernel} kernel at {r:.4f} x the bound")
        assert r <= 1.0, (c.name, kernel, r)


@pytest.mark.parametrize("c", da.COMPOSED, ids=IDS[len(da.CASES):])
def test_float32_emulation_of_the_composed_route_stays_within_its_bound(c):
    out, ref = _after(c, "composed")
    r = da.ratio(out, ref.want, da.bound(c, ref, "composed"))
    EMU_WORST["composed"] = max(EMU_WORST.get("composed", 0.0), r)
    print(f"{c.name}: float32 emulation of rope_kv_append + the tiled forward at {r:.4f} x the bound")
    assert r <= 1.0, (c.name, r)


def test_emulated_split_counts_agree_within_twice_the_bound():
    c = da.CASES[7]                                                     # positions 1023, 1024, 4
    ref = da.case_reference(c)
    outs = [da.emulate(c, "split", ns)[0].double() for ns in (1, 2, 3)]
    bnd = torch.stack([da.bound(c, ref, "split", ns) for ns in (1, 2, 3)]).amax(0)
    for o in outs[1:]:
        assert bool(((o - outs[0]).abs() <= 2 * bnd).all())


def test_every_key_masked_gives_exact_finite_zeros():
    c = next(c for c in da.CASES if c.mask == "all")
    hd = c.H * c.D
    for kernel in ("one", "split"):
        out = da.emulate(c, kernel)[0]
        assert bool((out[1] == 0).all()) and bool(torch.isfinite(out.float()).all())
        assert bool((da.bound(c, da.case_reference(c), kernel)[1] == 0).all()) and da.case_reference(c).want[1].abs().max() == 0
        assert bool((out[0] != 0).any()) and out.shape == (da.B, hd)


def test_the_case_table_covers_what_it_claims():
    assert any(c.mask == "std" for c in da.CASES) and sum(c.real for c in da.CASES) in (1, 2) and any(c.wide for c in da.CASES)
    assert all(c.max_ctx <= 2100 and max(c.pos) < c.max_ctx for c in ALL)
    sl = next(c for c in da.CASES if c.mask == "slice")               # a workgroup whose every key is masked publishes m = -inf
    assert not bool(da.visible(sl, 0)[128:256].any()) and sl.pos[0] >= 256 and sl.nsplit >= 2
    assert not bool(da.visible(sl, 1)[:128].any()) and sl.pos[1] >= 128
    al = next(c for c in da.CASES if c.mask == "all")
    assert not bool(da.visible(al, 1).any())
    wide = next(c for c in da.CASES if c.wide)
    i = da.inputs(wide)
    mags = i["kc"].float().abs().amax(1)
    mags = mags[torch.isfinite(mags) & (mags > 0)]
    assert float(mags.max()) / float(mags.min()) >= 2.0 ** 30
    x = i["qkv"].reshape(da.B, 3, wide.H, wide.D)
    assert not bool(x[1, 1, 1].any()) and not bool(i["kc"][wide.max_ctx + 3, :wide.D].any())      # a zero new K row, a zero K row in the cache


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_nan_filler_is_where_the_module_says(c):
    """row pos[b], every masked key below it and every row after it are NaN before the call; and every decode case has NaN rows above pos
    inside the first up-front load"""
    first = da.nan_filler_holds(c)
    assert first > 0, c.name
    if c.mask is not None:                                               # a NaN row at a masked key BELOW pos
        i = da.inputs(c)
        assert any(bool((~da.visible(c, b)[:p]).any()) for b, p in enumerate(c.pos))
        if c.route == "decode":
            for b, p in enumerate(c.pos):
                hidden = ~da.visible(c, b)[:p]
                assert bool(torch.isnan(i["vc"][b * c.max_ctx:b * c.max_ctx + p][hidden].float()).all())


def test_rotation_restated_here_equals_the_one_of_kv8_cases():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(5, 128, generator=g).to(da.BF)
    cos, sin = da.model_tables(9, 128)
    assert torch.equal(da.rotate64(x, cos[7], sin[7])[0], kv.rotate64(x, cos[7], sin[7]))
    c, s = da.exact_tables(3, 9, 64)
    assert bool(((c.abs() + s.abs()) == 1).all()) and bool(((c * s) == 0).all())
    assert torch.equal(da.bf16_spacing(torch.tensor([1.0, 1.5, 2.0, 0.75, 0.0], dtype=F64)),
                       torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -133], dtype=F64))


def test_accumulate_counts():
    assert da.acc_one(0) == da.acc_one(511) == 36 and da.acc_one(512) == 53
    assert da.acc_split(127, 1) == 9 + 11 + 2 and da.acc_split(128, 1) == 18 + 11 + 2
    assert da.acc_split(2047, 16) == 9 + 11 + 32 and da.acc_split(2048, 16) == 18 + 11 + 32 and da.acc_split(300, 16) == 9 + 11 + 6
    assert da.acc_composed(63) == 67 and da.acc_composed(64) == 132


def test_integer_models_of_the_step_bookkeeping():
    state = torch.tensor([7, 0, 0, 0], dtype=torch.int32)
    desc = torch.full((2, 8), -1, dtype=torch.int32)
    pos = torch.full((2,), -1, dtype=torch.int32)
    cos, sin = da.model_tables(12, 128)
    cs = torch.zeros(2, 128)
    da.advance_model(state, desc, pos, 2, 10, 2, cos, sin, cs)
    assert desc.tolist() == [[0, 1, 0, 8, 8, 7, -1, -1], [1, 1, 10, 8, 8, 7, -1, -1]] and pos.tolist() == [7, 7] and state.tolist() == [9, 0, 0, 0]
    assert torch.equal(cs[1, :64], cos[7]) and torch.equal(cs[0, 64:], sin[7])
    out_ids, tok32 = torch.full((2, 2), -1, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    state[1] = 1
    da.emit_model(torch.tensor([5, 6]), tok32, out_ids, state, 2, 2)
    da.emit_model(torch.tensor([8, 9]), tok32, out_ids, state, 2, 2)                    # state[1] == max_new: no column left
    assert out_ids.tolist() == [[-1, 5], [-1, 6]] and tok32.tolist() == [8, 9] and state.tolist() == [9, 3, 0, 0]


def test_worst_ratio_of_the_emulations():
    """last in the file: the largest error / bound of the float32 emulations (allowed: 1)"""
    for k in sorted(EMU_WORST):
        print(f"EMULATION WORST {k:9s} {EMU_WORST[k]:.4f}")
