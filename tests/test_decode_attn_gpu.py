"""The bf16 decode attention of csrc/decode_attn.hip on an MI355X against the float64 restatement of tests/decode_attn_cases.py:
hk.decode_attn and hk.decode_attn_split on every case of its table, the composed route hk.rope_kv_append + hk.attn_fwd at head_dim 128 and
64, the exported hk.kv_append, the step bookkeeping hk.decode_advance / hk.decode_emit against integer models, and which of them generate()
reaches.

Buffers: qkv with a row stride above 3 H D, NaN in the extra columns and a NaN row after the last; the output inside an int16 -1 sentinel
buffer whose extra rows and columns must come back untouched; `part` filled with NaN, `tickets` zero before and after; a key mask with a
row stride above max_ctx; caches that are NaN wherever the kernel must not read (every row from pos on, every masked key's row).
Per case: the output per element inside the derived bound (ratio <= 1, printed) and finite, the appended K row exact (exact tables) or
within the rotation tolerance (model tables), the appended V row and every other cache element bit-identical, NaN payloads included.
Composed route only: the tiled forward multiplies a masked key's V row by its weight of exactly 0 (csrc/attention.hip,
lhrs_attn_fwd_kmask), so those rows - and only those - hold a finite filler (2^100) instead of NaN; masked K rows and every row from pos
on are NaN there too.

Worst error / bound: the float32 emulations of decode_attn_cases give 0.8830 (one workgroup), 0.8843 (split) and 0.5159 (composed); measured
on an MI355X: 0.8830, 0.8843 and 0.5159 - the same figures to four digits, set by the bf16 store (DESIGN.md "Decode attention vs fp64")."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from lhrs_bot_amd import kernels as hk  # noqa: E402
from lhrs_bot_amd.text import TextModal  # noqa: E402

import decode_attn_cases as da  # noqa: E402

DEV = "cuda"
BF, F32, I16, I32, I64, U8 = torch.bfloat16, torch.float32, torch.int16, torch.int32, torch.int64, torch.uint8
IDS = [da.ident(c) for c in da.CASES]
CIDS = [da.ident(c) for c in da.COMPOSED]


# ------------------------------------------------------------------------------------------------------------------------- 1. the two kernels
def _buffers(c):
    """device copies of a case's inputs in guarded buffers -> dict"""
    i = da.inputs(c)
    hd = c.H * c.D
    qbuf = torch.full((da.B + 1, 3 * hd + 8), float("nan"), dtype=BF)          # NaN columns past the row and a NaN row after the last
    qbuf[:da.B, :3 * hd] = i["qkv"]
    qbuf = qbuf.to(DEV)
    obuf = torch.full((da.B + 2, hd + 8), -1, dtype=I16, device=DEV)
    km = None
    if i["kmask"] is not None:
        kmbuf = torch.full((da.B, c.max_ctx + 5), 0, dtype=U8)                  # row stride above max_ctx; a kernel that ignored it would see zeros
        kmbuf[:, :c.max_ctx] = i["kmask"]
        km = kmbuf.to(DEV)[:, :c.max_ctx]
    return dict(qbuf=qbuf, qkv=qbuf[:da.B, :3 * hd], obuf=obuf, out=obuf.view(BF)[:da.B, :hd], km=km, kc=i["kc"].to(DEV), vc=i["vc"].to(DEV),
                cos=i["cos"].to(DEV), sin=i["sin"].to(DEV), pos=torch.tensor(c.pos, dtype=I32, device=DEV))


def _after(c, d):
    """the checks every route shares, after the launch -> (out, kc, vc) on the host"""
    torch.cuda.synchronize()
    hd = c.H * c.D
    ob = d["obuf"]
    assert bool((ob[da.B:] == -1).all()) and bool((ob[:, hd:] == -1).all()), f"{c.name}: an element outside the output was written"
    out = d["out"].cpu()
    assert bool(torch.isfinite(out.float()).all()), f"{c.name}: non-finite output"
    return out, d["kc"].cpu(), d["vc"].cpu()


def _run(c, kernel, nsplit=None, use_cs=False):
    """one launch of hk.decode_attn ("one") or hk.decode_attn_split ("split") -> (out bf16 [B, H D], kc, vc) on the host"""
    i = da.inputs(c)
    d = _buffers(c)
    args = (d["qkv"], d["kc"], d["vc"], d["cos"], d["sin"], d["pos"], d["out"], da.B, c.H, c.D, c.max_ctx, da.scale_of(c))
    if kernel == "one":
        hk.decode_attn(*args, key_mask=d["km"])
    else:
        NS = c.nsplit if nsplit is None else nsplit
        part = torch.full((da.B, c.H, NS, 132), float("nan"), device=DEV, dtype=F32)
        tickets = torch.zeros((da.B, c.H), device=DEV, dtype=I32)
        cs = torch.cat((i["cos"][list(c.pos)], i["sin"][list(c.pos)]), 1).contiguous().to(DEV) if use_cs else None
        hk.decode_attn_split(*args, NS, part, tickets, key_mask=d["km"], cs=cs)
        torch.cuda.synchronize()
        assert not bool(tickets.any()), f"{c.name}: a ticket was left non-zero"
    res = _after(c, d)
    qb = torch.full((da.B + 1, 3 * c.H * c.D + 8), float("nan"), dtype=BF)
    qb[:da.B, :3 * c.H * c.D] = i["qkv"]
    assert torch.equal(da.bits(d["qbuf"].cpu()), da.bits(qb)), f"{c.name}: qkv was written"      # these kernels take it const
    return res


def _judge(c, kernel, out, kc, vc, nsplit=None):
    da.check_caches(c, kc, vc)
    ref = da.reference(c, kc, vc) if c.real else da.case_reference(c)
    name = {"one": "decode_attn", "split": "decode_attn_split", "composed": "rope_kv_append+attn_fwd"}[kernel]
    r = da.ratio(out, ref.want, da.bound(c, ref, kernel, nsplit), name)
    print(f"{c.name}: {name} at {r:.4f} x the bound")
    return r


@pytest.mark.parametrize("c", da.CASES, ids=IDS)
def test_decode_attn_case_vs_fp64(c):
    out, kc, vc = _run(c, "one")
    r = _judge(c, "one", out, kc, vc)
    assert r <= 1.0, (c.name, r)


@pytest.mark.parametrize("c", da.CASES, ids=IDS)
def test_decode_attn_split_case_vs_fp64(c):
    out, kc, vc = _run(c, "split")
    r = _judge(c, "split", out, kc, vc)
    assert r <= 1.0, (c.name, r)


@pytest.mark.parametrize("c", da.CASES, ids=IDS)
def test_decode_attn_split_cs_rows_change_nothing(c):
    """with the cos | sin rows of the new position handed in (what decode_advance leaves) the output and the caches are bit-identical"""
    a = _run(c, "split")
    b = _run(c, "split", use_cs=True)
    assert all(torch.equal(da.bits(x), da.bits(y)) for x, y in zip(a, b)), c.name


def test_every_key_masked_gives_exact_zeros_on_the_device():
    c = next(c for c in da.CASES if c.mask == "all")
    for kernel in ("one", "split"):
        out = _run(c, kernel)[0]
        assert bool((da.bits(out[1]) == 0).all()) and bool((out[0] != 0).any()), kernel


def test_decode_attn_split_counts_agree():
    """nsplit 1, 2 and 3 on the same inputs: identical caches, each output inside its bound and within twice the bound of the others"""
    c = da.CASES[7]
    ref = da.case_reference(c)
    runs = [_run(c, "split", ns) for ns in (1, 2, 3)]
    bnd = torch.stack([da.bound(c, ref, "split", ns) for ns in (1, 2, 3)]).amax(0)
    for ns, (out, kc, vc) in zip((1, 2, 3), runs):
        assert torch.equal(da.bits(kc), da.bits(runs[0][1])) and torch.equal(da.bits(vc), da.bits(runs[0][2]))
        assert _judge(c, "split", out, kc, vc, ns) <= 1.0, ns
        assert bool(((out.double() - runs[0][0].double()).abs() <= 2 * bnd).all()), ns


# ------------------------------------------------------------------------------------------------------------------------- 2. composed route
@pytest.mark.parametrize("c", da.COMPOSED, ids=CIDS)
def test_rope_kv_append_then_attn_fwd_vs_fp64(c):
    """the decode step of a model whose head_dim is not 128 (TextModal._decode_session): rope_kv_append rotates q and k in place and appends,
    the tiled forward attends at q_len 1 behind the descriptor rows decode_advance writes"""
    i = da.inputs(c)
    d = _buffers(c)
    hd = c.H * c.D
    hk.rope_kv_append(d["qkv"], d["kc"], d["vc"], d["cos"], d["sin"], d["pos"], da.B, c.H, c.D, c.max_ctx)
    desc = hk.make_desc([(b, 1, b * c.max_ctx, p + 1, p + 1, p) for b, p in enumerate(c.pos)], DEV)
    hk.attn_fwd(d["qkv"][:, :hd], d["kc"], d["vc"], d["out"], None, desc, da.B, c.H, c.D, 1, 1 << 30, 64, True, da.scale_of(c), key_mask=d["km"])
    out, kc, vc = _after(c, d)
    q, q64, k64, qtol, ktol = da.rotated(c)
    qb = d["qbuf"].cpu()
    assert bool(torch.isnan(qb[da.B].float()).all()) and bool(torch.isnan(qb[:, 3 * hd:].float()).all()), f"{c.name}: the qkv surround was written"
    got = qb[:da.B, :3 * hd].reshape(da.B, 3, c.H, c.D)
    assert torch.equal(da.bits(got[:, 2]), da.bits(i["qkv"].reshape(da.B, 3, c.H, c.D)[:, 2])), f"{c.name}: the v block changed"
    if c.real:
        assert bool(((got[:, 0].double() - q64).abs() <= qtol).all()) and bool(((got[:, 1].double() - k64).abs() <= ktol).all()), c.name
        assert torch.equal(got[:, 0].double(), q), c.name          # no q element is near a rounding boundary: one admissible value
    else:
        assert torch.equal(da.bits(got[:, 0]), da.bits(q64.to(BF))) and torch.equal(da.bits(got[:, 1]), da.bits(k64.to(BF))), c.name
    for b, p in enumerate(c.pos):                                    # the cache rows at pos ARE the rotated k block and the v block
        assert torch.equal(da.bits(kc[b * c.max_ctx + p]), da.bits(got[b, 1].reshape(-1))), (c.name, b)
    r = _judge(c, "composed", out, kc, vc)                           # every other cache row bit-unchanged: check_caches
    assert r <= 1.0, (c.name, r)


# ------------------------------------------------------------------------------------------------------------------------- 3. kv_append
def test_kv_append_copies_the_k_and_v_blocks_to_row_pos():
    Bn, d, max_ctx = 3, 8 * 300, 7                                   # d / 8 = 300 chunks: two workgroups, the second partly idle
    g = torch.Generator().manual_seed(61)
    src = torch.full((Bn + 1, 3 * d + 8), float("nan"), dtype=BF)
    src[:Bn, :3 * d] = torch.randn(Bn, 3 * d, generator=g).to(BF)
    src[1, d + 5], src[2, 2 * d + 9] = float("nan"), -0.0            # a copy keeps a NaN and a signed zero
    pos = (0, 3, 6)
    kc0, vc0 = da.nan_rows(Bn * max_ctx + 2, d), da.nan_rows(Bn * max_ctx + 2, d)
    kc, vc, qd = kc0.to(DEV), vc0.to(DEV), src.to(DEV)
    hk.kv_append(qd[:Bn, :3 * d], kc, vc, torch.tensor(pos, dtype=I32, device=DEV), Bn, d, max_ctx)
    torch.cuda.synchronize()
    for b, p in enumerate(pos):
        kc0[b * max_ctx + p], vc0[b * max_ctx + p] = src[b, d:2 * d], src[b, 2 * d:3 * d]
    assert torch.equal(da.bits(kc.cpu()), da.bits(kc0)) and torch.equal(da.bits(vc.cpu()), da.bits(vc0))
    assert torch.equal(da.bits(qd.cpu()), da.bits(src))


# ------------------------------------------------------------------------------------------------------------------------- 4. bookkeeping
@pytest.mark.parametrize("Bn", [1, 5, 64])
def test_decode_advance_and_emit_follow_the_integer_models(Bn):
    max_ctx, max_new, ctx0 = 40, 3, 11
    cos, sin = da.model_tables(max_ctx, 128)
    cosd, sind = cos.to(DEV), sin.to(DEV)
    pad = 3                                                           # guard rows / columns behind every array
    for with_cs in (False, True):
        state = torch.tensor([ctx0, 1, -7, -8], dtype=I32)
        desc = torch.full((Bn + pad, 8), -5, dtype=I32)
        pos = torch.full((Bn + pad,), -5, dtype=I32)
        cs = torch.full((Bn + pad, 128), -5.0)
        sd, dd, pd, cd = state.to(DEV), desc.to(DEV), pos.to(DEV), cs.to(DEV)
        for inc in (1, 2, 1, 2):                                      # consecutive calls: the state carries over
            old = int(state[0])
            hk.decode_advance(sd, dd, pd, Bn, max_ctx, inc, *((cosd, sind, cd) if with_cs else ()))
            da.advance_model(state, desc, pos, Bn, max_ctx, inc, cos, sin, cs if with_cs else None)
            torch.cuda.synchronize()
            assert torch.equal(sd.cpu(), state) and torch.equal(dd.cpu(), desc) and torch.equal(pd.cpu(), pos), (Bn, with_cs, inc)
            assert torch.equal(cd.cpu(), cs), (Bn, with_cs, inc)
            if with_cs:                                               # the table rows of the OLD state[0], for every b
                assert all(torch.equal(cd[b, :64].cpu(), cos[old]) and torch.equal(cd[b, 64:].cpu(), sin[old]) for b in range(Bn))
        assert int(state[0]) == ctx0 + 6 and bool((cd[Bn:] == -5).all())
        # emit: state[1] below, at and above max_new; out_ids sits inside a sentinel surround
        g = torch.Generator().manual_seed(Bn)
        out_ids = torch.full((Bn + pad, max_new), -9, dtype=I64)
        tok32 = torch.full((Bn + pad,), -9, dtype=I32)
        od, td = out_ids.to(DEV), tok32.to(DEV)
        for step in range(4):                                         # state[1] = 1, 2 (below), 3 (at), 4 (above max_new)
            nxt = torch.randint(0, 1 << 40, (Bn + pad,), generator=g)
            hk.decode_emit(nxt.to(DEV), td, od, sd, Bn, max_new)
            da.emit_model(nxt, tok32, out_ids, state, Bn, max_new)
            torch.cuda.synchronize()
            assert torch.equal(od.cpu(), out_ids) and torch.equal(td.cpu(), tok32) and torch.equal(sd.cpu(), state), (Bn, step)
        assert int(state[1]) == 5 and bool((out_ids[:Bn, 0] == -9).all()) and bool((out_ids[Bn:] == -9).all())


# ------------------------------------------------------------------------------------------------------------------------- 5. dispatch
def test_generate_reaches_each_kernel(monkeypatch):
    calls = []

    def counted(name):
        real = getattr(hk, name)

        def f(*a, **k):
            calls.append((name, a[10] if name != "rope_kv_append" else a[9], a[12] if name == "decode_attn_split" else None))
            return real(*a, **k)
        monkeypatch.setattr(hk, name, f)

    for name in ("decode_attn", "decode_attn_split", "rope_kv_append"):
        counted(name)
    kw = dict(do_sample=False, max_new_tokens=4, eos_token_id=None)
    tm = TextModal(device=DEV, layers=2, dim=2048, ff=2048, heads=16)        # head_dim 128
    tm.init_random(seed=3)
    g = torch.Generator().manual_seed(4)
    for S0 in (6, 130, 2060):                                                # max_ctx 10, 134, 2064: nsplit 1, 2 and the cap of 16
        calls.clear()
        ids = torch.randint(3, 32000, (2, S0), generator=g)
        assert tm.generate(ids, **kw).shape == (2, 4)
        want_ns = min(16, math.ceil((S0 + 4) / 128))
        names = {n for n, _, _ in calls}
        assert names == ({"decode_attn_split"} if want_ns > 1 else {"decode_attn"}), (S0, names)        # max_ctx <= 128: one slice, one workgroup
        assert len(calls) >= 2 * 2 and all(mc == S0 + 4 for _, mc, _ in calls), (S0, calls[:3])
        assert want_ns == 1 or all(ns == want_ns for _, _, ns in calls), (S0, calls[:3])
    monkeypatch.setenv("LHRS_DECODE_SPLIT", "0")
    calls.clear()
    tm.generate(torch.randint(3, 32000, (2, 130), generator=g), **kw)
    assert {n for n, _, _ in calls} == {"decode_attn"} and len(calls) >= 4
    monkeypatch.delenv("LHRS_DECODE_SPLIT")
    del tm
    tm = TextModal(device=DEV, layers=2, dim=2048, ff=2048, heads=32)        # head_dim 64
    tm.init_random(seed=3)
    calls.clear()
    assert tm.generate(torch.randint(3, 32000, (2, 130), generator=g), **kw).shape == (2, 4)
    assert {n for n, _, _ in calls} == {"rope_kv_append"} and len(calls) >= 4 and all(mc == 134 for _, mc, _ in calls)


def test_worst_ratio_seen_on_the_device():
    """last in the file: the largest error / bound the comparisons above saw, per kernel (allowed: 1)"""
    for k in sorted(da.WORST):
        print(f"WORST {k:24s} {da.WORST[k]:.4f}")
