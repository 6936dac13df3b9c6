"""Every dispatch path of csrc/attention.hip against the float64 reference of tests/attention_cases.py, cell by cell.

Each case is a shape that lands in one (forward, dQ, dK/dV) kernel pairing (asserted with path_of); inside it the same inputs run through
attn_bwd (delta from attn_delta) and attn_bwd_o (NaN-filled delta), without and with the inverse RoPE, into 16-byte aligned rows and into
narrow rows (the 8-byte-store path, which must be bit-identical).  The inputs are laid out the way the product passes them (column slices
of one packed qkv buffer, the compact tail of text.py:532, the pooler's [T, 2*H*D] kv buffer) and poisoned: NaN in every element the
kernels must not read, large finite keys in [kv_len, kv_rows), NaN operands left in the LDS by a launch in front of every call, and a
NaN sentinel in every output element the kernels must not write."""
import math

import pytest
import torch

from lhrs_bot_amd import kernels as hk

from attention_cases import (RES_ROWS, Seq, check, path_of, reachable_cells, ref_attention64, rope_tables,  # noqa: E402
                             self_entries)

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -1                   # bf16 bits 0xFFFF: a NaN that no kernel computes and that no store of a number leaves behind
BIG = 1.0e4                 # keys in [kv_len, kv_rows): large, finite, never to be seen by a query
MARGIN = 8                  # sentinel columns in front of and behind the result columns


def bits(t):
    return t.view(torch.int16)


def poison_lds(D):
    """A resident forward over NaN keys and values on every CU: the whole 160 KiB of LDS holds NaN when the next kernel starts there, so a
    kernel that multiplies LDS rows it did not load (even by a probability of 0) shows it."""
    R, H, nseq = RES_ROWS[D], 16, 64
    kv = torch.full((R, 2 * H * D), float("nan"), device=DEV, dtype=torch.bfloat16)
    q = torch.zeros((64, H * D), device=DEV, dtype=torch.bfloat16)
    o = torch.empty((64, H * D), device=DEV, dtype=torch.bfloat16)
    desc = hk.make_desc([(0, 64, 0, R, R, 0)] * nseq, DEV)
    hk.attn_fwd(q, kv[:, :H * D], kv[:, H * D:], o, None, desc, nseq, H, D, 64, R, 64, False, 1.0)


class Case:
    def __init__(self, name, D, H, seqs, causal, pair, runs, narrow=None, pooler=None, LTq=None, gap=3, rope_tail=False):
        self.name, self.D, self.H, self.seqs, self.causal, self.pair, self.runs = name, D, H, seqs, causal, pair, runs
        self.narrow, self.pooler, self.LTq_, self.gap, self.rope_tail = narrow, pooler, LTq, gap, rope_tail

    def __repr__(self):
        return self.name


# runs: (entry, rope) pairs; every case runs them into wide rows, a case with `narrow` ("offset": results at an 8-byte offset, "stride": row
# stride = 4 mod 8) once more into narrow rows (the separate RoPE pass is not run on narrow rows: reachable_cells)
ALL_RUNS = (("bwd", False), ("bwd_o", False), ("bwd", True), ("bwd_o", True))
TAIL_RUNS = (("bwd_o", True), ("bwd", False))   # the product's call (text.py:1149) and the plain one

CASES = [
    # backward kernel pairing, D = 128: resident up to max_kv 320; dK/dV resident up to max_q 288
    Case("d128_res_res_q288", 128, 2, [Seq(288, 270, 0, 288), Seq(100, 100, 0, 100)], True, ("res", "res"), ALL_RUNS, narrow="offset"),
    Case("d128_res_tiled_q289_kv320", 128, 2, [Seq(289, 289, 0, 289), Seq(320, 300, 0, 33)], True, ("res", "tiled"), ALL_RUNS, narrow="stride"),
    Case("d128_tiled_res_q288_kv321", 128, 2, [Seq(321, 321, 33, 288), Seq(100, 90, 0, 100)], False, ("tiled", "res"), ALL_RUNS, narrow="offset"),
    Case("d128_tiled_tiled", 128, 2, [Seq(400, 390, 0, 400), Seq(64, 64, 0, 64)], True, ("tiled", "tiled"), ALL_RUNS, narrow="stride"),
    # D = 64: resident up to max_kv 640; dK/dV resident up to max_q 576
    Case("d64_res_res_q576", 64, 2, [Seq(576, 560, 0, 576), Seq(64, 64, 0, 64)], True, ("res", "res"), ALL_RUNS, narrow="stride"),
    Case("d64_res_tiled_q577_kv640", 64, 2, [Seq(577, 577, 0, 577), Seq(640, 600, 0, 33)], True, ("res", "tiled"), ALL_RUNS, narrow="offset"),
    Case("d64_tiled_res_q576_kv641", 64, 2, [Seq(641, 641, 65, 576), Seq(50, 50, 0, 50)], True, ("tiled", "res"), ALL_RUNS, narrow="stride"),
    Case("d64_tiled_tiled", 64, 2, [Seq(700, 680, 0, 700)], False, ("tiled", "tiled"), ALL_RUNS, narrow="offset"),
    # the compact tail (text.py:532): causal_off = p0 > 0, q_len = n < kv_rows = S, LTq = pad64(S); n mod 64 in {1, 17, 32, 33, 63, 0}
    Case("tail_d128_h32_s273", 128, 32, [Seq(273, 260, 250, 1), Seq(273, 273, 200, 17), Seq(273, 240, 150, 32), Seq(273, 273, 100, 33),
                                         Seq(273, 200, 30, 63), Seq(273, 273, 209, 64)], True, ("res", "res"), TAIL_RUNS, gap=0, rope_tail=True),
    Case("tail_d64_s600", 64, 2, [Seq(600, 590, 500, 1), Seq(600, 600, 440, 17), Seq(600, 560, 40, 32), Seq(600, 600, 7, 33),
                                  Seq(600, 400, 300, 63), Seq(600, 600, 472, 128)], True, ("res", "res"), TAIL_RUNS, gap=0, rope_tail=True),
    Case("tail_d128_s700_tiled", 128, 2, [Seq(700, 690, 600, 17), Seq(700, 700, 300, 321), Seq(700, 400, 5, 64)], True, ("tiled", "tiled"),
         TAIL_RUNS, gap=0, rope_tail=True),
    Case("tail_d64_s900_tiled", 64, 2, [Seq(900, 880, 800, 33), Seq(900, 900, 100, 577), Seq(900, 50, 3, 1)], True, ("tiled", "tiled"),
         TAIL_RUNS, gap=0, rope_tail=True),
    # the pooler: q [T, H*D], k / v column slices of one [T, 2*H*D] buffer, lq != lk, not causal
    Case("pooler_d64", 64, 4, None, False, ("res", "res"), (("bwd", False), ("bwd_o", False)), pooler=[(64, 320), (48, 304), (32, 288)]),
]


def _layout(case):
    """Poisoned inputs of a case on the device -> entries, Tq, Tk, q, k, v, do, query-row mask [Tq], key-row mask [Tk]"""
    g = torch.Generator().manual_seed(len(case.name) * 7 + case.D)
    H, D = case.H, case.D
    HD = H * D
    nan = float("nan")
    if case.pooler is None:
        entries, T = self_entries(case.seqs, case.gap, case.causal)
        Tq = Tk = T
        qkv = torch.full((T, 3 * HD), nan, dtype=torch.bfloat16)
        q, k, v = qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:]
    else:
        entries, qo, ko = [], 0, 0
        for lq, lk in case.pooler:
            entries.append((qo, lq, ko, lk, lk, 0))
            qo, ko = qo + lq + case.gap, ko + lk + case.gap
        Tq, Tk = qo, ko
        qb = torch.full((Tq, HD), nan, dtype=torch.bfloat16)
        kv = torch.full((Tk, 2 * HD), nan, dtype=torch.bfloat16)
        q, k, v = qb, kv[:, :HD], kv[:, HD:]
    do = torch.full((Tq, HD), nan, dtype=torch.bfloat16)
    qrows = torch.zeros(Tq, dtype=torch.bool)
    kvrows = torch.zeros(Tk, dtype=torch.bool)
    for (q_off, q_len, kv_off, kv_len, kv_rows, _) in entries:
        q[q_off:q_off + q_len] = torch.randn(q_len, HD, generator=g).to(torch.bfloat16)
        do[q_off:q_off + q_len] = torch.randn(q_len, HD, generator=g).to(torch.bfloat16)
        k[kv_off:kv_off + kv_len] = torch.randn(kv_len, HD, generator=g).to(torch.bfloat16)
        v[kv_off:kv_off + kv_len] = torch.randn(kv_len, HD, generator=g).to(torch.bfloat16)
        npad = kv_rows - kv_len
        sign = torch.randint(0, 2, (2, npad, HD), generator=g).float() * 2 - 1
        k[kv_off + kv_len:kv_off + kv_rows] = (sign[0] * BIG).to(torch.bfloat16)
        v[kv_off + kv_len:kv_off + kv_rows] = (sign[1] * BIG).to(torch.bfloat16)
        qrows[q_off:q_off + q_len] = True
        kvrows[kv_off:kv_off + kv_rows] = True
    if case.pooler is None:
        qkv = qkv.to(DEV)
        q, k, v = qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:]
    else:
        qb, kv = qb.to(DEV), kv.to(DEV)
        q, k, v = qb, kv[:, :HD], kv[:, HD:]
    return entries, Tq, Tk, q, k, v, do.to(DEV), qrows.to(DEV), kvrows.to(DEV)


def _out(rows, ncols, narrow):
    """Sentinel-filled buffer holding `ncols` result blocks of H*D columns with MARGIN sentinel columns around them -> (buffer, c0, ld)."""
    width = ncols + 2 * MARGIN + (-4 if narrow == "stride" else 0)
    c0 = MARGIN - 4 if narrow == "offset" else MARGIN
    buf = torch.full((rows, width), SENT, device=DEV, dtype=torch.int16).view(torch.bfloat16)
    return buf, c0


def _untouched(buf, c0, ncols, rows_in, what, nan_ok_cols=()):
    """Every element outside [c0, c0 + ncols) x rows_in keeps the sentinel; columns in nan_ok_cols (ranges) only have to stay NaN outside
    rows_in (the separate RoPE pass rotates every row [0, rows), by contract)."""
    b = bits(buf)
    assert bool((b[:, :c0] == SENT).all()) and bool((b[:, c0 + ncols:] == SENT).all()), f"{what}: a margin column was written"
    out_rows = b[~rows_in, c0:c0 + ncols]
    strict = torch.ones(ncols, dtype=torch.bool, device=DEV)
    for a, z in nan_ok_cols:
        strict[a:z] = False
        assert bool(torch.isnan(buf[~rows_in, c0 + a:c0 + z]).all()), f"{what}: a row outside the sequences lost its NaN"
    assert bool((out_rows[:, strict] == SENT).all()), f"{what}: a row outside the sequences was written"


def _fwd(case, ctx, narrow):
    D, H, HD = case.D, case.H, case.H * case.D
    entries, Tq, q, k, v, desc, max_q, max_kv, LTq = (ctx[n] for n in ("entries", "Tq", "q", "k", "v", "desc", "max_q", "max_kv", "LTq"))
    obuf, c0 = _out(Tq, HD, narrow)
    o = obuf[:, c0:c0 + HD]
    lse = torch.full((len(entries), H, LTq), float("nan"), device=DEV)
    poison_lds(D)
    hk.attn_fwd(q, k, v, o, lse, desc, len(entries), H, D, max_q, max_kv, LTq, case.causal, ctx["scale"])
    torch.cuda.synchronize()
    return obuf, c0, o, lse


def _check_fwd(case, ctx, obuf, c0, o, lse, what):
    H, D, HD, ref = case.H, case.D, case.H * case.D, ctx["ref"]
    got_o, got_l = [], []
    for si, e in enumerate(ctx["entries"]):
        q_off, q_len = e[0], e[1]
        got_o.append(o[q_off:q_off + q_len].reshape(q_len, H, D))
        got_l.append(lse[si, :, :q_len].t())
        assert bool(torch.isnan(lse[si, :, q_len:]).all()), f"{what}: lse written past q_len"
    check("o", got_o, [r["o"] for r in ref], what=what)
    check("lse", got_l, [r["lse"] for r in ref], what=what)
    _untouched(obuf, c0, HD, ctx["qrows"], what + " o")


def _bwd(case, ctx, entry, rope, narrow, o, lse):
    D, H, HD = case.D, case.H, case.H * case.D
    entries, Tq, Tk, q, k, v, do, desc, max_q, max_kv, LTq = (ctx[n] for n in ("entries", "Tq", "Tk", "q", "k", "v", "do", "desc", "max_q",
                                                                                   "max_kv", "LTq"))
    nseq = len(entries)
    if case.pooler is None:
        gbuf, c0 = _out(Tq, 3 * HD, narrow)
        dq, dk, dv = gbuf[:, c0:c0 + HD], gbuf[:, c0 + HD:c0 + 2 * HD], gbuf[:, c0 + 2 * HD:c0 + 3 * HD]
        bufs = [(gbuf, c0, 3 * HD)]
    else:
        qbuf, c0 = _out(Tq, HD, narrow)
        kbuf, c1 = _out(Tk, 2 * HD, narrow)
        dq, dk, dv = qbuf[:, c0:c0 + HD], kbuf[:, c1:c1 + HD], kbuf[:, c1 + HD:c1 + 2 * HD]
        bufs = [(qbuf, c0, HD), (kbuf, c1, 2 * HD)]
    o_in = o if narrow is None else o.contiguous()   # an input here: the kernels read it with 16-byte loads
    delta = torch.full((nseq, H, LTq), float("nan"), device=DEV)
    rp = ctx["rope"] if rope else None
    poison_lds(D)
    if entry == "bwd":
        hk.attn_delta(o_in, do, delta, desc, nseq, H, D, max_q, LTq)
        hk.attn_bwd(q, k, v, do, lse, delta, dq, dk, dv, desc, nseq, H, D, max_q, max_kv, LTq, case.causal, ctx["scale"], rope=rp)
    else:
        hk.attn_bwd_o(q, k, v, do, o_in, lse, delta, dq, dk, dv, desc, nseq, H, D, max_q, max_kv, LTq, case.causal, ctx["scale"], rope=rp)
    torch.cuda.synchronize()
    return bufs, dq, dk, dv, delta


def _check_bwd(case, ctx, entry, rope, narrow, o, bufs, dq, dk, dv, delta, what):
    H, D, HD = case.H, case.D, case.H * case.D
    ref = ctx["ref_rope"] if rope else ctx["ref"]
    gq, gk, gv, gd, wd = [], [], [], [], []
    for si, (q_off, q_len, kv_off, kv_len, kv_rows, _) in enumerate(ctx["entries"]):
        gq.append(dq[q_off:q_off + q_len].reshape(q_len, H, D))
        gk.append(dk[kv_off:kv_off + kv_rows].reshape(kv_rows, H, D))
        gv.append(dv[kv_off:kv_off + kv_rows].reshape(kv_rows, H, D))
        gd.append(delta[si, :, :q_len].t())
        wd.append((ctx["do"][q_off:q_off + q_len].double() * o[q_off:q_off + q_len].double()).reshape(q_len, H, D).sum(-1))
        assert bool(torch.isnan(delta[si, :, q_len:]).all()), f"{what}: delta written past q_len"
        # padded keys: exactly zero (large finite K / V there must meet an exact 0 probability)
        assert bool((dk[kv_off + kv_len:kv_off + kv_rows] == 0).all()) and bool((dv[kv_off + kv_len:kv_off + kv_rows] == 0).all()), \
            f"{what}: seq {si}: padded keys got a gradient"
    for name, got in (("dq", gq), ("dk", gk), ("dv", gv)):
        assert all(bool(torch.isfinite(t).all()) for t in got), f"{what}: {name} not finite"
        check(name, got, [r[name] for r in ref], what=what)
    if entry == "bwd_o":   # the delta this call returns: rowsum(dO * O) of the O rows it was given, in fp64 (against the exact O the delta of
        check("delta", gd, wd, what=what)   # a one-row sequence that happens to be near 0 carries O's bf16 rounding at rel 0.8: measured)
    sep = rope and ctx["path_rope"] == "separate"
    if case.pooler is None:
        gbuf, c0, n = bufs[0]
        rows_in = ctx["qrows"] | ctx["kvrows"]
        _untouched(gbuf, c0, n, rows_in, what + " dq|dk|dv", nan_ok_cols=[(0, 2 * HD)] if sep else ())
        # dq rows that are keys but not queries (the tail): untouched unless the separate RoPE pass rotated them
        extra = ctx["kvrows"] & ~ctx["qrows"]
        if bool(extra.any()):
            if sep:
                assert bool(torch.isnan(dq[extra]).all()), f"{what}: dq written outside the query rows"
            else:
                assert bool((bits(dq[extra]) == SENT).all()), f"{what}: dq written outside the query rows"
    else:
        _untouched(bufs[0][0], bufs[0][1], bufs[0][2], ctx["qrows"], what + " dq")
        _untouched(bufs[1][0], bufs[1][1], bufs[1][2], ctx["kvrows"], what + " dk|dv")


def _context(case):
    entries, Tq, Tk, q, k, v, do, qrows, kvrows = _layout(case)
    D, H = case.D, case.H
    max_q = max(e[1] for e in entries)
    max_kv = max(e[4] for e in entries)
    LTq = case.LTq_ or (hk.pad64(max(e[4] for e in entries)) if case.rope_tail else hk.pad64(max_q))
    scale = 1.0 / math.sqrt(D)
    ctx = dict(entries=entries, Tq=Tq, Tk=Tk, q=q, k=k, v=v, do=do, qrows=qrows, kvrows=kvrows, max_q=max_q, max_kv=max_kv, LTq=LTq,
               scale=scale, desc=hk.make_desc(entries, DEV))
    if case.rope_tail:   # the product's call: positions row % S (text.py:1149)
        S = case.seqs[0].kv_rows
        cos_t, sin_t = rope_tables(S, D, DEV)
        ctx["rope"] = (cos_t, sin_t, S, 0)
    else:                # any positions: row % pos_mod + pos0
        cos_t, sin_t = rope_tables(Tq + 5, D, DEV)
        ctx["rope"] = (cos_t, sin_t, Tq, 5)
    ctx["ref"] = ref_attention64(q, k, v, do, entries, H, D, scale, case.causal)
    if any(r for _, r in case.runs):
        ctx["ref_rope"] = ref_attention64(q, k, v, do, entries, H, D, scale, case.causal, rope=ctx["rope"])
    ctx["path_rope"] = path_of(D, max_q, max_kv, LTq, rope=True).rope
    return ctx


def case_cells(case):
    """The (D, Path) cells a case reaches, from its shape alone (what the coverage test counts)."""
    if case.pooler is None:
        entries, _ = self_entries(case.seqs, case.gap, case.causal)
    else:
        entries = [(0, lq, 0, lk, lk, 0) for lq, lk in case.pooler]
    max_q, max_kv = max(e[1] for e in entries), max(e[4] for e in entries)
    LTq = case.LTq_ or (hk.pad64(max_kv) if case.rope_tail else hk.pad64(max_q))
    cells = []
    for narrow in (None, case.narrow) if case.narrow else (None,):
        for entry, rope in case.runs:
            p = path_of(case.D, max_q, max_kv, LTq, rope=rope, bwd_o=entry == "bwd_o")
            if narrow is not None and p.rope == "separate":
                continue
            cells.append((case.D, p._replace(wide=int(narrow is None)), entry, rope, narrow))
    return cells, max(e[5] for e in entries)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_attention_path(case):
    ctx = _context(case)
    D = case.D
    fwd_bits, bwd_bits = {}, {}
    for narrow in (None, case.narrow) if case.narrow else (None,):
        obuf, c0, o, lse = _fwd(case, ctx, narrow)
        p = path_of(D, ctx["max_q"], ctx["max_kv"], ctx["LTq"], strides=[o.stride(0)], ptrs=[o.data_ptr()])
        assert (p.fwd, p.wide) == (case.pair[0], int(narrow is None)), (case.name, narrow, p)
        what = f"{case.name} fwd narrow={narrow}"
        _check_fwd(case, ctx, obuf, c0, o, lse, what)
        fwd_bits[narrow] = (bits(o).clone(), lse.clone())
        for entry, rope in case.runs:
            p = path_of(D, ctx["max_q"], ctx["max_kv"], ctx["LTq"], rope=rope, bwd_o=entry == "bwd_o")
            if narrow is not None and p.rope == "separate":
                continue
            what = f"{case.name} {entry} rope={rope} narrow={narrow}"
            bufs, dq, dk, dv, delta = _bwd(case, ctx, entry, rope, narrow, o, lse)
            p = path_of(D, ctx["max_q"], ctx["max_kv"], ctx["LTq"], rope=rope, bwd_o=entry == "bwd_o",
                        strides=[t.stride(0) for t in (dq, dk, dv)], ptrs=[t.data_ptr() for t in (dq, dk, dv)])
            assert (p.dq, p.dkv, p.wide) == (case.pair[0], case.pair[1], int(narrow is None)), (what, p)
            _check_bwd(case, ctx, entry, rope, narrow, o, bufs, dq, dk, dv, delta, what)
            bwd_bits[(entry, rope, narrow)] = [bits(t).clone() for t in (dq, dk, dv)] + [delta.clone()]
    if case.narrow:   # the 8-byte-store path: the same numbers, bit for bit
        assert torch.equal(fwd_bits[None][0], fwd_bits[case.narrow][0]), f"{case.name}: o narrow != wide"
        assert torch.equal(fwd_bits[None][1].nan_to_num(), fwd_bits[case.narrow][1].nan_to_num()), f"{case.name}: lse narrow != wide"
        for (entry, rope, narrow), got in bwd_bits.items():
            if narrow is None:
                continue
            want = bwd_bits[(entry, rope, None)]
            for name, a, b in zip(("dq", "dk", "dv"), got, want):
                assert torch.equal(a, b), f"{case.name} {entry} rope={rope}: {name} narrow != wide"
            assert torch.equal(got[3].nan_to_num(), want[3].nan_to_num()), f"{case.name} {entry}: delta narrow != wide"


def test_attention_key_mask_d128_with_causal_off():
    """The key-mask forward (lhrs_attn_fwd_kmask: tiled kernel only) at D = 128 with causal_off > 0 and a max_kv the resident kernel would
    take, left padding and holes in the mask; a query row that sees no key returns 0 and lse = -inf."""
    D, H, S = 128, 2, 200
    seqs = [Seq(S, 190, 20, 150), Seq(S, S, 40, 100)]
    entries, T = self_entries(seqs)
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(T, 3 * H * D, generator=g).to(torch.bfloat16).to(DEV)
    q, k, v = qkv[:, :H * D], qkv[:, H * D:2 * H * D], qkv[:, 2 * H * D:]
    km = torch.ones(2, S, dtype=torch.uint8)
    km[0, :45] = 0                                  # left padding: query rows 0..24 of sequence 0 (keys <= row + 20) see nothing
    km[1, torch.randperm(S, generator=g)[:60]] = 0  # holes
    km = km.to(DEV)
    desc = hk.make_desc(entries, DEV)
    LTq = hk.pad64(S)
    max_q = max(e[1] for e in entries)
    p = path_of(D, max_q, S, LTq, key_mask=True)
    assert p.fwd == "tiled" and path_of(D, max_q, S, LTq).fwd == "res"
    obuf, c0 = _out(T, H * D, None)
    o = obuf[:, c0:c0 + H * D]
    lse = torch.full((2, H, LTq), float("nan"), device=DEV)
    hk.attn_fwd(q, k, v, o, lse, desc, 2, H, D, max_q, S, LTq, True, 1.0 / math.sqrt(D), key_mask=km)
    torch.cuda.synchronize()
    ref = ref_attention64(q, k, v, q, entries, H, D, 1.0 / math.sqrt(D), True, key_mask=km)
    got_o = [o[e[0]:e[0] + e[1]].reshape(e[1], H, D) for e in entries]
    got_l = [lse[i, :, :e[1]].t() for i, e in enumerate(entries)]
    assert bool((got_o[0][:25] == 0).all()) and bool(torch.isneginf(got_l[0][:25]).all())
    check("o", got_o, [r["o"] for r in ref], what="key mask")
    check("lse", got_l, [r["lse"] for r in ref], what="key mask")
    rows = torch.zeros(T, dtype=torch.bool, device=DEV)
    for e in entries:
        rows[e[0]:e[0] + e[1]] = True
    _untouched(obuf, c0, H * D, rows, "key mask o")


def test_attention_table_reaches_every_cell():
    """The table above reaches every reachable (forward, dQ, dK/dV, rope, delta, wide) cell at D = 64 and D = 128, and causal_off > 0 runs
    on the resident and on the tiled kernels."""
    reached, coff_kernels = set(), set()
    for case in CASES:
        cells, coff = case_cells(case)
        for D, p, _, _, _ in cells:
            reached.add((D, p))
            if case.causal and coff > 0:
                coff_kernels |= {("fwd", p.fwd), ("dq", p.dq), ("dkv", p.dkv)}
    missing = reachable_cells() - reached
    assert not missing, sorted(missing)
    assert coff_kernels >= {(k, m) for k in ("fwd", "dq", "dkv") for m in ("res", "tiled")}, coff_kernels
