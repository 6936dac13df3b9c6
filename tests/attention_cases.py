"""Attention cases shared by tests/test_attention_paths_gpu.py and tests/test_attention_cases_cpu.py: a float64 reference of the
sequence-descriptor semantics of csrc/attention.hip, a restatement of its host dispatch rules, and a comparator that measures every
(sequence, head) cell on its own."""
from collections import namedtuple

import torch

# attn_res_rows(D) = 163840 / (2 * D * 2) (csrc/attn_plan.h): the rows of ONE operand matrix that the resident kernels keep in the LDS
RES_ROWS = {64: 640, 128: 320}

# Bounds per output: (rel-L2 of one (sequence, head) cell, max |got - want| of the cell / max |want| of the cell).  Worst values measured on
# an MI355X over every case of test_attention_paths_gpu.py (bf16 inputs, fp64 reference of the same inputs; delta against rowsum(dO * O) of
# the O rows the call was given), bound ~2.5x that:
#   o      rel 2.5e-3  max 4.7e-3        lse    rel 1.1e-7  max 1.5e-7       delta  rel 1.6e-6  max 1.6e-6
#   dq     rel 4.0e-3  max 7.3e-3        dk     rel 4.2e-3  max 8.6e-3       dv     rel 3.0e-3  max 6.2e-3
BOUNDS = {
    "o": (6.5e-3, 1.2e-2),
    "lse": (3e-7, 4e-7),
    "delta": (4e-6, 4e-6),
    "dq": (1e-2, 1.8e-2),
    "dk": (1e-2, 2.2e-2),
    "dv": (7.5e-3, 1.6e-2),
}

# worst (rel, max) per output name seen by check() in this process (how the values above were measured)
WORST = {}

Seq = namedtuple("Seq", "kv_rows kv_len p0 n")   # one sequence of a self-attention token layout: queries are rows [p0, p0 + n) of its kv_rows
Path = namedtuple("Path", "fwd dq dkv rope delta wide")


def ceil32(n):
    return (n + 31) // 32 * 32


def path_of(D, max_q, max_kv, LTq, rope=False, bwd_o=False, key_mask=False, strides=(), ptrs=()):
    """The host dispatch of csrc/attn_plan.h (attn_plan, which attention.hip runs and lhrs_attn_plan exports) restated: which forward, dQ and dK/dV kernel runs ('res' | 'tiled'),
    where the inverse RoPE happens ('none' | 'fused' into the resident stores | 'separate' lhrs_rope pass), where delta comes from ('input':
    lhrs_attn_bwd reads it | 'dq_res': lhrs_attn_bwd_o, written by the resident dQ kernel | 'delta_kernel': lhrs_attn_bwd_o, a launch of
    attn_delta_kernel first) and whether result rows leave as 16-byte stores.  strides / ptrs: of the outputs the call writes."""
    R = RES_ROWS[D]
    fwd = "res" if not key_mask and 0 < max_kv <= R else "tiled"                        # attn_plan: the forward rule (key mask: tiled only)
    dq = "res" if max_kv <= R else "tiled"                                               # attn_plan: dq_res
    dkv_fits = max_q <= R and ceil32(max_q) * D * 2 + 2 * LTq * 4 <= R * D * 2           # attn_plan: dkv_res (the dkv_fits expression)
    dkv = "res" if dkv_fits else "tiled"                                                 # attn_plan: dkv_res
    rope_mode = "none" if not rope else ("fused" if dq == "res" and dkv == "res" else "separate")   # attn_plan: rope_fused, else the two lhrs_rope passes
    delta = "input" if not bwd_o else ("dq_res" if max_kv <= R else "delta_kernel")      # attn_plan: delta_by_dq, else the delta kernel first
    wide = int(all(s % 8 == 0 for s in strides) and all(p % 16 == 0 for p in ptrs))      # the entry points' out_wide (attention.hip)
    return Path(fwd, dq, dkv, rope_mode, delta, wide)


def reachable_cells():
    """Every (D, path) a call without a key mask can reach.  The forward follows the dQ kernel (the same max_kv rule).  The separate RoPE pass
    (lhrs_rope: 16-byte row accesses, ld % 8 == 0) is not run on narrow rows: with a row stride not a multiple of 8 lhrs_rope refuses it."""
    cells = set()
    for D in (64, 128):
        for dq in ("res", "tiled"):
            for dkv in ("res", "tiled"):
                for rope in (False, True):
                    rope_mode = "none" if not rope else ("fused" if dq == dkv == "res" else "separate")
                    for bwd_o in (False, True):
                        delta = "input" if not bwd_o else ("dq_res" if dq == "res" else "delta_kernel")
                        for wide in (0, 1):
                            if rope_mode == "separate" and not wide:
                                continue
                            cells.add((D, Path(dq, dq, dkv, rope_mode, delta, wide)))
    return cells


def self_entries(seqs, gap=0, causal=True):
    """Descriptor rows of the self-attention layout of text.py (compact tail: text.py:532): sequence b owns token rows [base_b, base_b +
    kv_rows), `gap` poisoned rows between and after sequences, its queries are rows [p0, p0 + n), causal_off = p0.  -> (entries, tokens)"""
    entries, base = [], 0
    for s in seqs:
        assert 0 <= s.p0 and s.p0 + s.n <= s.kv_rows and 0 < s.kv_len <= s.kv_rows
        entries.append((base + s.p0, s.n, base, s.kv_len, s.kv_rows, s.p0 if causal else 0))
        base += s.kv_rows + gap
    return entries, base


def rope_tables(npos, D, device):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    f = torch.outer(torch.arange(npos, dtype=torch.float64), inv)
    return f.cos().float().to(device), f.sin().float().to(device)


def rotate64(x, rows, cos_t, sin_t, pos_mod, pos0, inverse=False):
    """x [n, H, D] float64 at token rows `rows` [n]: the rotation of rope_ / lhrs_rope (pairs (i, i + D/2), position m % pos_mod + pos0)."""
    pos = (rows % pos_mod + pos0).to(cos_t.device)
    c = cos_t[pos].double()[:, None, :].to(x.device)
    s = sin_t[pos].double()[:, None, :].to(x.device)
    if inverse:
        s = -s
    h = x.shape[-1] // 2
    a, b = x[..., :h], x[..., h:]
    return torch.cat([a * c - b * s, b * c + a * s], dim=-1)


def ref_attention64(q, k, v, do, entries, H, D, scale, causal, rope=None, key_mask=None):
    """Forward and backward in float64 from the bf16 inputs the kernels read.  q, do: [tokens, >= H*D], k, v: [tokens, >= H*D] (column
    slices are fine: the first H*D columns are used).  entries: descriptor rows (q_off, q_len, kv_off, kv_len, kv_rows, causal_off).
    Query i of a sequence sees key j iff j < kv_len, and j <= i + causal_off when causal, and key_mask[seq, j] != 0 when a mask is given.
    rope = (cos_t, sin_t, pos_mod, pos0): the inputs are the ROTATED rows (what the forward multiplies); the scores are those of the rotated
    q / k and dq / dk are returned for the un-rotated projections, i.e. through the transpose of the rotation at each token row's position.
    -> one dict per sequence: o [q_len, H, D], lse [q_len, H] (natural log of sum exp(scale * q.k), -inf for a row that sees no key),
    delta [q_len, H] (rowsum(dO * O)), dq [q_len, H, D], dk / dv [kv_rows, H, D] (keys in [kv_len, kv_rows) get exactly 0)."""
    out = []
    for si, e in enumerate(entries):
        q_off, q_len, kv_off, kv_len, kv_rows, coff = (int(x) for x in e[:6])
        Q = q[q_off:q_off + q_len, :H * D].double().reshape(q_len, H, D)
        dO = do[q_off:q_off + q_len, :H * D].double().reshape(q_len, H, D)
        K = k[kv_off:kv_off + kv_rows, :H * D].double().reshape(kv_rows, H, D)
        V = v[kv_off:kv_off + kv_rows, :H * D].double().reshape(kv_rows, H, D)
        i = torch.arange(q_len, device=Q.device)[:, None]
        j = torch.arange(kv_rows, device=Q.device)[None, :]
        vis = j < kv_len
        if causal:
            vis = vis & (j <= i + coff)
        if key_mask is not None:
            vis = vis & (key_mask[si, :kv_rows].to(Q.device) != 0)[None, :]
        s = torch.einsum("qhd,khd->hqk", Q, K) * scale
        s = s.masked_fill(~vis[None], float("-inf"))
        lse = torch.logsumexp(s, dim=-1)                                   # [H, q]
        P = torch.where(vis[None], torch.exp(s - lse[..., None]), torch.zeros((), dtype=s.dtype, device=s.device))
        O = torch.einsum("hqk,khd->qhd", P, V)
        delta = (dO * O).sum(-1)                                           # [q, H]
        dP = torch.einsum("qhd,khd->hqk", dO, V)
        dS = P * (dP - delta.t()[..., None])
        dq = torch.einsum("hqk,khd->qhd", dS, K) * scale
        dk = torch.einsum("hqk,qhd->khd", dS, Q) * scale
        dv = torch.einsum("hqk,qhd->khd", P, dO)
        if rope is not None:
            cos_t, sin_t, pos_mod, pos0 = rope
            dq = rotate64(dq, torch.arange(q_off, q_off + q_len), cos_t, sin_t, pos_mod, pos0, inverse=True)
            dk = rotate64(dk, torch.arange(kv_off, kv_off + kv_rows), cos_t, sin_t, pos_mod, pos0, inverse=True)
        out.append(dict(o=O, lse=lse.t(), delta=delta, dq=dq, dk=dk, dv=dv))
    return out


Report = namedtuple("Report", "ratio rel mx where")


def measure(name, got, want, bound=None):
    """got / want: one tensor per sequence, [rows, H] or [rows, H, D].  Per (sequence, head) cell: the rel-L2 error and the max-abs error
    scaled by the cell's max |want|; a NaN where a number is wanted, or a mismatch where the reference is +-inf, counts as infinite.
    A cell whose exact answer is 0 (dq of a one-row sequence whose query sees one key) has no relative error to measure: cases avoid it.
    -> Report(ratio = worst of rel / bound and max / bound, worst rel, worst max, the worst cell by name)."""
    rel_b, mx_b = bound or BOUNDS[name]
    best = Report(0.0, 0.0, 0.0, f"{name}: no cells")
    for s, (g, w) in enumerate(zip(got, want)):
        g, w = g.double(), w.double().to(g.device)
        if g.dim() == 2:
            g, w = g[..., None], w[..., None]
        if w.shape[0] == 0:
            continue
        assert g.shape == w.shape, (name, s, tuple(g.shape), tuple(w.shape))
        inf = torch.isinf(w)
        bad = (inf & (g != w)) | torch.isnan(g) | (torch.isinf(g) & ~inf)
        zero = torch.zeros((), dtype=w.dtype, device=w.device)
        err = torch.where(inf | bad, zero, g - w).abs()
        w = torch.where(inf, zero, w)
        err = torch.where(bad, torch.full_like(err, float("inf")), err)
        rel = err.pow(2).sum((0, 2)).sqrt() / w.pow(2).sum((0, 2)).sqrt().clamp_min(1e-300)
        scaled = err / w.abs().amax((0, 2)).clamp_min(1e-300)[None, :, None]
        mx = scaled.amax((0, 2))
        row = scaled.amax(2).argmax(0)
        for h, (r, m, rw) in enumerate(zip(rel.tolist(), mx.tolist(), row.tolist())):
            ratio = max(r / rel_b, m / mx_b)
            if ratio >= best.ratio:
                g0 = rw // 16 * 16
                best = Report(ratio, max(r, best.rel), max(m, best.mx),
                              f"{name}: seq {s} head {h} rows {g0}..{g0 + 15}: rel-L2 {r:.3g} (bound {rel_b:.3g}), "
                              f"max-abs / max|want| {m:.3g} (bound {mx_b:.3g})")
            else:
                best = best._replace(rel=max(r, best.rel), mx=max(m, best.mx))
    return best


def check(name, got, want, bound=None, what=""):
    """measure() and fail on the worst cell; the worst values per output name are kept in WORST."""
    rep = measure(name, got, want, bound)
    r0, m0 = WORST.get(name, (0.0, 0.0))
    WORST[name] = (max(r0, rep.rel), max(m0, rep.mx))
    assert rep.ratio <= 1.0, f"{what}: {rep.where}"
    return rep
