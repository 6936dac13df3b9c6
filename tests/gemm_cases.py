"""GEMM cases shared by tests/test_gemm_paths_gpu.py and tests/test_gemm_cases_cpu.py: float64 references of the entry points of
csrc/gemm.hip, csrc/gemm_u4.hip, csrc/gemm_tn.hip and csrc/lora.hip, a restatement of their host dispatch rules (path_of), and a
comparator that bounds every element and every 64x64 cell of a result.

bf16 and e4m3 inputs are exact in float64, so the references carry only float64 summation error.  Where every kernel of an entry point
stores an intermediate in bf16 before a nonlinear step (gate|up before the SwiGLU, d_act before SwiGLU', the projection before the RoPE),
the reference rounds at the same point.  Roundings that only some kernels make in front of an addition (the product before the residual in
the 16-wave and four-wave epilogues, the base product before the pair in the two-launch LoRA fallback) are not restated: the reference
hands the magnitude of that intermediate to the comparator as `pre`, and the bound grants it half an ulp."""
from collections import Counter, namedtuple

import torch

M32 = 0xFFFFFFFF

# ---------------------------------------------------------------------------------------------------------------------- references


def act64(x, act):
    """The activations of common.h in float64: 0 none, 1 QuickGELU, 2 erf-GELU, 3 SiLU."""
    if act == 1:
        return x * torch.sigmoid(1.702 * x)
    if act == 2:
        return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))
    if act == 3:
        return x * torch.sigmoid(x)
    return x


def _mul32(x, c):
    """(x * c) mod 2^32 for int64 x in [0, 2^32) without overflowing int64."""
    return (x * (c & 0xFFFF) + ((x * (c >> 16)) << 16)) & M32


def drop_keep(seed, idx, thresh):
    """common.h drop_keep: element idx (int64 tensor) is kept iff lowbias32(idx, seed) >= thresh."""
    lo, hi = idx & M32, (idx >> 32) & M32
    x = _mul32(lo, 0x9E3779B1) ^ _mul32(hi, 0x85EBCA77) ^ (seed & M32)
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846CA68B)
    x = x ^ (x >> 16)
    return x >= thresh


def drop_params(p):
    """(thresh, scale) as lhrs_gemm_bf16_nt_dropmask derives them from p (float32 arithmetic)."""
    p32 = torch.tensor(p, dtype=torch.float32)
    return int(float(p32.double()) * 4294967296.0), float(1.0 / (1.0 - p32))


def drop_mask(M, N, seed, p, device):
    """[M, N] float64 mask * 1/(1-p) over the result elements, index m * N + n."""
    thresh, scale = drop_params(p)
    idx = torch.arange(M, device=device, dtype=torch.int64)[:, None] * N + torch.arange(N, device=device, dtype=torch.int64)[None, :]
    return drop_keep(seed, idx, thresh).double() * scale


def d64(t):
    return t.double()


def bf16_round(x):
    return x.to(torch.bfloat16).double()


Ref = namedtuple("Ref", "want pre S K_eff")


def ref_nt(A, B, *, alpha=1.0, bias=None, residual=None, act=0, A2=None, B2=None, mask=None, old=None):
    """act(alpha * (A.B^T + A2.B2^T) * mask + bias) + residual (+ old: f32 accumulate) in float64.  A [M, K], B [N, K] (the first K columns
    are used), bias [N], residual [M, N].  -> Ref(want, pre = |the value in front of the residual / accumulate|, S = |alpha| (|A|.|B|^T +
    |A2|.|B2|^T) (* mask), K_eff = K + K2)."""
    a, b = d64(A), d64(B)
    prod = a @ b.t()
    S = a.abs() @ b.abs().t()
    K_eff = a.shape[1]
    base = None
    if A2 is not None:     # the two-launch fallback stores bf16(alpha A.B^T + bias + residual), then adds the pair on top of it
        base = (alpha * prod + (0 if bias is None else d64(bias)[None, :]) + (0 if residual is None else d64(residual))).abs()
        a2, b2 = d64(A2), d64(B2)
        prod = prod + a2 @ b2.t()
        S = S + a2.abs() @ b2.abs().t()
        K_eff += a2.shape[1]
    y = alpha * prod
    S = abs(alpha) * S
    if mask is not None:
        y, S = y * mask, S * mask
    if bias is not None:
        y = y + d64(bias)[None, :]
    y = act64(y, act)
    pre = y.abs() if base is None else y.abs() + base
    if residual is not None:
        y = y + d64(residual)
    if old is not None:
        y = y + d64(old)
    return Ref(y, pre, S, K_eff)


def ref_swiglu_fwd(X, Wgu, ff, A2=None, B2=None):
    """-> (Ref of gate|up [M, 2ff], Ref of act = silu(gate) * up [M, ff] on the bf16-rounded gate|up)."""
    gu = ref_nt(X, Wgu, A2=A2, B2=B2)
    g, u = bf16_round(gu.want[:, :ff]), bf16_round(gu.want[:, ff:])
    sg = torch.sigmoid(g)
    want = g * sg * u
    dsilu = sg * (1 + g * (1 - sg))
    S = gu.S[:, :ff] * (dsilu * u).abs() + gu.S[:, ff:] * (g * sg).abs()
    return gu, Ref(want, want.abs(), S, gu.K_eff)


def ref_swiglu_bwd(dY, WdT, gu, ff, A2=None, B2=None):
    """d(gate|up) [M, 2ff] = SwiGLU'(gu) * d_act, d_act = bf16(dY . WdT^T (+ pair)) (rounded where the unfused path stores it)."""
    d = ref_nt(dY, WdT, A2=A2, B2=B2)
    da = bf16_round(d.want)
    g, u = d64(gu[:, :ff]), d64(gu[:, ff:2 * ff])
    sg = torch.sigmoid(g)
    fg = u * sg * (1 + g * (1 - sg))
    fu = g * sg
    want = torch.cat([da * fg, da * fu], 1)
    S = torch.cat([d.S * fg.abs(), d.S * fu.abs()], 1)
    return Ref(want, want.abs(), S, d.K_eff)


def rope_tables(npos, D, device):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    f = torch.outer(torch.arange(npos, dtype=torch.float64), inv)
    return f.cos().float().to(device), f.sin().float().to(device)


def ref_rope(X, W, cos_t, sin_t, pos_mod, pos0, rope_cols, head_dim, A2=None, B2=None):
    """x = bf16(X . W^T (+ pair)); heads of head_dim in columns [0, rope_cols) rotated (rotate_half) at position m % pos_mod + pos0."""
    p = ref_nt(X, W, A2=A2, B2=B2)
    x = bf16_round(p.want)
    want, S = x.clone(), p.S.clone()
    pre = x.abs()
    M = x.shape[0]
    pos = torch.arange(M, device=x.device) % pos_mod + pos0
    c, s = cos_t.double()[pos], sin_t.double()[pos]
    h = head_dim // 2
    for c0 in range(0, rope_cols, head_dim):
        x1, x2 = x[:, c0:c0 + h], x[:, c0 + h:c0 + head_dim]
        s1, s2 = p.S[:, c0:c0 + h], p.S[:, c0 + h:c0 + head_dim]
        want[:, c0:c0 + h] = x1 * c - x2 * s
        want[:, c0 + h:c0 + head_dim] = x2 * c + x1 * s
        pre[:, c0:c0 + h] = (x1 * c).abs() + (x2 * s).abs()
        pre[:, c0 + h:c0 + head_dim] = (x2 * c).abs() + (x1 * s).abs()
        S[:, c0:c0 + h] = s1 * c.abs() + s2 * s.abs()
        S[:, c0 + h:c0 + head_dim] = s2 * c.abs() + s1 * s.abs()
    return Ref(want, pre, S, p.K_eff)


def e4m3_64(a8, scale):
    """uint8 e4m3 rows with per-row fp32 scales -> exact float64 values."""
    return a8.view(torch.float8_e4m3fn).double() * scale.double()[:, None]


def ref_fp8(A8, sa, B8, sb, *, alpha=1.0, residual=None, A2=None, B2=None):
    """alpha * (sa[m] sb[n] (A8 . B8^T) + A2.B2^T) + residual on exactly dequantised operands."""
    return ref_nt(e4m3_64(A8, sa), e4m3_64(B8, sb), alpha=alpha, residual=residual, A2=A2, B2=B2)


def ref_tn(P, Q, old=None):
    """P[T, Mo]^T . Q[T, No] (+ old): the token-major products gemm_tn_f32 / gemm_tn_skinny."""
    return ref_nt(d64(P).t(), d64(Q).t(), old=old)


# ---------------------------------------------------------------------------------------------------------------------- comparator

# Bounds per output kind: (c_out, c_acc, cell).  Per element |got - want| <= c_out 2^-8 (|want| + |pre|) + c_acc 2^-24 sqrt(K_eff) S
# (f32 outputs: the second term alone), and per 64x64 cell rel-L2 <= cell.  Worst values measured on an MI355X over every case of
# test_gemm_paths_gpu.py (element: |err| / (2^-8 (|want| + |pre|) + 2^-24 sqrt(K_eff) S), resp. |err| / (2^-24 sqrt(K_eff) S);
# cell: rel-L2), bound ~2.5x that:
#   bf16   element 1.80   cell 2.9e-3            f32    element 0.190  cell 5.5e-7 (splitk_f32, K = 27392)
#   gu     element 0.50   cell 1.9e-3            act    element 1.52   cell 2.2e-3
#   dgu    element 1.40   cell 2.2e-3            rope   element 1.40   cell 1.8e-3
BOUNDS = {
    "bf16": (4.5, 4.5, 7.2e-3),
    "f32": (0.0, 0.48, 1.4e-6),
    "gu": (1.25, 1.25, 4.7e-3),
    "act": (3.8, 3.8, 5.5e-3),
    "dgu": (3.5, 3.5, 5.5e-3),
    "rope": (3.5, 3.5, 4.4e-3),
}

# worst (element ratio at c = 1, cell rel-L2) per output kind seen by check() in this process (how the values above were measured)
WORST = {}

Report = namedtuple("Report", "ratio elem cell where")


def _segment_of(row, segments):
    for r0, r1, kern in segments or ():
        if r0 <= row < r1:
            return f"{kern} rows {r0}..{r1 - 1}"
    return "?"


def measure(kind, got, ref, segments=None, bound=None):
    """got: [M, N] result (any float dtype), ref: Ref.  -> Report(ratio = worst of element error / bound and cell rel-L2 / bound, the
    worst element ratio at c_out = c_acc = 1, the worst cell rel-L2, where: the path segment, worst cell and worst element)."""
    c_out, c_acc, cell_b = bound or BOUNDS[kind]
    want = ref.want.to(got.device)
    g = got.double()
    assert g.shape == want.shape, (kind, tuple(g.shape), tuple(want.shape))
    err = (g - want).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    acc_t = 2.0 ** -24 * ref.K_eff ** 0.5 * ref.S.to(got.device)
    out_t = 2.0 ** -8 * (want.abs() + ref.pre.to(got.device))
    unit = acc_t if kind == "f32" else out_t + acc_t
    ratio1 = err / unit.clamp_min(1e-300)
    bound_e = (c_acc * acc_t if kind == "f32" else c_out * out_t + c_acc * acc_t).clamp_min(1e-300)
    r_el = err / bound_e
    M, N = want.shape
    Mp, Np = -(-M // 64) * 64, -(-N // 64) * 64
    e2 = torch.zeros(Mp, Np, dtype=torch.float64, device=g.device)
    w2 = torch.zeros_like(e2)
    e2[:M, :N] = err.pow(2)
    w2[:M, :N] = want.pow(2)
    ce = e2.reshape(Mp // 64, 64, Np // 64, 64).sum((1, 3)).sqrt()
    cw = w2.reshape(Mp // 64, 64, Np // 64, 64).sum((1, 3)).sqrt()
    rel = ce / cw.clamp_min(1e-300)
    rel = torch.where(torch.isnan(rel), torch.full_like(rel, float("inf")), rel)
    i_el = int(r_el.reshape(-1).nan_to_num(float("inf")).argmax())
    i_c = int(rel.reshape(-1).argmax())
    em, en = divmod(i_el, N)
    cm, cn = divmod(i_c, rel.shape[1])
    worst_el, worst_cell = float(r_el.reshape(-1)[i_el]), float(rel.reshape(-1)[i_c])
    ratio = max(worst_el, worst_cell / cell_b)
    where = (f"{kind}: element ({em}, {en}) [{_segment_of(em, segments)}] got {float(g[em, en]):.6g} want {float(want[em, en]):.6g}, "
             f"{worst_el:.3g}x its bound; cell rows {cm * 64}..{cm * 64 + 63} cols {cn * 64}..{cn * 64 + 63} "
             f"[{_segment_of(cm * 64, segments)}] rel-L2 {worst_cell:.3g} ({worst_cell / cell_b:.3g}x the bound {cell_b:.3g})")
    return Report(ratio, float(ratio1.max()), worst_cell, where)


def check(kind, got, ref, segments=None, what=""):
    """measure() and fail on the worst element or cell; the worst values per output kind are kept in WORST."""
    rep = measure(kind, got, ref, segments)
    e0, c0 = WORST.get(kind, (0.0, 0.0))
    WORST[kind] = (max(e0, rep.elem), max(c0, rep.cell))
    assert rep.ratio <= 1.0, f"{what}: {rep.where}"
    return rep


# ---------------------------------------------------------------------------------------------------------------------- host rules
# Default settings: gemm_set_u4 on, lhrs_gemm_set_policy 2, set_bm144 1, set_min_tiles 128, set_tail_split 1, set_small_thresh 256, and a
# registered GEMM workspace.  `cus`: the CU count num_cus() returns (256 without a device).


def cdiv(a, b):
    return -(-a // b)


class Plan:
    """segments: [(row0, row1, kernel)] in launch order; kinds: Counter of gemm_kernel_census kinds; launches: GEMM launches counted by
    the library's profile (lhrs_gemm_profile_read out[3])."""

    def __init__(self):
        self.segments, self.kinds, self.launches = [], Counter(), 0

    def add(self, r0, r1, kernel, kind=None):
        self.segments.append((r0, r1, kernel))
        self.launches += 1
        if kind is not None:
            self.kinds[kind] += 1

    def kernels(self):
        return tuple(k for _, _, k in self.segments)


def u4_takes(M, N, K, lda, ldb, ldc, ldr=0, bias=False, act=0, out_f32=False, accumulate=False, alpha=1.0, cus=256):
    """lhrs_gemm_u4_takes (gemm_plan.h: u4_takes)"""
    tiles = cdiv(M, 256) * cdiv(N, 256)
    return (not bias and act == 0 and not out_f32 and not accumulate and alpha == 1.0 and K >= 4096 and K % 64 == 0 and M >= 1024 and
            N >= 1024 and 5 * tiles >= 4 * cus and lda % 8 == 0 and ldb % 8 == 0 and ldc % 8 == 0 and ldr % 8 == 0)


def u4_fused_takes(kind, M, tiles_n, K, K2, cus=256):
    """lhrs_gemm_u4_fused_takes (gemm_plan.h: u4_fused_takes); kind 0 RoPE, 1 SwiGLU forward, 2 SwiGLU backward"""
    T = cdiv(M, 256) * tiles_n
    R = (T + cus - 1) // cus * cus
    idle_ok = 100 * R <= 105 * T if kind == 2 else 20 * R <= 23 * T
    return (K2 % 64 == 0 if kind == 0 else K2 == 0) and K >= 4096 and K % 64 == 0 and M >= 1024 and 5 * T >= 4 * cus and idle_ok


def u4_main_rows(M, tiles_n, cus=256):
    """lhrs_gemm_u4_main_rows (gemm_plan.h: u4_main_rows)"""
    tm = cdiv(M, 256)
    T = tm * tiles_n
    full = T // cus
    if T % cus == 0 or full < 1 or 20 * ((T + cus - 1) // cus * cus) <= 23 * T:
        return M
    tm_main = full * cus // tiles_n
    return tm_main * 256 if 1 <= tm_main < tm else M


def swiglu_fusable(tiles, ff, K, K2, lda=8, ldb=8):
    """gemm_plan.h: swiglu_fusable"""
    return ff % 256 == 0 and K % 64 == 0 and K2 % 64 == 0 and K + K2 >= 128 and tiles >= 128 and lda % 8 == 0 and ldb % 8 == 0


def pick_144(M, tiles_n, K, K2, drop, cus=256):
    """gemm_plan.h: pick_144 at set_bm144(1)"""
    if K2 > 0 or drop or K < 192:
        return False
    t256, t144 = cdiv(M, 256) * tiles_n, cdiv(M, 144) * tiles_n
    nk = K // 64
    r144, r256 = cdiv(t144, cus), cdiv(t256, cus)
    if nk <= 32:
        return r144 * (1.15 * nk + 5.0) < r256 * (1.5 * nk + 20.0)
    return r144 * 0.8 < r256


def _tail_split(M, tiles_n, cus, rounds_by_cus):
    """The tail-row rule (gemm_plan.h: tail_main_rows) -> main rows or None.  rounds_by_cus: the cost of the unsplit walk counts rounds of
    the CU count (plan_rows: its unsplit_cus argument) or of 256 (the SwiGLU-forward and e4m3 callers)."""
    tm = cdiv(M, 256)
    T = tm * tiles_n
    full = T // 256
    tm_main = full * 256 // tiles_n
    if not (full >= 1 and T % 256 != 0 and 1 <= tm_main < tm):
        return None
    t_main = tm_main * tiles_n
    cost = (t_main + 255) // 256 + 2.5 * (T - t_main) / 256.0 + 0.05
    unsplit = cdiv(T, cus) if rounds_by_cus else (T + 255) // 256
    return tm_main * 256 if cost < unsplit else None


def splitk_tail_splits(M_tail, N, K, cus=256, workspace=True):
    """gemm_plan.h: splitk_tail_splits: slab count, or 0 when it does not apply"""
    splits = (K + 2048) // 4096 if K >= 8192 else 1
    if splits <= 1 or N % 128 != 0 or not workspace or splits * M_tail * N * 4 > cus * 256 * 256 * 4:
        return 0
    return splits


def _gemm_launch(P, r0, M, N, K, *, K2=0, bias=False, res=False, act=0, out_f32=False, accumulate=False, drop=False, ldc=None,
                 ldr=None, split_ok=True, cus=256, workspace=True):
    """gemm_plan.h: plan_rows"""
    ldc = N if ldc is None else ldc
    ldr = N if ldr is None else ldr
    t128, t64x128, t256 = cdiv(M, 128) * cdiv(N, 128), cdiv(M, 64) * cdiv(N, 128), cdiv(M, 256) * cdiv(N, 256)
    al16 = out_f32 or (N % 8 == 0 and ldc % 8 == 0 and (not res or ldr % 8 == 0))
    use256 = t256 >= 128 and K >= 128 and al16
    if (not use256 and al16 and not out_f32 and K % 64 == 0 and K >= 192 and K2 == 0 and not drop and t256 >= 64 and
            200 <= cdiv(M, 144) * cdiv(N, 256) <= cus):
        use256 = True
    if K2 > 0 and not use256:
        _gemm_launch(P, r0, M, N, K, bias=bias, res=res, act=act, out_f32=out_f32, accumulate=accumulate, drop=drop, ldc=ldc, ldr=ldr,
                     split_ok=split_ok, cus=cus, workspace=workspace)
        _gemm_launch(P, r0, M, N, K2, res=not out_f32, out_f32=out_f32, accumulate=out_f32, ldc=ldc, ldr=ldc, split_ok=split_ok, cus=cus,
                     workspace=workspace)
        return
    bm144 = use256 and not out_f32 and pick_144(M, cdiv(N, 256), K, K2, drop, cus)
    if use256 and not bm144 and split_ok and not drop:
        Mm = _tail_split(M, cdiv(N, 256), cus, True)
        if Mm is not None:
            _gemm_launch(P, r0, Mm, N, K, K2=K2, bias=bias, res=res, act=act, out_f32=out_f32, accumulate=accumulate, ldc=ldc, ldr=ldr,
                         split_ok=False, cus=cus, workspace=workspace)
            if not out_f32 and K2 == 0 and not bias and act == 0 and splitk_tail_splits(M - Mm, N, K, cus, workspace):
                P.add(r0 + Mm, r0 + M, "splitk_tail")
                return
            _gemm_launch(P, r0 + Mm, M - Mm, N, K, K2=K2, bias=bias, res=res, act=act, out_f32=out_f32, accumulate=accumulate, ldc=ldc,
                         ldr=ldr, split_ok=False, cus=cus, workspace=workspace)
            return
    if use256:
        P.add(r0, r0 + M, "144" if bm144 else "256", 4 if bm144 else 0)
    elif t128 >= 384:
        P.add(r0, r0 + M, "t128")
    elif t64x128 >= 256:
        P.add(r0, r0 + M, "t64x128")
    else:
        P.add(r0, r0 + M, "t64x64")


def path_of(entry, M, N, K, *, K2=0, bias=False, res=False, act=0, out_f32=False, accumulate=False, alpha=1.0, lda=None, ldb=None,
            ldc=None, ldr=None, al16_ptrs=True, ff=None, ld_gu=None, ld_act=None, rope_cols=0, head_dim=128, cus=256, workspace=True):
    """The host dispatch of one call restated -> Plan.  entry: 'nt' (lhrs_gemm_bf16_nt), 'lora' (lhrs_gemm_bf16_nt_lora), 'mask'
    (lhrs_gemm_bf16_nt_dropmask), 'swiglu_fwd' / 'swiglu_bwd' (N ignored: ff), 'rope' (lhrs_gemm_rope_fwd), 'fp8' (lhrs_gemm_fp8_nt(_lora)),
    'splitk_f32' (lhrs_gemm_bf16_nt_splitk_f32), 'int8' (lhrs_gemm_int8_nt: always one 'i8_256' segment).  al16_ptrs: every operand / result pointer 16-byte aligned.  Kernels: 'u4', 'splitk_tail',
    '256', '144', 't128', 't64x128', 't64x64' (the small tiles), 'u4_swiglu_fwd' ..., 'swiglu_fwd_256' ..., 'fp8_256', 'fp8_small',
    'splitk_f32'; the SwiGLU and RoPE elementwise passes of the unfused fallbacks are no GEMM launches and are not listed."""
    P = Plan()
    lda, ldb = K if lda is None else lda, K if ldb is None else ldb
    kw = dict(cus=cus, workspace=workspace)
    if entry in ("nt", "lora"):
        ldc = N if ldc is None else ldc
        ldr_u4 = (N if ldr is None else ldr) if res else 0
        if u4_takes(M, N, K, lda, ldb, ldc, ldr_u4, bias, act, out_f32, accumulate, alpha, cus) and al16_ptrs:
            Mu = u4_main_rows(M, cdiv(N, 256), cus)
            P.add(0, Mu, "u4", 5 if res else 6)
            if Mu < M:
                if K2 == 0 and splitk_tail_splits(M - Mu, N, K, **kw):
                    P.add(Mu, M, "splitk_tail")
                else:
                    _gemm_launch(P, Mu, M - Mu, N, K, K2=K2, res=res, ldc=ldc, ldr=ldr, **kw)
            return P
        _gemm_launch(P, 0, M, N, K, K2=K2, bias=bias, res=res, act=act, out_f32=out_f32, accumulate=accumulate, ldc=ldc, ldr=ldr, **kw)
    elif entry == "mask":
        _gemm_launch(P, 0, M, N, K, res=res, drop=True, ldc=ldc, ldr=ldr, **kw)
    elif entry == "swiglu_fwd":
        _swiglu_fwd(P, 0, M, ff, K, K2, 2 * ff if ld_gu is None else ld_gu, ff if ld_act is None else ld_act, True, cus, workspace)
    elif entry == "swiglu_bwd":
        if u4_fused_takes(2, M, cdiv(ff, 256), K, K2, cus):
            P.add(0, M, "u4_swiglu_bwd", 8)
        elif not swiglu_fusable(cdiv(M, 256) * cdiv(ff, 256), ff, K, K2, lda, ldb):
            _gemm_launch(P, 0, M, ff, K, K2=K2, **kw)
        else:
            b144 = pick_144(M, cdiv(ff, 256), K, K2, False, cus)
            P.add(0, M, "swiglu_bwd_144" if b144 else "swiglu_bwd_256", 2)
    elif entry == "rope":
        fused = (head_dim == 128 and rope_cols % 256 == 0 and N % 8 == 0 and K % 64 == 0 and K2 % 64 == 0 and K + K2 >= 128 and
                 cdiv(M, 256) * cdiv(N, 256) >= 128 and lda % 8 == 0 and ldb % 8 == 0)
        if not fused:
            _gemm_launch(P, 0, M, N, K, K2=K2, **kw)
        elif u4_fused_takes(0, M, cdiv(N, 256), K, K2, cus):
            P.add(0, M, "u4_rope", 9)
        else:
            P.add(0, M, "rope_144" if pick_144(M, cdiv(N, 256), K, K2, False, cus) else "rope_256", 3)
    elif entry == "fp8":
        Mm = _tail_split(M, cdiv(N, 256), cus, False)
        if Mm is not None:
            P.add(0, Mm, "fp8_256")
            P.add(Mm, M, "fp8_small")
        else:
            P.add(0, M, "fp8_256")
    elif entry == "int8":
        P.add(0, M, "i8_256")      # gemm_plan takes no tail split for int8: the small-tile sibling exists for e4m3 only
    elif entry == "splitk_f32":
        if splitk_splits(M, N, K) == 1:
            _gemm_launch(P, 0, M, N, K, out_f32=True, ldc=ldc, **kw)
        else:
            P.add(0, M, "splitk_f32")
    else:
        raise ValueError(entry)
    return P


def _swiglu_fwd(P, r0, M, ff, K, K2, ld_gu, ld_act, split_ok, cus, workspace):
    """lhrs_gemm_swiglu_fwd (gemm_plan.h: plan_swiglu_fwd)"""
    if ff % 128 == 0 and u4_fused_takes(1, M, ff // 128, K, K2, cus):
        P.add(r0, r0 + M, "u4_swiglu_fwd", 7)
        return
    if not swiglu_fusable(cdiv(M, 256) * (ff // 128), ff, K, K2):
        _gemm_launch(P, r0, M, 2 * ff, K, K2=K2, cus=cus, workspace=workspace)
        return
    b144 = pick_144(M, ff // 128, K, K2, False, cus)
    if not b144 and split_ok and ld_gu == 2 * ff and ld_act == ff:
        Mm = _tail_split(M, ff // 128, cus, False)
        if Mm is not None:
            _swiglu_fwd(P, r0, Mm, ff, K, K2, ld_gu, ld_act, False, cus, workspace)
            _gemm_launch(P, r0 + Mm, M - Mm, 2 * ff, K, K2=K2, cus=cus, workspace=workspace)
            return
    P.add(r0, r0 + M, "swiglu_fwd_144" if b144 else "swiglu_fwd_256", 1)


def splitk_splits(M, N, K):
    """lhrs_gemm_splitk_splits (gemm_plan.h: splitk_f32_splits)"""
    tiles = cdiv(M, 128) * cdiv(N, 128)
    return max(1, min((512 + tiles // 2) // tiles, K // 1024, 8))


def skinny_splits(K, N):
    """lhrs_gemm_skinny_splits (gemm.hip)"""
    return max(1, min(K // 512, 16 if N <= 128 else 4))


def tn_splits(T, Mo, No):
    """lhrs_gemm_tn_splits (gemm_tn.hip), 64-token stages"""
    tiles = (Mo // 128) * (No // 128)
    if tiles < 1 or T < 1:
        return 1
    stages = cdiv(T, 64)
    return max(1, min(cdiv(512, tiles), stages // 8, 32))


def tn_skinny_splits(M, N):
    """lhrs_tn_skinny_splits (lora.hip)"""
    return max(1, min(cdiv(1024, cdiv(N, 64)), cdiv(M, 64), 16))


# the (entry, kernels) combinations default settings reach, by a sweep of the host rules over the shapes the product and its boundaries use
_SWEEP_M = (300, 2000, 2184, 3000, 3839, 4000, 4096, 7710, 8190, 8736)
_SWEEP_N = (264, 1024, 2048, 4096, 4100, 11008)
_SWEEP_K = (256, 320, 512, 1024, 4096, 11008)


_LAUNCH_KERNELS = {"256", "144", "t128", "t64x128", "t64x64", "splitk_tail"}


def cells_of(entry, kernels):
    """{(entry, kernel)} of one path.  The unfused fallbacks of the SwiGLU and RoPE entry points run the plain launcher (plan_rows, whose kernels the 'nt' cells
    cover) and an elementwise pass: one cell 'unfused' each."""
    if entry in ("swiglu_fwd", "swiglu_bwd", "rope"):
        return {(entry, "unfused" if k in _LAUNCH_KERNELS else k) for k in kernels}
    return {(entry, k) for k in kernels}


def reachable_cells(cus=256):
    """-> {(entry, kernel)}: every kernel each entry point reaches in the sweep (combinations of segments: reachable_paths)"""
    return set().union(*(cells_of(e, ks) for e, ks in reachable_paths(cus)))


def reachable_paths(cus=256):
    cells = set()
    for M in _SWEEP_M:
        for N in _SWEEP_N:
            for K in _SWEEP_K:
                for entry, kw in (("nt", {}), ("nt", dict(bias=True)), ("lora", dict(K2=64)), ("mask", {})):
                    cells.add((entry, path_of(entry, M, N, K, cus=cus, **kw).kernels()))
                if N % 8 == 0 and K % 128 == 0 and K >= 256:
                    cells.add(("fp8", path_of("fp8", M, N, K, cus=cus).kernels()))
                    cells.add(("int8", path_of("int8", M, N, K, cus=cus).kernels()))
                if N % 256 == 0:
                    cells.add(("rope", path_of("rope", M, N, K, rope_cols=N // 2, cus=cus).kernels()))
                    cells.add(("rope", path_of("rope", M, N, K, K2=64, rope_cols=N // 2, cus=cus).kernels()))
            for ff in (1000, 2048, 4096, 11008):
                for K in _SWEEP_K:
                    cells.add(("swiglu_fwd", path_of("swiglu_fwd", M, 0, K, ff=ff, cus=cus).kernels()))
                    cells.add(("swiglu_bwd", path_of("swiglu_bwd", M, 0, K, ff=ff, cus=cus).kernels()))
    return cells
