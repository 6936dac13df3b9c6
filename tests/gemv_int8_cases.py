"""Cases of the int8 decode weight stream (csrc/gemv_int8.hip: int8_decode_prepare_kernel, repack_int8_mfma_kernel, gemv_int8_kernel behind
lhrs_int8_decode_prepare / lhrs_repack_int8_mfma / lhrs_gemv_int8), shared by tests/test_gemv_int8_gpu.py and
tests/test_gemv_int8_cases_cpu.py.  Imports no GPU and shares no code with the HIP source.

Reference.  int8_cases.ref_prepare / ref_linear (imported, not restated): everything the prepare writes is a function of bf16 inputs through
single correctly rounded fp32 operations and has ONE right answer; the linear is the float64 value on the int8 codes,
    sx[b] sw[n] sum_k XQ WQ + sum_j xo[b, j] bf16(WQ[n, idx[j]] sw[n]) + residual.

Emulation.  emu_prepare is int8_cases.emu_prepare (a model of the same rules, with its mutants) read without its padding: idx[:n] and
xo[:, :n] are all this kernel writes, and meta holds n alone.  emu_gemv restates the ORDER of gemv_int8_kernel:
    exact integer sum -> one conversion to fp32 -> one multiply by fl(sx[b] * sw[n]) -> the outlier term as 64 fp32 chains (lane l takes
    j = l, l + 64, ...; the products of two bf16 values are exact in fp32) folded by the 64-lane butterfly, added to the scaled sum -> residual
    -> one store.

Bounds (none of them sized from the kernel):
  prepare outputs, the operand-map probe            exact equality
  fp32 output, n = 0, no residual                   bit-equal to f32(acc) * fl(sx * sw): the sum is exact, the rest is two correctly rounded
                                                    fp32 operations in a fixed order
  bf16 output, n = 0, no residual                   int8_cases.tight_bound_ok: (2^-8 + 2^-21) |want|
  everything else                                   gemv_cases.measure's form with c = 4 x EMU_WORST, the emulation's worst ratio against
                                                    float64 over the cases (tests/test_gemv_int8_cases_cpu.py recomputes and asserts it)
"""
import math
from collections import namedtuple

import torch

import gemv_cases as gc
import int8_cases as ic

BF, F32 = torch.bfloat16, torch.float32
THR = ic.THR
KSTEP = 64                     # one v_mfma_i32_16x16x64_i8 per step
PREPARE_MAX_K = 1024 * 2 * 8   # the prepare keeps two 8-column chunks per thread of a 1024-thread block
NAN = float("nan")

# kind -> worst ratio at c = 1 of the unmutated emulation against float64 over GEMV + STRIDED + the reuse calls (recomputed on the CPU)
EMU_WORST = {"bf16": 1.967, "f32": 0.008641}
BOUNDS = {k: 4.0 * v for k, v in EMU_WORST.items()}
WORST = {}
Report = namedtuple("Report", "ratio unit where")


def measure(kind, got, ref, op="", case=""):
    """gemv_cases.measure with this file's constants: got [rows >= B, N], rows past ref.want must still hold NaN"""
    want = ref.want.double()
    g = got.double().cpu()
    rows = want.shape[0]
    assert g.shape[0] >= rows and g.shape[1:] == want.shape[1:], (op, case, kind, tuple(g.shape), tuple(want.shape))
    guard, g = g[rows:], g[:rows]
    unit = 2.0 ** -24 * math.sqrt(ref.n) * ref.A.double()
    if not ref.f32:
        unit = unit + 2.0 ** -9 * want.abs()
    err = (g - want).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    r1 = torch.where(err == 0, torch.zeros_like(err), err / unit.clamp_min(1e-300))
    i = int(r1.reshape(-1).nan_to_num(float("inf")).argmax())
    row, col = divmod(i, want.shape[1])
    u = float(r1.reshape(-1)[i])
    where = (f"{op} [{case}] {kind}: row {row} col {col} got {float(g[row, col]):.9g} want {float(want[row, col]):.9g}, "
             f"{u / BOUNDS[kind]:.3g}x its bound ({u:.3g} at c = 1, c = {BOUNDS[kind]:.3g})")
    if guard.numel() and not bool(torch.isnan(guard).all()):
        u, where = float("inf"), f"{op} [{case}] {kind}: a batch row past B was written"
    return Report(u / BOUNDS[kind], u, where)


def check(kind, got, ref, op="", case=""):
    rep = measure(kind, got, ref, op, case)
    WORST[kind] = max(WORST.get(kind, 0.0), rep.unit)
    assert rep.ratio <= 1.0, rep.where
    return rep


# ------------------------------------------------------------------------------------------------------------------------- emulation
MUTANTS = ("k_half_of_a_fragment_dropped", "outlier_term_dropped", "outlier_term_doubled", "stale_meta", "residual_after_bf16_store",
           "factor_product_wrong_order", "gt_instead_of_ge", "absmax_counts_outlier_entries", "outlier_columns_not_zeroed",
           "round_half_away_from_zero")
PREPARE_MUTANTS = MUTANTS[6:]


class EmuWorkspace:
    """Model of hk.Int8DecodeWorkspace: idx, xo and meta survive a call (the kernels write idx[:n] / xo[:, :n] only)."""

    def __init__(self, B, kmax):
        self.idx = torch.zeros(kmax, dtype=torch.int32)
        self.xo = torch.zeros(B, kmax, dtype=BF)
        self.meta, self.prev_meta = 0, 0


def emu_prepare(h, ws, mut=()):
    """-> (XQ int8 [B, K], sx fp32 [B]); ws.idx[:n], ws.xo[:B, :n], ws.meta = n"""
    B, K = h.shape
    w = ic.EmuWorkspace(K)
    A2 = torch.zeros(B, ic.ceil64(K), dtype=BF)
    B2 = torch.zeros(1, ic.ceil64(K), dtype=BF)
    XQ, sx, _ = ic.emu_prepare(h, torch.zeros(1, K, dtype=torch.int8), torch.zeros(1), w, A2, B2, THR, tuple(m for m in mut if m in PREPARE_MUTANTS))
    n = w.meta[0]
    ws.prev_meta, ws.meta = ws.meta, n
    ws.idx[:n] = w.idx[:n]
    ws.xo[:B, :n] = A2[:, :n]
    return XQ, sx


def emu_gemv(XQ, sx, wq, sw, ws, res=None, f32=False, mut=()):
    """gemv_int8_kernel -> [B + 1, N] with one guard row of NaN"""
    B, K = XQ.shape
    N = wq.shape[0]
    acc = XQ.long() @ wq.long().t()
    if "k_half_of_a_fragment_dropped" in mut:          # bytes [8, 16) of the first lane group's 16-byte fragment of step 0
        acc = acc - XQ[:, 8:16].long() @ wq[:, 8:16].long().t()
    t = acc.float()
    if "factor_product_wrong_order" in mut:
        t = (t * sx[:, None]) * sw[None, :]
    else:
        t = t * (sx[:, None] * sw[None, :])
    n = ws.prev_meta if "stale_meta" in mut else ws.meta
    if "outlier_term_dropped" in mut:
        n = 0
    if n > 0:
        k = ws.idx[:n].long()
        wd = (wq[:, k].float() * sw[:, None]).to(BF).float()          # [N, n]
        xo = ws.xo[:B, :n].float()                                     # [B, n]
        J = -(-n // 64)
        terms = torch.zeros(B, N, J * 64)
        terms[:, :, :n] = xo[:, None, :] * wd[None, :, :]
        terms = terms.reshape(B, N, J, 64)
        o = torch.zeros(B, N, 64)
        for j in range(J):                                             # lane l: j = l, l + 64, ... in order
            o = o + terms[:, :, j]
        for sh in (32, 16, 8, 4, 2, 1):                                # the 64-lane butterfly
            o = o + o[..., torch.arange(64) ^ sh]
        o = o[..., 0]
        t = t + o
        if "outlier_term_doubled" in mut:
            t = t + o
    out = torch.full((B + 1, N), NAN, dtype=F32 if f32 else BF)
    if res is not None and "residual_after_bf16_store" in mut and not f32:
        out[:B] = (t.to(BF).float() + res.float()).to(BF)
        return out
    if res is not None:
        t = t + res.float()
    out[:B] = t if f32 else t.to(BF)
    return out


# ------------------------------------------------------------------------------------------------------------------------- host rules
class Rejected(ValueError):
    pass


def gemv_rule(B, N, K, *, packed=False, ldw=None, ldq=None, ldo=None, ldr=None, ldy=None, res=False, align=True):
    """lhrs_gemv_int8's host rule, restated; strides default to the dense ones"""
    ldw, ldq, ldo, ldy = K if ldw is None else ldw, K if ldq is None else ldq, K if ldo is None else ldo, N if ldy is None else ldy
    if not (1 <= B <= 16 and N > 0 and K >= KSTEP and K % KSTEP == 0):
        raise Rejected("B / N / K")
    if not align or (not packed and (ldw % 16 or ldw < K)) or ldq % 16 or ldq < K or ldo < 1 or ldy < N or (res and (N if ldr is None else ldr) < N):
        raise Rejected("pointers / strides")


def prepare_rule(B, K, *, pro=0, norm_w=True, thr=THR, ldx=None, ldq=None, ldo=None, align=True):
    ldx, ldq, ldo = (2 * K if pro == 2 else K) if ldx is None else ldx, K if ldq is None else ldq, K if ldo is None else ldo
    if not (1 <= B <= 16 and K >= KSTEP and K % KSTEP == 0 and K <= PREPARE_MAX_K):
        raise Rejected("B / K")
    if pro not in (0, 1, 2) or (pro == 1 and not norm_w) or not thr > 0:
        raise Rejected("prologue / thr")
    if not align or ldx % 8 or ldx < (2 * K if pro == 2 else K) or ldq % 16 or ldq < K or ldo < K:
        raise Rejected("pointers / strides")


def repack_rule(N, K, *, ldw=None, align=True):
    ldw = K if ldw is None else ldw
    if not (N > 0 and K >= KSTEP and K % KSTEP == 0):
        raise Rejected("N / K")
    if not align or ldw % 16 or ldw < K:
        raise Rejected("pointers / strides")


# name -> (entry point, keyword arguments of the rule, a fragment of the message lhrs_last_error must hold)
REJECTS = {
    "gemv_B0": ("gemv", dict(B=0, N=16, K=128), "B=0 (1..16)"),
    "gemv_B17": ("gemv", dict(B=17, N=16, K=128), "B=17 (1..16)"),
    "gemv_K96": ("gemv", dict(B=1, N=16, K=96), "K=96 (K % 64 == 0)"),
    "gemv_unaligned": ("gemv", dict(B=1, N=16, K=128, align=False), "pointers / strides"),
    "gemv_ldw_not_16": ("gemv", dict(B=1, N=16, K=128, ldw=136), "pointers / strides"),
    "gemv_ldq_short": ("gemv", dict(B=1, N=16, K=128, ldq=64), "pointers / strides"),
    "gemv_ldy_short": ("gemv", dict(B=1, N=16, K=128, ldy=8), "pointers / strides"),
    "prepare_B17": ("prepare", dict(B=17, K=128), "B=17 (1..16)"),
    "prepare_K96": ("prepare", dict(B=1, K=96), "K=96"),
    "prepare_K_too_long": ("prepare", dict(B=1, K=PREPARE_MAX_K + 64), f"K <= {PREPARE_MAX_K}"),
    "prepare_rms_without_weight": ("prepare", dict(B=1, K=128, pro=1, norm_w=False), "prologue=1"),
    "prepare_thr0": ("prepare", dict(B=1, K=128, thr=0.0), "thr=0"),
    "prepare_ldq_not_16": ("prepare", dict(B=1, K=128, ldq=136), "pointers / strides"),
    "prepare_ldo_short": ("prepare", dict(B=1, K=128, ldo=64), "pointers / strides"),
    "repack_K96": ("repack", dict(N=16, K=96), "K=96 (K % 64 == 0)"),
    "repack_unaligned": ("repack", dict(N=16, K=128, align=False), "pointers / strides"),
}
ACCEPTS = (("gemv", dict(B=1, N=4096, K=4096)), ("gemv", dict(B=16, N=4096, K=11008, packed=True, ldw=0)), ("prepare", dict(B=16, K=11008, pro=2)),
           ("prepare", dict(B=1, K=4096, pro=1)), ("repack", dict(N=4099, K=11008)))
RULES = {"gemv": gemv_rule, "prepare": prepare_rule, "repack": repack_rule}


def wave_steps(K):
    """per wave the (begin, end) of its 64-k steps"""
    ns = K // KSTEP
    per = -(-ns // 8)
    return [(min(w * per, ns), min(min(w * per, ns) + per, ns)) for w in range(8)]


def repack(wq):
    """int8 [N, K] -> the tiled copy [ceil(N/16), K/64, 64, 16] as lhrs_repack_int8_mfma writes it"""
    N, K = wq.shape
    G = (N + 15) // 16
    p = torch.zeros(G * 16, K, dtype=torch.int8)
    p[:N] = wq
    return p.reshape(G, 16, K // 64, 4, 16).permute(0, 2, 3, 1, 4).reshape(G, K // 64, 64, 16).contiguous()


# ------------------------------------------------------------------------------------------------------------------------- GEMV cases
Case = namedtuple("Case", "name edge B N K n f32 res build")


def _x_boundaries(seed, B, K, n):
    """n outlier columns that include 0, 1, 63, 64, 127, 128 and K - 1 (either side of every 64-k step boundary); rows alternate 0 / B - 1"""
    g = ic._gen(seed)
    x = ic.base_x(g, B, K)
    special = [0, 1, 63, 64, 127, 128, K - 1]
    rest = [c for c in torch.randperm(K, generator=g).tolist() if c not in special][:n - len(special)]
    for j, c in enumerate(sorted(special + rest)):
        x[(0, B - 1)[j % 2], c] = ic.VALS[j % len(ic.VALS)]
    return x


def _x_zero_row(seed, B, K):
    x = ic.make_x(seed, B, K, 0)
    x[1] = 0
    return x


GEMV = [
    Case("b1_n16_k128_n0_f32", "the minimum: one row block, two steps on waves 0 and 1", 1, 16, 128, 0, True, False, lambda: ic.make_x(71, 1, 128, 0)),
    Case("b16_n48_k384_n0", "fewer k-steps (6) than waves; a full batch", 16, 48, 384, 0, False, False, lambda: ic.make_x(72, 16, 384, 0)),
    Case("b3_n40_k1152_n1_res", "ragged last row block; 18 steps split 3 3 3 3 3 3 0 0; the outlier at column K - 1, set by the last row alone",
         3, 40, 1152, 1, False, True, lambda: ic.make_x(73, 3, 1152, 1, first=1)),
    Case("b5_n64_k1152_n65_res", "columns 0, 1, 63, 64, 127, 128, K - 1 on either side of every step boundary", 5, 64, 1152, 65, False, True,
         lambda: _x_boundaries(74, 5, 1152, 65)),
    Case("b2_n32_k256_nK", "every column an outlier; row 1 holds nothing below 6: sx = 0, codes 0, the result is the 16-bit term alone",
         2, 32, 256, 256, False, False, lambda: ic._x_full_row(75, 2, 256, 1)),
    Case("b16_n16_k11008_n300_f32", "the real down_proj depth: 172 steps, 22 per wave and 18 on the last", 16, 16, 11008, 300, True, False,
         lambda: ic.make_x(76, 16, 11008, 300)),
    Case("b4_n32_k256_n0_zero_rows", "an all-zero weight row (wscale 0) and an all-zero activation row (sx 0)", 4, 32, 256, 0, False, False,
         lambda: _x_zero_row(77, 4, 256)),
]
STRIDED = Case("b3_n40_k384_n3_res_strided", "ldw, ldq, ldo, ldr, ldy all larger than the logical widths", 3, 40, 384, 3, False, True,
               lambda: ic.make_x(78, 3, 384, 3))
STRIDES = dict(ldw=384 + 64, ldq=384 + 128, ldo=384 + 8, ldr=40 + 3, ldy=40 + 5)
REUSE = (4, 32, 256)           # (B, N, K) of the three calls in a row on one workspace: int8_cases.REUSE_N outlier columns


def kind_of(c):
    return "f32" if c.f32 else "bf16"


_INPUTS, _REFS = {}, {}


def inputs(c):
    """seeded CPU tensors of a case (computed once, shared, never modified): h bf16 [B, K], wq int8 [N, K], wscale fp32 [N], res bf16 [B, N] | None"""
    if c.name not in _INPUTS:
        h = c.build()
        w = ic.make_w(200 + c.N + c.K, c.N, c.K)
        if "zero_rows" in c.name:
            w[5] = 0
        wq, wscale, _ = ic.ref_quant_rows(w)
        g = ic._gen(300 + c.B + c.N + c.K)
        res = (torch.randn(c.B, c.N, generator=g) * 0.5 * math.sqrt(c.K) * 0.03).to(BF) if c.res else None
        _INPUTS[c.name] = dict(h=h, wq=wq, wscale=wscale, res=res)
    return _INPUTS[c.name]


def make_ref(h, wq, wscale, res, f32):
    """-> (int8_cases.Prepared, gemv_cases.Ref) of one linear"""
    r = ic.ref_linear(h, wq, wscale, THR, residual=res)
    A = r.S if res is None else r.S + res.double().abs()
    return ic.ref_prepare(h, wq, wscale, THR), gc.R(r.want, A, r.K_eff, None, f32, None)


def reference(c):
    if c.name not in _REFS:
        i = inputs(c)
        p, ref = make_ref(i["h"], i["wq"], i["wscale"], i["res"], c.f32)
        assert p.n == c.n, (c.name, p.n)
        _REFS[c.name] = (p, ref)
    return _REFS[c.name]


def emulate(c, mut=()):
    i = inputs(c)
    ws = EmuWorkspace(c.B, c.K)
    if "stale_meta" in mut:          # what an earlier linear of the step left behind: no outliers for a case with some, 16 for one without
        ws.meta = 16 if c.n == 0 else 0
    XQ, sx = emu_prepare(i["h"], ws, mut)
    return emu_gemv(XQ, sx, i["wq"], i["wscale"], ws, i["res"], c.f32, mut)


def verdict(c, got, p):
    """Every comparison the GPU test applies to the output `got` [B + 1, N] of case c (p = its int8_cases.Prepared) -> the list of failures."""
    i, ref = inputs(c), reference(c)[1]
    bad = []
    rep = measure(kind_of(c), got, ref, "gemv_int8", c.name)
    if not rep.ratio <= 1.0:
        bad.append(rep.where)
    if c.n == 0 and not c.res:
        if c.f32:
            if not torch.equal(ic.bits32(got[:c.B].cpu()), ic.bits32(exact_f32(p.XQ, p.sx, i["wq"], i["wscale"]))):
                bad.append(f"{c.name}: not bit-equal to f32(acc) * fl(sx * sw)")
        else:
            ok, r = ic.tight_bound_ok(got[:c.B].cpu(), ref.want)
            if not ok:
                bad.append(f"{c.name}: {r:.3g}x the (2^-8 + 2^-21) |want| bound")
    return bad


def reuse_operands():
    B, N, K = REUSE
    w = ic.make_w(400, N, K)
    wq, wscale, _ = ic.ref_quant_rows(w)
    return ic.reuse_inputs(B, K), wq, wscale


def exact_f32(XQ, sx, wq, wscale):
    """f32(acc) * fl(sx * sw): what an fp32 output without outliers and residual must equal bit for bit"""
    return (XQ.long() @ wq.long().t()).float() * (sx[:, None] * wscale[None, :])


# ------------------------------------------------------------------------------------------------------------------------- operand-map probe
PROBE_K = (128, 1152)
PROBE_N = 32


def probe_weights(K):
    """an asymmetric int8 [32, K]: no two (n, k) neighbours agree by construction of the seed, and a transposed or permuted read shows"""
    return torch.randint(-127, 128, (PROBE_N, K), generator=ic._gen(500 + K), dtype=torch.int64).to(torch.int8)


def probe_factors():
    g = ic._gen(501)
    return (0.01 + torch.rand(16, generator=g)).float(), (0.001 + 0.01 * torch.rand(PROBE_N, generator=g)).float()


# ------------------------------------------------------------------------------------------------------------------------- prepare cases
PrepCase = namedtuple("PrepCase", "name edge B K n build")


def _prep_cases():
    cs = []
    for B in (1, 3, 16):
        for K in (128, 1152, 11008):
            s = 600 + 31 * B + K % 97
            cs.append(PrepCase(f"b{B}_k{K}_thr_edges", "6.0 and -6.0 flag a column, 5.96875 does not and is the row's absmax", B, K, 2,
                               lambda s=s, B=B, K=K: ic._x_thr_edges(s, B, K)))
            cs.append(PrepCase(f"b{B}_k{K}_last_row", "the only outlier sits in the last row, column K - 1", B, K, 1,
                               lambda s=s, B=B, K=K: ic.make_x(s + 1, B, K, 1, first=1)))
            cs.append(PrepCase(f"b{B}_k{K}_cols5", "columns 0 | 1 | 31 | 32 | K - 1", B, K, 5, lambda s=s, B=B, K=K: ic.make_x(s + 2, B, K, 5)))
            cs.append(PrepCase(f"b{B}_k{K}_nK", "n = K: every column flagged, one row without a counted entry (sx = 0)", B, K, K,
                               lambda s=s, B=B, K=K: ic._x_full_row(s + 3, B, K, B // 2)))
            if B >= 10:
                cs.append(PrepCase(f"b{B}_k{K}_row_rules", "absmax inside a column flagged by another row; an all-zero row; rows of exact .5 ties", B, K, 1,
                                   lambda s=s, B=B, K=K: ic._x_row_rules(s + 4, B, K)))
    return cs


PREPARE = _prep_cases()

ProCase = namedtuple("ProCase", "name edge pro B K flagged clear build")


def _pro_rms(seed, B, K):
    """row 0: small entries and one 4.0 -> RMSNorm lifts column 5 over 6 although |x| < 6.  Row B - 1: large entries and one 7.0 in column 9 ->
    the normalised value is below 6 although |x| >= 6."""
    g = ic._gen(seed)
    x = (torch.randn(B, K, generator=g) * 0.25).to(BF)
    x[0, 5] = 4.0
    x[B - 1] = (torch.randn(K, generator=g) * 3.0).clamp(-5.5, 5.5).to(BF)
    x[B - 1, 9] = 7.0
    w = torch.ones(K, dtype=BF)
    return x, w


def _pro_swiglu(seed, B, K):
    """gate | up [B, 2K]: silu(3) * 3 = 8.57 in column 5 (inputs below 6); silu(7) * 0.25 = 1.75 in column 9 (an input above 6)"""
    g = ic._gen(seed)
    x = (torch.randn(B, 2 * K, generator=g) * 0.5).clamp(-2.0, 2.0).to(BF)
    x[0, 5], x[0, K + 5] = 3.0, 3.0
    x[B - 1, 9], x[B - 1, K + 9] = 7.0, 0.25
    return x, None


PROLOGUE = [
    ProCase("rms_b3_k1152", "pro(x) crosses 6 where x does not, and the reverse: the flag is taken on pro(x)", 1, 3, 1152, (5,), (9,), lambda: _pro_rms(700, 3, 1152)),
    ProCase("rms_b16_k11008", "the same over two chunks per thread", 1, 16, 11008, (5,), (9,), lambda: _pro_rms(701, 16, 11008)),
    ProCase("swiglu_b3_k1152", "pro(x) crosses 6 where x does not, and the reverse", 2, 3, 1152, (5,), (9,), lambda: _pro_swiglu(702, 3, 1152)),
    ProCase("swiglu_b1_k128", "one row, the minimum K", 2, 1, 128, (5,), (9,), lambda: _pro_swiglu(703, 1, 128)),
]


def prologue_ok(h_out, x, pro, norm_w):
    """h_out bf16 [B, K] lies inside the FLIP window of gemv_cases.ref_prologue element by element -> (ok, elements with two admissible values)"""
    act = gc.ref_prologue(x, pro, norm_w, gc.EPS)
    h = h_out.double().cpu()
    lo, hi = torch.minimum(act.lo, act.hi), torch.maximum(act.lo, act.hi)
    return bool(((h >= lo) & (h <= hi)).all()), int((act.lo != act.hi).sum())


def prepare_mismatches(got, ref):
    """got: dict(n, idx int32 [>= n], sx [B], XQ [B, K], xo [B, >= n]) -> names of what is not bit-equal to ref (an int8_cases.Prepared)"""
    bad = []
    n = ref.n
    if int(got["n"]) != n:
        return [f"meta[0] {int(got['n'])} != {n}"]
    if not torch.equal(got["idx"][:n].cpu().int(), ref.idx[:n]):
        bad.append("idx")
    if not torch.equal(ic.bits32(got["sx"].cpu().float()), ic.bits32(ref.sx)):
        bad.append("sx")
    if not torch.equal(got["XQ"].cpu(), ref.XQ):
        bad.append("XQ")
    if not torch.equal(ic.bits16(got["xo"].cpu()[:, :n]), ic.bits16(ref.A2[:, :n])):
        bad.append("xo")
    return bad
