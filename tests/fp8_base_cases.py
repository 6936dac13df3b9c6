"""Cases of the e4m3 base (quantize_base(8, "e4m3")) shared by tests/test_fp8_base_paths_gpu.py and tests/test_fp8_base_cases_cpu.py: the
case tables of the two quantising SwiGLU kernels of csrc/fp8.hip, the comparisons the GPU file applies to them and to every recorded call of
the base8 branches of lhrs_bot_amd/text.py, float32 emulations of those operations in plain torch (the CPU file plants errors into them),
and `paths`, the table of cells the GPU file must reach.

Nothing here carries a bound of its own.  bf16 results go through rowwise_cases.check (kinds swiglu_act / swiglu_dgu / rms_y / rms_dx /
rope) and gemm_cases.check (kinds bf16 / f32) against the float64 references of those files; e4m3 codes and scales are compared with
gemv_cases.ref_quant of the kernel's OWN bf16 output and must match exactly (quant_mismatch == (0, 0)).  ref_quant admits either
neighbouring code where the quotient lies within FLIP of a rounding boundary, so the inputs keep that share small: every non-zero row
carries a planted maximum whose bf16 significand is odd (v 448 / max then falls on an e4m3 tie only for v = +-max itself); the CPU file
holds the share of every case, forward and backward, under BORDER_CAP.

Row kinds planted into the SwiGLU cases (one per row, as many as the case has rows):
  plain       random, the maximum somewhere in the row (forward)
  zero        all zero: scale exactly 1, every code 0
  dominant    one element 1e5 x the rest: the other quotients lie below the e4m3 normals, most below half the smallest subnormal
  last_chunk  the maximum in the row's last 8 columns (backward: the last 8 of the up half, i.e. of all 2F)
  large       large g u (forward): products up to 7e4, the maximum's fp32 quotient m * (1 / (m / 448)) lands ABOVE 448 and must saturate
  max_gate / max_up   the row's |max| in the gate / the up half of d(gate|up) (backward): the scale is one per row over all 2F columns

The emulations restate the operations from their definitions (fp32 arithmetic, IEEE exp and division, bf16 stores, max -> scale -> multiply
by the fp32 reciprocal -> RNE) and share no code with the HIP sources."""
import zlib
from collections import namedtuple

import torch

import gemm_cases as gc
import gemv_cases as gv
import rowwise_cases as rc

BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
THREADS, CHUNK, FCH = 256, 8, 6                 # threads of a block, columns of a chunk, chunks a thread keeps in registers
F_MAX = FCH * THREADS * CHUNK                   # 12288
BORDER_CAP = 0.005                              # share of elements whose code ref_quant leaves open, per case

# ------------------------------------------------------------------------------------------------------------------------- SwiGLU cases
SwCase = namedtuple("SwCase", "op name rows F kinds variants")

_FWD_ROWS = {(1, 16): ("last_chunk",), (3, 2048): ("zero", "dominant", "last_chunk"), (5, 2064): ("plain", "zero", "dominant", "last_chunk", "large"),
             (3, 11008): ("plain", "last_chunk", "large"), (2, 12288): ("zero", "last_chunk")}
_BWD_ROWS = {(1, 16): ("max_up",), (3, 2048): ("zero", "max_gate", "max_up"), (5, 2064): ("zero", "dominant", "last_chunk", "max_gate", "max_up"),
             (3, 11008): ("dominant", "max_gate", "max_up"), (2, 12288): ("last_chunk", "max_gate")}
FWD_VARIANTS, BWD_VARIANTS = ("act", "null"), ("separate", "alias", "null")


def _build_swiglu():
    cs = []
    for (rows, F), kinds in _FWD_ROWS.items():
        cs.append(SwCase("swiglu_fwd_q", f"fwd_{rows}x{F}", rows, F, kinds, FWD_VARIANTS))
    for (rows, F), kinds in _BWD_ROWS.items():
        cs.append(SwCase("swiglu_bwd_q", f"bwd_{rows}x{F}", rows, F, kinds, BWD_VARIANTS))
    return cs


SWIGLU = _build_swiglu()
SWIGLU_REJECTS = (dict(rows=3, F=24), dict(rows=3, F=F_MAX + 16), dict(rows=0, F=2048))     # F % 16 != 0, F = 12304, rows = 0


def chunks_per_thread(F):
    """(fewest, most) 8-column chunks a thread of the 256 holds"""
    nch = F // CHUNK
    return nch // THREADS, -(-nch // THREADS)


def swiglu_cells(c):
    lo, hi = chunks_per_thread(c.F)
    return {(c.op, f"chunks_{lo}_{hi}")} | {(c.op, "out_" + v) for v in c.variants} | {(c.op, "row_" + k) for k in c.kinds}


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _sig64(g):
    return 1.0 / (1.0 + torch.exp(-g))


def _odd(v):
    """v: 0-dim bf16 -> its 8-bit significand is odd (the last mantissa bit is set)"""
    return bool(int(v.view(torch.int16)) & 1)


def _above_448(m):
    """the fp32 quotient of the row maximum m (a bf16 value) as the kernels form it: m * (1 / (m / 448)) > 448"""
    m = torch.tensor(float(m), dtype=F32).abs()
    return bool(m * (1.0 / (m / 448.0)) > 448.0)


def _plant(fn, v0, above=None):
    """the bf16 value v nearest above v0 (steps of 1/128 of v0) for which bf16(fn(v)) has an odd significand and sits clear of a bf16 tie
    (so fp32 and float64 round it alike); above = True / False: the fp32 quotient of that maximum lands above 448 / does not"""
    for k in range(512):
        v = torch.tensor(v0 * (1 + k / 128.0), dtype=torch.float64).to(BF)
        f = fn(v.double())
        out = f.to(BF)
        ulp = float(torch.abs(out.double())) * 2.0 ** -8
        if _odd(out) and abs(float(f - out.double())) < 0.25 * ulp and (above is None or _above_448(out) == above):
            return float(v)
    raise AssertionError("no plant found")


def _silu64(g):
    return g * _sig64(g)


def swiglu_q_inputs(c):
    """-> dict(gu bf16 [rows, 2F], dact bf16 [rows, F] (backward)), seeded by the case's name, with the case's row kinds planted"""
    g = _gen(c.name)
    rows, F = c.rows, c.F
    gu = torch.randn(rows, 2 * F, generator=g)
    dact = torch.randn(rows, F, generator=g) * 0.1
    one = lambda v: torch.tensor(v, dtype=torch.float64)
    for r, kind in enumerate(c.kinds):
        p = (5 + 37 * r) % F if kind != "last_chunk" else F - 3
        if kind == "zero":
            gu[r], dact[r] = 0.0, 0.0
            continue
        if c.op == "swiglu_fwd_q":
            if kind == "dominant":
                gu[r] *= 0.03
            if kind == "large":
                gu[r] *= 30.0
            gate = {"plain": 2.5, "last_chunk": -1.5, "dominant": 16.0, "large": 16.0}[kind]
            want = {"plain": 40.0, "last_chunk": 40.0, "dominant": 302.0, "large": 74240.0}[kind]
            gu[r, p] = gate
            gu[r, F + p] = _plant(lambda u: _silu64(one(gate)) * u, want / float(_silu64(one(gate))), above=True if kind == "large" else None)
        else:
            if kind == "dominant":
                gu[r, :F] *= 0.01
                dact[r] *= 0.1
            gate, up, want = {"max_up": (2.5, 0.125, 9.0), "last_chunk": (-2.0, 0.125, 9.0), "max_gate": (0.5, 4.0, 9.0), "dominant": (0.5, 4.0, 302.0)}[kind]
            gt, ut = one(gate), one(up)
            sg = _sig64(gt)
            f_up, f_gate = gt * sg, ut * sg * (1 + gt * (1 - sg))
            f = f_gate if kind in ("max_gate", "dominant") else f_up
            gu[r, p], gu[r, F + p] = gate, up
            dact[r, p] = _plant(lambda d: d * f, want / abs(float(f)))
    return dict(gu=gu.to(BF), dact=dact.to(BF))


def swiglu_q_ref(c, inp):
    """-> (rowwise kind, rowwise Ref) of the bf16 output of the case"""
    if c.op == "swiglu_fwd_q":
        return "swiglu_act", rc.ref_swiglu_fwd(inp["gu"], c.F)["act"]
    return "swiglu_dgu", rc.ref_swiglu_bwd(inp["dact"], inp["gu"], c.F)["dgu"]


def border_share(c, inp=None):
    """share of the elements of the case whose e4m3 code the reference leaves open (on the bf16 rounding of the float64 result)"""
    inp = inp or swiglu_q_inputs(c)
    want = swiglu_q_ref(c, inp)[1].want.to(BF)
    return gv.ref_quant(want).border / want.numel()


# ------------------------------------------------------------------------------------------------------------------------- comparisons
def check_quant(src, scale, codes, what):
    """scale / codes are the per-row e4m3 quantisation of the bf16 matrix src: scales within one fp32 ulp, every code one of the admissible
    ones, a zero row has scale exactly 1 and codes 0.  -> share of the elements whose code the reference leaves open"""
    src = src.detach().cpu()
    q = gv.ref_quant(src)
    bad = gv.quant_mismatch(scale.detach().cpu(), codes.detach().cpu(), q)
    assert bad == (0, 0), f"{what}: {bad[0]} scales and {bad[1]} codes differ from the reference quantisation of the bf16 values"
    zero = src.float().abs().amax(1) == 0
    if bool(zero.any()):                # the codes of a zero row are +-0 with the sign of the bf16 value (the comparison above pins the sign)
        assert bool((scale.detach().cpu()[zero] == 1.0).all()) and not bool((codes.detach().cpu()[zero] & 0x7F).any()), f"{what}: zero row"
    return q.border / src.numel()


def compare_swiglu_q(c, inp, out, scale, codes, what=""):
    """the comparisons of one run of a SwiGLU case that wrote its bf16 output: the output per element against float64, codes and scales
    against the reference quantisation of that output"""
    kind, ref = swiglu_q_ref(c, inp)
    rc.check(kind, out, ref, c.op, c.name + " " + what)
    assert bool(torch.isfinite(out.float()).all()), c.name
    for r, kind in enumerate(c.kinds):
        if kind == "zero":              # an all-zero input row: scale exactly 1, every code (and every bf16 bit) 0
            assert float(scale[r]) == 1.0 and not bool(codes[r].any()) and not bool(out[r].view(torch.int16).any()), f"{c.name} {what}: zero row {r}"
    return check_quant(out, scale, codes, f"{c.op} [{c.name}] {what}")


def check_fp8_gemm(out, a8, sa, b8, sb, residual=None, a2=None, b2=None, alpha=1.0, what=""):
    """gemm_fp8_nt(_lora) per element and 64x64 cell against float64 of its own operands"""
    return gc.check("bf16", out, gc.ref_fp8(a8, sa, b8, sb, alpha=alpha, residual=residual, A2=a2, B2=b2), what=what)


def ref_dropmask(U, AT, p, seed, base, alpha=1.0):
    """float64 of gemm_nt_dropmask(U, AT, p, seed, residual=base): base is the recorded bf16 operand"""
    M, N = U.shape[0], AT.shape[0]
    return gc.ref_nt(U, AT, alpha=alpha, mask=gc.drop_mask(M, N, seed, p, U.device), residual=base)


def ref_drop_branch(dy8, sdy, WT8, sWT, U, AT, p, seed):
    """float64 of the unfused `drop` branch as a whole: dx = bf16(dy8 . WT8^T) + mask (U . AT^T) / (1 - p).  Two roundings: the base product
    is stored in bf16 before the masked adapter term is added, the reference rounds there too and hands |that intermediate| over as pre."""
    base = gc.ref_fp8(dy8, sdy, WT8, sWT)
    b16 = gc.bf16_round(base.want)
    M, N = U.shape[0], AT.shape[0]
    pair = gc.ref_nt(U, AT, mask=gc.drop_mask(M, N, seed, p, U.device))
    return gc.Ref(b16 + pair.want, pair.pre + b16.abs(), base.S + pair.S, base.K_eff + pair.K_eff)


def ref_blockdiag(g, r, w, active):
    """blockdiag_mask: element (row, col) survives iff row // r == col // w and that block's bit of `active` is set"""
    rows, cols = g.shape
    pr = torch.arange(rows, device=g.device)[:, None] // r
    pc = torch.arange(cols, device=g.device)[None, :] // w
    bit = torch.bitwise_right_shift(torch.full_like(pr, int(active)), pr.clamp_max(30)) & 1
    keep = (pr == pc) & (bit == 1)
    return torch.where(keep, g, torch.zeros_like(g))


def check_weight_operand(b8, sb, L, key, what=""):
    """the weight side of a recorded e4m3 product is the stored copy L[key + "8"] with ITS scales L[key + "8s"] (key = "qkv_w" forward,
    "qkv_wT" backward, ...), bit for bit"""
    assert b8.shape == L[key + "8"].shape and torch.equal(b8, L[key + "8"]), f"{what}: the codes are not {key}8"
    assert sb.shape == L[key + "8s"].shape and torch.equal(sb, L[key + "8s"]), f"{what}: the scales are not {key}8s"


# ------------------------------------------------------------------------------------------------------------------------- emulations
def _sig32(x):
    return 1.0 / (1.0 + torch.exp(-x))


def _e4m3_grid(q, mut=None):
    """fp32 quotients -> e4m3 bytes: nearest even on the e4m3 grid (3 mantissa bits, subnormal step 2^-9), saturating at 448.  mut "no_sat":
    a conversion that does not saturate - whatever exceeds 448, by one fp32 ulp of the row maximum's own quotient already, becomes NaN (0x7F)"""
    mag = q.double().abs()
    _, e = torch.frexp(mag)
    step = torch.exp2((e - 1).clamp(-6, 8).double() - 3)
    n = mag / step
    val = (torch.floor(n) if mut == "trunc" else torch.round(n)) * step
    over = mag > 448.0
    val = torch.copysign(val.clamp_max(448.0), q.double())
    b = val.float().to(gv.E4).view(U8)
    if mut == "no_sat":
        b = torch.where(over, torch.full_like(b, 0x7F), b)
    return torch.where(torch.isnan(q), torch.full_like(b, 0x7F), b)


def emu_quant(v, m, mut=None):
    """v fp32 [rows, n], m fp32 [rows] the row maximum -> (scale fp32, e4m3 bytes)"""
    sc = torch.where(m > 0, m / 448.0, torch.full_like(m, 0.0 if mut == "zero_scale_0" else 1.0))
    return sc, _e4m3_grid(v * (1.0 / sc)[:, None], mut)


def emu_swiglu_fwd_q(gu, F, mut=None):
    g, u = gu.float()[:, :F], gu.float()[:, F:2 * F]
    p = (g * _sig32(g)) * u
    act = p.to(BF)
    m = (p if mut == "max_before_round" else act.float()).abs().amax(1)
    sc, codes = emu_quant(act.float(), m, mut)
    return dict(out=act, scale=sc, codes=codes)


def emu_swiglu_bwd_q(dact, gu, F, mut=None):
    d, g, u = dact.float(), gu.float()[:, :F], gu.float()[:, F:2 * F]
    sg = _sig32(g)
    p = torch.cat([d * u * sg * (1.0 + g * (1.0 - sg)), d * g * sg], 1)
    dgu = p.to(BF)
    src = p if mut == "max_before_round" else dgu.float()
    m = (src[:, :F] if mut == "scale_gate_only" else src).abs().amax(1)
    sc, codes = emu_quant(dgu.float(), m, mut)
    return dict(out=dgu, scale=sc, codes=codes)


def emulate_swiglu(c, inp, mut=None):
    if c.op == "swiglu_fwd_q":
        return emu_swiglu_fwd_q(inp["gu"], c.F, mut)
    return emu_swiglu_bwd_q(inp["dact"], inp["gu"], c.F, mut)


SWIGLU_MUTATIONS = ("trunc", "no_sat", "scale_gate_only", "zero_scale_0", "max_before_round")


def emu_fp8_linear(a8, sa, b8, sb, residual=None, a2=None, b2=None, alpha=1.0, mut=None):
    """alpha (sa[m] sb[n] (a8 . b8^T) + a2 . b2^T) + residual in fp32, stored in bf16"""
    acc = a8.view(gv.E4).float() @ b8.view(gv.E4).float().t()
    s_m, s_n = (sb, sa) if mut == "sa_sb_swapped" else (sa, sb)
    y = acc * s_m[:, None] * s_n[None, :]
    if a2 is not None and mut != "no_pair":
        y = y + a2.float() @ b2.float().t()
    y = alpha * y
    if residual is not None:
        y = y + residual.float() * (2.0 if mut == "residual_twice" else 1.0)
    return y.to(BF)


def emu_drop_branch(dy8, sdy, WT8, sWT, U, AT, p, seed, mut=None):
    """the unfused branch: (base bf16, dx bf16)"""
    base = emu_fp8_linear(dy8, sdy, WT8, sWT)
    mask = gc.drop_mask(U.shape[0], AT.shape[0], seed, p, U.device).float()
    pair = U.float() @ AT.float().t()
    dx = mask * (pair + base.float()) if mut == "mask_on_base" else mask * pair + base.float()
    return base, dx.to(BF)


LINEAR_MUTATIONS = ("sa_sb_swapped", "no_pair", "residual_twice")


def linear_operands(seed=7, M=256, N=256, K=256, KP=64):
    """seeded operands of one e4m3 linear with its adapter pair and residual; M == N == K so that swapped scale vectors still index and the
    transposed weight's copy (bT8, sbT) has the shape of the weight's own"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(BF)
    W = (torch.randn(N, K, generator=g) * 0.02 * (1 + torch.arange(N)[:, None] % 5)).to(BF)      # row scales that differ by row
    qx, qw, qwt = gv.ref_quant(x), gv.ref_quant(W), gv.ref_quant(W.t().contiguous())
    return dict(x=x, W=W, a8=qx.codes, sa=qx.scale, b8=qw.codes, sb=qw.scale, bT8=qwt.codes, sbT=qwt.scale,
                a2=(torch.randn(M, KP, generator=g) * 0.3).to(BF), b2=(torch.randn(N, KP, generator=g) * 0.1).to(BF),
                residual=torch.randn(M, N, generator=g).to(BF))


# ------------------------------------------------------------------------------------------------------------------------- the model
# the smallest widths every entry point of the path takes: the RMSNorm kernels need cols % 512 == 0 (one 8-column chunk per lane of a wave),
# the e4m3 GEMM K >= 256 and K % 128 == 0, attention head_dim 128
MODEL = dict(layers=1, dim=512, ff=512, heads=4, vocab=512)
M_ROWS = 80                                                      # token rows of the call-by-call tests: not a multiple of 64
SETTINGS = {                                                     # name -> enable_lora arguments (None: no adapters), train mode
    "none": None,
    "qkvo_r8": dict(r=8, alpha=16, targets=("q", "k", "v", "o"), dropout=0.0),
    "all_drop": dict(r=8, alpha=16, targets=("q", "k", "v", "o", "gate", "up", "down"), dropout=0.05),
}
RECORDED = ("quant_fp8_rows", "rmsnorm_fwd_q", "rmsnorm_bwd_q", "swiglu_fwd_q", "swiglu_bwd_q", "gemm_fp8_nt", "gemm_nt_skinny", "gemm_nt_dropmask",
            "gemm_tn_skinny", "blockdiag_mask", "dropout", "rope_")
# the calls of part 2: (cell, method, options)
LIN_CALLS = (
    ("lin_xq_given_rope", "_lin", dict(group="qkv", xq=True, rope=True, residual=False)),
    ("lin_xq_absent_residual", "_lin", dict(group="o", xq=False, rope=False, residual=True)),
    ("gu_fwd", "_gu_fwd", {}),
    ("lin_bwd_dyq_given", "_lin_bwd", dict(group="gu", dyq=True)),
    ("lin_bwd_dyq_absent", "_lin_bwd", dict(group="qkv", dyq=False)),
    ("down_bwd", "_down_bwd", {}),
)
LAYER_RUNS = ("every_row", "tail")

# ------------------------------------------------------------------------------------------------------------------------- paths
paths = set()
for _op in ("swiglu_fwd_q", "swiglu_bwd_q"):
    paths |= {(_op, "chunks_0_1"), (_op, "chunks_1_1"), (_op, "chunks_1_2"), (_op, "chunks_5_6"), (_op, "chunks_6_6"),
              (_op, "row_zero"), (_op, "row_dominant"), (_op, "row_last_chunk")}
paths |= {("swiglu_fwd_q", x) for x in ("out_act", "out_null", "row_plain", "row_large")}
paths |= {("swiglu_bwd_q", x) for x in ("out_separate", "out_alias", "out_null", "row_max_gate", "row_max_up")}
paths |= {("linear", x) for x in ("lin_xq_given_rope", "lin_xq_absent_residual", "gu_fwd", "lin_bwd_dyq_given", "lin_bwd_dyq_absent", "down_bwd")}
paths |= {("adapters", x) for x in ("none", "qkvo_r8", "all_drop")}
paths |= {("layer", x) for x in ("every_row", "tail")}


def reached():
    """the cells the case tables of this file reach"""
    out = set().union(*(swiglu_cells(c) for c in SWIGLU))
    out |= {("linear", cell) for cell, _, _ in LIN_CALLS} | {("adapters", s) for s in SETTINGS} | {("layer", r) for r in LAYER_RUNS}
    return out
