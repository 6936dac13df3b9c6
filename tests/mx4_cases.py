"""OCP MXFP4 decode weights (csrc/gemv_mx4.hip), restated for tests/test_mx4_cases_cpu.py and tests/test_mx4_gpu.py.  Shares no code with
the HIP source.

Format.  A bf16 weight W [N, K], K % 32 == 0, becomes `codes` uint8 [N, K/2] (element k in byte k/2, even k in the low nibble; a code is
s m m m: the sign, then an index into LEVELS, the e2m1 values) and `scales` uint8 [N, K/32], e8m0: a block of 32 consecutive k shares
2^(byte - 127).  Quantisation (OCP MX v1.0): m = max|v| of the block; m == 0 gives byte 127 and +0 codes; else byte = clamp(floor(log2 m) - 2
+ 127, 0, 254) and every element is v / 2^(byte - 127) rounded to the nearest level, ties to the even code, saturating at 6, sign kept.
All of it is exact in float64 (a bf16 value over a power of two), so codes and scales are compared byte for byte.

Tiled form (the only one the GEMV reads).  codes_t [ceil(N/16)][K/128][64][16]: lane (r, g) of step s holds the 16 code bytes of block
4 s + g of row 16 rg + r.  scales_t [ceil(N/16)][ceil(K/512)][64][4]: byte j of the dword t of lane (r, g) is the scale of block
4 (4 t + j) + g of that row.  Rows past N: zero codes, byte 127; steps past K/128: byte 127.  The eight waves of a workgroup take runs of
`per` = ceil(ceil(steps / 8) / 4) * 4 consecutive steps, so every run starts on a multiple of 4 (the scale byte is an immediate).

Bound of a GEMV output, derived, never measured on the kernel.  With p_k = x8[b][k] w[n][k] in float64 and G the groups of 8 consecutive k:

    |got - want| <= c ( xscale[b] ( 2^-13 sum_G 8 max_{k in G} |p_k|  +  2^-23 (K/128 + 8) sum_k |p_k| )  [+ 2^-9 |want|, bf16 output] )  + extra

  - first term: v_mfma_scale_f32_16x16x128_f8f6f4 truncates every product onto 2^-13 of the largest exponent of its group of 8 (what
    tests/gemv_cases.py documents for e4m3 x e4m3), so each of the 8 products loses less than 2^-13 of the group's largest product;
  - second term: one fp32 rounding (2^-24 relative, doubled for slack) per accumulate (K/128 steps at most) and per fold (8 waves);
  - bf16 output: round-to-nearest of a bf16 store is off by at most half a unit in the last place, 2^-9 .. 2^-8 of the value depending on
    where in its binade the value lies; with c = 2 the term is 2^-8 |want|, that worst case;
  - c = 2: the exponent the hardware reads off the e2m1 subnormal 0.5 (0, as an e4m3 subnormal reads -6, or -1) moves a group's grid by
    at most one binade;
  - extra: the fused prologue's allowance - an activation whose float64 pre-rounding value lies within FLIP = 2^-20 of a rounding boundary
    may come out as either neighbour: sum over such k of |w[n][k]| times the distance of the two, and nothing elsewhere.
`ratio` below is the error less extra over the bracket at c = 1: at most 2 passes.  The float32 emulation below reaches 0.014 (x8) / 0.018
(fused) on fp32 outputs and 1.656 / 1.443 on bf16 outputs, where the store's half unit in the last place alone can reach 2; an MI355X gives
the same four figures (tests/test_mx4_gpu.py prints them; DESIGN.md "Decode from MXFP4 weights")."""
from collections import namedtuple

import torch

BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
E4 = torch.float8_e4m3fn
FLIP = 2.0 ** -20
EPS = 1e-5
C = 2.0
LEVELS = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)
WAVES = 8


# ------------------------------------------------------------------------------------------------------------------------- format
def quant(W):
    """bf16 [N, K] -> (codes uint8 [N, K/2], scales uint8 [N, K/32])"""
    N, K = W.shape
    v = W.double().reshape(N, K // 32, 32)
    m = v.abs().amax(-1)
    _, ex = torch.frexp(m)                                      # m = f 2^ex, f in [0.5, 1): floor(log2 m) = ex - 1
    byte = torch.where(m > 0, (ex - 1 - 2 + 127).clamp(0, 254), torch.full_like(ex, 127))
    q = (v.abs() / torch.exp2((byte - 127).double())[..., None])
    # nearest level; at a midpoint the even index.  Midpoints .25 .75 1.25 1.75 2.5 3.5 5: the even neighbour is below at .25, 1.25, 2.5, 5
    idx = torch.zeros(q.shape, dtype=torch.int64)
    for mid, up_on_tie in ((0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False), (3.5, True), (5.0, False)):
        idx += (q >= mid) if up_on_tie else (q > mid)
    sign = torch.signbit(v).long() * (m > 0)[..., None].long()  # a zero block is all +0
    c = (sign * 8 + idx).reshape(N, K // 2, 2)
    return (c[..., 0] + 16 * c[..., 1]).to(U8), byte.to(U8)


def unpack(codes):
    """uint8 [N, K/2] -> int64 [N, K] of 4-bit codes"""
    c = codes.long()
    return torch.stack((c & 15, c >> 4), -1).reshape(codes.shape[0], -1)


def dequant(codes, scales):
    """-> float64 [N, K] = level * 2^(byte - 127) (signed zeros kept)"""
    c = unpack(codes)
    mag = LEVELS[c & 7]
    val = torch.where((c & 8) != 0, -mag, mag)
    return val * torch.exp2(scales.double() - 127).repeat_interleave(32, 1)


def levels_of(codes):
    c = unpack(codes)
    return torch.where((c & 8) != 0, -LEVELS[c & 7], LEVELS[c & 7])


# ------------------------------------------------------------------------------------------------------------------------- tiled maps
def groups_of(N):
    return -(-N // 16)


def code_byte_index(n, kb, K):
    """row n, code byte kb (0 .. K/2) -> flat offset in codes_t"""
    blk, j = kb // 16, kb % 16
    step, g = blk // 4, blk % 4
    lane = (n % 16) + 16 * g
    return (((n // 16) * (K // 128) + step) * 64 + lane) * 16 + j


def scale_byte_index(n, blk, K):
    """row n, block blk (0 .. K/32) -> flat offset in scales_t"""
    step, g = blk // 4, blk % 4
    nd = -(-(K // 128) // 4)
    lane = (n % 16) + 16 * g
    return (((n // 16) * nd + step // 4) * 64 + lane) * 4 + step % 4


def tile(codes, scales, N, K):
    """-> (codes_t uint8 [G, K/128, 64, 16], scales_t uint8 [G, ceil(K/512), 64, 4]) through the two index functions"""
    G, S = groups_of(N), K // 128
    nd = -(-S // 4)
    ct = torch.zeros(G * S * 1024, dtype=U8)
    st = torch.full((G * nd * 256,), 127, dtype=U8)
    n = torch.arange(N)[:, None]
    ct[code_byte_index(n, torch.arange(K // 2)[None], K).reshape(-1)] = codes[:N, :K // 2].reshape(-1)
    st[scale_byte_index(n, torch.arange(K // 32)[None], K).reshape(-1)] = scales[:N, :K // 32].reshape(-1)
    return ct.reshape(G, S, 64, 16), st.reshape(G, nd, 64, 4)


def wave_steps(K):
    """per wave the (begin, end) of its 128-k steps"""
    ns = K // 128
    per = -(-(-(-ns // WAVES)) // 4) * 4
    return [(min(w * per, ns), min(ns, min(w * per, ns) + per)) for w in range(WAVES)]


# ------------------------------------------------------------------------------------------------------------------------- e4m3 activations
def bf16_round(x):
    return x.to(BF).double()


def e4m3_rne(q):
    """float64 -> nearest OCP e4m3 value, ties to even, saturating at 448 (subnormal step 2^-9)"""
    mag = q.abs()
    _, e = torch.frexp(mag)
    step = torch.exp2((e - 1).clamp(-6, 8).double() - 3)
    return torch.copysign((torch.round(mag / step) * step).clamp_max(448.0), q)


def e4m3_bytes(val):
    return val.float().to(E4).view(U8)


def e4m3_values(b):
    return b.view(E4).float().double()


def quant_rows_e4m3(rows):
    """bf16 [B, K] -> (e4m3 bytes, fp32 scale): scale = max|row| / 448 in fp32 (1 for a zero row), RNE of the float64 quotient"""
    m = rows.float().abs().amax(1)
    scale = torch.where(m > 0, m / 448.0, torch.ones_like(m))
    return e4m3_bytes(e4m3_rne(rows.double() / scale.double()[:, None])), scale


Act = namedtuple("Act", "a lo hi")


def prologue(x, pro, norm_w=None, eps=EPS):
    """x bf16 [B, K] (SwiGLU: [B, 2K]) -> Act of float64 [B, K]: the bf16 value the product sees and the two ends of its FLIP window"""
    x = x.double()
    if pro == 0:
        return Act(x, x, x)
    if pro == 1:
        w = norm_w.double()
        xh = x * ((x * x).mean(1, keepdim=True) + float(torch.tensor(eps, dtype=F32))).rsqrt()
        f = lambda t: bf16_round(w * bf16_round(t))
    else:
        K = x.shape[1] // 2
        g, u = x[:, :K], x[:, K:]
        xh = g * torch.sigmoid(g) * u
        f = bf16_round
    return Act(f(xh), f(xh * (1 - FLIP)), f(xh * (1 + FLIP)))


def fused_activations(x, pro, norm_w, eps=EPS):
    """the fused kernel's operand: prologue, then the per-row e4m3 quantisation -> (Act of e4m3 VALUES, fp32-valued scale [B] as float64)"""
    act = prologue(x, pro, norm_w, eps)
    m = act.lo.abs().amax(1)
    assert torch.equal(m, act.hi.abs().amax(1)), "the row maximum sits on a rounding boundary of the prologue: the in-kernel scale is ambiguous"
    sc = torch.where(m > 0, (m.float() / 448.0).double(), torch.ones_like(m))[:, None]
    return Act(e4m3_rne(act.a / sc), e4m3_rne(act.lo / sc * (1 - FLIP)), e4m3_rne(act.hi / sc * (1 + FLIP))), sc[:, 0]


# ------------------------------------------------------------------------------------------------------------------------- reference and bound
Ref = namedtuple("Ref", "want unit extra f32")


def reference(act8, xscale, Wd, res=None, f32=False):
    """act8: Act of e4m3 values [B, K] (a == lo == hi for the x8 entry point), xscale float64 [B], Wd float64 [N, K] dequantised weight.
    unit = the bracket of the module docstring at c = 1."""
    B, K = act8.a.shape
    xs = xscale.double()[:, None]
    want = (act8.a @ Wd.t()) * xs
    absW = Wd.abs()
    gmax = torch.zeros(B, Wd.shape[0], dtype=torch.float64)
    for b in range(B):                                          # [N, K/8, 8] at a time: the [B, N, K] product would be 58 MB at K 11008
        gmax[b] = (absW * act8.a[b].abs()[None]).reshape(-1, K // 8, 8).amax(-1).sum(-1)
    A = act8.a.abs() @ absW.t()
    unit = xs * (2.0 ** -13 * 8 * gmax + 2.0 ** -23 * (K // 128 + 8) * A)
    extra = ((act8.hi - act8.lo).abs() @ absW.t()) * xs
    if res is not None:
        want = want + res.double()
    if not f32:
        unit = unit + 2.0 ** -9 * want.abs()
    return Ref(want, unit, extra, f32)


WORST = {}


def ratio(got, ref, what=None):
    """-> the largest (|got - want| - extra) / unit; recorded per `what` for the report"""
    g = got.detach().double().cpu()
    assert g.shape == ref.want.shape, (g.shape, ref.want.shape)
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite output"
    err = ((g - ref.want).abs() - ref.extra).clamp_min(0)
    r = torch.where(err > 0, err / ref.unit.clamp_min(1e-300), torch.zeros_like(err))
    w = float(r.max())
    if what is not None:
        WORST[what] = max(WORST.get(what, 0.0), w)
    return w


def check(got, ref, what, name):
    w = ratio(got, ref, what)
    assert w <= C, f"{name}: |got - want| is {w:.3f} x the bound at c = 1 (allowed: c = {C})"
    return w


# ------------------------------------------------------------------------------------------------------------------------- float32 emulation
def _exp_e4m3(v):
    """floor(log2 |v|), -6 for a subnormal; zero takes part in no maximum"""
    _, e = torch.frexp(v.abs())
    return torch.where(v == 0, torch.full_like(v, -1e6), (e - 1).clamp_min(-6).to(v.dtype))


def _exp_e2m1(level):
    """the exponent field of an e2m1 code less its bias 1; the subnormal 0.5 reads 0 like 1.0 (the assumption c = 2 covers)"""
    _, e = torch.frexp(level.abs())
    return torch.where(level == 0, torch.full_like(level, -1e6), (e - 1).clamp_min(0).to(level.dtype))


def _onto(v, e, bits, rnd):
    g = torch.exp2((e - bits).clamp_min(-400.0))
    return rnd(v / g) * g


def emulate(a8, xscale, codes, scales, res=None, f32=False):
    """the model of tests/gemv_cases.py for the block-scaled MFMA, with a product's exponent e(x8) + e(code) + (byte - 127): products of a
    group of 8 truncated onto 2^(E - 13), group sums of a pair rounded down onto 2^(E2 - 24), one fp32 rounding per step; the steps of a
    wave in order, the waves folded in order, times xscale, plus the residual, one store.  -> [B, N] fp32 or bf16"""
    B, K = a8.shape
    N = codes.shape[0]
    lv = levels_of(codes)
    sh = (scales.double() - 127).repeat_interleave(32, 1)
    Wd = lv * torch.exp2(sh)
    ew = _exp_e2m1(lv) + sh
    ea = _exp_e4m3(a8)
    out = torch.zeros(B, N, dtype=F32)
    for b in range(B):
        p = (Wd * a8[b][None]).reshape(N, K // 8, 8)
        e = (ew + ea[b][None]).reshape(N, K // 8, 8).amax(-1)
        g = _onto(p, e[..., None], 13, torch.trunc).sum(-1)
        e2 = e.reshape(N, K // 16, 2).amax(-1, keepdim=True).expand(N, K // 16, 2).reshape(N, K // 8)
        S = _onto(g, e2, 24, torch.floor).reshape(N, K // 128, 16).sum(-1)
        v = torch.zeros(N, dtype=F32)
        for s0, s1 in wave_steps(K):
            acc = torch.zeros(N, dtype=F32)
            for s in range(s0, s1):
                acc = (acc.double() + S[:, s]).float()
            v = v + acc
        out[b] = v * xscale[b].float()
    if res is not None:
        out = out + res.float()
    return out if f32 else out.to(BF)


# ------------------------------------------------------------------------------------------------------------------------- cases
Case = namedtuple("Case", "name op B N K pro f32 res seed")
KS = (128, 512, 640, 1152, 4096)
NS = (16, 24, 40)
OUT = ((False, False), (True, True), (False, True), (True, False))   # (f32, residual)


def _build():
    """every (B, K) of the x8 entry point and every (B, prologue, K) of the fused one; N and the (output, residual) pair rotate with the
    row AND the column of that table, so that each entry point meets every N and every pair at every K; plus one K = 11008 case each"""
    cases = []

    def add(op, B, pro, j, ki, K):
        f32, res = OUT[(j + ki) % 4]
        N = NS[(j + ki) % 3]
        head = f"x8 B{B}" if op == "x8" else f"fused B{B} pro{pro}"
        cases.append(Case(f"{head} N{N} K{K} {'f32' if f32 else 'bf16'}{' res' if res else ''}", op, B, N, K, pro, f32, res, 100 + len(cases)))

    for j, B in enumerate((1, 3, 5, 16)):
        for ki, K in enumerate(KS):
            add("x8", B, -1, j, ki, K)
    cases.append(Case("x8 B5 N24 K11008 bf16 res", "x8", 5, 24, 11008, -1, False, True, 100 + len(cases)))
    for j, (B, pro) in enumerate((b, p) for b in (1, 2) for p in (0, 1, 2)):
        for ki, K in enumerate(KS):
            add("fused", B, pro, j, ki, K)
    cases.append(Case("fused B2 pro2 N40 K11008 f32 res", "fused", 2, 40, 11008, 2, True, True, 100 + len(cases)))
    return cases


CASES = _build()


def weight(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.02 * torch.randn(N, K, generator=g)).to(BF)


_INPUTS = {}


MARKED_MAX = 0.005


def marked_fraction(act):
    """the worst row's fraction of activations with two admissible e4m3 values"""
    return float((act.lo != act.hi).double().mean(1).max())


def inputs(c):
    """-> dict: W (bf16), codes, scales (restated quantiser), x (bf16 activations; the x8 op also x8 / xscale), norm_w, res.  Made once.
    A row whose maximum is 7 * 2^j has a power-of-two e4m3 scale, and then one bf16 activation in 16 sits EXACTLY on an e4m3 rounding
    boundary and would be excused by `extra`: the fused cases take the first seed whose rows mark fewer than MARKED_MAX of their elements."""
    if c.name not in _INPUTS:
        for t in range(8):
            g = torch.Generator().manual_seed(c.seed + 1000 * t)
            x = torch.randn(c.B, c.K * (2 if c.pro == 2 else 1), generator=g).to(BF)
            norm_w = (1.0 + 0.1 * torch.randn(c.K, generator=g)).to(BF)
            res = torch.randn(c.B, c.N, generator=g).to(BF) if c.res else None
            if c.op == "x8" or marked_fraction(fused_activations(x, c.pro, norm_w)[0]) < MARKED_MAX:
                break
        else:
            raise AssertionError(f"{c.name}: no seed with fewer than {MARKED_MAX} marked activations")
        W = weight(c.N, c.K, c.seed + 1000)
        codes, scales = quant(W)
        d = dict(W=W, codes=codes, scales=scales, x=x, norm_w=norm_w, res=res)
        if c.op == "x8":
            d["x8"], d["xscale"] = quant_rows_e4m3(x)
        _INPUTS[c.name] = d
    return _INPUTS[c.name]


_REFS = {}


def case_reference(c):
    """-> (Ref, Act of e4m3 values, xscale float64 [B]); computed once per case and shared"""
    if c.name not in _REFS:
        i = inputs(c)
        Wd = dequant(i["codes"], i["scales"])
        if c.op == "x8":
            a = e4m3_values(i["x8"])
            act, xs = Act(a, a, a), i["xscale"].double()
        else:
            act, xs = fused_activations(i["x"], c.pro, i["norm_w"])
        _REFS[c.name] = (reference(act, xs, Wd, i["res"], c.f32), act, xs)
    return _REFS[c.name]


# ------------------------------------------------------------------------------------------------------------------------- planted blocks
def planted():
    """bf16 [8, 128]: per row, block 0 planted, the other three blocks 0.02 randn.  Rows: 0 a zero block (with a -0.0 in it); 1 one outlier 2^10
    above the rest; 2 values near 2^-120; 3 exact ties; 4 the saturating range (6, 8) 2^e; 5 a negative value that rounds to zero;
    6 a bf16 subnormal block (the clamp at byte 0); 7 the largest finite bf16 (byte 252)"""
    g = torch.Generator().manual_seed(77)
    W = (0.02 * torch.randn(8, 128, generator=g)).to(BF)
    blk = lambda *v: torch.tensor(list(v) + [0.0] * (32 - len(v)), dtype=torch.float64)
    W[0, :32] = 0
    W[0, 3] = -0.0
    W[1, :32] = (0.01 * torch.randn(32, generator=g)).to(BF)
    W[1, 7] = 2.0 ** 4                                          # ~2^10 above 0.01
    W[2, :32] = (2.0 ** -120 * torch.randn(32, generator=g).double()).to(BF)
    # ties: the maximum 4 fixes e = 0 (byte 127); midpoints of neighbouring levels, both signs
    W[3, :32] = blk(4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, 0.125, 0.375).to(BF)
    # saturation: maximum 7.5 * 2^-3 -> e = -3, 7.5 clips to 6; 5 * 2^-3 is the tie 4 | 6 -> 4; 5.5 -> 6
    W[4, :32] = (blk(7.5, -7.0, 6.5, 5.0, -5.0, 5.5, 6.0, 4.5) * 2.0 ** -3).to(BF)
    W[5, :32] = blk(4.0, -0.125, -0.25, -2.0 ** -30, 0.2).to(BF)
    W[6, :32] = (blk(3.0, -2.0, 1.0, 5.0, 127.0) * 2.0 ** -133).to(BF)
    W[7, :32] = blk(float(torch.finfo(BF).max), -float(torch.finfo(BF).max), 2.0 ** 125, 2.0 ** 120).to(BF)
    return W
