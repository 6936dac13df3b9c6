"""Cases of the two live-adapter decode kernels of csrc/lora_decode.hip (lhrs_lora_down, lhrs_lora_up), shared by
tests/test_lora_decode_cases_cpu.py and tests/test_lora_decode_gpu.py: float64 references, a float32 emulation of each kernel's operation ORDER in
plain torch (no code shared with the HIP source), the comparator of tests/gemv_cases.py (`measure`: same formula, this module's constants) and
the case tables.

lora_down: tpart[i][b][j] = sum over K-slice i of pro(x)[b, k] A[j, k], fp32.  Slice i holds the 64-element chunks [i per, i per + per),
per = ceil(K / 64 / nsl), nsl = `splits(K, R)` (the host rule of lhrs_lora_down_splits restated).  The prologues are those of lhrs_gemv, so the
reference is `gemv_cases.ref_prologue` with its FLIP allowance (an activation whose float64 pre-rounding value lies within 2^-20 relative of a
bf16 boundary may come out as either neighbour: sum_marked |A[j, k]| step(x[b, k]) is added to that element's bound, nothing elsewhere).
Emulation: the staging loop of a 256-thread block (`gemv_cases.emu_prologue`), then per (row, batch row, slice) a 64-lane wave - lane l
adds the 16-B chunks l, l + 64, ... of the slice, each as one left-to-right expression of 8 products - and the xor butterfly.

lora_up: t[b][j] = bf16(s (tpart[0][b][j] + ... + tpart[nsl-1][b][j])), y[b][n] = bf16(acc[b][n] + sum_{j in cols(n)} t[b][j] Bw[n][j] + res[b][n]),
cols(n) = [(n // fout) r, +r).  The reference rounds the float64 s * sum to bf16; the kernel rounds an fp32 sum of up to 16 fp32 terms times an
fp32 s, which is within 2^-19 sum_i |tpart_i| |s| of it, so a t whose float64 value lies that close to a bf16 boundary may come out as either
neighbour: those are marked, and sum_marked |Bw[n][j]| ulp_bf16(t[b][j]) is added to the bound of y[b][n] (Ref.extra), nothing elsewhere.  The
`exact` cases build tpart from multiples of 1/8 and a power-of-two s: t is exact, nothing is marked (asserted on the CPU).
Emulation: fp32 sum in ascending slice order, times s, to bf16; lpr = the power of two >= r / 8 (at most 64) lanes share a row, lane g takes the
chunks g, g + lpr, ... of the row's block, each one expression of 8 products; butterfly below lpr; acc + dot, + res, to bf16.

Constants: c per kind = 4 x the emulation's worst ratio against float64 over the cases (EMU_WORST; the CPU test recomputes them and asserts
c >= 4 x each).  Nothing here was sized from the kernels."""
import math
import zlib
from collections import namedtuple

import torch

import gemv_cases as gc

BF, F32 = torch.bfloat16, torch.float32
EPS = 1e-5
MAX_SLICES = 16
TFLIP = 2.0 ** -19

# kind -> worst ratio at c = 1 of the EMULATION over the cases of that kind
EMU_WORST = {"down_plain": 0.1177, "down_rms": 0.0379, "down_swiglu": 0.1566, "up": 1.989}
BOUNDS = {k: 4.0 * v for k, v in EMU_WORST.items()}
WORST = {}

Report = namedtuple("Report", "ratio unit where")


def measure(kind, got, ref, live_cols=None, op="", case=""):
    """gemv_cases.measure with this module's constants and a guard column tail: got [rows >= ref rows, cols >= ref cols]; what lies past the
    reference's rows / columns are guards and must still hold NaN."""
    want = ref.want.double()
    g = got.double().cpu()
    rows, cols = want.shape
    assert g.shape[0] >= rows and g.shape[1] >= cols, (op, case, kind, tuple(g.shape), tuple(want.shape))
    guard_ok = bool(torch.isnan(g[rows:]).all()) and bool(torch.isnan(g[:, cols:]).all())
    g = g[:rows, :cols]
    unit = 2.0 ** -24 * math.sqrt(ref.n) * ref.A.double()
    if not ref.f32:
        unit = unit + 2.0 ** -9 * (want.abs() + (0.0 if ref.pre is None else ref.pre.double()))
    err = (g - want).abs()
    if ref.extra is not None:
        err = (err - ref.extra.double()).clamp_min(0.0)
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    r1 = torch.where(err == 0, torch.zeros_like(err), err / unit.clamp_min(1e-300))
    i = int(r1.reshape(-1).nan_to_num(float("inf")).argmax())
    row, col = divmod(i, cols)
    u = float(r1.reshape(-1)[i])
    where = (f"{op} [{case}] {kind}: row {row} col {col} got {float(g[row, col]):.9g} want {float(want[row, col]):.9g}, "
             f"{u / BOUNDS[kind]:.3g}x its bound ({u:.3g} at c = 1, c = {BOUNDS[kind]:.3g})")
    if not guard_ok:
        u, where = float("inf"), f"{op} [{case}] {kind}: a guard element (slice / batch row / column past the live ones) was written"
    return Report(u / BOUNDS[kind], u, where)


def check(kind, got, ref, op="", case=""):
    rep = measure(kind, got, ref, op=op, case=case)
    WORST[kind] = max(WORST.get(kind, 0.0), rep.unit)
    assert rep.ratio <= 1.0, rep.where
    return rep


# ------------------------------------------------------------------------------------------------------------------------- host rules
def splits(K, R):
    """lhrs_lora_down_splits restated: R / 8 row blocks x slices should reach 256 workgroups; whole 64-element chunks; at most 16; none empty"""
    nch, rb = K // 64, R // 8
    want = max(1, min(MAX_SLICES, nch, -(-256 // rb)))
    per = -(-nch // want)
    return -(-nch // per)


def slice_bounds(K, nsl):
    per = -(-(K // 64) // nsl) * 64
    return [(min(K, i * per), min(K, (i + 1) * per)) for i in range(nsl)]


def lanes_per_row(r):
    lpr = 1
    while lpr < r // 8 and lpr < 64:
        lpr *= 2
    return lpr


# ------------------------------------------------------------------------------------------------------------------------- cases
Down = namedtuple("Down", "B R K pro")
Up = namedtuple("Up", "name B parts fout r nsl res s dense exact zero")

DOWN_CASES = [Down(1, 8, 64, 0), Down(1, 24, 192, 1), Down(3, 40, 704, 2), Down(2, 64, 4096, 1), Down(5, 256, 4096, 0), Down(8, 384, 4096, 0),
              Down(16, 384, 4096, 1), Down(16, 128, 11008, 2), Down(1, 768, 64, 0),
              Down(16, 768, 6336, 0)]   # the last: 3 slices of 2112 activations x 16 rows = 66 KiB staged, past the default 64 KiB of dynamic LDS


def _up(B, parts, fout, r, nsl, res, s=2.0, dense=False, exact=False, zero=False):
    name = f"B={B} {parts}x{fout} r={r} nsl={nsl}{' res' if res else ''}{' dense' if dense else ''}{' exact' if exact else ''}{' t=0' if zero else ''}"
    return Up(name, B, parts, fout, r, nsl, res, s, dense, exact, zero)


UP_CASES = [_up(1, 3, 16, 8, 1, True), _up(2, 1, 40, 16, 2, False), _up(3, 2, 72, 128, 16, True, s=0.25), _up(16, 3, 16, 128, 3, True),
            _up(8, 1, 4099, 8, 2, False), _up(5, 2, 11008, 16, 16, True, s=0.015625), _up(4, 1, 48, 64, 2, True, dense=True),
            _up(3, 2, 16, 8, 2, True, zero=True),
            _up(2, 3, 16, 8, 4, True, s=2.0, exact=True), _up(3, 1, 40, 16, 3, False, s=0.5, exact=True), _up(1, 2, 72, 24, 2, True, s=4.0, exact=True)]


def down_kind(c):
    return ("down_plain", "down_rms", "down_swiglu")[c.pro]


def _gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()))


def down_inputs(c):
    g = _gen(f"down{tuple(c)}")
    x = torch.randn(c.B, 2 * c.K if c.pro == 2 else c.K, generator=g).to(BF)
    A = (torch.randn(c.R, c.K, generator=g) * 0.05).to(BF)
    norm_w = (1 + 0.1 * torch.randn(c.K, generator=g)).to(BF)
    return dict(x=x, A=A, norm_w=norm_w)


def down_reference(c, i=None):
    """-> (Ref over [nsl * B, R] rows (slice-major), nsl)"""
    i = i or down_inputs(c)
    act = gc.ref_prologue(i["x"], c.pro, i["norm_w"], EPS)
    A = i["A"].double()
    nsl = splits(c.K, c.R)
    want, mag, extra = [], [], []
    for k0, k1 in slice_bounds(c.K, nsl):
        want.append(act.a[:, k0:k1] @ A[:, k0:k1].t())
        mag.append(act.a[:, k0:k1].abs() @ A[:, k0:k1].abs().t())
        extra.append((act.hi[:, k0:k1] - act.lo[:, k0:k1]).abs() @ A[:, k0:k1].abs().t())
    n = max(k1 - k0 for k0, k1 in slice_bounds(c.K, nsl))
    return gc.R(torch.cat(want), torch.cat(mag), n, None, True, torch.cat(extra)), nsl


def _wave_sum(v, width=64):
    o = width // 2
    while o > 0:
        v = v + v[..., torch.arange(width) ^ o]
        o //= 2
    return v


def _lane_dot(w, a, lanes, mut=None):
    """w [N, L], a [B, N, L] or [B, 1, L] float32 -> [B, N]: `lanes` lanes share a row; lane l adds the 8-element chunks l, l + lanes, ... in order,
    each as one left-to-right expression of its 8 products; then the xor butterfly over the lanes.  drop_chunk: lane 0 skips its last chunk."""
    p = w[None] * a
    B, N, L = p.shape
    p = p.reshape(B, N, L // 8, 8)
    t = p[..., 0]
    for e in range(1, 8):
        t = t + p[..., e]
    nch = L // 8
    J = -(-nch // lanes)
    terms = torch.zeros(B, N, J * lanes)
    terms[:, :, :nch] = t
    terms = terms.reshape(B, N, J, lanes)
    if mut == "drop_chunk":
        terms[:, :, J - 1, 0] = 0
    acc = torch.zeros(B, N, lanes)
    for j in range(J):
        acc = acc + terms[:, :, j]
    return _wave_sum(acc, lanes)[..., 0]


def emu_down(c, i=None, mut=None):
    """-> float32 [(nsl + 1) * B + 1, R]: the live slices, then one guard slice and one guard batch row of NaN"""
    i = i or down_inputs(c)
    a = gc.emu_prologue(i["x"], c.pro, i["norm_w"], EPS, 256)
    A = i["A"].float()
    nsl = splits(c.K, c.R)
    out = torch.full(((nsl + 1) * c.B + 1, c.R), float("nan"), dtype=F32)
    for s_, (k0, k1) in enumerate(slice_bounds(c.K, nsl)):
        if mut == "drop_slice" and s_ == nsl - 1:
            out[s_ * c.B:(s_ + 1) * c.B] = 0
            continue
        out[s_ * c.B:(s_ + 1) * c.B] = _lane_dot(A[:, k0:k1], a[:, None, k0:k1], 64, mut)
    return out


def up_inputs(c):
    g = _gen("up" + c.name)
    N = c.parts * c.fout
    R = c.parts * c.r
    ldb = R + 8                                                # Bfull rows are wider than the rows in use (KP padding)
    acc = torch.randn(c.B, N, generator=g)
    if c.zero:
        tpart = torch.zeros(c.nsl, c.B, R)
    elif c.exact:
        tpart = torch.randint(-3, 4, (c.nsl, c.B, R), generator=g).float() / 8
    else:
        tpart = torch.randn(c.nsl, c.B, R, generator=g) / (abs(c.s) * math.sqrt(c.nsl))
        # batch row 0: t nearly constant (3.3 and a little noise) - against the alternating row below the products cancel to ~1 % of a term,
        # so an un-rounded t (up to 2^-9 of 3.3 per column) moves that y far outside a bound that is relative to y
        tpart[:, 0] = (3.3 + 0.01 * torch.randn(c.nsl, R, generator=g)) / (c.s * c.nsl)
    Bw = (torch.randn(N, ldb, generator=g) * 0.05).to(BF)      # off-block columns: finite non-zero garbage the reference never reads
    res = torch.randn(c.B, N, generator=g).to(BF) if c.res else None
    if not c.zero and not c.exact:
        n = min(1, N - 1)
        p = n // c.fout
        Bw[n, p * c.r:(p + 1) * c.r] = torch.tensor([1.0, -1.0] * (c.r // 2)).to(BF)
        acc[0, n] = 0.01
        if res is not None:
            res[0, n] = 0
    return dict(acc=acc, tpart=tpart, Bw=Bw, res=res, N=N, R=R)


def up_reference(c, i=None):
    i = i or up_inputs(c)
    N, R = i["N"], i["R"]
    tp = i["tpart"].double()
    s = float(torch.tensor(c.s, dtype=F32))
    tsum = s * tp.sum(0)
    tol = TFLIP * abs(s) * tp.abs().sum(0)
    t, lo, hi = gc.bf16_round(tsum), gc.bf16_round(tsum - tol), gc.bf16_round(tsum + tol)
    cols = (torch.arange(N) // c.fout)[:, None] * c.r + torch.arange(c.r)[None]      # [N, r]
    Bblk = i["Bw"].double().gather(1, cols)                                          # [N, r]
    want = i["acc"].double() + (t[:, cols] * Bblk[None]).sum(-1)
    A = i["acc"].double().abs() + (t[:, cols].abs() * Bblk[None].abs()).sum(-1)
    extra = ((hi - lo).abs()[:, cols] * Bblk[None].abs()).sum(-1)
    if c.exact or c.zero:                                       # t is exact in fp32 and in bf16: no allowance
        assert torch.equal(t, tsum) and float((tp.sum(0) - i["tpart"].sum(0).double()).abs().max()) == 0.0, c.name
        extra, lo, hi = torch.zeros_like(extra), t, t
    if i["res"] is not None:
        want, A = want + i["res"].double(), A + i["res"].double().abs()
    return gc.R(want, A, c.r, None, False, extra), int((lo != hi).sum())


def emu_up(c, i=None, mut=None):
    """-> bf16 [B + 1, N + 3]: one guard batch row and a guard column tail of NaN"""
    i = i or up_inputs(c)
    N, R, B = i["N"], i["R"], c.B
    tsum = torch.zeros(B, R)
    for s_ in range(c.nsl):
        if mut == "drop_slice" and s_ == c.nsl - 1:
            continue
        tsum = tsum + i["tpart"][s_]
    t = torch.tensor(c.s, dtype=F32) * tsum
    if mut != "t_not_rounded":
        t = t.to(BF).float()
    p = torch.arange(N) // c.fout
    if mut == "neighbour_block" and c.parts > 1:
        p = (p + 1) % c.parts
    cols = p[:, None] * c.r + torch.arange(c.r)[None]
    if mut == "neighbour_block" and c.parts == 1:
        cols = cols + 8                                          # dense: the row read one chunk further right
    Bblk = i["Bw"].float().gather(1, cols)
    tcols = (torch.arange(N) // c.fout)[:, None] * c.r + torch.arange(c.r)[None]
    v = i["acc"] + _lane_dot(Bblk, t[:, tcols], lanes_per_row(c.r), mut)
    if i["res"] is not None:
        r_ = i["res"].float().clone()
        if mut == "res_last_batch_row":
            r_[B - 1] = 0
        v = v + r_
    out = torch.full((B + 1, N + 3), float("nan"), dtype=BF)
    out[:B, :N] = v.to(BF)
    return out


# ------------------------------------------------------------------------------------------------------------------------- rejections
# (entry, argument overrides) of calls that must return -1 before any launch; the operands of the calls are complete and full-size
REJECT_BASE = dict(down=dict(B=2, R=16, K=128, pro=0, null=None), up=dict(B=2, R=24, nsl=2, r=8, fout=16, N=48, null=None))
REJECTS = [("down", dict(B=0)), ("down", dict(B=17)), ("down", dict(K=96)), ("down", dict(R=12)), ("down", dict(R=776)),
           ("down", dict(null="x")), ("down", dict(null="A")), ("down", dict(null="tpart")),
           ("up", dict(B=0)), ("up", dict(B=17)), ("up", dict(R=12)), ("up", dict(R=776)), ("up", dict(nsl=0)), ("up", dict(nsl=17)),
           ("up", dict(null="acc")), ("up", dict(null="tpart")), ("up", dict(null="Bw")), ("up", dict(null="y")), ("up", dict(fout=20))]
