"""Cases of the 4-bit decode weight stream (csrc/gemv4.hip: gemv4_kernel, gemv4_mfma_kernel behind lhrs_gemv4), shared by
tests/test_gemv4_gpu.py and tests/test_gemv4_cases_cpu.py: the float64 reference, a float32 emulation of each kernel's operation order in
plain torch, the comparator with its own BOUNDS, the case table, the restated host rule.

Reference.  Codes and block statistics come from oracle.nf4_oracle.quantize_4bit (imported, not restated); the weight every product sees
is dequantize_4bit of them cast to bf16 - the value bitsandbytes' Linear4bit multiplies with - and y = act . W^T (+ res) in float64.  The
prologue reference and its FLIP allowance are gemv_cases.ref_prologue / ref_gemv: the prologues round where the bf16 GEMVs round, and the
4-bit path adds no numerics of its own - against float64 it has the error model of the bf16 GEMVs.

Emulations.  They restate the ORDER of the two kernels and share no code with the HIP source:
  dequantisation   level[code] * absmax[k // 64] in fp32, one rounding to bf16; byte j of a row holds element 2j in its HIGH nibble
  emu_valu4        lane l of the row's wave takes the 32-element chunks l, l + 64, ...; a chunk adds four sums of 8 products (each one
                   expression, left to right; the products of two bf16 values are exact in fp32, so an FMA changes nothing) to the lane's
                   accumulator; then the 64-lane butterfly
  emu_mfma4        K in steps of 128; MFMA m of step s sums the 32 products of k = 128 s + 32 g + 8 m + j (g < 4, j < 8) exactly and rounds
                   once into the fp32 accumulator; wave w takes the steps [w per, (w + 1) per) with per = ceil(steps / 8), clipped; the
                   eight partial tiles are folded in wave order
The staging prologue is gemv_cases.emu_prologue with the block's thread count (256 / 512).

Comparator: the form of gemv_cases.measure,
    |got - want| <= c (2^-9 (|want| + pre) + 2^-24 sqrt(n) A) + extra      (bf16 outputs; fp32 outputs without the first term)
with c per output kind = 4 x the emulation's worst ratio against float64 over CASES (EMU_WORST; tests/test_gemv4_cases_cpu.py recomputes
the ratios and asserts c >= 4x each).  Nothing here was sized from the kernels.

Weights: the plants of tests/test_nf4_gpu.py::weight fitted to the small shapes - an all-zero block (absmax 0, the package's 0 * inf),
a block dominated by one outlier, a 1e-4 row next to ordinary ones, values ON the decision thresholds."""
import math
import zlib
from collections import namedtuple

import numpy as np
import torch

import gemv_cases as gc
from oracle import nf4_oracle as N4

BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
EPS = gc.EPS
LDS_BYTES = 160 * 1024
MFMA_STATIC_LDS = (8 + 8 * 16 * 17 + 16) * 4      # red + part + the level table of gemv4_mfma_kernel
VALU_STATIC_LDS = (4 + 16) * 4

# kind -> worst ratio at c = 1 of the unmutated emulation against float64 over CASES (recomputed and asserted on the CPU)
EMU_WORST = {
    "bf16_plain": 1.93, "f32_plain": 0.1212, "bf16_rms": 1.902, "f32_rms": 0.05483, "bf16_swiglu": 1.906, "f32_swiglu": 0.0856,
}
BOUNDS = {k: 4.0 * v for k, v in EMU_WORST.items()}
WORST = {}
Report = namedtuple("Report", "ratio unit where")


def measure(kind, got, ref, op="", case=""):
    """got: [rows >= B, N]; rows past those of ref.want are guard rows and must still hold NaN.
    -> Report(ratio = worst (|err| - extra) / bound, unit = the same at c = 1, where)"""
    want = ref.want.double()
    g = got.double().cpu()
    rows = want.shape[0]
    assert g.shape[0] >= rows and g.shape[1:] == want.shape[1:], (op, case, kind, tuple(g.shape), tuple(want.shape))
    guard, g = g[rows:], g[:rows]
    unit = 2.0 ** -24 * math.sqrt(ref.n) * ref.A.double()
    if not ref.f32:
        unit = unit + 2.0 ** -9 * (want.abs() + (0.0 if ref.pre is None else ref.pre.double()))
    err = (g - want).abs()
    if ref.extra is not None:
        err = (err - ref.extra.double()).clamp_min(0.0)
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


# ------------------------------------------------------------------------------------------------------------------------- weights
def weight(N, K, seed):
    """bf16 [N, K] with the plants of tests/test_nf4_gpu.py::weight, rows taken modulo N and blocks modulo K / 64"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * 0.02
    nb = K // 64
    b0 = (1 % nb) * 64
    w[3 % N, b0:b0 + 64] = 0.0                           # an all-zero block: absmax 0, 0 * inf in the package's arithmetic
    w[5 % N, 7] = 1.5                                    # a block dominated by one outlier
    w[9 % N] *= 1e-4                                     # small statistics next to large ones
    b1 = (2 % nb) * 64
    w[11 % N, b1:b1 + 64] = torch.tensor(N4.NF4_THR.tolist() + [0.0] * 48 + [1.0])[torch.randperm(64, generator=g)] * 0.25   # ON the thresholds
    return w.to(BF)


def quantise(W, fp4, dq):
    """bf16 [N, K] -> (oracle state, codes uint8 [N, K/2], absmax fp32 [N, K/64], the bf16 weight the reference's Linear4bit multiplies with)"""
    N, K = W.shape
    st = N4.quantize_4bit(W.float().numpy(), "fp4" if fp4 else "nf4", dq)
    codes = torch.from_numpy(st["packed"].copy()).reshape(N, K // 2)
    absmax = torch.from_numpy(np.ascontiguousarray(N4.absmax_of(st))).reshape(N, K // 64)
    Wq = torch.from_numpy(N4.dequantize_4bit(st)).to(BF)
    return st, codes, absmax, Wq


# ------------------------------------------------------------------------------------------------------------------------- emulations
_LEVEL = {False: torch.tensor(N4.NF4_LEVEL), True: torch.tensor(N4.FP4_LEVEL)}


def emu_dequant(codes, absmax, fp4, mut=None):
    """codes [N, K/2] uint8, absmax [N, K/64] fp32 -> the weights [N, K] as float32 holding bf16 values"""
    N, K = codes.shape[0], codes.shape[1] * 2
    hi, lo = (codes >> 4).long(), (codes & 15).long()
    if mut == "nibbles_swapped":
        hi, lo = lo, hi
    idx = torch.stack([hi, lo], -1).reshape(N, K)
    blk = torch.arange(K) // 64
    if mut == "absmax_neighbour":
        blk = (blk + 1) % (K // 64)
    w = _LEVEL[bool(fp4)][idx] * absmax.float()[:, blk]
    if mut == "weight_not_rounded":                             # what factoring the absmax out of the block sum computes with
        return w
    return w.to(BF).float()


def _lane_steps(v):
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., torch.arange(64) ^ o]
    return v


def _stored(v, res, f32, mut, spill=None):
    """v [B, N] float32 -> the stored rows plus one guard row (NaN unless a defect writes it)"""
    B, N = v.shape
    if res is not None:
        r = res.float().clone()
        if mut == "res_last_batch_row":
            r[B - 1] = 0
        v = v + r
    out = torch.full((B + 1, N), float("nan"), dtype=F32 if f32 else BF)
    out[:B] = v if f32 else v.to(BF)
    if spill is not None:
        out[B] = spill if f32 else spill.to(BF)
    return out


def emu_valu4(a, w, res=None, f32=False, mut=None):
    """gemv4_kernel.  a [B, K] float32 activations after the prologue, w [N, K] float32 weights"""
    B, K = a.shape
    N = w.shape[0]
    p = (w[None] * a[:, None]).reshape(B, N, K // 32, 4, 8)
    t = p[..., 0]
    for i in range(1, 8):
        t = t + p[..., i]                                       # [B, N, chunks, 4]: the four 8-product expressions of a chunk
    nch = K // 32
    J = -(-nch // 64)
    terms = torch.zeros(B, N, J * 64, 4)
    terms[:, :, :nch] = t
    terms = terms.reshape(B, N, J, 64, 4)
    if mut == "drop_chunk":
        terms[:, :, J - 1, 0] = 0                               # lane 0 skips its last chunk
    acc = torch.zeros(B, N, 64)
    for j in range(J):
        for q in range(4):
            acc = acc + terms[:, :, j, :, q]
    return _stored(_lane_steps(acc)[..., 0], res, f32, mut)


def mfma4_waves(K):
    """per wave the (begin, end) of its 128-k steps"""
    ns = K // 128
    per = -(-ns // 8)
    return [(min(w * per, ns), min(min(w * per, ns) + per, ns)) for w in range(8)]


def _mfma4_sums(a, w, mut=None):
    """exact sum of every MFMA: [B, N, steps, 4] float64; MFMA m of step s holds k = 128 s + 32 g + 8 m + j"""
    B, K = a.shape
    N = w.shape[0]
    ad = a.double().reshape(B, 1, K // 128, 4, 4, 8)            # [.., s, g, m, j]
    wd = w.double().reshape(1, N, K // 128, 4, 4, 8)
    if mut == "permutation_on_weights_only":                    # the activations in natural order: MFMA m takes k = 128 s + 32 m + 8 g + j of x
        ad = ad.transpose(3, 4)
    return (ad * wd).sum((3, 5))


def _fold(S, waves):
    v = torch.zeros(S.shape[:2])
    for b, e in waves:
        acc = torch.zeros(S.shape[:2])
        for s in range(b, e):
            for m in range(4):
                acc = (acc.double() + S[:, :, s, m]).float()
        v = v + acc
    return v


def emu_mfma4(a, w, res=None, f32=False, mut=None):
    """gemv4_mfma_kernel"""
    B, K = a.shape
    waves = mfma4_waves(K)
    if mut == "drop_chunk":
        waves[0] = (waves[0][0], waves[0][1] - 1)               # wave 0 loses its last step
    spill = _fold(_mfma4_sums(a[B - 1:], w, mut), waves)[0] if mut == "batch_column_B_live" else None
    return _stored(_fold(_mfma4_sums(a, w, mut), waves), res, f32, mut, spill)


# ------------------------------------------------------------------------------------------------------------------------- host rule
class Rejected(ValueError):
    pass


def plan(B, N, K, pro, absmax=True, ldc=None):
    """lhrs_gemv4's host rule -> [(kernel, batch rows)], one entry per launch; Rejected where the entry point refuses"""
    if not (1 <= B <= 16 and N > 0 and K >= 64 and K % 64 == 0):
        raise Rejected("B / N / K")
    if B > 8 and K % 128 != 0:
        raise Rejected("batches above 8 need K % 128 == 0")
    if not absmax:
        raise Rejected("null absmax")
    if ldc is not None and (ldc % 16 or ldc < K // 2):
        raise Rejected("code row stride")
    mfma = B >= 2 and K % 128 == 0
    bmax = min(152 * 1024, LDS_BYTES - (MFMA_STATIC_LDS if mfma else VALU_STATIC_LDS)) // (2 * K)
    if mfma and pro == 0:
        bmax = 16
    if bmax < 1:
        raise Rejected("one activation vector does not fit LDS")
    out = []
    for b0 in range(0, B, bmax):
        nb = min(bmax, B - b0)
        if nb >= 2 and K % 128 == 0:
            assert (0 if pro == 0 else nb * K * 2) + MFMA_STATIC_LDS <= LDS_BYTES
            out.append(("mfma", nb))
        else:
            assert nb <= 8 and nb * K * 2 + VALU_STATIC_LDS <= LDS_BYTES
            out.append(("valu", nb))
    return out


# ------------------------------------------------------------------------------------------------------------------------- cases
Case = namedtuple("Case", "name opt")


def _case(B, N, K, pro, f32, res, fp4=False, dq=True, strided=False):
    o = dict(B=B, N=N, K=K, pro=pro, f32=f32, res=res, fp4=fp4, dq=dq, strided=strided)
    name = (f"{'fp4' if fp4 else 'nf4'}{'' if dq else ' plain_absmax'} B={B} N={N} K={K} pro={pro} {'f32' if f32 else 'bf16'}"
            f"{' res' if res else ''}{' strided' if strided else ''}")
    return Case(name, o)


def _build_cases():
    T, F = True, False
    cs = []
    # VALU kernel, batch 1: one block (two chunks), below one lane trip (4, 6, 22, 36 chunks), exactly two trips (K 4096), five full trips and
    # a partial one (K 11008: 344 chunks); N ragged against 8 and 16 rows per block; N > 4096 takes the four-rows-per-wave instance
    cs += [_case(1, 3, 64, 0, F, T), _case(1, 16, 128, 1, T, F, fp4=T), _case(1, 35, 192, 2, F, T, strided=T), _case(1, 67, 704, 0, T, T, dq=F),
           _case(1, 35, 1152, 1, F, F, fp4=T, strided=T), _case(1, 16, 4096, 2, T, T), _case(1, 35, 11008, 0, F, F, fp4=T, dq=F),
           _case(1, 67, 4096, 1, F, T, dq=F, strided=T), _case(1, 4099, 64, 0, T, F)]
    # VALU kernel, batches 2..8, where the MFMA kernel cannot go (K % 128 != 0)
    for B in range(2, 9):
        cs.append(_case(B, (3, 35, 67)[B % 3], (64, 192, 704)[B % 3], B % 3, B % 2 == 0, B % 4 < 2, fp4=B % 2 == 1, dq=B % 3 != 0, strided=B % 2 == 1))
    # MFMA kernel: 1 step (wave 0 alone), 9 steps (2 2 2 2 1 and three idle waves), 32 steps (4 per wave: two full trips of 2); every
    # prologue at every K; dead batch columns and B = 16; ragged and full row blocks
    for i, (B, N, K) in enumerate(((2, 16, 128), (3, 35, 128), (16, 3, 128), (8, 67, 1152), (15, 35, 1152), (16, 16, 1152),
                                   (2, 35, 4096), (16, 3, 4096), (3, 16, 4096))):
        cs.append(_case(B, N, K, i % 3, i % 2 == 0, i % 3 != 1, fp4=i % 4 == 1, dq=i % 5 != 2, strided=i % 2 == 1))
    # every prologue at the K where it was missing above, on the other output type
    cs += [_case(8, 35, 128, 1, F, T, strided=T), _case(2, 16, 1152, 2, T, F, fp4=T), _case(3, 35, 4096, 1, T, T, dq=F)]
    # the LDS chunking at B = 8: 7 staged rows of K 11008 on the MFMA kernel (11 steps per wave, 9 for the last) + 1 on the VALU kernel
    cs.append(_case(8, 35, 11008, 1, F, T))
    return cs


CASES = _build_cases()

# name -> the arguments of a call lhrs_gemv4 must refuse (complete operands of full size: were it accepted it would run inside its buffers)
REJECTS = {
    "B17": dict(B=17, N=16, K=128), "B9_K192": dict(B=9, N=16, K=192), "K96": dict(B=1, N=16, K=96),
    "null_absmax": dict(B=1, N=16, K=128, absmax=False), "ldc_not_16": dict(B=1, N=16, K=128, ldc=72),
}


def kind_of(c):
    return ("f32" if c.opt["f32"] else "bf16") + ("_plain", "_rms", "_swiglu")[c.opt["pro"]]


def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(("gemv4" + c.name).encode()))


_INPUTS = {}


def inputs(c):
    """seeded CPU tensors of a case (computed once, shared, never modified): x, W (the planted bf16 weight), codes, absmax, Wq (the
    dequantised bf16 weight of the reference), norm_w, res, st (the oracle's state)"""
    if c.name not in _INPUTS:
        g, o = _gen(c), c.opt
        B, N, K, pro = o["B"], o["N"], o["K"], o["pro"]
        x = torch.randn(B, 2 * K if pro == 2 else K, generator=g).to(BF)
        W = weight(N, K, seed=N + K)
        norm_w = (1 + 0.1 * torch.randn(K, generator=g)).to(BF)
        res = torch.randn(B, N, generator=g).to(BF) if o["res"] else None
        st, codes, absmax, Wq = quantise(W, o["fp4"], o["dq"])
        _INPUTS[c.name] = dict(x=x, W=W, codes=codes, absmax=absmax, Wq=Wq, norm_w=norm_w, res=res, st=st)
    return _INPUTS[c.name]


_REFS = {}


def reference(c):
    """-> (Ref, Act): float64, on the oracle's dequantised bf16 weight"""
    if c.name not in _REFS:
        i, o = inputs(c), c.opt
        act = gc.ref_prologue(i["x"], o["pro"], i["norm_w"], EPS)
        _REFS[c.name] = (gc.ref_gemv(act, i["Wq"], None, i["res"], o["f32"]), act)
    return _REFS[c.name]


def emulate(c, mut=None):
    """-> got [B + 1, N]: the launches of the host rule, one after the other"""
    i, o = inputs(c), c.opt
    B, N = o["B"], o["N"]
    w = emu_dequant(i["codes"], i["absmax"], o["fp4"], mut)
    got = torch.full((B + 1, N), float("nan"), dtype=F32 if o["f32"] else BF)
    launches = plan(B, N, o["K"], o["pro"])
    b0 = 0
    for n, (kern, nb) in enumerate(launches):
        x, res = i["x"][b0:b0 + nb], None if i["res"] is None else i["res"][b0:b0 + nb]
        m = mut if n == len(launches) - 1 or mut == "drop_chunk" else None      # batch-row defects belong to the launch that holds the last row
        a = gc.emu_prologue(x, o["pro"], i["norm_w"], EPS, 256 if kern == "valu" else 512)
        got[b0:b0 + nb + 1] = (emu_valu4 if kern == "valu" else emu_mfma4)(a, w, res, o["f32"], m)
        b0 += nb
    return got
