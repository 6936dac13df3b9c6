"""The 8-bit KV cache "kv8" (csrc/decode_attn.hip behind hk.kv8_quant_rows / hk.decode_attn_kv8, generate(kv_cache="fp8")), restated for
tests/test_kv8_cases_cpu.py and tests/test_kv8_gpu.py.  Shares no code with the HIP source.

Format.  One cache position of one head is 128 values (keys after RoPE, already rounded to bf16).  It becomes 128 OCP e4m3fn codes and one
e8m0 scale byte.  With m = max|v|: m == 0 gives byte 127 and +0 codes; else e = floor(log2 m) - 8, raised by one if m > 448 * 2^e (the
smallest power of two with every |v| / 2^e <= 448), byte = clamp(e + 127, 0, 254), code = e4m3 round-to-nearest-even of v / 2^e.  Nothing
saturates, no code has all seven low bits set (NaN), and v / 2^e is exact in float64 (a bf16 value over a power of two): codes and bytes are
compared byte for byte.  Caches: codes uint8 [rows * max_ctx, H * 128], scales uint8 [rows * max_ctx, H], position-major.

Attention, from the cache bytes alone: with K_j = deq(codes, byte) of key j, the visible keys j <= pos that the key mask does not hide,
s_j = scale * q . K_j, M = max_j s_j, w_j = exp(s_j - M):   want = sum_j w_j deq(V_j) / sum_j w_j.   q is the rotated new query rounded to
bf16, `scale` the fp32 value the kernel is given, and key pos is the row the kernel itself appends (dequantised - not the unquantised row).

Bound of an output element, derived, never measured on the kernel:

    |got - want| <= 2^-8 |want| + 2.5 * delta * A,      A = sum_j w_j |v_j| / sum_j w_j  (per element),
    delta = 2 E_s + 2^-24 max_j |s_j - M| + (n_keys + 16) 2^-23,      E_s = 130 * 2^-24 * scale * max_j sum_i |q_i k_ji|

  - 2^-8 |want|: the bf16 store, half a unit in the last place at the bottom of a binade;
  - E_s: a score is a 128-term fp32 dot.  q_i * scale is rounded once, each product once (or not at all under an fma), each of the 127
    additions once, whatever their order; the multiply by 2^(byte - 127) is exact: at most 130 roundings of 2^-24 relative to the sum of the
    magnitudes.  A weight w_j = exp(s_j - M) sees the error of s_j and that of M: 2 E_s in the exponent, which is its relative error;
  - 2^-24 max |s_j - M|: __expf scales its argument by log2(e) in fp32, one rounding relative to the argument;
  - (n_keys + 16) 2^-23: one fp32 rounding (2^-24, doubled for slack, which also covers the 1-ulp hardware exp2) per accumulate - a lane
    group adds at most n_keys / 8 terms, then 3 folds across groups, 4 waves, up to 3 workgroup partials with one rescale each - and the
    final division;
  - 2.5: numerator and denominator each carry delta (2 to first order); the rest covers the second order and the rounding of an already
    perturbed value at the store.
`ratio` = error / bound; at most 1 passes.  The float32 emulation below (the kernel's order of operations) reaches 0.90, set by the
bf16 store alone (at the bottom of a binade half a unit in the last place IS the first term); tests/test_kv8_gpu.py prints the device's figures (DESIGN.md "Decode from an e4m3 KV cache").

Rotation.  The kernels take cos_t / sin_t as arguments.  The byte-exact cases pass tables whose per-frequency (cos, sin) pairs are drawn from
(1, 0), (0, 1), (-1, 0), (0, -1): RoPE is then an exact signed permutation and the bf16 rounding of the rotated rows has one answer.  One
case uses the model's tables (bf16-rounded cos / sin of pos * 10000^(-2i/128)): q is the float64 rotation rounded to bf16 - the case takes
the first seed for which no q element lies within FLIP = 2^-20 (relative) of a rounding boundary without being exactly on it (`marked`), so
no element has two admissible values -
the appended K row is checked by decoding it (every element within one e4m3 spacing, at its magnitude and scale, of the float64 rotation;
the byte one of those a row maximum within 2^-8 of the float64 one gives), and the attention against the bytes the kernel left."""
import math
from collections import namedtuple

import torch

BF, F32, F64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8
E4 = torch.float8_e4m3fn
FLIP = 2.0 ** -20
B, H, D, MAX_CTX = 3, 2, 128, 400
SCALE = float(torch.tensor(1.0 / math.sqrt(D), dtype=F32))     # the fp32 value the kernel receives
SLICE = 128


# ------------------------------------------------------------------------------------------------------------------------- format
def e4m3_rne(q):
    """float64 -> nearest OCP e4m3 value, ties to even (subnormal step 2^-9); the format never asks for more than 448"""
    mag = q.abs()
    _, e = torch.frexp(mag)
    step = torch.exp2((e - 1).clamp(-6, 8).double() - 3)
    r = torch.round(mag / step) * step
    assert bool((r <= 448).all())
    return torch.copysign(r, q)


def scale_byte(m):
    """m = max|v| (float64, >= 0) -> int64 byte"""
    _, ex = torch.frexp(m)                                      # m = f 2^ex, f in [0.5, 1): floor(log2 m) = ex - 1
    e = ex.long() - 1 - 8
    e = e + (m > 448.0 * torch.exp2(e.double())).long()
    return torch.where(m > 0, (e + 127).clamp(0, 254), torch.full_like(e, 127))


def quant(v):
    """[..., 128] (bf16 values in any float dtype) -> (codes uint8 [..., 128], bytes uint8 [...])"""
    v = v.double()
    m = v.abs().amax(-1)
    byte = scale_byte(m)
    val = e4m3_rne(v / torch.exp2((byte - 127).double())[..., None])
    codes = val.float().to(E4).view(U8)
    codes = torch.where((m > 0)[..., None], codes, torch.zeros_like(codes))     # a zero row is all +0
    return codes, byte.to(U8)


def code_values(codes):
    return codes.contiguous().view(E4).float().double()


def dequant(codes, byte):
    """-> float64 [..., 128] = e4m3 value * 2^(byte - 127)"""
    return code_values(codes) * torch.exp2(byte.double() - 127)[..., None]


def spacing(x, byte):
    """the e4m3 spacing at the magnitude of x (float64 [..., 128]) under scale byte `byte` [...]"""
    sc = torch.exp2(byte.double() - 127)[..., None]
    _, e = torch.frexp(x.abs() / sc)
    return torch.exp2((e - 1).clamp(-6, 8).double() - 3) * sc


# ------------------------------------------------------------------------------------------------------------------------- rotation
def exact_tables(seed):
    """cos, sin fp32 [MAX_CTX, 64] with every (cos, sin) pair one of (1, 0), (0, 1), (-1, 0), (0, -1)"""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(0, 4, (MAX_CTX, D // 2), generator=g)
    return torch.tensor([1.0, 0.0, -1.0, 0.0])[k].contiguous(), torch.tensor([0.0, 1.0, 0.0, -1.0])[k].contiguous()


def model_tables():
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    fr = torch.outer(torch.arange(MAX_CTX).float(), inv)
    return fr.cos().to(BF).float().contiguous(), fr.sin().to(BF).float().contiguous()


def rotate64(x, cos_row, sin_row):
    """HF rotate_half in float64: x [..., 128], cos_row / sin_row [64]"""
    x = x.double()
    a, b = x[..., :D // 2], x[..., D // 2:]
    c, s = cos_row.double(), sin_row.double()
    return torch.cat((a * c - b * s, b * c + a * s), -1)


def bf16_round(x):
    return x.to(BF).double()


def marked(x64):
    """elements of a float64 tensor within FLIP (relative) of a bf16 rounding boundary, but not exactly on it: a product of two bf16 values
    has 16 significant bits, so a rotated element that IS a midpoint of two bf16 values (9 bits) is formed without error in fp32 as well,
    and ties-to-even gives it one answer"""
    lo, hi = bf16_round(x64 * (1 - FLIP)), bf16_round(x64 * (1 + FLIP))
    return (lo != hi) & ((x64 - lo).abs() != (hi - x64).abs())


# ------------------------------------------------------------------------------------------------------------------------- cases
Case = namedtuple("Case", "name pos nsplit mask wide real seed")
CASES = [
    Case("first keys ns1", (0, 1, 7), 1, False, False, False, 11),
    Case("group and slice edge ns2", (8, 127, 128), 2, False, False, False, 12),
    Case("nact below NS ns3", (129, 255, 256), 3, False, False, False, 13),
    Case("last row ns2", (383, 399, 0), 2, False, False, False, 14),
    Case("slice loop in one workgroup ns1", (383, 399, 127), 1, False, False, False, 15),
    Case("slice loop with stride ns3", (399, 256, 7), 3, False, False, False, 16),
    Case("key mask ns2", (255, 129, 8), 2, True, False, False, 17),
    Case("wide magnitudes ns3", (128, 399, 1), 3, False, True, False, 18),
    Case("model tables ns2", (129, 383, 7), 2, False, False, True, 19),
]
assert {p for c in CASES for p in c.pos} == {0, 1, 7, 8, 127, 128, 129, 255, 256, 383, 399}

_INPUTS = {}


def _mask_of(c):
    """uint8 [B, MAX_CTX] or None: hides a prefix and one interior key; position pos[b] and everything after it stays visible"""
    if not c.mask:
        return None
    km = torch.ones(B, MAX_CTX, dtype=U8)
    for b, p in enumerate(c.pos):
        pre = min(5, p // 2)
        km[b, :pre] = 0
        km[b, pre + (p - pre) // 2] = 0                          # an interior key: pre < it < p for every p of the table
        assert km[b, p] == 1 and pre + (p - pre) // 2 < p
    return km


def _magnitudes(c, n, g):
    """per (position, head) factor of the stored rows: 1, or for the wide case powers of two that put the scale bytes at about 100 .. 140"""
    if not c.wide:
        return torch.ones(n, H, dtype=F64)
    return torch.exp2(torch.randint(-19, 21, (n, H), generator=g).double())


def inputs(c):
    """-> dict, made once per case: qkv bf16 [B, 3 H D]; cos, sin fp32 [MAX_CTX, 64]; kmask; kc, vc uint8 [B MAX_CTX, H D] and ks, vs uint8
    [B MAX_CTX, H] as they are BEFORE the call - the rows of the visible, unmasked keys below pos[b] hold quantised random rows, every other
    byte is NaN filler (codes 0x7F / 0xFF alternating, scale bytes 0xFF)"""
    if c.name in _INPUTS:
        return _INPUTS[c.name]
    cos, sin = model_tables() if c.real else exact_tables(c.seed)
    for t in range(64):
        g = torch.Generator().manual_seed(c.seed + 1000 * t)
        qkv = torch.randn(B, 3, H, D, generator=g).to(BF)
        if not c.real:
            break
        q64 = torch.stack([rotate64(qkv[b, 0], cos[p], sin[p]) for b, p in enumerate(c.pos)])
        if not bool(marked(q64).any()):
            break
    else:
        raise AssertionError(f"{c.name}: no seed without a query element on a bf16 rounding boundary")
    if c.wide:
        qkv[0, 1, 0] *= 2.0 ** 12                                   # the new K row of sequence 0, head 0: byte ~ 133
        qkv[0, 2, 1] *= 2.0 ** -20                                  # the new V row of sequence 0, head 1
        qkv[1, 1, 1] = 0                                            # a zero new K head row
        qkv[2, 2, 0] = qkv[2, 2, 0].double().clamp(-3, 3).to(BF)
        qkv[2, 2, 0, 5] = 448.0 * 2.0 ** -7                         # a new V row whose maximum is exactly 448 * 2^e
    km = _mask_of(c)
    filler = torch.tensor([0x7F, 0xFF], dtype=U8).repeat(H * D // 2)
    kc, vc = filler.repeat(B * MAX_CTX, 1), filler.repeat(B * MAX_CTX, 1)
    ks, vs = torch.full((B * MAX_CTX, H), 0xFF, dtype=U8), torch.full((B * MAX_CTX, H), 0xFF, dtype=U8)
    for b, p in enumerate(c.pos):
        if p == 0:
            continue
        K = (torch.randn(p, H, D, generator=g).double() * _magnitudes(c, p, g)[..., None]).to(BF)
        V = (torch.randn(p, H, D, generator=g).double() * _magnitudes(c, p, g)[..., None]).to(BF)
        if c.wide and p >= 8:
            K[3, 0] = 0                                             # a zero head row in the cache
            K[4, 1] = K[4, 1].double().clamp(-50, 50).to(BF)
            K[4, 1, 77] = -448.0 * 2.0 ** -3                        # maximum exactly 448 * 2^e
            K[5, 1] = K[5, 1].double().clamp(-50, 50).to(BF)
            K[5, 1, 3] = 450.0 * 2.0 ** -3                          # ... and the next bf16 above it: e goes up by one
        vis = torch.ones(p, dtype=torch.bool) if km is None else km[b, :p].bool()
        rows = torch.arange(p)[vis] + b * MAX_CTX
        for cache, sc, X in ((kc, ks, K), (vc, vs, V)):
            codes, byte = quant(X[vis])
            cache[rows] = codes.reshape(-1, H * D)
            sc[rows] = byte
    _INPUTS[c.name] = dict(qkv=qkv.reshape(B, 3 * H * D), cos=cos, sin=sin, kmask=km, kc=kc, vc=vc, ks=ks, vs=vs)
    return _INPUTS[c.name]


def rotated(c):
    """-> (q float64 [B, H, D]: the rotation rounded to bf16;  k64 [B, H, D]: the float64 rotation of the new key, not rounded)"""
    i = inputs(c)
    x = i["qkv"].reshape(B, 3, H, D)
    q = torch.stack([rotate64(x[b, 0], i["cos"][p], i["sin"][p]) for b, p in enumerate(c.pos)])
    k = torch.stack([rotate64(x[b, 1], i["cos"][p], i["sin"][p]) for b, p in enumerate(c.pos)])
    return bf16_round(q), k


def expected_append(c):
    """-> (k codes [B, H, D], k bytes [B, H], v codes, v bytes) of the appended position; the k pair is exact for the exact-rotation cases only"""
    i = inputs(c)
    _, k64 = rotated(c)
    kc, kb = quant(bf16_round(k64))
    vc, vb = quant(i["qkv"].reshape(B, 3, H, D)[:, 2])
    return kc, kb, vc, vb


def expected_caches(c):
    """the four cache arrays after the call (exact-rotation cases): the arrays of `inputs` with row pos[b] of every sequence replaced"""
    i = inputs(c)
    kc, kb, vc, vb = expected_append(c)
    out = {k: i[k].clone() for k in ("kc", "vc", "ks", "vs")}
    for b, p in enumerate(c.pos):
        r = b * MAX_CTX + p
        out["kc"][r], out["vc"][r], out["ks"][r], out["vs"][r] = kc[b].reshape(-1), vc[b].reshape(-1), kb[b], vb[b]
    return out


def check_real_append(c, kc, ks):
    """model-table case: the K row the kernel appended, decoded, against the float64 rotation"""
    _, k64 = rotated(c)
    for b, p in enumerate(c.pos):
        r = b * MAX_CTX + p
        codes, byte = kc[r].reshape(H, D), ks[r]
        m = k64[b].abs().amax(-1)
        ok = (byte.long() == scale_byte(m * (1 - 2.0 ** -8))) | (byte.long() == scale_byte(m)) | (byte.long() == scale_byte(m * (1 + 2.0 ** -8)))
        assert bool(ok.all()), (c.name, b, byte.tolist())
        assert not bool(((codes & 0x7F) == 0x7F).any()), (c.name, b)
        deq = dequant(codes, byte)
        sp = torch.maximum(spacing(k64[b], byte), spacing(deq, byte))
        assert bool(((deq - k64[b]).abs() <= sp).all()), (c.name, b, float(((deq - k64[b]).abs() / sp).max()))


# ------------------------------------------------------------------------------------------------------------------------- reference and bound
Ref = namedtuple("Ref", "want bound")


def visible(c, b):
    p = c.pos[b]
    km = inputs(c)["kmask"]
    return torch.ones(p + 1, dtype=torch.bool) if km is None else km[b, :p + 1].bool()


def attention64(q, kc, ks, vc, vs, vis, scale=SCALE):
    """one head: q float64 [D]; kc / vc uint8 [n, D], ks / vs uint8 [n] (the cache rows 0 .. pos); vis bool [n] -> (want [D], bound [D])"""
    K, V = dequant(kc[vis], ks[vis]), dequant(vc[vis], vs[vis])
    assert bool(torch.isfinite(K).all()) and bool(torch.isfinite(V).all())
    s = scale * (K @ q)
    M = s.max()
    w = torch.exp(s - M)
    want = (w @ V) / w.sum()
    A = (w @ V.abs()) / w.sum()
    E_s = 130 * 2.0 ** -24 * scale * (K.abs() @ q.abs()).max()
    delta = 2 * E_s + 2.0 ** -24 * (s - M).abs().max() + (int(vis.sum()) + 16) * 2.0 ** -23
    return want, 2.0 ** -8 * want.abs() + 2.5 * delta * A


def reference(c, caches):
    """caches: dict kc, vc, ks, vs AFTER the call (expected_caches, or the bytes a kernel left) -> Ref of float64 [B, H * D]"""
    q, _ = rotated(c)
    want, bound = torch.zeros(B, H, D, dtype=F64), torch.zeros(B, H, D, dtype=F64)
    for b, p in enumerate(c.pos):
        rows = slice(b * MAX_CTX, b * MAX_CTX + p + 1)
        vis = visible(c, b)
        for h in range(H):
            cols = slice(h * D, (h + 1) * D)
            want[b, h], bound[b, h] = attention64(q[b, h], caches["kc"][rows, cols], caches["ks"][rows, h], caches["vc"][rows, cols],
                                                  caches["vs"][rows, h], vis)
    return Ref(want.reshape(B, H * D), bound.reshape(B, H * D))


_REFS = {}


def case_reference(c):
    """exact-rotation cases: the reference from the expected cache bytes, computed once and shared"""
    assert not c.real
    if c.name not in _REFS:
        _REFS[c.name] = reference(c, expected_caches(c))
    return _REFS[c.name]


WORST = {}


def ratio(got, ref, what=None):
    """-> the largest |got - want| / bound"""
    g = got.detach().double().cpu()
    assert g.shape == ref.want.shape, (g.shape, ref.want.shape)
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite output"
    err = (g - ref.want).abs()
    r = float(torch.where(err > 0, err / ref.bound.clamp_min(1e-300), torch.zeros_like(err)).max())
    if what is not None:
        WORST[what] = max(WORST.get(what, 0.0), r)
    return r


# ------------------------------------------------------------------------------------------------------------------------- float32 emulation
def _fold(t, steps):
    """butterfly sum over the last axis: t += t[lane ^ s] for s in steps, fp32"""
    idx = torch.arange(t.shape[-1])
    for s in steps:
        t = t + t[..., idx ^ s]
    return t


def _emulate_head(q, kc, kb, vc, vb, vis, p, NS):
    """q fp32 [D] (rotated, bf16-rounded, times scale); kc / vc uint8 [p + 1, D], kb / vb uint8 [p + 1] including the appended row; the
    order of the kernel: per lane 16 products summed in order, a butterfly over the 8 lanes of a key, times the key's scale; per wave and
    slice an online-softmax step over its 32 keys (group g: keys g, g + 8, ...), groups folded, waves merged, workgroups merged"""
    n = p + 1
    kf = torch.where(vis[:, None], code_values(kc).float(), torch.zeros(n, D))
    vf = torch.where(vis[:, None], (code_values(vc) * torch.exp2(vb.double() - 127)[:, None]).float(), torch.zeros(n, D))
    prod = (q[None] * kf).reshape(n, 8, 16)
    acc = torch.zeros(n, 8)
    for e in range(16):
        acc = acc + prod[:, :, e]
    dot = _fold(acc, (1, 2, 4))[:, 0] * torch.exp2(kb.float() - 127)
    dot = torch.where(vis, dot, torch.zeros(n))
    ninf = torch.tensor(float("-inf"))
    parts = []
    for sp in range(NS):
        if sp * SLICE > p:
            continue
        wm = torch.full((4,), float("-inf"))
        wl, wo = torch.zeros(4, 8), torch.zeros(4, 8, D)
        for base in range(sp * SLICE, p + 1, NS * SLICE):
            for w in range(4):
                keys = base + w * 32 + torch.arange(8)[None] + 8 * torch.arange(4)[:, None]          # [i, grp]
                ok = keys <= p
                kk = keys.clamp_max(p)
                ok = ok & vis[kk]
                sc = torch.where(ok, dot[kk], ninf)
                m_new = torch.maximum(wm[w], sc.max())
                m_use = m_new if bool(torch.isfinite(m_new)) else torch.tensor(0.0)
                alpha = torch.exp(wm[w] - m_use)
                wl[w], wo[w] = wl[w] * alpha, wo[w] * alpha
                wm[w] = m_new
                for i in range(4):
                    pr = torch.where(ok[i], torch.exp(sc[i] - m_use), torch.zeros(8))
                    wl[w] = wl[w] + pr
                    wo[w] = wo[w] + pr[:, None] * vf[kk[i]]
        l, o = _fold(wl, (1, 2, 4))[:, 0], _fold(wo.transpose(1, 2), (1, 2, 4))[:, :, 0]
        M = wm.max()
        L, a = torch.tensor(0.0), torch.zeros(D)
        for w in range(4):
            f = torch.exp(wm[w] - M) if bool(torch.isfinite(wm[w])) else torch.tensor(0.0)
            L, a = L + f * l[w], a + f * o[w]
        parts.append((M, L, a))
    if len(parts) == 1:
        _, L, a = parts[0]
    else:
        Mx = torch.stack([m for m, _, _ in parts]).max()
        L, a = torch.tensor(0.0), torch.zeros(D)
        for m, l_, o_ in parts:
            f = torch.exp(m - Mx) if bool(torch.isfinite(m)) else torch.tensor(0.0)
            L, a = L + f * l_, a + f * o_
    return torch.where(L > 0, a / L, torch.zeros(D)).to(BF)


def emulate(c, nsplit=None):
    """float32 model of lhrs_decode_attn_kv8 on the inputs of a case -> (out bf16 [B, H D], dict of the four cache arrays afterwards)"""
    i = inputs(c)
    NS = c.nsplit if nsplit is None else nsplit
    x = i["qkv"].reshape(B, 3, H, D).float()
    caches = {k: i[k].clone() for k in ("kc", "vc", "ks", "vs")}
    out = torch.zeros(B, H, D, dtype=BF)
    for b, p in enumerate(c.pos):
        co, si = i["cos"][p], i["sin"][p]
        rot = lambda t: torch.cat((t[:, :64] * co - t[:, 64:] * si, t[:, 64:] * co + t[:, :64] * si), -1).to(BF)
        q = rot(x[b, 0]).float() * torch.tensor(SCALE, dtype=F32)
        kcod, kby = quant(rot(x[b, 1]))
        vcod, vby = quant(x[b, 2])
        r = b * MAX_CTX + p
        caches["kc"][r], caches["vc"][r], caches["ks"][r], caches["vs"][r] = kcod.reshape(-1), vcod.reshape(-1), kby, vby
        rows, vis = slice(b * MAX_CTX, r + 1), visible(c, b)
        for h in range(H):
            cols = slice(h * D, (h + 1) * D)
            out[b, h] = _emulate_head(q[h], caches["kc"][rows, cols], caches["ks"][rows, h], caches["vc"][rows, cols], caches["vs"][rows, h],
                                      vis, p, NS)
    return out.reshape(B, H * D), caches


# ------------------------------------------------------------------------------------------------------------------------- planted rows
def planted():
    """bf16 [8, 128], the rest of each row 0.02 randn clamped below the planted maximum.  Rows: 0 all zero (with a -0.0 in it); 1 the maximum
    exactly 448 * 2^-3; 2 the next bf16 above it (450 * 2^-3: e one higher); 3 exact e4m3 ties under e = 0 (maximum 256) and a negative value
    that rounds to -0; 4 values near 2^-130 (the clamp at byte 0); 5 the largest finite bf16 (byte 247); 6 one outlier 2^12 above the rest;
    7 the maximum exactly a power of two"""
    g = torch.Generator().manual_seed(78)
    R = (0.02 * torch.randn(8, D, generator=g)).to(BF)
    R[0] = 0
    R[0, 9] = -0.0
    R[1, 17] = 448.0 * 2.0 ** -3
    R[2, 100] = -450.0 * 2.0 ** -3
    row = [256.0, 0.5 * 2.0 ** -9, 1.5 * 2.0 ** -9, -2.5 * 2.0 ** -9, 17.0, 19.0, -21.0, 1.0625, 1.1875, -2.0 ** -12, 2.0 ** -10, 0.0, -0.0]
    R[3] = 0
    R[3, :len(row)] = torch.tensor(row, dtype=F64).to(BF)
    R[4] = (2.0 ** -130 * torch.randn(D, generator=g).double()).to(BF)
    R[5, 64] = float(torch.finfo(BF).max)
    R[6, 1] = 0.02 * 2.0 ** 12
    R[7] = R[7].double().clamp(-0.06, 0.06).to(BF)
    R[7, 127] = 0.0625
    return R
