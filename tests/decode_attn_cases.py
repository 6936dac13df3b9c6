"""The bf16 decode attention (csrc/decode_attn.hip behind hk.decode_attn / hk.decode_attn_split, and the composed route hk.rope_kv_append +
hk.attn_fwd of a model whose head_dim is not 128), the exported hk.kv_append and the step bookkeeping (hk.decode_advance / hk.decode_emit;
csrc/decode.hip),
restated for tests/test_decode_attn_cases_cpu.py and tests/test_decode_attn_gpu.py.  Shares no code with the HIP source.

Inputs.  B = 3 sequences, each at its own position pos[b]; H = 2 heads of D = 128 (the composed route also H = 4, D = 64).  qkv is bf16
[B, 3 H D].  The caches are bf16 [B * max_ctx, H * D]: random rows at the visible, unmasked keys below pos[b]; EVERY other element is a NaN
(two payloads alternating) - row pos[b] before the call, every masked key's row, every row after pos[b] - so a read of a row the kernel has
no business with turns the output into NaN, and a write there changes a payload.  max_ctx is per case and no larger than the case needs.

Rotation.  The kernels take cos_t / sin_t as arguments.  The exact cases pass tables whose (cos, sin) pairs are drawn from (1, 0), (0, 1),
(-1, 0), (0, -1): RoPE is an exact signed permutation, the rotated rows have one bf16 answer and appended rows are compared bit for bit.
The model-table cases use bf16-rounded cos / sin held in fp32 (as TextModal builds them): q is the float64 rotation rounded to bf16 - the
seed is the first for which no q element is `marked` (within 2^-20 of a rounding boundary) - and an appended or rotated element x = a c -+ b s
must satisfy  |got - x64| <= (bf16 spacing at |x64|) + 2^-22 (|a c| + |b s|):  the bf16 store, plus the fp32 rounding of the two products
and of the add (3 roundings of 2^-24 relative to at most |a c| + |b s|, rounded up to 4), which matters only under cancellation.  The
attention reference of those cases is computed from the K row the kernel left.

Reference, per head in float64 over the visible keys j <= pos the mask does not hide: s_j = scale * q . K_j, M = max s, w = exp(s - M),
want = sum w V / sum w; q is the rotation rounded to bf16, `scale` the fp32 value the kernel receives; no visible key gives want = 0.

Bound of an output element, derived, never measured on a kernel:

    |got - want| <= 2^-8 |want| + 2.5 * delta * A  (+ 2^-8 A on the composed route),       A = sum_j w_j |v_j| / sum_j w_j  (per element),
    delta = 2 E_s + 2^-24 max_j |s_j - M| + n_acc 2^-23,      E_s = 130 * 2^-24 * scale * max_j sum_i |q_i k_ji|

  - 2^-8 |want|: the bf16 store, half a unit in the last place at the bottom of a binade;
  - E_s: a score is a 128-term fp32 dot: q_i * scale rounded once, each product once (or not under an fma), each of the 127 additions once
    whatever their order (8 in a lane, then a butterfly over the 16 lanes of a key) - at most 130 roundings of 2^-24 relative to the sum of
    the magnitudes.  A weight exp(s_j - M) sees the error of s_j and that of M: 2 E_s in the exponent, which is its relative error;
  - 2^-24 max |s_j - M|: __expf scales its argument by log2(e) in fp32, one rounding relative to the argument;
  - n_acc 2^-23: one fp32 rounding (2^-24, doubled for slack, which also covers the 1-ulp hardware exp2) per accumulate an output element
    or the denominator goes through.  Counted from each kernel's own structure, P = the passes / slices ONE workgroup walks:
      one workgroup (`acc_one`):  a lane group adds 16 keys per 512-key pass and rescales once per pass (17 P, P = ceil((pos + 1) / 512));
        2 folds across the 4 groups of a wave; 8 waves merged, a multiply and an add each (16); the division (1):  17 P + 19.
      split (`acc_split`):  8 keys per group per 128-key slice and one rescale (9 P, P = ceil(slices / NS), slices = pos // 128 + 1); 2 folds;
        4 waves, a multiply and an add each (8); up to 16 workgroup partials with one rescale and one add each (2 nact, nact = min(NS,
        slices)); the division (1):  9 P + 11 + 2 nact.
      composed (`acc_composed`, the tiled MFMA forward at q_len 1):  a tile is 64 keys; the two P.V MFMAs add 64 products to an
        accumulator that was rescaled once (65 T, T = ceil((pos + 1) / 64)); the row sum of P likewise; the multiply by 1 / l and the
        reciprocal (2):  65 T + 2.  That kernel rounds P to bf16 before the MFMA while the denominator keeps the fp32 P: every term of
        the numerator is off by at most 2^-9 relative (round to nearest even), bounded with slack by the extra 2^-8 A.
  - 2.5: numerator and denominator each carry delta (2 to first order); the rest covers the second order and the rounding of an already
    perturbed value at the store.
`ratio` = error / bound; at most 1 passes.  The float32 emulations below follow each kernel's order of operations (pass / slice loop, one
online-softmax step per wave and pass, group folds, LDS merge, ticket merge) with __expf modelled as torch.exp in fp32;
tests/test_decode_attn_cases_cpu.py holds them to the bound on every case and prints their worst ratio, tests/test_decode_attn_gpu.py the
device's (DESIGN.md "Decode attention vs fp64")."""
from collections import namedtuple

import torch

from kv8_cases import BF, F32, F64, U8, SCALE, bf16_round, marked, _fold

I16 = torch.int16
B = 3
NAN_BITS = (0x7FC1, 0xFFA5 - 0x10000)                               # a quiet NaN of each sign, payloads that a copy must keep
FINITE_FILL = 2.0 ** 100                                            # composed route: what a masked V row below pos holds (see `inputs`)

Case = namedtuple("Case", "name pos max_ctx nsplit mask wide real seed H D route", defaults=(2, 128, "decode"))
# mask: None | "std" (a prefix and one interior key of every sequence, as kv8_cases._mask_of) | "slice" (sequence 0: keys 128..255, one whole
# slice; sequence 1: keys 0..127, slice 0; sequence 2: std) | "all" (sequence 1: every key up to and including pos; the others: std)
CASES = [
    Case("first keys clamp ns1", (0, 3, 4), 67, 1, None, False, False, 31),
    Case("wave edges nact below NS ns2", (63, 64, 31), 130, 2, None, False, False, 32),
    Case("slice edge last row ns1", (32, 127, 128), 129, 1, None, False, False, 33),
    Case("ns2 edges last row", (255, 256, 63), 257, 2, None, False, False, 34),
    Case("ns3 edges", (383, 384, 3), 386, 3, None, False, False, 35),
    Case("pass edge ns5", (511, 512, 513), 514, 5, None, False, False, 36),
    Case("ns5 edges last row", (639, 640, 64), 641, 5, None, False, False, 37),
    Case("two passes stride 3", (1023, 1024, 4), 1027, 3, None, False, False, 38),
    Case("all sixteen partials and the loop ns16", (2047, 2048, 2049), 2050, 16, None, False, False, 39),
    Case("sixteen partials from 1920 masked ns16", (1920, 127, 700), 1922, 16, "std", False, False, 40),
    Case("key mask ns2", (513, 129, 8), 520, 2, "std", False, False, 41),
    Case("a whole slice masked ns3", (300, 200, 140), 301, 3, "slice", False, False, 42),
    Case("every key of one sequence masked ns2", (5, 200, 130), 203, 2, "all", False, False, 43),
    Case("wide magnitudes ns3", (128, 399, 1), 402, 3, None, True, False, 44),
    Case("model tables ns2", (129, 383, 7), 385, 2, None, False, True, 45),
    Case("model tables masked ns5", (1024, 513, 31), 1030, 5, "std", False, True, 46),
]
_POS = {p for c in CASES for p in c.pos}
assert {0, 3, 4, 63, 64, 511, 512, 513, 1023, 1024} <= _POS                               # decode_attn: groups stride 4, wave 64 keys, pass 512
assert {0, 31, 32, 127, 128} <= _POS                                                       # decode_attn_split: wave 32 keys, slice 128
assert {c.nsplit for c in CASES} == {1, 2, 3, 5, 16}
for _ns in (1, 2, 3, 5, 16):                                                               # one slice per workgroup / workgroup 0 takes a second one
    assert any(c.nsplit == _ns and 128 * _ns - 1 in c.pos for c in CASES) and any(c.nsplit == _ns and 128 * _ns in c.pos for c in CASES), _ns
assert any(c.max_ctx % 4 and c.max_ctx - 1 in c.pos for c in CASES)                        # the min(key, max_ctx - 1) clamp at the last row
assert any(p // 128 + 1 < c.nsplit for c in CASES for p in c.pos if p >= 128)              # 1 < nact < NS
assert any(c.nsplit == 16 and 1920 <= p <= 2047 for c in CASES for p in c.pos) and any(c.nsplit == 16 and p >= 2048 for c in CASES for p in c.pos)

# rope_kv_append + attn_fwd (tile 64 keys): the head_dim-64 route of TextModal's decode step, at both head dims
COMPOSED = [
    Case("composed d128 tile edges", (0, 63, 64), 70, 1, None, False, False, 51, 2, 128, "composed"),
    Case("composed d128 masked", (65, 200, 130), 201, 1, "std", False, False, 52, 2, 128, "composed"),
    Case("composed d128 model tables", (129, 7, 64), 131, 1, "std", False, True, 53, 2, 128, "composed"),
    Case("composed d64 tile edges", (0, 63, 64), 70, 1, None, False, False, 54, 4, 64, "composed"),
    Case("composed d64 masked", (65, 200, 130), 201, 1, "std", False, False, 55, 4, 64, "composed"),
    Case("composed d64 model tables", (129, 7, 64), 131, 1, None, False, True, 56, 4, 64, "composed"),
]


def ident(c):
    return c.name.replace(" ", "_")


def scale_of(c):
    """the fp32 value the kernel receives"""
    return SCALE if c.D == 128 else float(torch.tensor(c.D ** -0.5, dtype=F32))


# ------------------------------------------------------------------------------------------------------------------------- rotation
def exact_tables(seed, n, half):
    """cos, sin fp32 [n, half] with every (cos, sin) pair one of (1, 0), (0, 1), (-1, 0), (0, -1)"""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(0, 4, (n, half), generator=g)
    return torch.tensor([1.0, 0.0, -1.0, 0.0])[k].contiguous(), torch.tensor([0.0, 1.0, 0.0, -1.0])[k].contiguous()


def model_tables(n, d):
    inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2).float() / d))
    fr = torch.outer(torch.arange(n).float(), inv)
    return fr.cos().to(BF).float().contiguous(), fr.sin().to(BF).float().contiguous()


def rotate64(x, cos_row, sin_row):
    """HF rotate_half in float64: x [..., D], cos_row / sin_row [D / 2] -> (rotation, |a c| + |b s| per element)"""
    x = x.double()
    h = x.shape[-1] // 2
    a, b = x[..., :h], x[..., h:]
    c, s = cos_row.double(), sin_row.double()
    return torch.cat((a * c - b * s, b * c + a * s), -1), torch.cat(((a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()), -1)


def bf16_spacing(x):
    """the distance between neighbouring bf16 values at the magnitude of x (float64); the smallest subnormal at 0"""
    _, e = torch.frexp(x.abs())
    return torch.where(x == 0, torch.full_like(x, 2.0 ** -133), torch.exp2((e - 1).clamp_min(-126).double() - 7))


# ------------------------------------------------------------------------------------------------------------------------- inputs
_INPUTS = {}


def mask_of(c):
    """uint8 [B, max_ctx] or None; everything after pos[b] stays visible"""
    if c.mask is None:
        return None
    km = torch.ones(B, c.max_ctx, dtype=U8)
    for b, p in enumerate(c.pos):
        if c.mask == "all" and b == 1:
            km[b, :p + 1] = 0
        elif c.mask == "slice" and b == 0:
            assert p >= 256
            km[b, 128:256] = 0
        elif c.mask == "slice" and b == 1:
            assert p >= 128
            km[b, :128] = 0
        else:
            pre = min(5, p // 2)
            km[b, :pre] = 0
            km[b, pre + (p - pre) // 2] = 0                          # an interior key: pre < it < p for every p of the tables
            assert km[b, p] == 1 and pre + (p - pre) // 2 < p
    return km


def visible(c, b):
    """bool [pos[b] + 1]: the keys sequence b attends to, the new one (pos[b]) last"""
    p = c.pos[b]
    km = inputs(c)["kmask"]
    return torch.ones(p + 1, dtype=torch.bool) if km is None else km[b, :p + 1].bool()


def nan_rows(rows, cols):
    """bf16 [rows, cols] of NaNs, the two payloads of NAN_BITS alternating"""
    return torch.tensor(NAN_BITS, dtype=I16).repeat(rows * cols // 2).reshape(rows, cols).view(BF)


def inputs(c):
    """-> dict, made once per case: qkv bf16 [B, 3 H D]; cos, sin fp32 [max_ctx, D / 2]; kmask; kc, vc bf16 [B max_ctx, H D] as they are
    BEFORE the call: random rows at the visible, unmasked keys below pos[b], NaN everywhere else.  Composed route only: the V rows of
    MASKED keys below pos[b] hold FINITE_FILL instead - that forward multiplies a masked key's V row by its weight of exactly 0 (see
    lhrs_attn_fwd_kmask), so the row has to be finite; its K row and every row from pos[b] on stay NaN there as well."""
    if c.name in _INPUTS:
        return _INPUTS[c.name]
    H, D, hd = c.H, c.D, c.H * c.D
    cos, sin = model_tables(c.max_ctx, D) if c.real else exact_tables(c.seed, c.max_ctx, D // 2)
    for t in range(64):
        g = torch.Generator().manual_seed(c.seed + 1000 * t)
        qkv = torch.randn(B, 3, H, D, generator=g).to(BF)
        if not c.real:
            break
        q64 = torch.stack([rotate64(qkv[b, 0], cos[p], sin[p])[0] for b, p in enumerate(c.pos)])
        if not bool(marked(q64).any()):
            break
    else:
        raise AssertionError(f"{c.name}: no seed without a query element on a bf16 rounding boundary")
    if c.wide:
        qkv[0, 1, 0] *= 2.0 ** 12                                   # the new K row of sequence 0, head 0
        qkv[0, 2, 1] *= 2.0 ** -20                                  # the new V row of sequence 0, head 1
        qkv[1, 1, 1] = 0                                            # a zero new K head row
    km = mask_of(c)
    kc, vc = nan_rows(B * c.max_ctx, hd), nan_rows(B * c.max_ctx, hd)
    for b, p in enumerate(c.pos):
        if p == 0:
            continue
        mk = torch.exp2(torch.randint(-19, 21, (p, H), generator=g).double()) if c.wide else torch.ones(p, H, dtype=F64)
        mv = torch.exp2(torch.randint(-19, 21, (p, H), generator=g).double()) if c.wide else torch.ones(p, H, dtype=F64)
        K = (torch.randn(p, H, D, generator=g).double() * mk[..., None]).to(BF)
        V = (torch.randn(p, H, D, generator=g).double() * mv[..., None]).to(BF)
        if c.wide and p >= 8:
            K[3, 0] = 0                                             # a zero head row in the cache
        vis = torch.ones(p, dtype=torch.bool) if km is None else km[b, :p].bool()
        rows = torch.arange(p)[vis] + b * c.max_ctx
        kc[rows], vc[rows] = K[vis].reshape(-1, hd), V[vis].reshape(-1, hd)
        if c.route == "composed":
            vc[torch.arange(p)[~vis] + b * c.max_ctx] = FINITE_FILL
    _INPUTS[c.name] = dict(qkv=qkv.reshape(B, 3 * hd), cos=cos, sin=sin, kmask=km, kc=kc, vc=vc)
    return _INPUTS[c.name]


def nan_filler_holds(c):
    """the claims of the docstring on the inputs of a case -> the number of NaN rows above pos that a kernel loads all the same (the
    one-workgroup kernel asks for keys 0..511 before it knows pos, the NS workgroups of the split kernel for keys 0..128 NS - 1, and both
    load a later pass / slice whole; both clamp at max_ctx - 1)"""
    i = inputs(c)
    first = 0
    for b, p in enumerate(c.pos):
        r0 = b * c.max_ctx
        vis = visible(c, b)[:p]
        for name in ("kc", "vc"):
            t = i[name]
            assert bool(torch.isnan(t[r0 + p:r0 + c.max_ctx].float()).all()), (c.name, name, b)                 # row pos and everything after it
            hidden = t[r0:r0 + p][~vis].float()
            if c.route == "composed" and name == "vc":
                assert bool((hidden == FINITE_FILL).all()), (c.name, b)
            else:
                assert bool(torch.isnan(hidden).all()), (c.name, name, b)                                         # every masked key below pos
            assert bool(torch.isfinite(t[r0:r0 + p][vis].float()).all()), (c.name, name, b)
        for span, up_front in ((512, 512), (128, 128 * c.nsplit)):       # a later pass / slice is loaded whole as well, once its base is <= pos
            first += min(max(up_front, -(-(p + 1) // span) * span), c.max_ctx) - (p + 1)
    return first


# ------------------------------------------------------------------------------------------------------------------------- expected rows
def rotated(c):
    """-> (q float64 [B, H, D]: the rotation rounded to bf16;  q64, k64 [B, H, D]: the float64 rotations, not rounded;  qtol, ktol: what a
    bf16 element the kernel formed from fp32 products may differ from them by)"""
    i = inputs(c)
    x = i["qkv"].reshape(B, 3, c.H, c.D)
    q, qm = zip(*[rotate64(x[b, 0], i["cos"][p], i["sin"][p]) for b, p in enumerate(c.pos)])
    k, km = zip(*[rotate64(x[b, 1], i["cos"][p], i["sin"][p]) for b, p in enumerate(c.pos)])
    q, qm, k, km = torch.stack(q), torch.stack(qm), torch.stack(k), torch.stack(km)
    return bf16_round(q), q, k, bf16_spacing(q) + 2.0 ** -22 * qm, bf16_spacing(k) + 2.0 ** -22 * km


def expected_caches(c):
    """(kc, vc) after the call: the arrays of `inputs` with row pos[b] of every sequence replaced; the K rows hold for exact tables only"""
    i = inputs(c)
    _, _, k64, _, _ = rotated(c)
    kc, vc = i["kc"].clone(), i["vc"].clone()
    hd = c.H * c.D
    for b, p in enumerate(c.pos):
        kc[b * c.max_ctx + p] = k64[b].to(BF).reshape(-1)
        vc[b * c.max_ctx + p] = i["qkv"][b, 2 * hd:]
    return kc, vc


def bits(t):
    return t.contiguous().view(I16)


def check_caches(c, kc, vc):
    """the caches a kernel (or an emulation) left, as host tensors: the appended V row bit-identical to the qkv V block, the appended K row
    exact (exact tables) or within the rotation tolerance (model tables), every other element bit-unchanged, NaN payloads included"""
    wk, wv = expected_caches(c)
    assert torch.equal(bits(vc), bits(wv)), f"{c.name}: the V cache differs from the expected bits"
    if not c.real:
        assert torch.equal(bits(kc), bits(wk)), f"{c.name}: the K cache differs from the expected bits"
        return
    keep = torch.ones(B * c.max_ctx, dtype=torch.bool)
    keep[[b * c.max_ctx + p for b, p in enumerate(c.pos)]] = False
    assert torch.equal(bits(kc)[keep], bits(wk)[keep]), f"{c.name}: a K cache row other than the appended ones changed"
    _, _, k64, _, ktol = rotated(c)
    for b, p in enumerate(c.pos):
        got = kc[b * c.max_ctx + p].double().reshape(c.H, c.D)
        assert bool(((got - k64[b]).abs() <= ktol[b]).all()), (c.name, b, float(((got - k64[b]).abs() / ktol[b]).max()))


# ------------------------------------------------------------------------------------------------------------------------- reference and bound
Ref = namedtuple("Ref", "want A delta0")       # float64 [B, H * D], [B, H * D], [B, H]: delta without the accumulate term


def attention64(q, K, V, scale):
    """one head over its visible keys: q float64 [D], K / V float64 [n, D] -> (want [D], A [D], delta0)"""
    if K.shape[0] == 0:
        z = torch.zeros_like(q)
        return z, z, torch.zeros((), dtype=F64)
    assert bool(torch.isfinite(K).all()) and bool(torch.isfinite(V).all())
    s = scale * (K @ q)
    M = s.max()
    w = torch.exp(s - M)
    want, A = (w @ V) / w.sum(), (w @ V.abs()) / w.sum()
    E_s = 130 * 2.0 ** -24 * scale * (K.abs() @ q.abs()).max()
    return want, A, 2 * E_s + 2.0 ** -24 * (s - M).abs().max()


def reference(c, kc, vc):
    """kc, vc: the caches AFTER the call (expected_caches, or what a kernel left) -> Ref"""
    q = rotated(c)[0]
    H, D = c.H, c.D
    want, A, d0 = torch.zeros(B, H, D, dtype=F64), torch.zeros(B, H, D, dtype=F64), torch.zeros(B, H, dtype=F64)
    for b, p in enumerate(c.pos):
        vis = visible(c, b)
        K = kc[b * c.max_ctx:b * c.max_ctx + p + 1].reshape(p + 1, H, D)[vis].double()
        V = vc[b * c.max_ctx:b * c.max_ctx + p + 1].reshape(p + 1, H, D)[vis].double()
        for h in range(H):
            want[b, h], A[b, h], d0[b, h] = attention64(q[b, h], K[:, h], V[:, h], scale_of(c))
    return Ref(want.reshape(B, H * D), A.reshape(B, H * D), d0)


_REFS = {}


def case_reference(c):
    """exact-table cases: the reference from the expected cache rows, computed once and shared"""
    assert not c.real
    if c.name not in _REFS:
        _REFS[c.name] = reference(c, *expected_caches(c))
    return _REFS[c.name]


def acc_one(p):
    return 17 * (-(-(p + 1) // 512)) + 19


def acc_split(p, ns):
    slices = p // 128 + 1
    return 9 * (-(-slices // ns)) + 11 + 2 * min(ns, slices)


def acc_composed(p):
    return 65 * (-(-(p + 1) // 64)) + 2


def bound(c, ref, kernel, nsplit=None):
    """kernel: "one" | "split" | "composed" -> float64 [B, H * D]"""
    ns = c.nsplit if nsplit is None else nsplit
    n = {"one": acc_one, "split": lambda p: acc_split(p, ns), "composed": acc_composed}[kernel]
    nacc = torch.tensor([n(p) for p in c.pos], dtype=F64)
    delta = (ref.delta0 + nacc[:, None] * 2.0 ** -23).repeat_interleave(c.D, 1)
    return 2.0 ** -8 * ref.want.abs() + 2.5 * delta * ref.A + (2.0 ** -8 * ref.A if kernel == "composed" else 0.0)


WORST = {}


def ratio(got, want, bnd, what=None):
    """-> the largest |got - want| / bound; an element that must be exact (bound 0) and is not counts as infinite"""
    g = got.detach().double().cpu()
    assert g.shape == want.shape, (g.shape, want.shape)
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite output"
    err = (g - want).abs()
    r = float(torch.where(err > 0, err / bnd.clamp_min(1e-300), torch.zeros_like(err)).max())
    if what is not None:
        WORST[what] = max(WORST.get(what, 0.0), r)
    return r


# ------------------------------------------------------------------------------------------------------------------------- float32 emulation
def _rot32(t, co, si):
    h = t.shape[-1] // 2
    return torch.cat((t[:, :h] * co - t[:, h:] * si, t[:, h:] * co + t[:, :h] * si), -1).to(BF)


def _emulate_head(qs, K, V, vis, p, kpg, waves, NS):
    """qs fp32 [128]: the rotated, bf16-rounded query times scale; K / V fp32 [p + 1, 128] with the appended row, zero where not visible.
    A workgroup covers 4 * kpg * waves keys per pass; wave w, lane group g: keys base + 4 kpg w + g + 4 i.  Per key 8 products summed in a
    lane, a butterfly over the 16 lanes; per wave and pass one online-softmax step with the wave-wide maximum, each group adding its keys in
    order; groups folded, waves merged in order, workgroup partials merged in order."""
    n, span = p + 1, 4 * kpg * waves
    prod = (qs[None] * K).reshape(n, 16, 8)
    acc = torch.zeros(n, 16)
    for e in range(8):
        acc = acc + prod[:, :, e]
    dot = _fold(acc, (1, 2, 4, 8))[:, 0]
    ninf, zero = torch.tensor(float("-inf")), torch.tensor(0.0)
    widx = torch.arange(waves)[:, None, None] * (4 * kpg) + torch.arange(kpg)[None, :, None] * 4 + torch.arange(4)[None, None, :]   # [w, i, g]
    parts = []
    for sp in range(NS):
        if sp * span > p:
            continue
        m = torch.full((waves,), float("-inf"))
        l, o = torch.zeros(waves, 4), torch.zeros(waves, 4, 128)
        for base in range(sp * span, p + 1, NS * span):
            keys = base + widx
            kk = keys.clamp_max(p)
            ok = (keys <= p) & vis[kk]
            sc = torch.where(ok, dot[kk], ninf)
            m_new = torch.maximum(m, sc.amax((1, 2)))
            m_use = torch.where(torch.isfinite(m_new), m_new, zero)
            alpha = torch.exp(m - m_use)
            l, o = l * alpha[:, None], o * alpha[:, None, None]
            m = m_new
            for i in range(kpg):
                pr = torch.where(ok[:, i], torch.exp(sc[:, i] - m_use[:, None]), zero)       # [w, g]
                l = l + pr
                o = o + pr[..., None] * V[kk[:, i]]
        lw, ow = _fold(l, (1, 2))[:, 0], _fold(o.transpose(1, 2), (1, 2))[:, :, 0]
        M = m.max()
        L, a = torch.tensor(0.0), torch.zeros(128)
        for w in range(waves):
            f = torch.exp(m[w] - M) if bool(torch.isfinite(m[w])) else zero
            L, a = L + f * lw[w], a + f * ow[w]
        parts.append((M, L, a))
    if len(parts) == 1:
        _, L, a = parts[0]
    else:
        Mx = torch.stack([x for x, _, _ in parts]).max()
        L, a = torch.tensor(0.0), torch.zeros(128)
        for ms, ls, os_ in parts:
            f = torch.exp(ms - Mx) if bool(torch.isfinite(ms)) else zero
            L, a = L + f * ls, a + f * os_
    return torch.where(L > 0, a / L, torch.zeros(128)).to(BF)


def _emulate_tiled_head(q, K, V, vis, p, scale):
    """the tiled forward at one query row: fp32 scores times scale, one online-softmax step per 64-key tile, the row sum from the fp32 weights,
    the weights rounded to bf16 for the product with V, the result times 1 / l"""
    s = torch.where(vis, (K @ q) * scale, torch.tensor(float("-inf")))
    m, l, o = torch.tensor(float("-inf")), torch.tensor(0.0), torch.zeros(q.shape[0])
    for t0 in range(0, p + 1, 64):
        st = s[t0:t0 + 64]
        m_new = torch.maximum(m, st.max())
        m_use = m_new if bool(torch.isfinite(m_new)) else torch.tensor(0.0)
        alpha = torch.exp(m - m_use)
        pw = torch.exp(st - m_use)
        l = l * alpha + pw.sum()
        o = o * alpha + pw.to(BF).float() @ V[t0:t0 + 64]
        m = m_new
    inv = 1.0 / l if bool(l > 0) else torch.tensor(0.0)
    return (o * inv).to(BF)


def emulate(c, kernel, nsplit=None):
    """float32 model of lhrs_decode_attn ("one"), lhrs_decode_attn_split ("split") or rope_kv_append + the tiled forward ("composed") on the
    inputs of a case -> (out bf16 [B, H D], kc, vc afterwards)"""
    i = inputs(c)
    H, D, hd = c.H, c.D, c.H * c.D
    NS = 1 if kernel != "split" else (c.nsplit if nsplit is None else nsplit)
    x = i["qkv"].reshape(B, 3, H, D).float()
    kc, vc = i["kc"].clone(), i["vc"].clone()
    out = torch.zeros(B, H, D, dtype=BF)
    scale = torch.tensor(scale_of(c), dtype=F32)
    for b, p in enumerate(c.pos):
        co, si = i["cos"][p], i["sin"][p]
        q = _rot32(x[b, 0], co, si).float()
        r = b * c.max_ctx + p
        kc[r], vc[r] = _rot32(x[b, 1], co, si).reshape(-1), i["qkv"][b, 2 * hd:]
        vis = visible(c, b)
        K = torch.where(vis[:, None, None], kc[r - p:r + 1].reshape(p + 1, H, D).float(), torch.zeros(()))
        V = torch.where(vis[:, None, None], vc[r - p:r + 1].reshape(p + 1, H, D).float(), torch.zeros(()))
        for h in range(H):
            if kernel == "composed":
                out[b, h] = _emulate_tiled_head(q[h], K[:, h], V[:, h], vis, p, scale)
            else:
                kpg, waves = (16, 8) if kernel == "one" else (8, 4)
                out[b, h] = _emulate_head(q[h] * scale, K[:, h], V[:, h], vis, p, kpg, waves, NS)
    return out.reshape(B, hd), kc, vc


# ------------------------------------------------------------------------------------------------------------------------- bookkeeping
def advance_model(state, desc, pos, Bn, max_ctx, inc, cos=None, sin=None, cs=None):
    """lhrs_decode_advance[_cs] on host int32 tensors, in place: state [4], desc [Bn, 8], pos [Bn]; cs fp32 [Bn, 128] with the tables"""
    ctx = int(state[0])
    for b in range(Bn):
        desc[b, :6] = torch.tensor([b, 1, b * max_ctx, ctx + 1, ctx + 1, ctx], dtype=desc.dtype)
        pos[b] = ctx
        if cs is not None:
            cs[b, :64], cs[b, 64:] = cos[ctx], sin[ctx]
    state[0] = ctx + inc


def emit_model(next_ids, tok32, out_ids, state, Bn, max_new):
    """lhrs_decode_emit on host tensors, in place: next_ids int64 [Bn], tok32 int32 [Bn], out_ids int64 [Bn, max_new], state int32 [4]"""
    t = int(state[1])
    tok32[:Bn] = next_ids[:Bn].to(tok32.dtype)
    if t < max_new:
        out_ids[:Bn, t] = next_ids[:Bn]
    state[1] = t + 1
