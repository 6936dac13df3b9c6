"""Sampling cases shared by tests/test_sampling_gpu.py and tests/test_sampling_cases_cpu.py: Philox4x32-10 restated, a float64 reference of
what lhrs_sample_rows (csrc/sample.hip) computes - HF's RepetitionPenaltyLogitsProcessor -> TemperatureLogitsWarper -> TopKLogitsWarper ->
TopPLogitsWarper -, the draw on Python integers, and a comparator that returns what it measured.

Bounds.  L1 = sum_i |w_i / W - p_i| over the non-excused tokens of a row: the kernel's integer weights against the float64 probabilities of the
same inputs.  Worst value per case (temperature, top_k, top_p, penalty) measured on an MI355X over all V, ld and n of test_sampling_gpu.py,
randn scale 1 | scale 8:
    (0.4, 50, 0.9,  1)     2.3e-8 | 1.9e-8        (0.2, 50, 0.9, 1)    2.2e-8 | 1.7e-8        (1.0, 50, 0.95, 1.05)  3.3e-8 | 2.3e-8
    (1.0, 0,  0.9,  1)     7.9e-8 | 2.2e-8        (1.0, 0,  0.5, 1.3)  5.6e-8 | 2.5e-8        (0.7, 5,  off,  1)     2.6e-8 | 1.4e-8
    (1.3, 0,  off,  1)     6.8e-8 | 2.1e-8        no token was excused in any case
    worst 7.9e-8   ->   L1_BOUND 2e-7   (~2.5x; whatever is measured, the bound may not exceed 1e-4)
It comes from the fp32 subtraction z - zmax (half an ulp of an argument near -10 is 5e-8 relative), the fp32 exp (1 ulp = 6e-8 relative) and the
rounding to a multiple of 2^-40; the errors of the tokens are independent and largely cancel in the normalised sum.  A missing 1.05 penalty
or a 5 % temperature error moves L1 by 1e-3 and more (test_sampling_cases_cpu.py).
Top-p: a token may be EXCUSED from the support comparison only if, in the reference, the mass strictly above it lies within TOP_P_BAND of
top_p * total; at most MAX_EXCUSED such tokens per row.  Top-k and the penalty are exact, no band."""
from collections import namedtuple

import numpy as np

L1_BOUND = 2e-7
TOP_P_BAND = 1e-5
MAX_EXCUSED = 4
WEIGHT_ONE = 1 << 40

Params = namedtuple("Params", "temperature top_k top_p penalty")   # top_k 0: off, top_p 1.0: off, penalty 1.0: off
GRID = [
    Params(0.4, 50, 0.9, 1.0),
    Params(0.2, 50, 0.9, 1.0),
    Params(1.0, 50, 0.95, 1.05),
    Params(1.0, 0, 0.9, 1.0),
    Params(1.0, 0, 0.5, 1.3),
    Params(0.7, 5, 1.0, 1.0),
    Params(1.3, 0, 1.0, 1.0),
]
SCALES = (1, 8)
ROWS = (1, 3, 16)
VOCABS = (32000, 32003, 1000)
N_SEEN = 200
N_STEPS = 64

Ref = namedtuple("Ref", "support probs ambiguous z")
Measured = namedtuple("Measured", "n_wrong n_excused l1")

# worst Measured fields seen by check() in this process (how L1_BOUND was measured)
WORST = {"l1": 0.0, "n_excused": 0}

_M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3, SC'11): 4 counter words, 2 key words -> 4 words."""
    c0, c1, c2, c3 = (int(c) & _M32 for c in ctr)
    k0, k1 = (int(k) & _M32 for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _M32, p1 & _M32, ((p0 >> 32) ^ c3 ^ k1) & _M32, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def bitmap_to_bool(words, V):
    """[ (V+31)//32 ] int32 bitmap -> bool [V]"""
    w = np.asarray(words).astype(np.int64) & _M32
    return ((w[:, None] >> np.arange(32)[None, :]) & 1).astype(bool).reshape(-1)[:V]


def bool_to_bitmap(seen):
    seen = np.asarray(seen, dtype=bool)
    pad = np.zeros((len(seen) + 31) // 32 * 32, dtype=np.int64)
    pad[: len(seen)] = seen
    w = (pad.reshape(-1, 32) << np.arange(32)[None, :]).sum(1)
    return w.astype(np.uint32).view(np.int32)


def penalised(logits, seen, penalty):
    """Step 1 in fp32, the arithmetic of HF's processor and of the kernel: x < 0 ? x * pen : x / pen on the seen tokens."""
    x = np.asarray(logits, dtype=np.float32)
    if penalty == 1.0 or seen is None:
        return x
    pen = np.float32(penalty)
    return np.where(np.asarray(seen, dtype=bool), np.where(x < 0, x * pen, x / pen), x).astype(np.float32)


def ref_sample64(logits, seen, params):
    """Steps 1-5 of lhrs_sample_rows for one row.  The penalty and z = x / temperature are fp32 operations (both are in HF, and the top-k cut is
    exact only on bit-identical z); everything after is float64.  -> Ref(support bool [V], probs float64 [V] summing to 1 over the support,
    ambiguous bool [V]: top-p only, mass strictly above within TOP_P_BAND of top_p * total, z fp32 [V])."""
    z32 = (penalised(logits, seen, params.penalty) / np.float32(params.temperature)).astype(np.float32)
    z = z32.astype(np.float64)
    V = len(z)
    keep = np.ones(V, dtype=bool)
    if 0 < params.top_k < V:
        kth = np.sort(z)[V - params.top_k]
        keep = z >= kth                                   # ties at the cut stay (TopKLogitsWarper: scores < kth are removed)
    p = np.where(keep, np.exp(z - z.max()), 0.0)
    total = p.sum()
    ambiguous = np.zeros(V, dtype=bool)
    support = keep.copy()
    if params.top_p < 1.0:
        order = np.argsort(-z, kind="stable")
        zs, ps = z[order], p[order]
        excl = np.cumsum(ps) - ps
        above_sorted = excl[np.searchsorted(-zs, -zs, side="left")]   # equal values share the mass strictly above them
        above = np.empty(V)
        above[order] = above_sorted
        thr = float(np.float32(params.top_p)) * total
        support = keep & (above < thr)
        ambiguous = keep & (np.abs(above - thr) <= TOP_P_BAND * total)
    probs = np.where(support, p, 0.0)
    return Ref(support, probs / probs.sum(), ambiguous, z32)


def emulate_weights(logits, seen, params, support=None):
    """The reference pushed through the kernel's number formats: q = rint(exp_fp32(z - zmax) * 2^40) on the reference support, -1 elsewhere."""
    ref = ref_sample64(logits, seen, params)
    support = ref.support if support is None else support
    d = (ref.z - ref.z.max()).astype(np.float32)                # the maximum always survives
    q = np.rint(np.exp(d, dtype=np.float32).astype(np.float64) * float(WEIGHT_ONE)).astype(np.int64)
    return np.where(support, q, -1)


def draw_from_weights(weights, seed, step, row, sorted_order=False):
    """Step 6 on integers: R = (rand64 * W) >> 64, the first index, in index order, whose inclusive prefix sum of surviving weights exceeds R.
    sorted_order (a mutation for the comparator's own test): the prefix runs over the weights in descending order instead."""
    w = np.asarray(weights, dtype=np.int64)
    w = np.where(w > 0, w, 0)
    W = int(w.sum())
    o = philox4x32_10((int(step) & _M32, row, 0, 0), (int(seed) & _M32, (int(seed) >> 32) & _M32))
    R = ((o[0] | (o[1] << 32)) * W) >> 64
    if sorted_order:
        order = np.argsort(-w, kind="stable")
        return int(order[np.searchsorted(np.cumsum(w[order]), R, side="right")])
    return int(np.searchsorted(np.cumsum(w), R, side="right"))


def measure(weights, ref):
    """-> Measured(tokens whose survival differs from the reference without excuse, excused tokens, L1 over the non-excused tokens)"""
    w = np.asarray(weights, dtype=np.int64)
    got = w >= 0
    diff = got != ref.support
    excused = diff & ref.ambiguous
    W = float(np.where(got, w, 0).sum())
    frac = np.where(got, w, 0) / W if W > 0 else np.zeros(len(w))
    l1 = float(np.abs(frac - ref.probs)[~excused].sum())
    return Measured(int((diff & ~ref.ambiguous).sum()), int(excused.sum()), l1)


def check(weights, ref, token=None, seed=None, step=None, row=None, what=""):
    """Asserts (a) support, (b) distribution and, when a token is given, (c) the draw; returns what it measured."""
    m = measure(weights, ref)
    WORST["l1"] = max(WORST["l1"], m.l1)
    WORST["n_excused"] = max(WORST["n_excused"], m.n_excused)
    assert m.n_wrong == 0, f"{what}: {m.n_wrong} tokens survive / are removed against the reference"
    assert m.n_excused <= MAX_EXCUSED, f"{what}: {m.n_excused} tokens at the top-p cut differ"
    assert m.l1 <= L1_BOUND, f"{what}: L1 {m.l1:.3e} > {L1_BOUND:.1e}"
    if token is not None:
        want = draw_from_weights(weights, seed, step, row)
        assert int(token) == want, f"{what}: token {int(token)}, the draw from its own weights gives {want} (step {step}, row {row})"
    return m


def hf_support(logits, seen_ids, params):
    """Support of the installed transformers' processors applied in HF's order (CPU)."""
    import torch
    from transformers.generation.logits_process import (RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper,
                                                        TopPLogitsWarper)

    s = torch.as_tensor(np.asarray(logits, dtype=np.float32))[None].clone()
    ids = torch.as_tensor(np.asarray(seen_ids, dtype=np.int64))[None]
    if params.penalty != 1.0:
        s = RepetitionPenaltyLogitsProcessor(params.penalty)(ids, s)
    if params.temperature != 1.0:
        s = TemperatureLogitsWarper(params.temperature)(ids, s)
    if 0 < params.top_k:
        s = TopKLogitsWarper(params.top_k)(ids, s)
    if params.top_p < 1.0:
        s = TopPLogitsWarper(params.top_p)(ids, s)
    return torch.isfinite(s)[0].numpy()


def make_logits(n, V, scale, seed):
    import torch

    return (torch.randn(n, V, generator=torch.Generator().manual_seed(seed)) * scale).float()


def make_seen(n, V, seed):
    """bool [n, V] with N_SEEN random bits per row"""
    rng = np.random.default_rng(seed)
    seen = np.zeros((n, V), dtype=bool)
    for r in range(n):
        seen[r, rng.choice(V, size=min(N_SEEN, V), replace=False)] = True
    return seen
