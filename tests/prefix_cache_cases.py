"""Keeping the KV cache across chat turns (generation.match_prefix / PrefixCache, generate(prefix_cache=...)), restated for
tests/test_prefix_cache_cpu.py and tests/test_prefix_cache_gpu.py.  Shares no code with lhrs_bot_amd.

Matching.  A prompt is a list of ids in placeholder form: IMG (-200) is one entry and stands for NI cache positions.  The reusable part of
a cached sequence is the longest common prefix of the two lists, where the placeholder matches only if both calls had the same image, cut
so that at least one position of the new prompt is left to prefill; a cut never falls inside the image block.  `brute` counts the same on
the EXPANDED sequences, position by position, and moves a cut out of the block.

Dequantisation.  kv8_dequant_rows gives e4m3(code) * 2^(byte - 127) rounded to bf16.  `exact_products` checks what the GPU test relies on:
for the scale bytes it uses, the float64 product, its float32 value and its bf16 rounding are one number."""
import random

import torch

import kv8_cases as kv

IMG = -200
NIS = (4, 144)


def positions(ids, NI):
    return sum(NI if t == IMG else 1 for t in ids)


def expand(ids, NI, image):
    """placeholder form -> one entry per cache position; an image position is (image identity, index in the block)"""
    out = []
    for t in ids:
        out += [(image, k) for k in range(NI)] if t == IMG else [t]
    return out


def brute(cached, new, NI, image_same):
    """-> positions reusable, counted on the expanded sequences"""
    a, b = expand(cached, NI, "A"), expand(new, NI, "A" if image_same else "B")
    p = 0
    while p < min(len(a), len(b)) and a[p] == b[p]:
        p += 1
    if p == len(b) and p > 0:
        p -= 1                                       # one position is always prefilled
    if IMG in new:
        start = new.index(IMG)                        # every entry before the placeholder is one position
        if start < p < start + NI:
            p = start                                # never inside the block
    return p


def inside_block(new, NI, p):
    if IMG not in new:
        return False
    start = new.index(IMG)
    return start < p < start + NI


# name, cached, new, image_same, tokens reused, positions reused as a function of NI
CASES = [
    ("extended by new tokens", [1, IMG, 5, 6, 7], [1, IMG, 5, 6, 7, 8, 9], True, 5, lambda NI: 4 + NI),
    ("same prompt again", [1, IMG, 5, 6, 7], [1, IMG, 5, 6, 7], True, 4, lambda NI: 3 + NI),
    ("new prompt is a strict prefix of the cache", [1, IMG, 5, 6, 7, 8], [1, IMG, 5, 6], True, 3, lambda NI: 2 + NI),
    ("divergence in the text after the image", [1, IMG, 5, 6, 7, 8], [1, IMG, 5, 6, 9, 8, 3], True, 4, lambda NI: 3 + NI),
    ("divergence on the first token after the image", [1, IMG, 5, 6], [1, IMG, 9, 6], True, 2, lambda NI: 1 + NI),
    ("a different image", [1, IMG, 5, 6], [1, IMG, 5, 6, 7], False, 1, lambda NI: 1),
    ("a different image, two tokens in front", [1, 2, IMG, 5], [1, 2, IMG, 5, 6], False, 2, lambda NI: 2),
    ("divergence before the image", [1, 2, IMG, 5], [1, 3, IMG, 5], True, 1, lambda NI: 1),
    ("no common prefix", [1, IMG, 5], [2, IMG, 5], True, 0, lambda NI: 0),
    ("empty cache", [], [1, IMG, 5], True, 0, lambda NI: 0),
    ("no placeholder, extended", [1, 5, 6], [1, 5, 6, 7], True, 3, lambda NI: 3),
    ("no placeholder, same again", [1, 5, 6], [1, 5, 6], True, 2, lambda NI: 2),
    ("no placeholder in the cache, one in the prompt", [1, 5, 6], [1, IMG, 6], True, 1, lambda NI: 1),
    ("the prompt ends with the cached placeholder", [1, IMG, 5], [1, IMG], True, 1, lambda NI: 1),
    ("one-token prompt that is cached", [1, IMG], [1], True, 0, lambda NI: 0),
]


def random_pairs(n=200, seed=0):
    """(cached, new, image_same): a shared stem, then two tails that may or may not diverge; small alphabet so that tails collide"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        def seq(k):
            return [rng.randint(1, 3) for _ in range(k)]
        stem = seq(rng.randint(0, 4))
        if rng.random() < 0.8:
            stem.insert(rng.randint(0, len(stem)), IMG)
        a, b = stem + seq(rng.randint(0, 3)), stem + seq(rng.randint(0, 3))
        if IMG not in stem and rng.random() < 0.3:
            b.insert(rng.randint(0, len(b)), IMG)
        out.append((a, b[:rng.randint(1, len(b))] if b and rng.random() < 0.3 else b, rng.random() < 0.7))
    return out


BYTES = (10, 100, 127, 200, 240)


def exact_products():
    """every non-NaN code x BYTES -> (float64 products [n, 1, 256 - 2], ...): asserts product == fp32(product) == bf16(product)"""
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=kv.U8)
    worst = 0
    for byte in BYTES:
        want = kv.dequant(codes[None], torch.tensor([byte], dtype=kv.U8))[0]
        assert bool(torch.isfinite(want).all())
        f32 = (kv.code_values(codes).float() * torch.exp2(torch.tensor(float(byte - 127), dtype=kv.F32))).double()
        assert torch.equal(f32, want), byte                                          # the product of the kernel, formed in fp32
        assert torch.equal(want.float().double(), want), byte                        # ... is the float64 one
        assert torch.equal(want.to(kv.BF).double(), want), byte                      # ... and bf16 holds it
        worst += 1
    return len(codes) * worst
