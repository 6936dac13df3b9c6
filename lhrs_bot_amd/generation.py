"""Single-token decoding and generation for `TextModal` (text.py binds the functions below under their `TextModal` names): FORMATS, the one
table of what `generate(weights=...)` can stream; PrefixCache, the KV cache of a conversation kept between calls; DecodeSession, the static
buffers and launch list of one single-token step; the token loops."""
import contextlib
import dataclasses
import math
import os
from typing import Callable, Optional

import torch

from . import kernels as hk

WEIGHT_NAMES = ("qkv_w", "o_w", "gu_w", "down_w")   # the fused decoder linears of a layer dict


# ------------------------------------------------------------------------------------------------- the weight formats
@dataclasses.dataclass
class WeightFormat:
    """One entry of FORMATS: what `generate(weights=...)` streams through the decoder linears of the single-token step."""
    operand: str                     # L[<weight name> + operand] is what the step streams ...
    pack_weight: Callable            # ... made by pack_weight(L, <weight name>) for every layer, at the first session that needs it
    acts: str                        # the activation side, and with it the linear (`linear`) and its static operand buffers (`buffers`)
    kernels: tuple                   # names of the hk wrappers of that linear
    scale: Optional[str] = None      # suffix of the per-row scales that go with the operand
    check: Callable = lambda m, pack: None   # -> error text on a model it cannot serve; pack: asked by the public pack method, not by generate()
    optional: bool = False           # the row-major weight streams as it is; the operand is made and read from batch 2 only ("bf16")
    own_head: bool = False           # lm_head has this form too; otherwise the "bf16" entry serves it, whatever the decoder streams
    stages: bool = True              # from batch 4 RMSNorm / SwiGLU may run once into s.hn / s.actb, not once per block of the weight stream
    int8_gemm: bool = False          # prefill and the batch > 16 step run the LLM.int8 products: the whole call is in that arithmetic

    def pack(self, m) -> None:
        err = self.check(m, True)
        if err:
            raise ValueError(err)
        if self.scale and "qkv_w" + self.scale not in m.p["layers"][0]:   # only "fp8" can lack them: int8's scales ARE its base (checked above)
            quantize_fp8(m)
        for L in m.p["layers"]:
            for k in WEIGHT_NAMES:
                L[k + self.operand] = self.pack_weight(L, k)
        if self.own_head:
            m.p["lm_head" + self.operand] = self.pack_weight(m.p, "lm_head")

    def ensure(self, m, packed16) -> None:
        """lazy packing, at the first session that needs it"""
        if (packed16 or not self.optional) and "qkv_w" + self.operand not in m.p["layers"][0]:
            self.pack(m)
        if packed16 and "lm_headp" not in m.p:  # lm_head alone: pack_bf16_decode() would add 13.5 GB of re-tiled decoder weights that this mode never reads
            m.p["lm_headp"] = hk.repack_bf16_mfma(m.p["lm_head"])

    def weight(self, L, name, packed16):
        """(weight, per-row scales or None) of L[name]; `L` may be the parameter dict itself and `name` "lm_head" """
        return L[name + (self.operand if packed16 or not self.optional else "")], (L[name + self.scale] if self.scale else None)

    def buffers(self, s) -> None:
        dev, B = s.m.device, s.B
        if self.acts == "e4m3":   # operands of the block-scaled MFMA: (codes, per-row scale) of both activation widths (graph capture: no allocation)
            s.x8 = (torch.zeros((B, s.m.d), device=dev, dtype=torch.uint8), torch.zeros(B, device=dev, dtype=torch.float32))
            s.a8 = (torch.zeros((B, s.m.ff), device=dev, dtype=torch.uint8), torch.zeros(B, device=dev, dtype=torch.float32))
        elif self.acts == "int8":
            s.i8ws = hk.Int8DecodeWorkspace(dev, B, max(s.m.d, s.m.ff), s.m._i8ws.threshold if s.m._i8ws is not None else 6.0)

    def linear(self, s, w, sc, x, out, K, pro, norm_w, **o):
        """out = pro(x) W^T (+ residual) on session `s`; o: residual, out_f32.  The "bf16" entry also runs as the HEAD format of the other formats'
        sessions: what it reads from `s` (`batched` behind `staged`) is set by the session's own format, whose `stages` must suit both."""
        k0, k1 = (getattr(hk, k) for k in self.kernels)
        ws = (w,) if sc is None else (w, sc)
        if self.acts == "int8":   # prologue, outlier split and quantisation in one launch, then the int8 weight stream
            k0(x, K, s.i8ws, prologue=pro, norm_w=norm_w, eps=s.m.eps)
            k1(w, sc, s.i8ws, out, K, **o)
        elif self.acts == "bf16":  # prologue inside the GEMV, or materialised once (`staged`)
            x, pro, norm_w = s.staged(x, pro, norm_w)
            k0(w, x, out, K, prologue=pro, norm_w=norm_w, eps=s.m.eps, **o)
        elif s.B <= 2:            # e4m3: prologue + activation quantisation inside the GEMV (five launches per layer) ...
            k0(*ws, x, out, K, prologue=pro, norm_w=norm_w, eps=s.m.eps, **o)
        else:                     # ... above batch 2 the quantising producer of the prologue, then the GEMV
            k1(*ws, *s.quantised(x, K, pro, norm_w), out, **o)


def quantize_fp8(m):
    for L, k in [(L, k) for L in m.p["layers"] for k in WEIGHT_NAMES] + [(m.p, "lm_head")]:
        L[k + "8"], L[k + "8s"] = hk.quant_fp8_rows(L[k])


def _check_int8(m, pack):
    if (pack and not m.p["layers"]) or "qkv_wi8" not in m.p["layers"][0]:
        return NO_BASE["int8"][pack]
    if not pack and (m.d % 64 or m.ff % 64 or max(m.d, m.ff) > 16384):
        return f'weights="int8" needs hidden sizes that are multiples of 64 (the MFMA step) and at most 16384, got {m.d} and {m.ff}'


def int8_gemm(weights) -> bool:   # False for a `weights` the table does not know: that is rejected where the session is built
    return weights in FORMATS and FORMATS[weights].int8_gemm


NO_BASE = {  # format -> (text of generate(weights=...), text of the public pack method) on a model without the base it streams
    "4bit": ('weights="4bit" needs the 4-bit base: quantize_base(4, quant_type, double_quant) (YAML `bits: 4`)',
             "pack4_decode: the decoder is not on the 4-bit base - call quantize_base(4, quant_type, double_quant) first"),
    "int8": ('weights="int8" needs the LLM.int8 base: quantize_base(8, "int8") (YAML `bits: 8`)',
             'pack_int8_decode: the decoder is not on the LLM.int8 base - call quantize_base(8, "int8") first')}
FORMATS = {  # lm_head is quantised in no base of the reference: it streams bf16 in every format but "fp8"
    "bf16": WeightFormat("p", lambda L, k: hk.repack_bf16_mfma(L[k]), "bf16", ("gemv_fused", "gemv_fused"), optional=True, own_head=True),
    "fp8": WeightFormat("8p", lambda L, k: hk.repack_fp8_mfma(L[k + "8"]), "e4m3", ("gemv_fp8_mfma_fused", "gemv_fp8_mfma"), scale="8s", own_head=True, stages=False),
    "4bit": WeightFormat("4p", lambda L, k: hk.pack4_decode(L[k + "q4"], *L[k].shape), "bf16", ("gemv4", "gemv4"),
                         check=lambda m, pack: None if m.base4 else NO_BASE["4bit"][pack]),
    "mxfp4": WeightFormat("mx4", lambda L, k: hk.repack_mx4_mfma(*hk.quant_mx4_rows(L[k])), "e4m3", ("gemv_mx4_fused", "gemv_mx4"), check=lambda m, pack: None
                          if pack or not (m.d % 128 or m.ff % 128) else f'weights="mxfp4" needs hidden sizes that are multiples of 128 (the MFMA step), got {m.d} and {m.ff}'),
    "int8": WeightFormat("i8p", lambda L, k: hk.repack_int8_mfma(L[k + "i8"]), "int8", ("int8_decode_prepare", "gemv_int8"), scale="i8s", check=_check_int8, int8_gemm=True),
}
DECODE_SUFFIXES = tuple(f.operand for f in FORMATS.values())   # the `<weight name><suffix>` keys the packers create (`quantize_fp8`: "8", "8s")


def check_kv_cache(m, kv_cache, rows, num_beams=1):
    """generate(kv_cache=...), "fp8" = the kv8 format of csrc/decode_attn.hip: what it cannot serve raises here, before anything is allocated"""
    if kv_cache not in ("bf16", "fp8"):
        raise ValueError(f"kv_cache={kv_cache!r}: expected 'bf16' or 'fp8'")
    if kv_cache == "bf16":
        return
    if m.hd != 128:
        raise ValueError(f'kv_cache="fp8" needs head_dim 128 (one scale byte per 128-value head row), this model has head_dim {m.hd}')
    if rows > 16:
        raise ValueError(f'kv_cache="fp8" with batch (x num_beams) {rows} > 16: beyond 16 rows the single-token step attends through attn_fwd '
                         'over bf16 caches, which the fp8 cache does not have')
    if num_beams > 1 and m.heads % 16:
        raise ValueError(f'kv_cache="fp8" with num_beams > 1 needs a head count that is a multiple of 16 (kv_beam_reorder moves the scale '
                         f'bytes of a position in 16-byte chunks), this model has {m.heads} heads')


def alloc_kv(m, rows, kv_cache):
    """per layer: (K, V) bf16 [rows, d], or for kv_cache="fp8" (K codes, V codes uint8 [rows, d], K scales, V scales uint8 [rows, H])"""
    def t(cols, dtype):
        return torch.empty((rows, cols), device=m.device, dtype=dtype)
    if kv_cache == "fp8":
        return [(t(m.d, torch.uint8), t(m.d, torch.uint8), t(m.heads, torch.uint8), t(m.heads, torch.uint8)) for _ in m.p["layers"]]
    return [(t(m.d, torch.bfloat16), t(m.d, torch.bfloat16)) for _ in m.p["layers"]]


# ------------------------------------------------------------------------------------------------- the cache of a conversation
IMAGE_PLACEHOLDER = -200   # IMAGE_TOKEN_INDEX of text.py (which imports this module)


def match_prefix(cached_ids, new_ids, NI, image_same):
    """How much of a cached sequence a new prompt can reuse -> (tokens, positions).  Both are Python lists of ids in placeholder form: the
    <image> placeholder (-200) is one entry and stands for NI cache positions.  The answer is the longest common prefix, with two rules:
    the cut never falls inside the image block - the placeholder is reused whole, and only if `image_same` (the cached block came from the
    image embedding of the new call) - and at least one position is left to prefill (its logits pick the first token): a new prompt that
    is cached entirely is reused up to its last entry, which for a trailing placeholder is the whole block."""
    tokens = positions = 0
    for a, b in zip(cached_ids, new_ids):
        if a != b or (a == IMAGE_PLACEHOLDER and not image_same):
            break
        tokens, positions = tokens + 1, positions + (NI if a == IMAGE_PLACEHOLDER else 1)
    if tokens == len(new_ids) and tokens > 0:
        tokens, positions = tokens - 1, positions - (NI if new_ids[-1] == IMAGE_PLACEHOLDER else 1)
    return tokens, positions


class PrefixCache:
    """The KV cache of ONE conversation (batch 1) of one model, kept between `generate(prefix_cache=...)` calls: from `new_prefix_cache` of
    `TextModal` / `UniBind`.  `caches`: `alloc_kv(max_positions, kv_cache)`, made at the first call (None before); `ids`: what the first
    `length` positions hold, in placeholder form (Python list); `image_embedding`: the image block behind the placeholder, and `pixels` a
    host copy of the pixel tensor it was encoded from (`UniBind.generate` keeps both, and skips the encoder when the pixels come again);
    `last_reused` / `last_prefilled`: positions of the most recent call.  Memory: max_positions x d x 2 (K, V) x layers x 2 B ("bf16"), or
    1 B + 1/128 B ("fp8": codes and one scale byte per head row of 128), held as long as the object lives."""

    def __init__(self, model_text, kv_cache="bf16", max_positions=None):
        check_kv_cache(model_text, kv_cache, 1)
        table = int(model_text.cos.shape[0])
        self.model, self.kv_cache, self.max_positions = model_text, kv_cache, table if max_positions is None else int(max_positions)
        if not 1 <= self.max_positions <= table:
            raise ValueError(f"max_positions={max_positions!r}: from 1 to the {table} positions of the RoPE table")
        self.caches = None
        self.reset()

    def reset(self):
        """forget the conversation (the cache tensors stay allocated)"""
        self.ids, self.length, self.image_embedding, self.pixels = [], 0, None, None
        self.last_reused = self.last_prefilled = 0

    def check(self, m, input_ids, attention_mask, num_beams, kv_cache, max_new_tokens, NI):
        """What a call with this cache cannot be raises here, before anything is allocated or changed.  kv_cache: the call's argument or
        None; NI: positions of the image block of this call (None: no embedding yet, the placeholder then counts as one position)."""
        if m is not self.model:
            raise ValueError(f"prefix_cache belongs to another model ({type(self.model).__name__} at {id(self.model):#x}, this one is at {id(m):#x})")
        if kv_cache is not None and kv_cache != self.kv_cache:
            raise ValueError(f"kv_cache={kv_cache!r} disagrees with the prefix cache, which holds kv_cache={self.kv_cache!r}")
        if input_ids.dim() != 2 or int(input_ids.shape[0]) != 1:
            raise ValueError(f"prefix_cache holds one conversation: batch 1, got input_ids of shape {tuple(input_ids.shape)}")
        if int(num_beams) != 1:
            raise ValueError(f"prefix_cache with num_beams={num_beams!r}: beam search replicates and reorders the cache rows, it starts from an empty cache")
        if attention_mask is not None and not bool(attention_mask.bool().all()):
            raise ValueError(f"prefix_cache with an attention_mask that hides {int((~attention_mask.bool()).sum())} positions: cached positions "
                             "are all visible (no padding)")
        ids = input_ids[0].tolist()
        n_img = ids.count(IMAGE_PLACEHOLDER)
        if n_img > 1:
            raise ValueError(f"prefix_cache with {n_img} <image> placeholders in the prompt: one image per conversation")
        S0 = len(ids) + n_img * ((NI or 1) - 1)
        if S0 + int(max_new_tokens) > self.max_positions:
            raise ValueError(f"prompt ({S0}) + max_new_tokens ({max_new_tokens}) exceeds the {self.max_positions} positions of the prefix cache")
        return ids

    def begin(self, ids, image_embedding):
        """Start a call whose prompt is `ids` with image block `image_embedding` (or None): -> the positions it reuses.  The cache is rolled
        back to them HERE, before the prefill writes anything: a call that dies half way leaves a valid, shorter cache."""
        old = self.image_embedding
        same = image_embedding is None or image_embedding is old or (old is not None and old.shape == image_embedding.shape and
                                                                     bool(torch.equal(old, image_embedding)))
        NI = 1 if image_embedding is None else int(image_embedding.shape[1])
        tokens, reuse = match_prefix(self.ids, ids, NI, same)
        self.ids, self.length = self.ids[:tokens], reuse
        if not same:
            self.image_embedding, self.pixels = image_embedding, None
        if self.caches is None:
            self.caches = alloc_kv(self.model, self.max_positions, self.kv_cache)
        return reuse

    def commit(self, ids, new_ids, S0, reuse):
        """the call emitted `new_ids` behind the prompt `ids` of S0 positions: every token but the last was fed, and is cached"""
        self.ids, self.length = list(ids) + list(new_ids[:-1]), S0 + len(new_ids) - 1
        self.last_reused, self.last_prefilled = reuse, S0 - reuse


# ------------------------------------------------------------------------------------------------- constrained decoding
class TokenAutomaton:
    """A deterministic automaton over token ids for `generate(constraint=...)`, in CSR form on the device (all int32): `off`
    [n_states + 1] edge ranges, `tok` [E] edge tokens - ascending and unique inside a state -, `nxt` [E] target states, `label` [n_states]
    -1 or the caller's index of a final state.  State 0 is the start; a state without out-edges is final.  `pad_token_id` is what rows
    behind a final state emit, `V` the vocabulary size the tokens were validated for.  Built by `from_edges` (which validates),
    `choice_automaton` or `vocab_loop_automaton`; `hk.constrain_rows` walks it."""

    def __init__(self, off, tok, nxt, label, pad_token_id, V):
        self.off, self.tok, self.nxt, self.label, self.pad_token_id, self.V = off, tok, nxt, label, int(pad_token_id), int(V)

    n_states = property(lambda self: int(self.label.numel()))
    n_edges = property(lambda self: int(self.tok.numel()))
    device = property(lambda self: self.off.device)

    @classmethod
    def from_edges(cls, off, tok, nxt, label, pad_token_id, V, device="cpu"):
        """Host arrays (anything `numpy.asarray` takes) -> the automaton on `device`.  Everything the kernel relies on is checked HERE, before
        anything is uploaded; cycles are allowed (max_new_tokens bounds the walk)."""
        import numpy as np

        def ints(a, name):
            a = np.asarray(a)
            if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
                raise ValueError(f"TokenAutomaton: {name} must be a 1-d integer array, got shape {a.shape} of {a.dtype}")
            return a.astype(np.int64)
        off, tok, nxt, label = ints(off, "off"), ints(tok, "tok"), ints(nxt, "nxt"), ints(label, "label")
        V, n_states, E = int(V), int(label.size), int(tok.size)
        if n_states < 1 or off.size != n_states + 1 or nxt.size != E:
            raise ValueError(f"TokenAutomaton: {n_states} labels need {n_states + 1} offsets (got {off.size}) and one target per edge "
                             f"({E} tokens, {nxt.size} targets)")
        if not 1 <= V <= 32768:
            raise ValueError(f"TokenAutomaton: V={V}: hk.constrain_rows serves 1..32768 tokens")
        if E >= 1 << 31 or not -(1 << 31) <= int(pad_token_id) < 1 << 31 or (label.size and (label.min() < -(1 << 31) or label.max() >= 1 << 31)):
            raise ValueError("TokenAutomaton: edge count, labels and pad_token_id must fit int32")
        if off[0] != 0 or off[-1] != E or bool((np.diff(off) < 0).any()):
            raise ValueError(f"TokenAutomaton: offsets must rise monotonically from 0 to the {E} edges, got {off[:8].tolist()}... ending in {int(off[-1])}")
        if E and (tok.min() < 0 or tok.max() >= V):
            raise ValueError(f"TokenAutomaton: edge tokens must be in [0, {V}), got {int(tok.min())}..{int(tok.max())}")
        if E and (nxt.min() < 0 or nxt.max() >= n_states):
            raise ValueError(f"TokenAutomaton: edge targets must be states in [0, {n_states}), got {int(nxt.min())}..{int(nxt.max())}")
        if off[1] == 0:
            raise ValueError("TokenAutomaton: state 0, the start, has no edge")
        inner = np.ones(E, dtype=bool)           # edges that have a predecessor in the same state
        inner[off[:-1][off[:-1] < E]] = False
        bad = np.nonzero(inner[1:] & (tok[1:] <= tok[:-1]))[0]
        if bad.size:
            e = int(bad[0]) + 1
            raise ValueError(f"TokenAutomaton: the edge tokens of a state must be ascending and unique (the tie rule is the lowest token): "
                             f"state {int(np.searchsorted(off, e, side='right')) - 1} has {int(tok[e - 1])} before {int(tok[e])}")
        def up(a):
            t = torch.from_numpy(a.astype(np.int32))
            return hk.h2d(t, device) if torch.device(device).type == "cuda" else t
        return cls(up(off), up(tok), up(nxt), up(label), pad_token_id, V)


def choice_automaton(token_lists, eos_token_id, pad_token_id, V, device="cpu"):
    """The trie of the given token-id sequences, each followed by `eos_token_id`: the final state behind choice i has label i.  A choice
    may be a strict prefix of another (the EOS edge tells them apart); duplicate or empty choices raise ValueError."""
    lists = [[int(t) for t in c] for c in token_lists]
    if not lists:
        raise ValueError("choice_automaton: no choices")
    children, label, seen = [{}], [-1], {}
    for i, c in enumerate(lists):
        if not c:
            raise ValueError(f"choice_automaton: choice {i} is empty")
        if tuple(c) in seen:
            raise ValueError(f"choice_automaton: choices {seen[tuple(c)]} and {i} are the same token sequence {c}")
        if int(eos_token_id) in c:
            raise ValueError(f"choice_automaton: choice {i} contains the EOS token {eos_token_id}, which ends a choice")
        seen[tuple(c)] = i
        s = 0
        for t in c + [int(eos_token_id)]:
            if t not in children[s]:
                children.append({})
                label.append(-1)
                children[s][t] = len(children) - 1
            s = children[s][t]
        label[s] = i
    off, tok, nxt = [0], [], []
    for ch in children:
        for t in sorted(ch):
            tok.append(t)
            nxt.append(ch[t])
        off.append(len(tok))
    return TokenAutomaton.from_edges(off, tok, nxt, label, pad_token_id, V, device)


def vocab_loop_automaton(V, eos_token_id=None, pad_token_id=0, device="cpu"):
    """One state whose V edges loop to itself: the pick is then plain greedy.  With an EOS that edge leads to a final state (label 0)
    instead, which gives greedy decoding its EOS handling on the device."""
    import numpy as np
    tok, nxt = np.arange(int(V), dtype=np.int64), np.zeros(int(V), dtype=np.int64)
    if eos_token_id is None:
        return TokenAutomaton.from_edges([0, V], tok, nxt, [-1], pad_token_id, V, device)
    if not 0 <= int(eos_token_id) < int(V):
        raise ValueError(f"vocab_loop_automaton: eos_token_id={eos_token_id} is outside [0, {V})")
    nxt[int(eos_token_id)] = 1
    return TokenAutomaton.from_edges([0, V, V], tok, nxt, [-1, 0], pad_token_id, V, device)


def _same_device(a, b) -> bool:
    a, b = torch.device(a), torch.device(b)
    index = lambda d: d.index if d.index is not None or d.type != "cuda" else torch.cuda.current_device()  # noqa: E731
    return a.type == b.type and index(a) == index(b)


def check_constraint(m, constraint, return_choices=False, do_sample=False, num_beams=1, repetition_penalty=1.0, prefix_cache=None):
    """generate(constraint=..., return_choices=...): what the constrained pick cannot be raises here, before anything is allocated"""
    if constraint is None:
        if return_choices:
            raise ValueError("return_choices=True needs a constraint: the choice is the label of the automaton's final state")
        return
    if not isinstance(constraint, TokenAutomaton):
        raise ValueError(f"constraint={type(constraint).__name__}: expected a TokenAutomaton (choice_constraint / choice_automaton / from_edges)")
    for bad, why in ((do_sample, "constraint with do_sample=True: the constrained pick is greedy (the best allowed token)"),
                     (int(num_beams) != 1, f"constraint with num_beams={num_beams!r}: beams over an automaton are not implemented"),
                     (float(repetition_penalty) != 1.0, f"constraint with repetition_penalty={repetition_penalty!r}: the penalty lives in the sampling kernel, "
                                                        "which knows no automaton"),
                     (prefix_cache is not None, "constraint with prefix_cache: the pads behind a final state must not enter a kept cache"),
                     (constraint.V != m.vocab, f"the constraint was validated for a vocabulary of {constraint.V}, the model has {m.vocab}")):
        if bad:
            raise ValueError(why)
    if not _same_device(constraint.device, m.device):
        raise ValueError(f"the constraint lives on {constraint.device}, the model on {m.device}")


# ------------------------------------------------------------------------------------------------- the GEMM step (prefill, batch > 16)
def layer_step(m, L, x, B, S_new, ctx, cache, desc, max_ctx, kmask=None, li=None, int8=False, scratch=None):
    """One decoder layer over S_new new positions per sequence behind `ctx` cached ones (prefill: ctx = 0).  li = the layer's index, under
    adapters="live" or int8: the linears are the training forward's (`_lin` / `_gu_fwd`; dropout is off) - adapters on the bf16 base weights,
    or with int8 (weights="int8" only) `hk.int8_linear` on the int8 rows with the adapters of a live store on top.  Which of the two `_lin`
    runs is the model's scheme (`m.base`: generate() has put the bf16 one in unless weights="int8"); `int8` is the caller's word for it.

    The e4m3 cache (four tensors) behind a context, ctx > 0 (generate(prefix_cache=...)): `scratch` = two bf16 tensors [B * (ctx + S_new), d]
    of the caller (`gemm_logits` makes them once for all layers).  The `ctx` cached K / V rows are dequantised into them
    (`hk.kv8_dequant_rows`: exact), the bf16 rows of the new positions copied behind, and `attn_fwd` - the kernel of the bf16 path - runs
    over the scratch (desc: kv_off = b * (ctx + S_new), kv_len = ctx + S_new, causal offset ctx).  The rule: the new positions attend EACH
    OTHER in exact bf16, as the positions of any prompt do, and the cached positions THROUGH THE CODES, as the single-token step does."""
    d, H, hd, ff = m.d, m.heads, m.hd, m.ff
    M = x.shape[0]
    assert li is None or int8 == m.base_int8, "layer_step(int8=...) and the model's base scheme disagree"
    h = hk.rmsnorm_fwd(x, L["ln1_w"], m.eps)
    if li is None:
        qkv = hk.gemm_rope_fwd(h, L["qkv_w"], m.cos, m.sin, pos_mod=S_new, pos0=ctx, rope_cols=2 * d, head_dim=hd)
    else:
        qkv = m._lin(li, "qkv", h, L, rope=(S_new, ctx))
    o = torch.empty((M, d), device=m.device, dtype=torch.bfloat16)
    if len(cache) == 4:
        # kv_cache="fp8", prefill: attention reads the exact bf16 K / V of the prompt straight out of `qkv` (desc: kv_off = b * S_new),
        # so the prompt's logits are those of the bf16-cache mode bit for bit; the rows enter the cache as codes + scale bytes.
        # Behind a context (ctx > 0) the cached rows are read back through the caller's scratch; without one there is no such step
        assert ctx == 0 or scratch is not None, "the kv8 cache has no multi-row step after the prefill (generate() rejects batch > 16)"
        kc8, vc8, ks, vs = cache
        if ctx == 0:
            hk.attn_fwd(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], o, None, desc, B, H, hd, S_new, 1 << 30, hk.pad64(S_new), True,
                        1.0 / math.sqrt(hd), key_mask=kmask)
        else:
            kb, vb = scratch
            row_b, n = d * 2, ctx + S_new
            for b in range(B):
                src = qkv.data_ptr() + b * S_new * 3 * row_b
                hk.kv8_dequant_rows(kc8, ks, b * max_ctx, ctx, H, kb[b * n:(b + 1) * n])
                hk.kv8_dequant_rows(vc8, vs, b * max_ctx, ctx, H, vb[b * n:(b + 1) * n])
                hk.copy_2d(kb.data_ptr() + (b * n + ctx) * row_b, row_b, src + row_b, 3 * row_b, row_b, S_new)
                hk.copy_2d(vb.data_ptr() + (b * n + ctx) * row_b, row_b, src + 2 * row_b, 3 * row_b, row_b, S_new)
            hk.attn_fwd(qkv[:, :d], kb, vb, o, None, desc, B, H, hd, S_new, 1 << 30, hk.pad64(S_new), True, 1.0 / math.sqrt(hd), key_mask=kmask)
        for b in range(B):
            rows = qkv[b * S_new:(b + 1) * S_new]
            hk.kv8_quant_rows(rows[:, d:2 * d], kc8, ks, b * max_ctx + ctx, H)
            hk.kv8_quant_rows(rows[:, 2 * d:], vc8, vs, b * max_ctx + ctx, H)
    else:
        kc, vc = cache
        row_b = d * 2
        for b in range(B):  # append the new K / V rows of sequence b at position ctx of its cache
            src = qkv.data_ptr() + b * S_new * 3 * row_b
            hk.copy_2d(kc.data_ptr() + (b * max_ctx + ctx) * row_b, row_b, src + row_b, 3 * row_b, row_b, S_new)
            hk.copy_2d(vc.data_ptr() + (b * max_ctx + ctx) * row_b, row_b, src + 2 * row_b, 3 * row_b, row_b, S_new)
        hk.attn_fwd(qkv[:, :d], kc, vc, o, None, desc, B, H, hd, S_new, 1 << 30, hk.pad64(S_new), True, 1.0 / math.sqrt(hd), key_mask=kmask)
    if li is not None:   # the fused gate|up + SwiGLU GEMM of the training forward; the arm below runs gemm_nt + swiglu_fwd (different kernels)
        x = m._lin(li, "o", o, L, residual=x)
        h = hk.rmsnorm_fwd(x, L["ln2_w"], m.eps, out=h)
        _, act, _ = m._gu_fwd(li, h, L, None)
        return m._lin(li, "down", act, L, residual=x)
    x = hk.gemm_nt(o, L["o_w"], residual=x)
    h = hk.rmsnorm_fwd(x, L["ln2_w"], m.eps, out=h)
    act = hk.swiglu_fwd(hk.gemm_nt(h, L["gu_w"]), ff)
    return hk.gemm_nt(act, L["down_w"], residual=x)


def gemm_logits(m, x, B, S, ctx, caches, row_stride, kv8, kmask, lora, weights):
    """S new positions per sequence (rows of x) behind `ctx` cached ones through the GEMM path -> fp32 logits [B, V] of the last one: the
    prefill (ctx = 0) and the step of a batch > 16.  Sequence b owns the cache rows from b * row_stride (`num_beams * max_ctx` under beams).
    kv8: the attention reads K / V out of the qkv buffer itself, where sequence b starts at row b * S (prefill), or behind a context out of
    two bf16 scratch tensors made here for all layers, where sequence b starts at row b * (ctx + S) (see `layer_step`)."""
    i8 = int8_gemm(weights)
    desc = hk.make_desc([(b * S, S, b * (ctx + S if kv8 else row_stride), ctx + S, ctx + S, ctx) for b in range(B)], m.device)
    step_kw = {}
    if kv8 and ctx > 0:
        step_kw["scratch"] = tuple(torch.empty((B * (ctx + S), m.d), device=m.device, dtype=torch.bfloat16) for _ in range(2))
    for li, (L, cache) in enumerate(zip(m.p["layers"], caches)):
        x = m._layer_step(L, x, B, S, ctx, cache, desc, row_stride, kmask, li=li if lora is not None or i8 else None, int8=i8, **step_kw)
    hn = hk.rmsnorm_fwd(x.view(B, S, -1)[:, -1].contiguous(), m.p["norm_w"], m.eps)
    return hk.gemm_nt(hn, m.p["lm_head"], out_f32=True)


def decode_context(m, mask, B, S0, max_new_tokens):
    """-> (max_ctx checked against the RoPE table, key mask [B, max_ctx] of LEFT-padded prompts or None).  Batched evaluation (main_vqa.py:205-214):
    HF keeps position_ids = arange and hides the keys whose (spliced) attention_mask is 0; every generated position is visible."""
    max_ctx = S0 + max_new_tokens
    if max_ctx > m.cos.shape[0]:
        raise ValueError(f"prompt ({S0}) + max_new_tokens ({max_new_tokens}) exceeds the {m.cos.shape[0]} positions of the RoPE table")
    kmask = None
    if mask is not None and not bool(mask.bool().all()):
        kmask = torch.ones((B, max_ctx), device=m.device, dtype=torch.uint8)
        kmask[:, :S0] = mask.to(device=m.device, dtype=torch.uint8)
    return max_ctx, kmask


def step_or_replay(s, step, use_graph, n_done):
    """One more token of session `s`: `step()` eagerly first (lazy kernel attributes), captured at the second token, a replay from then on"""
    if use_graph and s.graph is None and n_done >= 2:
        g = hk.HipGraph()
        g.begin()
        step()
        g.end()
        s.graph = g
    if s.graph is not None:
        s.graph.launch()
    else:
        step()


# ------------------------------------------------------------------------------------------------- the single-token step
class DecodeSession:
    """Static buffers + one captured hipGraph for the single-token step (batch <= 16): embedding gather, 32 x [QKV GEMV with RMSNorm, RoPE +
    KV append + attention over the cache, O GEMV + residual, gate|up GEMV with RMSNorm, down GEMV with SwiGLU + residual], lm_head GEMV with the
    final norm -> fp32 logits.  Context length / positions live on the device (decode_advance): one capture serves every token.

    lora = a LoraStore (adapters="live"): a linear of an adapted group becomes `hk.lora_down` on the activation the base product sees, the
    format's GEMV into the fp32 `acc` without its residual, `hk.lora_up` into the output with the residual - y = bf16(x W^T + (s x A^T) B^T
    + residual) on one fp32 value, as training's `_lin`.  The store's bf16 shadow and `Bfull` are read in place (`LoraStore.refresh` rewrites
    their storage): no copy of an adapter is held.  kv_cache="fp8": `caches` holds (K codes, V codes, K scales, V scales) per layer."""

    def __init__(self, m, B, max_ctx, caches, max_new, weights="bf16", kmask=None, lora=None, kv_cache="bf16"):
        m._check_kv_cache(kv_cache, B)
        if weights not in FORMATS:
            raise ValueError(f"weights={weights!r}: expected 'bf16', 'fp8', '4bit', 'mxfp4' or 'int8'")
        fmt = FORMATS[weights]
        err = fmt.check(m, False)
        if err:
            raise ValueError(err)
        dev, d, ff, bf = m.device, m.d, m.ff, torch.bfloat16
        self.m, self.fmt, self.B, self.max_ctx, self.max_new, self.caches, self.kmask, self.lora = m, fmt, B, max_ctx, max_new, caches, kmask, lora
        self.kv8, self.graph, self.head = kv_cache == "fp8", None, fmt if fmt.own_head else FORMATS["bf16"]
        self.packed16 = self.head.optional and B >= 2 and d % 128 == 0 and ff % 128 == 0   # batched bf16: the MFMA GEMV on re-tiled weights
        fmt.ensure(m, self.packed16)

        def z(*shape, dtype=bf):
            return torch.zeros(shape, device=dev, dtype=dtype)
        self.x, self.x2, self.o, self.qkv, self.gu = z(B, d), z(B, d), z(B, d), z(B, 3 * d), z(B, 2 * ff)
        self.logits, self.next_ids, self.out_ids = z(B, m.vocab, dtype=torch.float32), z(B, dtype=torch.int64), z(B, max_new, dtype=torch.int64)
        self.tok32, self.state, self.desc, self.pos = (z(*sh, dtype=torch.int32) for sh in ((B,), (4,), (B, 8), (B,)))
        # the MFMA weight streams (bf16 and 4-bit alike) read x from L2 with prologue 0: norm / SwiGLU run once, not once per block (pays from batch 4)
        self.batched = fmt.stages and B >= 4
        if self.batched:
            self.hn, self.actb = z(B, d), z(B, ff)
        fmt.buffers(self)
        self.ad = {}   # (layer, group) -> (A [KP, in], Bfull [out_total, KP], R rows in use, r, fout) of the adapted groups
        for gname, G in (lora.groups.items() if lora is not None else ()):
            # blocks of r columns need 16-B lane loads; any other rank runs the dense form over the padded rows (their A rows and B columns are zero)
            R, r_up, fo = (lora.r * len(G["projs"]), lora.r, G["fout"]) if lora.r % 8 == 0 else (G["KP"], G["KP"], G["out_total"])
            if R > 768:
                raise ValueError(f'adapters="live": group {gname!r} stacks {R} adapter rows, the decode kernels take at most 768 - use adapters="merged"')
            if hk.lora_down_lds_bytes(B, G["fin"], R) > hk.LORA_DOWN_MAX_LDS:   # the rule of lhrs_lora_down, applied before anything is enqueued or captured
                raise ValueError(f'adapters="live": a K-slice of group {gname!r} (K = {G["fin"]}, {R} adapter rows) for {B} rows does not fit the LDS - '
                                 'use adapters="merged"')
            for li in range(len(m.p["layers"])):
                self.ad[(li, gname)] = (lora.view(lora.shadow, li, gname, "A"), lora.derived[(li, gname, "Bfull")], R, r_up, fo)
        if self.ad:
            self.acc = z(B, max(3 * d, 2 * ff), dtype=torch.float32)
            self.tpart = z(hk.LORA_DOWN_MAX_SLICES * B * max(a[2] for a in self.ad.values()), dtype=torch.float32)
        # split-context attention: 128-key slices, one workgroup each (32 * nsplit CUs); LHRS_DECODE_SPLIT=0 keeps one workgroup per head (A/B runs)
        self.nsplit = min(16, -(-max_ctx // 128)) if os.environ.get("LHRS_DECODE_SPLIT", "1") != "0" else 1
        self.attn_part = self.attn_tickets = self.attn_cs = None
        if self.nsplit > 1 and m.hd == 128:
            self.attn_part, self.attn_tickets = z(B, m.heads, self.nsplit, 132, dtype=torch.float32), z(B, m.heads, dtype=torch.int32)
            self.attn_cs = z(B, 128, dtype=torch.float32)   # cos | sin of the new position, written by decode_advance

    def staged(self, x, pro, norm_w):
        """the batched path's materialised activation (RMSNorm / SwiGLU run once into hn / actb, the linear then has no prologue)"""
        if self.batched and pro == hk.PRO_RMSNORM:
            hk.rmsnorm_fwd(x, norm_w, self.m.eps, out=self.hn)
            return self.hn, hk.PRO_NONE, None
        if self.batched and pro == hk.PRO_SWIGLU:
            hk.swiglu_fwd(x, self.m.ff, out=self.actb)
            return self.actb, hk.PRO_NONE, norm_w
        return x, pro, norm_w

    def quantised(self, x, K, pro, norm_w):
        """batch > 2 on e4m3 activations: the quantising producer of the prologue -> (e4m3 rows, per-row scales) in x8 / a8"""
        if pro == hk.PRO_RMSNORM:
            return hk.rmsnorm_fwd_q(x, norm_w, self.m.eps, want_bf16=False, q_out=self.x8)[1]
        if pro == hk.PRO_SWIGLU:
            return hk.swiglu_fwd_q(x, self.m.ff, q_out=self.a8)[1:]
        # K = ff: the materialised SwiGLU of the batched live-adapter path (MXFP4); fp8 never stages, so its prologue-free linears have K = d
        return hk.quant_fp8_rows(x, out=self.x8 if K == self.m.d else self.a8)

    def lin(self, fmt, L, name, x, out, K, pro=hk.PRO_NONE, norm_w=None, residual=None, out_f32=False, adapter=None):
        """out = pro(x) L[name]^T (+ residual) in weight format `fmt`, with the adapters of the linear's group around the base product"""
        w, sc = fmt.weight(L, name, self.packed16)
        if adapter is None:
            return fmt.linear(self, w, sc, x, out, K, pro, norm_w, residual=residual, out_f32=out_f32)
        x, pro, norm_w = self.staged(x, pro, norm_w)   # once, for the adapter and the base alike (base() then finds no prologue left)
        A, Bfull, R, r_up, fo = adapter
        acc = self.acc[:, :out.shape[1]]
        nsl = hk.lora_down(x, A, self.tpart, K, R, prologue=pro, norm_w=norm_w, eps=self.m.eps)
        fmt.linear(self, w, sc, x, acc, K, pro, norm_w, residual=None, out_f32=True)
        hk.lora_up(acc, self.tpart, nsl, self.lora.s, Bfull, r_up, fo, out, residual=residual, R=R)

    def attend(self, cache):
        """RoPE of the new q / k, KV append and attention over the cache: qkv -> o"""
        m, B, H, hd, max_ctx, scale = self.m, self.B, self.m.heads, self.m.hd, self.max_ctx, 1.0 / math.sqrt(self.m.hd)
        kc, vc = cache[:2]
        if self.kv8:  # kv_cache="fp8": the same launch on e4m3 codes + scale bytes, the new rows quantised as they are appended
            hk.decode_attn_kv8(self.qkv, kc, vc, cache[2], cache[3], m.cos, m.sin, self.pos, self.o, B, H, hd, max_ctx, scale, self.nsplit,
                               self.attn_part, self.attn_tickets, key_mask=self.kmask, cs=self.attn_cs)
        elif hd == 128 and self.nsplit > 1:  # RoPE + KV append + attention over the cache in one launch, context split over workgroups
            hk.decode_attn_split(self.qkv, kc, vc, m.cos, m.sin, self.pos, self.o, B, H, hd, max_ctx, scale, self.nsplit, self.attn_part,
                                 self.attn_tickets, key_mask=self.kmask, cs=self.attn_cs)
        elif hd == 128:
            hk.decode_attn(self.qkv, kc, vc, m.cos, m.sin, self.pos, self.o, B, H, hd, max_ctx, scale, key_mask=self.kmask)
        else:
            hk.rope_kv_append(self.qkv, kc, vc, m.cos, m.sin, self.pos, B, H, hd, max_ctx)
            hk.attn_fwd(self.qkv[:, :m.d], kc, vc, self.o, None, self.desc, B, H, hd, 1, 1 << 30, 64, True, scale, key_mask=self.kmask)

    def enqueue(self):
        """the step: token ids in tok32 -> fp32 logits"""
        m, fmt, d, ad = self.m, self.fmt, self.m.d, self.ad
        hk.decode_advance(self.state, self.desc, self.pos, self.B, self.max_ctx, 1, m.cos, m.sin, self.attn_cs)
        hk.gather_rows(m.p["embed"], self.tok32, out=self.x)
        x, x2 = self.x, self.x2
        for li, (L, cache) in enumerate(zip(m.p["layers"], self.caches)):
            self.lin(fmt, L, "qkv_w", x, self.qkv, d, hk.PRO_RMSNORM, L["ln1_w"], adapter=ad.get((li, "qkv")))
            self.attend(cache)
            self.lin(fmt, L, "o_w", self.o, x2, d, residual=x, adapter=ad.get((li, "o")))
            self.lin(fmt, L, "gu_w", x2, self.gu, d, hk.PRO_RMSNORM, L["ln2_w"], adapter=ad.get((li, "gu")))
            self.lin(fmt, L, "down_w", self.gu, x, m.ff, hk.PRO_SWIGLU, residual=x2, adapter=ad.get((li, "down")))
        self.lin(self.head, m.p, "lm_head", x, self.logits, d, hk.PRO_RMSNORM, m.p["norm_w"], out_f32=True)


# ------------------------------------------------------------------------------------------------- the token loops
def warp_logits(logits: torch.Tensor, temperature: float = 1.0, top_k: Optional[int] = None, top_p: Optional[float] = None) -> torch.Tensor:
    """HF `generate(do_sample=True)`'s score processing before the multinomial draw, in HF's order: Temperature -> TopK -> TopP LogitsWarper
    (cli_qa.py:176-186 passes temperature, the Llama-2 generation config top-k / top-p).  fp32 logits [B, V] in, filtered (-inf) logits out, on
    whatever device they live; pinned to the HF classes by tests/test_host_cpu.py::test_sampling_warpers_match_hf."""
    z = logits / max(float(temperature), 1e-6)
    if top_k:
        k = min(int(top_k), z.shape[-1])
        kth = torch.topk(z, k, dim=-1).values[:, -1:]
        z = z.masked_fill(z < kth, float("-inf"))
    if top_p is not None and top_p < 1.0:
        sz, si = torch.sort(z, descending=False, dim=-1)
        cp = torch.softmax(sz, -1).cumsum(-1)
        rm = cp <= (1 - top_p)
        rm[:, -1] = False  # keep at least the most likely token
        z = z.masked_fill(rm.scatter(1, si, rm), float("-inf"))
    return z



# ------------------------------------------------------------------------------------------------- the request of one generate() call
@dataclasses.dataclass(frozen=True)
class GenRequest:
    """What one `generate()` call has decided before anything is allocated, merged or changed: the keywords as resolved by `resolve_request`
    (which also makes every rejection of the call, once), and the facts derived from them.  The token loops read nothing else."""
    m: object
    input_ids: torch.Tensor
    image_embedding: Optional[torch.Tensor]   # with a prefix cache and no embedding of the call's own: the cached one
    attention_mask: Optional[torch.Tensor]
    do_sample: bool
    temperature: float
    top_p: Optional[float]                    # "default" resolved, as top_k
    top_k: Optional[int]
    max_new_tokens: int
    stopping_criteria: Optional[list]
    streamer: object
    eos_token_id: Optional[int]               # "default" resolved: the tokenizer's, None under a constraint
    return_logits: bool
    use_graph: bool
    weights: str
    seed: Optional[int]                       # of the device pick (`torch.initial_seed()` for None); None without it
    length_penalty: float
    early_stopping: bool
    return_beam_scores: bool
    kv_cache: str                             # with a prefix cache: the kind of that cache
    prefix_cache: Optional[PrefixCache]
    constraint: Optional[TokenAutomaton]
    return_choices: bool
    adapters: Optional[str]                   # how un-merged adapters run: "merged" | "live"; None: there are none, or `generate_rows` was called itself
    pen: float                                # repetition_penalty
    nb: int                                   # num_beams
    device_pick: bool                         # every pick is `hk.sample_rows`: sampler="device" when sampling, or a penalty
    host_checks: bool                         # the host looks at every token: eos / stopping criteria / streamer
    kv8: bool
    live_lora: bool
    prompt: Optional[list]                    # with a prefix cache: the prompt in placeholder form, as `PrefixCache.check` returned it

    lora = property(lambda self: self.m.lora if self.live_lora else None)   # adapters="live": the store the session and the GEMM steps read


def resolve_request(m, kw, rows=False) -> GenRequest:
    """kw: the keywords of a keyword entry point by name -> the request.  rows: the entry point is `generate_rows`, which has no `adapters`
    keyword - the weights are left as they are and its `live_lora` says whether the adapter store is read; `TextModal.generate` has no
    `live_lora`.  Every rejection of the call is made here, once and in this order: adapters, constraint, prefix cache, KV cache, int8 without
    its base, sampler, beams, 4bit / int8 on merged copies.  (`DecodeSession` keeps its own checks: it is an entry point too.)"""
    k = dict(kw)
    adapters, pc, nb, B = None if rows else k["adapters"], k["prefix_cache"], int(k["num_beams"]), int(k["input_ids"].shape[0])
    if not rows and adapters not in ("merged", "live"):
        raise ValueError(f"adapters={adapters!r}: expected 'merged' or 'live'")
    check_constraint(m, k["constraint"], k["return_choices"], k["do_sample"], k["num_beams"], k["repetition_penalty"], pc)
    if k["constraint"] is not None and k["eos_token_id"] == "default":
        k["eos_token_id"] = None
    k["prompt"] = None
    if pc is not None:
        if k["image_embedding"] is None:
            k["image_embedding"] = pc.image_embedding
        emb = k["image_embedding"]
        k["prompt"] = pc.check(m, k["input_ids"], k["attention_mask"], k["num_beams"], k["kv_cache"], k["max_new_tokens"], None if emb is None else emb.shape[1])
        k["kv_cache"] = pc.kv_cache
    elif k["kv_cache"] is None:
        k["kv_cache"] = "bf16"
    m._check_kv_cache(k["kv_cache"], B * max(nb, 1), max(nb, 1))
    if int8_gemm(k["weights"]) and not m.base_int8:
        raise ValueError(NO_BASE["int8"][0])
    if k["sampler"] not in ("torch", "device"):
        raise ValueError(f"sampler={k['sampler']!r}: expected 'torch' or 'device'")
    for bad, why in () if nb == 1 else (
                     (nb < 1, f"num_beams={k['num_beams']!r}: must be >= 1"),
                     (k["do_sample"], "do_sample=True with num_beams > 1 (beam-multinomial sampling) is not implemented"),
                     (k["streamer"] is not None, "streamer is not supported with num_beams > 1 (HF: beam search has no token stream)"),
                     (k["stopping_criteria"] is not None, "stopping_criteria is not supported with num_beams > 1: stopping is eos_token_id / max_new_tokens, on the device"),
                     (int(k["num_return_sequences"]) != 1, f"num_return_sequences={k['num_return_sequences']!r}: only the best hypothesis of each row is returned"),
                     (k["early_stopping"] not in (False, True), f"early_stopping={k['early_stopping']!r}: False or True ('never' is not implemented)"),
                     (nb > 8 or B * nb > 16, f"num_beams={nb} with batch {B}: batch * num_beams must be <= 16 (and num_beams <= 8)")):
        if bad:
            raise ValueError(why)
    if m.lora is None:
        adapters = None
    elif adapters == "merged" and k["weights"] in ("4bit", "int8"):
        raise ValueError(MERGED_COPIES[k["weights"]])
    if k["eos_token_id"] == "default":
        k["eos_token_id"] = getattr(m.tokenizer, "eos_token_id", None)
    # sampling defaults of the reference's callers: HF GenerationConfig top_k = 50 and the Llama-2 generation_config.json top_p = 0.9
    # apply when the caller (cli_qa.py:176-186 passes only temperature) does not say otherwise
    for name, default in (("top_k", 50), ("top_p", 0.9)):
        if k[name] == "default":
            k[name] = default if k["do_sample"] else None
    pen = float(k["repetition_penalty"])
    device_pick = (k["sampler"] == "device" and bool(k["do_sample"])) or pen != 1.0
    if device_pick:
        k["seed"] = int(torch.initial_seed() if k["seed"] is None else k["seed"])
    k.update(m=m, adapters=adapters, pen=pen, nb=nb, device_pick=device_pick, kv8=k["kv_cache"] == "fp8",
             live_lora=bool(k["live_lora"]) if rows else adapters == "live",
             host_checks=k["eos_token_id"] is not None or k["stopping_criteria"] is not None or k["streamer"] is not None)
    return GenRequest(**{f.name: k[f.name] for f in dataclasses.fields(GenRequest)})


MERGED_COPIES = {  # weights -> text of generate(weights=..., adapters="merged") with un-merged adapters
    "4bit": 'weights="4bit" with un-merged LoRA adapters: generate() then runs on merged 16-bit COPIES, which have no 4-bit form - '
            'call merge_lora() first (it re-quantises the merged weights, as peft does for a merged Linear4bit), or pass '
            'adapters="live" (the adapters then run next to the 4-bit codes)',
    "int8": 'weights="int8" with un-merged LoRA adapters: generate() then runs on merged 16-bit COPIES, which have no int8 form - '
            'call merge_lora() first (it re-quantises the merged weights), or pass adapters="live" (the adapters then run '
            'next to the int8 rows)'}


def run_request(req):
    """the resolved call, on the weights its `adapters` mode asks for (`TextModal._adapters_on`)"""
    with req.m._adapters_on(req.adapters, req.weights):
        return (generate_beam if req.nb != 1 else generate_tokens)(req)


# ------------------------------------------------------------------------------------------------- what the loops share
@contextlib.contextmanager
def side_stream(device):
    """the launches of the body run on a side stream behind everything queued so far (graph capture needs a non-default stream); the
    current stream waits for them afterwards"""
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        yield
    torch.cuda.current_stream().wait_stream(side)


def open_session(req, rows, max_ctx, caches, kmask, S0):
    """the session of the call over `rows` cache rows, its state words behind the S0 positions of the prompt and before the first token"""
    s = req.m._decode_session(rows, max_ctx, caches, req.max_new_tokens, req.weights, kmask, req.lora, req.kv_cache)
    s.state[0], s.state[1] = S0, 0
    return s


def results(*values):
    """what a call returns: the values that are not None as a tuple - or the ids alone"""
    out = tuple(v for v in values if v is not None)
    return out if len(out) > 1 else out[0]


class Picker:
    """The pick of a non-beam call, chosen once from the request: `pick(logits, out, step_host)` -> the next ids, int64 [B] - in `out`
    (None: a new tensor) for the arms that are one launch, a new tensor from the host multinomial, which ignores `out`.  It owns what the
    arms keep between tokens: the `ConstraintState`, the `seen` bitmap of the penalty, the seed, and `step_dev`, the device counter of
    emitted tokens that numbers the draws of a session (None: `step_host` does)."""

    def __init__(self, req, B):
        self.req, self.seen, self.step_dev = req, None, None
        self.cs = hk.ConstraintState(B, req.m.device) if req.constraint is not None else None
        if req.device_pick and req.pen != 1.0:  # bitmap of the tokens generated so far in this call (HF started from inputs_embeds: the prompt is not in it)
            self.seen = torch.zeros((B, (req.m.vocab + 31) // 32), device=req.m.device, dtype=torch.int32)
        P = Picker   # the arm as a plain function: a bound method kept on the object would be a reference cycle that holds device memory until the collector runs
        self.arm = P.constrained if self.cs is not None else P.device if req.device_pick else P.multinomial if req.do_sample else P.argmax

    def pick(self, logits, out, step_host):
        return self.arm(self, logits, out, step_host)

    def constrained(self, logits, out, step_host):
        return hk.constrain_rows(logits, self.req.constraint, self.cs, out, score=self.req.return_choices)

    def device(self, logits, out, step_host):   # mode 0 draws, mode 1 is the first maximum of the penalised logits
        r = self.req
        return hk.sample_rows(logits, out, mode=0 if r.do_sample else 1, temperature=r.temperature, top_k=r.top_k, top_p=r.top_p,
                              repetition_penalty=r.pen, seen=self.seen, seed=r.seed, step_dev=self.step_dev, step_host=step_host)

    def multinomial(self, logits, out, step_host):
        r = self.req
        return torch.multinomial(torch.softmax(warp_logits(logits, r.temperature, r.top_k, r.top_p), -1), 1).squeeze(1)

    def argmax(self, logits, out, step_host):
        return hk.argmax_rows(logits, out=out)


class SessionStepper:
    """batch <= 16: a step is a graph replay over the session's static buffers, the ids live in `s.out_ids`"""

    def __init__(self, req, s):
        self.req, self.s, self.out = req, s, s.next_ids   # out: where a one-launch pick writes

    def emit(self, nxt):
        s = self.s
        if nxt is not s.next_ids:   # the prefill's argmax / multinomial token, a host-side pick or pad replacement: through copy_, not written there
            s.next_ids.copy_(nxt)
        hk.decode_emit(s.next_ids, s.tok32, s.out_ids, s.state, s.B, s.max_new)

    def step(self, n_done):
        step_or_replay(self.s, self.s.enqueue, self.req.use_graph, n_done)
        return self.s.logits, 0            # the draw's step counter is the session's, on the device

    def ids(self, n):
        return self.s.out_ids[:, :n]


class GemmStepper:
    """batch > 16: a step is `gather_rows` + `gemm_logits` over one new position, the ids live in a Python list"""
    out = None

    def __init__(self, req, B, S0, max_ctx, caches, kmask):
        self.req, self.B, self.S0, self.cache_args, self.toks = req, B, S0, (caches, max_ctx, False, kmask, req.lora, req.weights), []

    def emit(self, nxt):
        self.toks.append(nxt)

    def step(self, n_done):
        m = self.req.m
        x = hk.gather_rows(m.p["embed"], self.toks[-1].clamp(0, m.vocab - 1).to(torch.int32))
        return gemm_logits(m, x, self.B, 1, self.S0 + n_done - 1, *self.cache_args), n_done   # the draw's step counter is the host's

    def ids(self, n):
        return torch.stack(self.toks, 1)


# ------------------------------------------------------------------------------------------------- the token loops
def generate_rows(m, input_ids, image_embedding=None, attention_mask=None, do_sample=False, temperature=1.0, top_p=None, top_k=None,
                  max_new_tokens=512, use_cache=True, stopping_criteria=None, streamer=None, eos_token_id=None, return_logits=False,
                  use_graph=True, weights="bf16", sampler="torch", seed=None, repetition_penalty=1.0, num_beams=1, length_penalty=1.0,
                  early_stopping=False, return_beam_scores=False, num_return_sequences=1, live_lora=False, kv_cache="bf16", prefix_cache=None,
                  constraint=None, return_choices=False, **_kw):
    """TextModal.generate (text_modal.py:528-627): prefill over the spliced embeddings, then one token at a time with a KV cache; returns only
    the NEW token ids [B, n_new] (HF generate started from inputs_embeds).  Greedy (the evaluation scripts' mode) runs entirely in HIP kernels;
    with do_sample=True the fp32 logits go through HF's temperature / top-k / top-p warpers and one multinomial draw per token.  The step is a
    captured hipGraph over static buffers (batch <= 16); without eos / stopping criteria / streamer the host never synchronises inside the loop.

    sampler="device" (with do_sample=True) replaces the warpers and `torch.multinomial` by ONE launch of `hk.sample_rows` per token, between the
    graph replay and `decode_emit`: same distribution as HF, drawn by Philox from (`seed`, step, row); `seed=None` takes `torch.initial_seed()`.
    `repetition_penalty != 1` (HF RepetitionPenaltyLogitsProcessor over the tokens generated so far in this call) exists in that kernel only
    and routes every pick through it whatever `sampler` says: mode 0 when sampling, mode 1 (first maximum of the penalised logits) when greedy.
    With `eos_token_id` set the pad replacement of finished rows and the host's check still run between the pick and `decode_emit`; the kernel
    has then already set the drawn token's bit in the seen bitmap of a finished row, which nothing reads any more.

    prefix_cache = a `PrefixCache` (batch 1, no beams): the caches are its own and outlive the call.  The prompt is matched against what
    they hold (`match_prefix`), only the positions behind the common prefix are prefilled (`gemm_logits` with ctx = the reused positions),
    and the token loop runs as ever, on a session over the cache's rows.  The new positions attend each other in exact bf16, as the
    positions of any prompt do; they attend the reused ones through what the cache holds - bf16 rows, or with kv_cache="fp8" the codes,
    as the single-token step does (`layer_step`).  On return the cache holds the prompt and every emitted token but the last.

    constraint = a `TokenAutomaton` (greedy only, no beams, penalty or prefix cache): every pick, the prefill's included, is ONE launch of
    `hk.constrain_rows` where `argmax_rows` runs otherwise - the best token among the out-edges of the row's state, and the walk along it.
    The model step, the graph and `decode_emit` are as ever.  Rows behind a final state emit pad_token_id; the host reads the rows' `fin`
    every fourth token (every token on the host path of eos / stopping criteria / streamer) and stops when all are final; the ids are cut to
    the longest row, its EOS included.  return_choices=True appends (choice [B] int64: the final state's label, -1 where max_new_tokens ran
    out first; score [B] fp32: the sum of the picked tokens' log-probabilities over the full vocabulary) - only then is the score computed.

    A keyword entry point: the work is `resolve_request` (every rejection), then `generate_tokens` or `generate_beam` on the request."""
    return run_request(resolve_request(m, locals(), rows=True))


def generate_tokens(req):
    """the non-beam call: prefill, first pick, then ONE loop of [emit, host's look, step, pick] over a `SessionStepper` or a `GemmStepper`"""
    m, pc, dev, streamer, max_new = req.m, req.prefix_cache, req.m.device, req.streamer, req.max_new_tokens
    if streamer is not None and getattr(streamer, "skip_prompt", False):
        streamer.put(req.input_ids.cpu())  # transformers.TextStreamer protocol: the first put() is the prompt, which skip_prompt drops
    embeds, _, mask, _ = m.prepare_inputs_for_multimodal(req.input_ids, req.attention_mask, None, req.image_embedding)
    B, S0, d = embeds.shape
    if pc is None:
        max_ctx, kmask = decode_context(m, mask, B, S0, max_new)
        caches, reuse = m._alloc_kv(B * max_ctx, req.kv_cache), 0
    else:   # the cache's own rows, all of them visible; it is rolled back to the reused positions before the prefill writes behind them
        max_ctx, kmask = pc.max_positions, None
        reuse = pc.begin(req.prompt, req.image_embedding)
        caches = pc.caches
    picker = Picker(req, B)
    cs, one_launch_pick = picker.cs, req.device_pick or req.constraint is not None
    # ORDER KEPT: with batch <= 16 the session is built BEFORE the prefill only for the picks that write into it (device pick, constraint) ...
    s = open_session(req, B, max_ctx, caches, kmask, S0) if B <= 16 and one_launch_pick else None
    if s is not None and req.device_pick:
        picker.step_dev = s.state[1:2]
    # ---- prefill (GEMM path) -> logits of the last prompt position -> first new token
    # (behind the `reuse` positions a prefix cache already holds: B = 1, the rows of embeds[0, reuse:])
    logits = gemm_logits(m, embeds.reshape(B * S0, d)[reuse:], B, S0 - reuse, reuse, caches, max_ctx, req.kv8, kmask, req.lora, req.weights)
    all_logits = [logits.clone()] if req.return_logits else []
    nxt = picker.pick(logits, None if s is None else s.next_ids, 0)
    if B <= 16 and s is None:
        s = open_session(req, B, max_ctx, caches, kmask, S0)   # ... and AFTER the prefill and its pick otherwise (`SessionStepper.emit` copies that token in)
    stepper = SessionStepper(req, s) if B <= 16 else GemmStepper(req, B, S0, max_ctx, caches, kmask)
    finished, pad = torch.zeros(B, dtype=torch.bool, device=dev), m.tokenizer.pad_token_id

    def host_step(ids_so_far, lg):  # -> stop?
        nonlocal finished
        if streamer is not None:
            streamer.put(ids_so_far[:, -1].cpu())
        if req.eos_token_id is not None:
            finished |= ids_so_far[:, -1] == req.eos_token_id
            if bool(finished.all()):
                return True
        if cs is not None and bool(cs.fin.all()):
            return True
        return req.stopping_criteria is not None and any(c(ids_so_far, lg) for c in req.stopping_criteria)

    n_done = 0
    with side_stream(dev) if B <= 16 else contextlib.nullcontext():
        while True:
            stepper.emit(nxt)
            n_done += 1
            if req.host_checks:
                stop = host_step(stepper.ids(n_done), logits)
            else:   # as generate_beam reads its done word
                stop = cs is not None and n_done % 4 == 0 and bool(cs.fin.all())
            if stop or n_done >= max_new:
                break
            logits, step_host = stepper.step(n_done)
            if req.return_logits:
                all_logits.append(logits.clone())
            nxt = picker.pick(logits, stepper.out, step_host)
            if req.eos_token_id is not None:   # finished rows emit pads
                nxt = torch.where(finished, torch.full_like(nxt, pad), nxt)
    ids = stepper.ids(n_done).clone()
    if cs is not None:   # the longest row with its EOS: the columns behind it (the picks since the last look at `fin`) hold pads only
        n_done = int(cs.len.max().item())
        ids, all_logits = ids[:, :n_done].contiguous(), all_logits[:n_done]
    if pc is not None:
        pc.commit(req.prompt, ids[0].tolist(), S0, reuse)
    if streamer is not None:
        streamer.end()
    return results(ids, torch.stack(all_logits, 1) if req.return_logits else None,
                   *((cs.choice.to(torch.int64), cs.score.clone()) if req.return_choices else ()))


def generate_beam(req):
    """Deterministic beam search, HF `generate(num_beams=nb, do_sample=False)` (generation/utils.py _beam_search): the prompt is prefilled ONCE per
    batch row into cache row b * nb and replicated to the row's other beams by `hk.kv_beam_reorder`; every further token is one single-stream
    graph of [model step over B * nb rows, beam_topk_rows, beam_step, kv_beam_reorder, decode_emit] (csrc/beam.hip).  All bookkeeping lives on
    the device; the host reads the batch-wide `done` word every fourth token when an EOS is set (once done, the kernels change nothing) and never
    without one.  -> ids [B, L] of each row's best hypothesis, pad_token_id past its end (, logits [B * nb, n, V])(, scores [B])."""
    m, nb, max_new, dev = req.m, req.nb, req.max_new_tokens, req.m.device
    embeds, _, mask, _ = m.prepare_inputs_for_multimodal(req.input_ids, req.attention_mask, None, req.image_embedding)
    B, S0, d = embeds.shape
    R = B * nb
    max_ctx, kmask = decode_context(m, mask, B, S0, max_new)   # left-padded prompts, as in generate_tokens; every beam hides its row's padding
    kmask_r = None if kmask is None else kmask.repeat_interleave(nb, 0).contiguous()
    caches = m._alloc_kv(R * max_ctx, req.kv_cache)
    s = open_session(req, R, max_ctx, caches, kmask_r, S0)
    st = hk.BeamState(B, nb, m.vocab, max_new, req.length_penalty, dev)
    # kv_beam_reorder is a byte copy in 16-byte chunks whose `d` counts 2-byte units: the bf16 caches with d, the kv8 code caches with d / 2
    # and the scale arrays with H / 2 - codes and scales move together, in two launches
    tables = [(hk.kv_cache_table(caches, dev), d)] if not req.kv8 else [(hk.kv_cache_table([c[:2] for c in caches], dev), d // 2),
                                                                        (hk.kv_cache_table([c[2:] for c in caches], dev), m.heads // 2)]

    # ---- prefill: sequence b into cache row b * nb (a cache "row" of nb * max_ctx positions), logits of the last prompt position
    logits = gemm_logits(m, embeds.reshape(B * S0, d), B, S0, 0, caches, nb * max_ctx, req.kv8, kmask, req.lora, req.weights)
    logits = logits.repeat_interleave(nb, 0).contiguous()   # the row's beams all start from it
    all_logits = [logits] if req.return_logits else []

    def beam_tail(lg, t0, t1):
        hk.beam_topk_rows(lg, st, req.pen)
        hk.beam_step(st, s.next_ids, req.eos_token_id, req.early_stopping)
        for table, units in tables:
            hk.kv_beam_reorder(table, B, nb, max_ctx, units, st.parent, t0, t1, S0 if t0 == 0 else max_new, done=st.bstate[1:2])
        hk.decode_emit(s.next_ids, s.tok32, s.out_ids, s.state, R, max_new)

    def step():
        s.enqueue()
        beam_tail(s.logits, S0, s.state[0:1])

    with side_stream(dev):
        beam_tail(logits, 0, S0)          # parents are all 0: replicates the prompt's cache to every beam of the row
        n_done = 1
        while n_done < max_new:
            step_or_replay(s, step, req.use_graph, n_done)
            if req.return_logits:
                all_logits.append(s.logits.clone())
            n_done += 1
            if req.eos_token_id is not None and n_done % 4 == 0 and int(st.bstate[1].item()):
                break
    # ---- the result of each row: its best finished hypothesis, else its best running beam (tiny host-side epilogue, once per call)
    n = int(st.bstate[0].item())
    fin_score, fin_len, fin_slot = st.fin_score.view(B, nb).cpu(), st.fin_len.view(B, nb).cpu(), st.fin_slot.view(B, nb).cpu()
    fin_seq, hist, run = st.fin_seq.view(B, nb, -1).cpu(), st.hist[n & 1].view(B, nb, -1).cpu(), st.run_score.view(B, nb).cpu()
    rows, scores = [], []
    for b in range(B):
        if int(fin_len[b, 0]) > 0:
            rows.append(fin_seq[b, int(fin_slot[b, 0]), :int(fin_len[b, 0])])
            scores.append(float(fin_score[b, 0]))
        else:
            rows.append(hist[b, 0, :n])
            scores.append(float(run[b, 0]))
    ids = torch.full((B, max(len(r) for r in rows)), int(m.tokenizer.pad_token_id), dtype=torch.int64)
    for b, r in enumerate(rows):
        ids[b, :len(r)] = r
    return results(ids.to(dev), torch.stack(all_logits[:n], 1) if req.return_logits else None,
                   torch.tensor(scores, dtype=torch.float32, device=dev) if req.return_beam_scores else None)
