"""TextModal: image-token splice + LLaMA-2 forward / activation-gradient backward + causal-LM loss on gfx950.

Mirrors /root/reference lhrs/models/text_modal.py: `TextModal.decode` (:258-294), `prepare_inputs_for_multimodal`
(:296-526), `CustomLlamaForCausalLM` (:30-60) over HF LlamaForCausalLM.  Stage 1 trains the projector only, so the
backward pass propagates dX through the frozen decoder (no dW): every linear's backward is one NT GEMM against a
pre-transposed copy of its weight that stays resident in HBM (2 x 13.5 GB of 288 GB).

Activation memory per layer and token: x_in, x_mid, o (3 x 4096), qkv (12288), gate|up (22016) in bf16 = 93 KB;
32 layers x 2184 tokens (B=8, S=273) = 6.5 GB - no gradient checkpointing (the reference needs it on 80 GB parts).
"""
from __future__ import annotations

import contextlib
import math
import os
import types
from typing import Dict, List, Optional

import torch

from . import generation, kernels as hk
from .base_scheme import Bf16Base, E4m3Base, Int8Base
from .generation import warp_logits  # noqa: F401  (callers import it from here)

IGNORE_INDEX = -100
IMAGE_TOKEN_INDEX = -200
DEFAULT_IMAGE_TOKEN = "<image>"
DEFAULT_IMAGE_PATCH_TOKEN = "<im_patch>"
DEFAULT_IM_START_TOKEN = "<im_start>"
DEFAULT_IM_END_TOKEN = "<im_end>"


class SyntheticTokenizer:
    """Stands in for LlamaTokenizerFast when no tokenizer files exist offline (pad = unk = 0, bos = 1, eos = 2).  Text is split on
    whitespace and every word hashed to a stable id in [3, 32000) ("\n" -> 13, "</s>" -> 2): enough to drive the data pipeline, the
    prompt templates and the stopping criteria end to end in synthetic runs; it is NOT the LLaMA vocabulary and decoding is lossy
    (`decode` prints `<id>` for ids it has never encoded)."""
    unk_token_id = pad_token_id = 0
    bos_token_id = 1
    eos_token_id = 2
    model_max_length = 2048
    is_synthetic = True

    def __init__(self):
        self._words = {0: "<unk>", 1: "<s>", 2: "</s>", 13: "\n"}

    def __len__(self):
        return 32000

    def _id(self, w: str) -> int:
        if w == "\n":
            return 13
        if w == "</s>":
            return 2
        h = 2166136261
        for ch in w.encode():
            h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
        i = 14 + h % (32000 - 14)
        self._words.setdefault(i, w)
        return i

    def __call__(self, text, **_kw):
        ids = [self.bos_token_id] + [self._id(w) for w in text.replace("\n", " \n ").split(" ") if w]
        return types.SimpleNamespace(input_ids=ids)

    def decode(self, ids, skip_special_tokens: bool = False, **_kw) -> str:
        ids = ids.tolist() if hasattr(ids, "tolist") else list(ids)
        words = [self._words.get(int(i), f"<{int(i)}>") for i in ids if not (skip_special_tokens and int(i) in (0, 1, 2))]
        return " ".join(words).replace(" \n ", "\n")

    def batch_decode(self, rows, skip_special_tokens: bool = False, **_kw):
        return [self.decode(r, skip_special_tokens=skip_special_tokens) for r in rows]


LORA_GROUPS = {  # fused GEMM group -> (sub-projections, in_features, out_features per projection)
    "qkv": (("q", "k", "v"), 4096, 4096), "o": (("o",), 4096, 4096), "gu": (("gate", "up"), 4096, 11008), "down": (("down",), 11008, 4096)}
LORA_ALL = ("q", "k", "v", "o", "gate", "up", "down")  # find_all_linear_names: every nn.Linear except lm_head (text_modal.py:658-667)


class LoraStore:
    """peft-style LoRA adapters (lora.Linear: y = W x + (alpha/r) B A x; A ~ kaiming-uniform(a=sqrt 5), B = 0) for the fused
    GEMM groups, in three flat buffers (fp32 master, bf16 shadow, fp32 grad) ordered layer-major so that a layer's
    gradients form one contiguous all-reduce bucket.  Per (layer, group) two stacked tensors:
        A  [KP, in]          rows p*r..p*r+r = A_p                      (KP = r * n_proj padded to 64, padding rows stay 0)
        BD [KP, out_total]   block p = B_p^T at rows p*r.., cols p*out.. (block diagonal; off-blocks are masked to 0)
    and two derived bf16 operands rebuilt after every optimizer step: AT = A^T [in, KP], Bfull = BD^T [out_total, KP]."""

    def __init__(self, n_layers, r, alpha, targets, dims, device, seed=0, dropout=0.0):
        self.r, self.s, self.targets, self.device, self.nl = int(r), float(alpha) / float(r), tuple(targets), device, n_layers
        # peft lora_dropout: applied to the adapter input in train mode only; ONE counter-based mask per fused group and forward pass
        # (peft draws one per wrapped nn.Linear: q, k, v - and gate, up - share a mask here because they share the stacked A product)
        self.dropout, self.train_mode, self.drop_seed, self.drop_epoch = float(dropout), True, int(seed) * 2654435761 % (1 << 32), 0
        self.groups = {}
        for gname, (projs, fin, fout) in dims.items():
            mask = sum(1 << i for i, p in enumerate(projs) if p in self.targets)
            if mask:
                self.groups[gname] = dict(projs=projs, fin=fin, fout=fout, mask=mask, KP=(self.r * len(projs) + 63) // 64 * 64,
                                          out_total=fout * len(projs))
        self.offsets, off = {}, 0
        self.layer_range = []
        for l in range(n_layers):
            start = off
            for gname, G in self.groups.items():
                for kind, shape in (("A", (G["KP"], G["fin"])), ("BD", (G["KP"], G["out_total"]))):
                    self.offsets[(l, gname, kind)] = (off, shape)
                    off += shape[0] * shape[1]
            self.layer_range.append((start, off))
        self.numel = off
        self.master = torch.zeros(off, device=device, dtype=torch.float32)
        self.shadow = torch.zeros(off, device=device, dtype=torch.bfloat16)
        self.grad = torch.zeros(off, device=device, dtype=torch.float32)
        self.derived = {}
        g = torch.Generator(device=device).manual_seed(seed)
        for l in range(n_layers):
            for gname, G in self.groups.items():
                A = self.view(self.master, l, gname, "A")
                bound = 1.0 / math.sqrt(G["fin"])
                for i, p in enumerate(G["projs"]):
                    if (G["mask"] >> i) & 1:
                        A[i * self.r:(i + 1) * self.r].copy_((torch.rand((self.r, G["fin"]), device=device, generator=g) * 2 - 1) * bound)
        self.refresh()

    def view(self, flat, l, gname, kind):
        off, shape = self.offsets[(l, gname, kind)]
        return flat[off: off + shape[0] * shape[1]].view(*shape)

    def num_parameters(self):
        n = 0
        for G in self.groups.values():
            n += bin(G["mask"]).count("1") * self.r * (G["fin"] + G["fout"])
        return n * self.nl

    def active_dropout(self) -> float:
        return self.dropout if self.train_mode else 0.0

    def seed_for(self, l: int, gname: str) -> int:
        gid = list(self.groups).index(gname)
        return (self.drop_seed + self.drop_epoch * 0x85EBCA77 + (l * 8 + gid) * 0x9E3779B1) & 0xFFFFFFFF

    def refresh(self):
        """bf16 shadow + transposed operands after a load / optimizer step (all 8 transposes of every layer in one launch).  Bumps `version`:
        whatever was derived from the adapters (generate()'s merged decode weights) is stale from here on."""
        self.version = getattr(self, "version", 0) + 1
        hk.cast_f32_to_bf16(self.master, self.shadow)
        if getattr(self, "_bt", None) is None:
            pairs = []
            for l in range(self.nl):
                for gname in self.groups:
                    for kind, dk in (("A", "AT"), ("BD", "Bfull")):
                        src = self.view(self.shadow, l, gname, kind)
                        dst = torch.empty((src.shape[1], src.shape[0]), device=src.device, dtype=torch.bfloat16)
                        self.derived[(l, gname, dk)] = dst
                        pairs.append((src, dst))
            self._bt = hk.BatchedTranspose(pairs)
        self._bt.run()

    # peft-layout accessors (A_p [r, in], B_p [out, r]) for tests / checkpoints
    def get_adapter(self, l, proj):
        for gname, G in self.groups.items():
            if proj in G["projs"]:
                i = G["projs"].index(proj)
                A = self.view(self.master, l, gname, "A")[i * self.r:(i + 1) * self.r]
                Bt = self.view(self.master, l, gname, "BD")[i * self.r:(i + 1) * self.r, i * G["fout"]:(i + 1) * G["fout"]]
                return A, Bt.t()
        raise KeyError(proj)

    def set_adapter(self, l, proj, A, B):
        for gname, G in self.groups.items():
            if proj in G["projs"]:
                i = G["projs"].index(proj)
                self.view(self.master, l, gname, "A")[i * self.r:(i + 1) * self.r].copy_(A.to(self.device))
                self.view(self.master, l, gname, "BD")[i * self.r:(i + 1) * self.r, i * G["fout"]:(i + 1) * G["fout"]].copy_(B.t().to(self.device))
                return
        raise KeyError(proj)

    def grad_adapter(self, l, proj):
        for gname, G in self.groups.items():
            if proj in G["projs"]:
                i = G["projs"].index(proj)
                dA = self.view(self.grad, l, gname, "A")[i * self.r:(i + 1) * self.r]
                dBt = self.view(self.grad, l, gname, "BD")[i * self.r:(i + 1) * self.r, i * G["fout"]:(i + 1) * G["fout"]]
                return dA, dBt.t()
        raise KeyError(proj)


class TextModal:
    def __init__(self, config=None, device="cuda", layers=32, dim=4096, ff=11008, heads=32, vocab=32000, eps=1e-5,
                 rope_theta=10000.0, max_pos=4096):  # LLaMA-2 max_position_embeddings; S reaches model_max_length 2048 + 143 image tokens
        self.device = torch.device(device)
        hk.ensure_gemm_workspace(self.device)
        self.nl, self.d, self.ff, self.heads, self.vocab, self.eps = layers, dim, ff, heads, vocab, float(eps)
        self.hd = dim // heads
        self.tokenizer = SyntheticTokenizer()
        self.p: Dict = {}
        inv = 1.0 / (rope_theta ** (torch.arange(0, self.hd, 2).float() / self.hd))
        fr = torch.outer(torch.arange(max_pos).float(), inv)
        # HF casts cos/sin to the activation dtype before use; keep bf16-representable values in an fp32 table
        self.cos = fr.cos().to(torch.bfloat16).float().to(self.device).contiguous()
        self.sin = fr.sin().to(torch.bfloat16).float().to(self.device).contiguous()
        self._ctx = None
        self.lora: Optional[LoraStore] = None
        self.base = Bf16Base()  # arithmetic of the frozen decoder linears (base_scheme.py); quantize_base installs another
        self._merged_cache = None
        # training forward: run the last decoder layer's post-attention half on the supervised rows only when they are one contiguous
        # range per sequence (_layer_fwd `tail`); LHRS_TAIL_ROWS_ONLY=0 / attribute False: every row, as HF does
        self.tail_rows_only = os.environ.get("LHRS_TAIL_ROWS_ONLY", "1") != "0"
        self.text_encoder = self  # attribute path used by the entry scripts (.text.text_encoder)

    def get_text_encoder(self):
        return self

    # read-only views of `self.base` (what the entry scripts, generation.py and the tests ask)
    base8 = property(lambda self: isinstance(self.base, E4m3Base))      # frozen decoder linears in e4m3 (quantize_base(8, "e4m3"))
    base_int8 = property(lambda self: isinstance(self.base, Int8Base))  # ... as LLM.int8 (quantize_base(8, "int8"): the reference's bitsandbytes arithmetic)
    base4 = property(lambda self: self.base.storage4)  # (quant_type, double_quant) once they are bitsandbytes 4-bit storage (quantize_base(4, ...))
    _i8ws = property(lambda self: self.base.ws)

    # ------------------------------------------------------------------ parameters
    def _finish(self):
        """Build the transposed copies used by the dX GEMMs (weights are frozen: done once)."""
        for L in self.p["layers"]:
            for k in ("qkv_w", "o_w", "gu_w", "down_w"):
                L[k + "T"] = hk.transpose(L[k])
        self.p["lm_headT"] = hk.transpose(self.p["lm_head"])

    def load_params(self, p: Dict) -> None:
        dev, bf = self.device, torch.bfloat16
        self.p = {"embed": p["embed"].to(dev, bf), "norm_w": p["norm_w"].to(dev, bf), "lm_head": p["lm_head"].to(dev, bf),
                  "layers": [{k: v.to(dev, bf).contiguous() for k, v in L.items()} for L in p["layers"]]}
        self.nl = len(self.p["layers"])
        self._merged_cache = None     # merged copies of the previous weights are stale
        self._finish()

    def from_pretrained(self, path: str, n_layers: Optional[int] = None) -> None:
        """CustomLlamaForCausalLM.from_pretrained(config.text.path) (text_modal.py:79-131): HF checkpoint directory ->
        engine layout.  Architecture numbers come from the checkpoint's own config.json, as in the reference."""
        import json
        import os
        from .checkpoint import llama_from_hf, load_hf_dir
        cfg = json.load(open(os.path.join(path, "config.json")))
        assert cfg["hidden_size"] == self.d and cfg["intermediate_size"] == self.ff and cfg["num_attention_heads"] == self.heads, cfg
        assert cfg.get("num_key_value_heads", self.heads) == self.heads, "GQA checkpoints are outside the reference's LLaMA-2-7B path"
        self.eps = float(cfg.get("rms_norm_eps", self.eps))
        self.load_params(llama_from_hf(load_hf_dir(path), n_layers))

    def merge_lora(self) -> None:
        """peft merge_and_unload (UniBind.custom_load_state_dict, stage == 0; lhrs/models/UniBind.py:112-115):
        W <- W + (alpha/r) B A, computed per fused group as one GEMM  W + s * Bfull . AT^T, then the adapters are dropped."""
        lo = self.lora
        if lo is None:
            return
        for li, L in enumerate(self.p["layers"]):
            for gname in lo.groups:
                W = L[gname + "_w"]
                hk.gemm_nt(lo.derived[(li, gname, "Bfull")], lo.derived[(li, gname, "AT")], out=W, residual=W, alpha=lo.s)
                L[gname + "_w" + "T"] = hk.transpose(W)
            self._drop_derived(L)
        self.lora, self._merged_cache = None, None
        self.base.install(self)   # the stored copies (8-bit operands, 4-bit states) are a function of the (now merged) weights

    # rebuilt from a weight `<name>` / `<name>T`: the decode operands of generation.FORMATS + e4m3 copies, int8 rows and factors, 4-bit states
    DERIVED_SUFFIXES = generation.DECODE_SUFFIXES + ("8", "8s", "i8", "i8s", "q4")

    def _drop_derived(self, L) -> None:
        """Forget every tensor that was computed FROM a decoder weight of layer dict `L` (decode re-tilings, e4m3 copies): after the weight
        changes in place (merge_lora, a checkpoint load) they are stale; their builders re-create them on next use."""
        for base in ("qkv_w", "o_w", "gu_w", "down_w", "qkv_wT", "o_wT", "gu_wT", "down_wT"):
            for suf in self.DERIVED_SUFFIXES:
                L.pop(base + suf, None)

    def init_random(self, seed: int = 0) -> None:
        """Random-init LLaMA-2-7B shapes, N(0, 0.02) (HF initializer_range) - no weights exist offline."""
        g = torch.Generator(device=self.device).manual_seed(seed)
        dev, bf, d, ff = self.device, torch.bfloat16, self.d, self.ff

        def rn(*shape, std=0.02, mean=0.0):
            out = torch.empty(*shape, device=dev, dtype=bf)
            rows = shape[0]
            step = max(1, (1 << 26) // max(1, out[0].numel())) if len(shape) > 1 else rows
            for r0 in range(0, rows, step):  # chunked so the fp32 temporary stays small
                r1 = min(rows, r0 + step)
                out[r0:r1] = (torch.randn((r1 - r0,) + tuple(shape[1:]), device=dev, generator=g) * std + mean).to(bf)
            return out

        self.p = {"embed": rn(self.vocab, d), "norm_w": rn(d, std=0.0, mean=1.0), "lm_head": rn(self.vocab, d), "layers": []}
        for _ in range(self.nl):
            self.p["layers"].append({"ln1_w": rn(d, std=0.0, mean=1.0), "qkv_w": rn(3 * d, d), "o_w": rn(d, d),
                                     "ln2_w": rn(d, std=0.0, mean=1.0), "gu_w": rn(2 * ff, d), "down_w": rn(d, ff)})
        self._finish()

    def enable_lora(self, r=128, alpha=256, targets=LORA_ALL, seed=0, dropout=0.0) -> LoraStore:
        """TextModal.__init__ LoRA branch (text_modal.py:133-151): LoraConfig(r, lora_alpha, target_modules=all linears).
        BASELINE config 4 uses r=8 on ("q","k","v","o").  dropout = lora_dropout (0.05 in the stage-2 YAML; train mode only - stage 3
        runs text.eval())."""
        dims = {"qkv": (("q", "k", "v"), self.d, self.d), "o": (("o",), self.d, self.d), "gu": (("gate", "up"), self.d, self.ff),
                "down": (("down",), self.ff, self.d)}
        self.lora = LoraStore(len(self.p["layers"]), r, alpha, targets, dims, self.device, seed, dropout)
        return self.lora

    def _drop(self, rec, gname):
        """(p, seed) of the dropout mask this group's forward used, or None"""
        seed = rec.get("seed_" + gname)
        return None if seed is None else (self.lora.dropout, seed)

    def _has(self, gname) -> bool:
        return self.lora is not None and gname in self.lora.groups

    def _adapter_down(self, li, gname, x, save):
        """-> (T, Bfull), the adapter pair of the group's forward product: T [M, KP] = s * dropout(x) A^T; (None, None) without adapters.
        T and the dropout seed go into `save` for the backward."""
        lo = self.lora
        if lo is None or gname not in lo.groups:
            return None, None
        xa, pd = x, lo.active_dropout()
        if pd > 0:  # lora_A(dropout(x)): the mask is regenerated from the saved seed in the backward
            seed = lo.seed_for(li, gname)
            xa = hk.dropout(x, pd, seed)
            if save is not None:
                save["seed_" + gname] = seed
        T = hk.gemm_nt_skinny(xa, lo.view(lo.shadow, li, gname, "A"), alpha=lo.s)
        if save is not None:
            save["T_" + gname] = T
        return T, lo.derived[(li, gname, "Bfull")]

    def _lin(self, li, gname, x, L, residual=None, save=None, xq=None, rope=None):
        """y = x W^T (+ s (x A^T) B^T when the group carries adapters) (+ residual), W = L[gname + "_w"] in the arithmetic of `self.base`; the
        adapter update stays bf16 and rides on the same accumulators.  xq: the producer already emitted the 8-bit operand of x.
        rope = (pos_mod, pos0): the qkv projection - RoPE of the q / k heads."""
        T, Bfull = self._adapter_down(li, gname, x, save)
        return self.base.product(self, L, gname + "_w", x, xq, residual, T, Bfull, rope)

    def _gu_fwd(self, li, h, L, save, xq=None):
        """gate|up projection + SwiGLU -> (gu [M, 2ff], act [M, ff] or None, 8-bit operand of act or None)"""
        return self.base.gu_fwd(self, li, h, xq, L, save)

    def _down_bwd(self, li, dy, L, gu, act, T, dyq=None, drop=None):
        """-> (dgu = swiglu'(gu) * d_act, written over gu, or None; its 8-bit operand for the gate|up dX product or None), d_act = dy W_down (+ LoRA)"""
        return self.base.down_bwd(self, li, dy, dyq, L, gu, act, T, drop)

    def _lin_bwd(self, li, gname, dy, L, x, T, dyq=None, drop=None, **fused):
        """dx = dy W (+ s (dy B) A), W^T = L[gname + "_wT"]; adapter gradients dA = (s dy B)^T x, dB^T = (s x A^T)^T dy written into lora.grad.
        dyq: the producer's 8-bit operand of dy; drop = `_drop` of the forward; fused: see Bf16Base._dx."""
        lo, base, name = self.lora, self.base, gname + "_wT"
        dyq = base.operand(dy, dyq)
        if lo is None or gname not in lo.groups:
            return base.dx(L, name, dy, dyq, **fused)
        G = lo.groups[gname]
        U = hk.gemm_nt_skinny(dy, lo.view(lo.shadow, li, gname, "BD"), alpha=lo.s)         # [M, KP] = s * dy B
        dx = base.dx(L, name, dy, dyq, U, lo.derived[(li, gname, "AT")], drop, **fused)
        if drop is not None:
            x = hk.dropout(x, drop[0], drop[1])                                            # dA sees the same masked input
        hk.gemm_tn_skinny(U, x, lo.view(lo.grad, li, gname, "A"))
        dBD = hk.gemm_tn_skinny(T, dy, lo.view(lo.grad, li, gname, "BD"))
        hk.blockdiag_mask(dBD, lo.r, G["fout"], G["mask"])
        return dx

    # ------------------------------------------------------------------ splice
    def prepare_inputs_for_multimodal(self, input_ids, attention_mask, labels, image_embedding):
        """Device-side restatement of text_modal.py:296-526 (tune_im_start off) -> (embeds, labels, mask, img_pos).  One placeholder per sample:
        everything on the device (`lhrs_splice_fwd`).  Several placeholders in a sample (or an image tensor with one slot per placeholder): the
        walk runs on the host (`splice_plan_host`), the device copies rows through its map; the fourth value is then the inverse map."""
        ids = input_ids.to(self.device)
        B, T = ids.shape
        if image_embedding is None:  # text-only turn (text_modal.py:321-339): no <image> token may be present, plain embeddings
            if bool((ids == IMAGE_TOKEN_INDEX).any()):
                raise ValueError("input_ids contain the <image> placeholder but no image embedding was given")
            image_embedding = torch.zeros((B, 1, self.d), device=self.device, dtype=torch.bfloat16)
        NI = image_embedding.shape[1]
        has_img = (ids == IMAGE_TOKEN_INDEX).any(dim=1)
        n_img = (ids == IMAGE_TOKEN_INDEX).sum(dim=1)
        if int(n_img.max()) > 1 or image_embedding.shape[0] != B:   # several placeholders in a sample: host walk + mapped copy (text_modal.py:341-438)
            ids_h, lab_h, msk_h = self._ints_to_host(input_ids, labels, attention_mask)
            plan = self.splice_plan_host(ids_h, lab_h, msk_h, NI)
            self._check_slots(plan, image_embedding)
            embeds = hk.splice_map_fwd(ids, hk.h2d(plan["src_tok"], self.device), hk.h2d(plan["src_img"], self.device), image_embedding.contiguous(),
                                       self.p["embed"], plan["S"])
            return embeds, hk.h2d(plan["labels"], self.device), hk.h2d(plan["mask"], self.device), hk.h2d(plan["inv"], self.device)
        S = T - 1 + NI if bool(has_img.any()) else T
        lab = None if labels is None else labels.to(self.device)
        msk = None if attention_mask is None else attention_mask.to(self.device)
        return hk.splice_fwd(ids, lab, msk, image_embedding.contiguous(), self.p["embed"], S)

    # ------------------------------------------------------------------ forward
    def _layer_fwd(self, L, x, B, S, desc, LT, save, li=0, tail=None):
        """One decoder layer.  tail = (rows int32 [n], desc, max_q): the LAST layer of a training forward whose supervised positions
        form one contiguous range per sequence - only those rows of its output are ever read (final norm -> lm_head -> loss), so the
        attention runs for those queries only (all keys), and o_proj / residual / RMSNorm / MLP run on the n gathered rows instead of
        all B*S.  HF computes every row and the loss ignores them: same loss, same gradients, ~0.4 of a layer's linear work less."""
        d, H, hd, ff = self.d, self.heads, self.hd, self.ff
        M = x.shape[0]
        if self._native_layer(tail):   # frozen bf16 base, no adapters, every row: the whole layer is ONE call into the library (same launches, same order)
            if getattr(self, "_h_scratch", None) is None or self._h_scratch.shape != x.shape:
                self._h_scratch = torch.empty_like(x)
            x_out, rec = hk.llama_layer_forward(x, L, self.cos, self.sin, desc, B, S, LT, H, ff, self.eps, self._h_scratch)
            if save is not None:
                save.append(rec)
            return x_out
        rec = {} if save is not None else None
        base = self.base  # its norms and SwiGLU hand the 8-bit operand of the next product on (hq, actq; None in bf16)
        h, hq = base.norm_fwd(x, L["ln1_w"], self.eps, self._has("qkv"))
        qkv = self._lin(li, "qkv", h, L, save=rec, xq=hq, rope=(S, 0))
        o = torch.empty((M, d), device=self.device, dtype=torch.bfloat16)
        lse = torch.empty((B, H, LT), device=self.device, dtype=torch.float32)
        o_full, x_res = o, x
        if tail is None:
            hk.attn_fwd(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], o, lse, desc, B, H, hd, S, S, LT, True, 1.0 / math.sqrt(hd))
        else:
            rows, tdesc, max_q = tail
            hk.attn_fwd(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], o, lse, tdesc, B, H, hd, max_q, S, LT, True, 1.0 / math.sqrt(hd))
            o, x_res = hk.gather_rows(o_full, rows), hk.gather_rows(x, rows)   # from here on: n rows
        x_mid = self._lin(li, "o", o, L, residual=x_res, save=rec)
        h, hq = base.norm_fwd(x_mid, L["ln2_w"], self.eps, self._has("gu"), out=h if tail is None else None)
        gu, act, actq = self._gu_fwd(li, h, L, rec, xq=hq)
        x_out = self._lin(li, "down", act, L, residual=x_mid, save=rec, xq=actq)
        if save is not None:
            rec.update(x_in=x, qkv=qkv, o=o, o_full=o_full, lse=lse, x_mid=x_mid, gu=gu)
            save.append(rec)
        return x_out

    def _native_layer(self, tail) -> bool:
        """True when a decoder layer can go through the module-level entry points (lhrs_llama_layer_forward / _backward): the frozen bf16
        base without adapters, on every row (the compact last layer keeps the operator path).  LHRS_NATIVE_LAYER=0: operator path (A/B, tests)."""
        return tail is None and self.lora is None and self.base.native_layer and self.hd == 128 and os.environ.get("LHRS_NATIVE_LAYER", "1") != "0"

    def forward_hidden(self, embeds, mask_u8, save_ctx=True, kv_len=None, tail=None):
        """embeds [B,S,d] bf16, mask [B,S] uint8 (right padding) -> final-norm hidden [B*S, d].  kv_len: the per-sequence key counts when
        the caller already has them on the host (saves the device round trip of summing the mask).  tail = [(p0, n)] per sequence: only
        the positions [p0, p0 + n) are needed from the last layer on (see _layer_fwd) -> hidden [sum n, d] of those rows, sequence-major."""
        B, S, d = embeds.shape
        if S > self.cos.shape[0]:
            raise ValueError(f"sequence length {S} exceeds the {self.cos.shape[0]} positions of the RoPE table")
        if kv_len is None:
            kv_len = mask_u8.to(torch.int32).sum(dim=1).tolist() if mask_u8 is not None else [S] * B
        desc = hk.make_desc([(b * S, S, b * S, int(kv_len[b]), S, 0) for b in range(B)], self.device)
        LT = hk.pad64(S)
        saved: Optional[List] = [] if save_ctx else None
        if self.lora is not None:
            self.lora.drop_epoch += 1  # a fresh dropout mask per forward pass
        x = embeds.reshape(B * S, d)
        nl = len(self.p["layers"])
        tail_t = None
        if tail is not None and nl > 0:
            rows = torch.cat([torch.arange(b * S + p0, b * S + p0 + n, dtype=torch.int32) for b, (p0, n) in enumerate(tail)])
            tdesc = hk.make_desc([(b * S + p0, n, b * S, int(kv_len[b]), S, p0) for b, (p0, n) in enumerate(tail)], self.device)
            tail_t = (hk.h2d(rows, self.device), tdesc, max(n for _, n in tail))
        for li, L in enumerate(self.p["layers"]):
            x = self._layer_fwd(L, x, B, S, desc, LT, saved, li, tail=tail_t if li == nl - 1 else None)
        hidden = hk.rmsnorm_fwd(x, self.p["norm_w"], self.eps)
        if save_ctx:
            self._ctx = dict(B=B, S=S, desc=desc, LT=LT, layers=saved, x_last=x, tail=tail_t)
        return hidden

    @staticmethod
    def splice_ints_host(ids, labels, mask, NI):
        """Host mirror of the INTEGER outputs of `lhrs_splice_fwd` (text_modal.py:296-526: spliced length, labels, mask) on CPU tensors -
        what the training step needs on the host anyway (attention descriptor, supervised rows), computed without asking the device.
        -> (S, has_image [B] bool, new_labels [B,S] int64, new_mask [B,S] uint8); tests pin it to the device kernel."""
        B, T = ids.shape
        is_img = ids == IMAGE_TOKEN_INDEX
        n_img = is_img.sum(dim=1)
        if int(n_img.max()) > 1:
            raise ValueError("several <image> placeholders in a sample: use splice_plan_host (the general walk)")
        has = n_img > 0
        S = T - 1 + NI if bool(has.any()) else T
        p = torch.where(has, is_img.to(torch.int64).argmax(dim=1), torch.full((B,), T, dtype=torch.int64))[:, None]
        hasb = has[:, None]
        j = torch.arange(S, dtype=torch.int64)[None, :]
        new_len = torch.where(hasb, torch.full_like(p, T - 1 + NI), torch.full_like(p, T))
        shift = new_len - T
        src_tok = torch.where(~hasb | (j < p), j.expand(B, S), torch.where(j < p + NI, torch.full((B, S), -1, dtype=torch.int64), j - NI + 1))
        src_tok = torch.where(j < new_len, src_tok, torch.full_like(src_tok, -1))
        if labels is None:
            new_labels = torch.full((B, S), IGNORE_INDEX, dtype=torch.int64)
        else:
            new_labels = torch.where(src_tok >= 0, labels.to(torch.int64).gather(1, src_tok.clamp(0, T - 1)), torch.full((B, S), IGNORE_INDEX, dtype=torch.int64))
        m = torch.ones((B, T), dtype=torch.uint8) if mask is None else mask.to(torch.uint8)
        new_mask = torch.where(j < new_len, torch.where(j < shift, torch.ones((B, S), dtype=torch.uint8), m.gather(1, (j - shift).clamp(0, T - 1))),
                               torch.zeros((B, S), dtype=torch.uint8))
        return S, has, new_labels, new_mask

    @staticmethod
    def splice_plan_host(ids, labels, mask, NI, tune_im_start=False):
        """The GENERAL walk of prepare_inputs_for_multimodal (text_modal.py:318-438) on CPU tensors: any number of <image> placeholders per
        sample, each one taking the next image SLOT of a counter that runs over the batch and that a placeholder-free sample advances too
        (`cur_image_idx`, :339, :402).  -> dict(S, n_slots, labels int64 [B,S], mask uint8 [B,S], src_tok int32 [B,S] (token index or -1),
        src_img int32 [B,S] (row of the flattened slots [n_slots * NI] or -1), inv int32 [n_slots * NI] (flat output row b * S + j that copies
        image row r, -1 for a slot nobody took)).  tune_im_start: the integer side of the `tune_pooler and tune_im_start` branch (:353-387) -
        the token map is the plain one, the label kept behind the image is the placeholder's own and the walk resumes two tokens on."""
        B, T = ids.shape
        rows_tok, rows_img, rows_lab = [], [], []
        slot = 0
        for b in range(B):
            cur = ids[b].tolist()
            lab = labels[b].tolist() if labels is not None else None
            tok, img, nl = [], [], []
            base = 0
            if IMAGE_TOKEN_INDEX not in cur:
                tok, img, nl = list(range(T)), [-1] * T, (list(lab) if lab is not None else [])
                slot += 1
            else:
                while IMAGE_TOKEN_INDEX in cur:
                    p = cur.index(IMAGE_TOKEN_INDEX)
                    tok += [base + i for i in range(p)] + [-1] * NI
                    img += [-1] * p + [slot * NI + k for k in range(NI)]
                    step = 1
                    if tune_im_start:
                        if p + 1 >= len(cur):
                            raise ValueError("tune_im_start: every <image> placeholder needs its <im_end> neighbour (cap_dataset.py:875-876)")
                        tok.append(base + p + 1)
                        img.append(-1)
                        step = 2
                    if lab is not None:
                        nl += lab[:p] + [IGNORE_INDEX] * NI + (lab[p:p + 1] if tune_im_start else [])
                        lab = lab[p + step:]
                    cur = cur[p + step:]
                    base += p + step
                    slot += 1
                tok += [base + i for i in range(len(cur))]
                img += [-1] * len(cur)
                if lab is not None:
                    nl += lab
            rows_tok.append(tok); rows_img.append(img); rows_lab.append(nl)
        S = max(len(r) for r in rows_tok)
        src_tok = torch.full((B, S), -1, dtype=torch.int32)
        src_img = torch.full((B, S), -1, dtype=torch.int32)
        new_labels = torch.full((B, S), IGNORE_INDEX, dtype=torch.int64)
        new_mask = torch.zeros((B, S), dtype=torch.uint8)
        inv = torch.full((max(slot, 1) * NI,), -1, dtype=torch.int32)
        m = torch.ones((B, T), dtype=torch.uint8) if mask is None else mask.to(torch.uint8)
        for b in range(B):
            n = len(rows_tok[b])
            src_tok[b, :n] = torch.tensor(rows_tok[b], dtype=torch.int32)
            src_img[b, :n] = torch.tensor(rows_img[b], dtype=torch.int32)
            if labels is not None:
                new_labels[b, :n] = torch.tensor(rows_lab[b], dtype=torch.int64)
            new_mask[b, : n - T] = 1                      # the reference left-extends the mask by the growth of the row (:511-524)
            new_mask[b, n - T: n] = m[b]
            j = torch.nonzero(src_img[b] >= 0).squeeze(1)
            inv[src_img[b, j].long()] = (b * S + j).to(torch.int32)
        return dict(S=S, n_slots=slot, labels=new_labels, mask=new_mask, src_tok=src_tok, src_img=src_img, inv=inv)

    def _splice_general(self, ids_h, image_embedding, NI):
        """True when the batch needs the general walk: a sample with several placeholders, or an image tensor that is not one slot per sample."""
        n_img = (ids_h == IMAGE_TOKEN_INDEX).sum(dim=1)
        return int(n_img.max()) > 1 or image_embedding.shape[0] != ids_h.shape[0]

    def _check_slots(self, plan, image_embedding):
        if plan["n_slots"] > image_embedding.shape[0]:   # the reference: IndexError at image_embedding[cur_image_idx] (text_modal.py:343-345)
            raise IndexError(f"the batch takes {plan['n_slots']} image slots (one per <image> placeholder, one per placeholder-free sample) but "
                             f"image_embedding holds {image_embedding.shape[0]}")

    def _ints_to_host(self, *ts):
        """CPU views of the small integer inputs.  Host tensors (what a DataLoader delivers) pass through; device tensors cost ONE
        synchronising copy for all of them."""
        if not any(t is not None and t.is_cuda for t in ts):
            return list(ts)
        if os.environ.get("LHRS_INTS_PAGEABLE") == "1":   # the pre-round-5 path (A/B of the shared-device NaN hunt): async copies into PAGEABLE host memory
            out = [None if t is None else (t if not t.is_cuda else t.to("cpu", non_blocking=True)) for t in ts]
            torch.cuda.current_stream().synchronize()
            return out
        # device -> PINNED staging buffers of this model, one synchronisation, then plain host copies of them: the runtime does not have to pin / stage / unpin
        # pageable pages around an asynchronous copy at the start of every step.  ONE flat pinned buffer per (argument slot, dtype), grown geometrically to the
        # largest element count seen and viewed per call: ragged batches (every distinct (B, T)) do not accumulate page-locked memory
        cache = self.__dict__.setdefault("_ints_pinned", {})
        stage = []
        for i, t in enumerate(ts):
            if t is None or not t.is_cuda:
                stage.append(None)
                continue
            key = (i, t.dtype)
            n = t.numel()
            if key not in cache or cache[key].numel() < n:
                cache[key] = torch.empty(max(n, 2 * cache[key].numel() if key in cache else n), dtype=t.dtype, pin_memory=True)
            view = cache[key][:n].view(t.shape)
            view.copy_(t, non_blocking=True)
            stage.append(view)
        torch.cuda.current_stream().synchronize()
        return [t if p is None else p.clone() for t, p in zip(ts, stage)]

    def decode(self, input_ids, image_embedding=None, attention_mask=None, labels=None, save_ctx=True, host_ints=None):
        """TextModal.decode: returns the scalar text loss (0-dim fp32 device tensor).  All integer bookkeeping of the step (spliced
        length, key counts, supervised rows, shifted targets) happens on the host from the host copies of ids / labels / mask, so the
        launch queue is never drained in the middle of a step; the device splice only moves embedding rows.  host_ints: those copies
        when the caller fetched them already (UniBind.forward does, before it enqueues the ViT)."""
        if labels is None:
            raise ValueError("decode() computes the training loss: labels are required")
        if save_ctx:
            self._merged_cache = None     # a training step follows: do not pin ~13.5 GB of merged generate() weights through it
        ids_h, lab_h, msk_h = host_ints if host_ints is not None else self._ints_to_host(input_ids, labels, attention_mask)
        B, T = ids_h.shape
        if image_embedding is None:
            if bool((ids_h == IMAGE_TOKEN_INDEX).any()):
                raise ValueError("input_ids contain the <image> placeholder but no image embedding was given")
            image_embedding = torch.zeros((B, 1, self.d), device=self.device, dtype=torch.bfloat16)
        NI = image_embedding.shape[1]
        plan = None
        if self._splice_general(ids_h, image_embedding, NI):
            plan = self.splice_plan_host(ids_h, lab_h, msk_h, NI)
            self._check_slots(plan, image_embedding)
            S, new_labels, new_mask = plan["S"], plan["labels"], plan["mask"]
        else:
            S, _, new_labels, new_mask = self.splice_ints_host(ids_h, lab_h, msk_h, NI)
        # shifted targets: position j predicts label j+1 (HF LlamaForCausalLM.forward); ignore_index rows are skipped
        tgt = torch.full_like(new_labels, IGNORE_INDEX)
        tgt[:, :-1] = new_labels[:, 1:]
        flat = tgt.reshape(-1)
        rows = torch.nonzero(flat != IGNORE_INDEX).squeeze(1)
        if rows.numel() == 0:
            raise ValueError("no valid target token in the micro-batch (loss would be NaN in the reference)")
        rows32 = hk.h2d(rows.to(torch.int32), self.device)
        targets = hk.h2d(flat[rows].to(torch.int32), self.device)
        ids_d = input_ids if input_ids.is_cuda else hk.h2d(ids_h.contiguous(), self.device)
        if plan is None:
            embeds, _, _, img_pos = hk.splice_fwd(ids_d, None, None, image_embedding.contiguous(), self.p["embed"], S)
            img_inv = None
        else:
            embeds = hk.splice_map_fwd(ids_d, hk.h2d(plan["src_tok"], self.device), hk.h2d(plan["src_img"], self.device),
                                       image_embedding.contiguous(), self.p["embed"], S)
            img_pos, img_inv = None, (hk.h2d(plan["inv"], self.device), image_embedding.shape[0])
        # supervised positions of each sequence: when they form ONE contiguous range (stage 1: the caption at the end of the sequence; any
        # single-answer sample) the last decoder layer only has to produce those rows
        tail = None
        if self.tail_rows_only and self.p["layers"]:
            valid = tgt != IGNORE_INDEX
            cnt = valid.sum(dim=1)
            first = valid.to(torch.int64).argmax(dim=1)
            last = S - 1 - valid.flip(1).to(torch.int64).argmax(dim=1)
            if bool((cnt > 0).all()) and bool((last - first + 1 == cnt).all()):
                tail = list(zip(first.tolist(), cnt.tolist()))
        hidden = self.forward_hidden(embeds, None, save_ctx, kv_len=new_mask.to(torch.int32).sum(dim=1).tolist(), tail=tail)
        self.last_hidden = hidden  # final-norm output of this call: [B*S, d], or the supervised rows only in tail mode (tests read it)
        hv = hidden if tail is not None else hk.gather_rows(hidden, rows32)
        logits = hk.gemm_nt(hv, self.p["lm_head"])
        loss, dlogits = hk.cross_entropy(logits, targets, want_grad=save_ctx, inplace=True)
        if save_ctx:
            self._ctx.update(rows=rows32, dlogits=dlogits, img_pos=img_pos, img_inv=img_inv, NI=NI)
        return loss

    __call__ = decode

    # ------------------------------------------------------------------ generate (KV cache): generation.py, bound here so that callers go through the model
    _layer_step, _check_kv_cache, _alloc_kv = generation.layer_step, generation.check_kv_cache, generation.alloc_kv
    _generate = generation.generate_rows

    def _decode_session(self, B, max_ctx, caches, max_new, weights="bf16", kmask=None, lora=None, kv_cache="bf16"):
        return generation.DecodeSession(self, B, max_ctx, caches, max_new, weights, kmask, lora, kv_cache)

    def choice_constraint(self, choices, eos_token_id=None):
        """-> generation.TokenAutomaton on this model's device for `generate(constraint=...)`: the answer is exactly one of `choices`
        (strings, tokenised without special tokens, or token-id lists) followed by EOS (default: the tokenizer's); choice i ends in the
        final state of label i."""
        tok = self.tokenizer
        eos = getattr(tok, "eos_token_id", None) if eos_token_id is None else eos_token_id
        if eos is None:
            raise ValueError("choice_constraint: the tokenizer has no eos_token_id - pass one")
        lists = []
        for c in choices:
            if isinstance(c, str):
                ids = list(tok(c, add_special_tokens=False).input_ids)
                if ids and ids[0] == getattr(tok, "bos_token_id", None):   # a tokenizer that adds its BOS whatever it is told (SyntheticTokenizer)
                    ids = ids[1:]
                c = ids
            lists.append([int(t) for t in c])
        pad = getattr(tok, "pad_token_id", None)
        return generation.choice_automaton(lists, int(eos), 0 if pad is None else int(pad), self.vocab, self.device)

    def new_prefix_cache(self, kv_cache="bf16", max_positions=None):
        """-> generation.PrefixCache of this model for `generate(prefix_cache=...)`: the KV cache of one conversation, kept between calls"""
        return generation.PrefixCache(self, kv_cache, max_positions)

    def quantize_fp8(self):
        """e4m3 copies (per-output-row scale) of every LLaMA linear for the decode step: 6.7 GB instead of 13.5 GB per token."""
        generation.quantize_fp8(self)

    def pack_fp8_decode(self):
        """Decode-only copies of the e4m3 weights in the MFMA GEMV's operand order (hk.repack_fp8_mfma): the batch-1 weight stream then
        reads consecutive 1-KiB lines instead of 64-B segments of 16 strided rows (+6.7 GB of HBM next to the row-major copies that
        the prefill / training GEMMs use)."""
        generation.FORMATS["fp8"].pack(self)

    def pack_bf16_decode(self):
        """Decode-only copies of the bf16 weights in the batched MFMA GEMV's operand order (hk.repack_bf16_mfma; +13.5 GB of HBM): from
        batch 2 the shared weight stream of generate() reads consecutive 1-KiB lines instead of 64-B segments of 16 strided rows."""
        generation.FORMATS["bf16"].pack(self)

    def pack4_decode(self):
        """Decode-only form of the 4-bit base (`weights="4bit"`): per fused weight the stored codes of its reference Linears side by side and
        their block statistics in fp32 (`hk.pack4_decode`: +3.6 GB next to the `q4` states; nothing is quantised anew).  lm_head is not
        quantised in the reference and has no 4-bit form."""
        generation.FORMATS["4bit"].pack(self)

    def pack_mx4_decode(self):
        """Decode-only MXFP4 form of the decoder linears (`weights="mxfp4"`): whatever bf16 weight the decoder currently holds is quantised to
        OCP MXFP4 (`hk.quant_mx4_rows`: e2m1 codes, one e8m0 scale per 32 consecutive k) and re-tiled into the operand order of `hk.gemv_mx4`;
        only the tiled pair stays, under `L[name + "mx4"]` (+3.5 GB at full depth; the row-major temporaries of a weight are freed before the
        next one is made).  Lossy, like `quantize_fp8`.  lm_head has no MXFP4 form."""
        generation.FORMATS["mxfp4"].pack(self)

    def pack_int8_decode(self):
        """Decode-only copies of the int8 rows of the LLM.int8 base in the operand order of `hk.gemv_int8` (`hk.repack_int8_mfma`), under
        `L[name + "i8p"]` (+6.7 GB at full depth next to the row-major rows that the prefill and training products read): the single-token
        weight stream then reads consecutive 1-KiB lines.  The codes are the base's own; nothing is quantised anew.  lm_head is not
        quantised in the reference and has no int8 form."""
        generation.FORMATS["int8"].pack(self)

    def quantize_base(self, bits: int = 8, scheme: str = "e4m3", quant_type: str = "nf4", double_quant: bool = True):
        """`bits: 8` of Config/multi_modal_stage{2,3}.yaml (text_modal.py:91-131: the reference loads the frozen LLaMA through bitsandbytes
        LLM.int8 for stages 2/3; lm_head stays 16-bit there and here).  Two schemes:

        * "int8" - the reference's arithmetic (what `UniBind.prepare_for_training` picks for the YAML key): every decoder linear is stored as
          int8 rows + absmax factors (vector-wise), the forward is bitsandbytes' MatMul8bitLt - int8 x int8 -> int32 on the MFMA with
          the activation's outlier columns (any |x| >= 6.0) taken out into a 16-bit product (`hk.int8_linear`) -, the backward multiplies
          with the DEquantised weight in 16 bit.  The bf16 weights of this object BECOME the dequantised ones (generate, merges and the dX
          GEMMs read them).  Parity: oracle/int8_oracle.py (bitsandbytes itself is not installed: unpinned against the package).
        * "e4m3" - MI355X-native fast path: OCP e4m3 copies with one fp32 scale per output row - of W for the forward product and of W^T for
          the dX product - on the 2x-rate block-scaled MFMA, activations / gradients quantised per row on the fly, no outlier split.
        LoRA adapters, norms, attention and the loss stay bf16 / fp32 in both.

        `bits: 4` (text_modal.py:91-107 `load_in_4bit`, `quant_type` nf4 | fp4, `double_quant`): bitsandbytes' Linear4bit stores 4-bit codes
        per block of 64 and computes every product on the DEquantised weight in the compute dtype, forward and backward.  Here each
        reference Linear (q, k, v, o, gate, up, down - the statistics of `double_quant` are per Linear) is quantised by `hk.quant4_blocks`,
        the codes and statistics stay beside the weight (`<name>q4`), and the bf16 weight BECOMES `hk.dequant4_blocks` of them: the ordinary
        bf16 kernels then run the arithmetic bitsandbytes runs.  Parity: oracle/nf4_oracle.py (unpinned against the package)."""
        self._merged_cache = None     # generate() must not answer from pre-quantisation merged weights
        if bits == 4:
            base = Bf16Base(storage4=(quant_type, bool(double_quant)))
        elif bits not in (8, 16):
            raise NotImplementedError(f"bits={bits}: 16 (bf16), 8 (LLM.int8 / e4m3 base weights) or 4 (nf4 / fp4 storage)")
        elif scheme not in ("e4m3", "int8"):
            raise ValueError(f"quantize_base scheme {scheme!r}: 'int8' (LLM.int8, the reference's) or 'e4m3'")
        else:
            base = Bf16Base() if bits == 16 else Int8Base() if scheme == "int8" else E4m3Base()
        base.install(self)
        self.base = base
        return self

    def _lora_merged_layers(self):
        """Decoder layers with W + s B A in place of every adapted weight (copies; the base stays untouched) for generate() with un-merged
        adapters.  Cached together with the decode re-tilings / e4m3 copies that `_decode_session` hangs onto the dicts, keyed on the adapter
        store's `version` (bumped by every optimizer step and load): an evaluation loop between two optimizer steps merges ONCE."""
        lo = self.lora
        cache = self._merged_cache
        if cache is not None and cache[0] == (id(lo), lo.version):
            return cache[1]
        out = []
        for li, L in enumerate(self.p["layers"]):
            M = {k: L[k] for k in ("ln1_w", "ln2_w", "qkv_w", "o_w", "gu_w", "down_w")}
            for gname in lo.groups:
                W = L[gname + "_w"]
                M[gname + "_w"] = hk.gemm_nt(lo.derived[(li, gname, "Bfull")], lo.derived[(li, gname, "AT")], residual=W, alpha=lo.s)
            out.append(M)
        self._merged_cache = ((id(lo), lo.version), out)
        return out

    @contextlib.contextmanager
    def _decoding_on(self, weights, layers=None):
        """generate() with un-merged adapters: the GEMM steps (prefill, batch > 16) run `_lin` / `_gu_fwd` on the bf16 weights - the 4-bit
        storage keeps its name, `weights="int8"` keeps the LLM.int8 base it streams - and on `layers` (merged copies) when given.  The model's
        own scheme and layers come back however the call ends."""
        saved = self.base, self.p["layers"]
        if not generation.int8_gemm(weights):
            self.base = Bf16Base(self.base.storage4)
        if layers is not None:
            self.p["layers"] = layers
        try:
            yield
        finally:
            self.base, self.p["layers"] = saved

    @contextlib.contextmanager
    def _adapters_on(self, adapters, weights):
        """generate() with un-merged adapters (`adapters` None: there are none): "live" - nothing is merged or swapped, the bf16 base weights
        serve prefill, `weights` picks the decode stream, dropout is off; "merged" - merged 16-bit copies (no 8-bit operands of them exist)"""
        if adapters is None:
            yield
        elif adapters == "live":
            lo = self.lora
            train, lo.train_mode = lo.train_mode, False
            try:
                with self._decoding_on(weights):
                    yield
            finally:
                lo.train_mode = train
        else:
            with self._decoding_on(weights, self._lora_merged_layers()):
                yield

    @torch.no_grad()
    def generate(self, input_ids, image_embedding=None, attention_mask=None, do_sample=False, temperature=1.0, top_p="default",
                 top_k="default", max_new_tokens=512, use_cache=True, stopping_criteria=None, streamer=None, eos_token_id="default",
                 return_logits=False, use_graph=True, weights="bf16", sampler="torch", seed=None, repetition_penalty=1.0, num_beams=1,
                 length_penalty=1.0, early_stopping=False, return_beam_scores=False, adapters="merged", kv_cache=None, prefix_cache=None,
                 constraint=None, return_choices=False, **_kw):
        """See `_generate`.  Two things happen here first: (1) `eos_token_id` defaults to the tokenizer's EOS, as HF `generate` stops on
        the generation config's EOS (pass None to disable); (2) if LoRA adapters are attached and not merged, `adapters` says how they run:
        "merged" (default) - on merged COPIES of the affected weights (`_lora_merged_layers`), the base weights come back untouched;
        "live" - no copies: prefill and the batch > 16 steps run the training forward with dropout off, and the single-token step runs
        `hk.lora_down` / `hk.lora_up` around the base GEMV of whatever `weights` streams (`_decode_session`), "4bit" included and "fp8" on the
        e4m3 copies of the BASE weights; what it computes is x W^T + (s x A^T) B^T on one fp32 value, as training does, where "merged" rounds
        W + s B A to bf16 first.  Without adapters "live" changes nothing.

        `weights`: what the single-token step streams - "bf16" (default, whatever the base), "fp8" (e4m3 copies on the block-scaled MFMA) or
        "4bit" (the codes and block statistics of `quantize_base(4)` through `hk.gemv4`; the decoder linears then compute what "bf16" computes
        on the dequantised weights up to the order of the fp32 sums; lm_head stays bf16).  "4bit" raises ValueError without the 4-bit base and
        with un-merged adapters unless `adapters="live"`.
        "mxfp4" - on any base: the decoder linears stream OCP MXFP4 copies (e2m1 codes + one e8m0 scale per 32 k, 0.53 B per weight, made by
        `pack_mx4_decode` from whatever bf16 weights the decoder holds at the first call - merged copies included) against per-row e4m3
        activations on the block-scaled MFMA (`hk.gemv_mx4`).  Lossy like "fp8"; the prefill stays on the bf16 GEMMs in every mode but "int8".
        "int8" - only on the LLM.int8 base (`quantize_base(8, "int8")`, else ValueError): the decoder linears stream the base's own int8 rows
        and row factors (1 B per weight, re-tiled once by `pack_int8_decode`) in the arithmetic of bitsandbytes' MatMul8bitLt (per linear
        `hk.int8_decode_prepare` + `hk.gemv_int8`), and the prefill and the batch > 16 step run `hk.int8_linear`: the whole call computes what
        the reference's `generate` computes on a `load_in_8bit` model.  With un-merged adapters it needs `adapters="live"`.  lm_head stays bf16
        in every format but "fp8".

        `kv_cache`: "bf16" (default) or "fp8" - e4m3 codes and one e8m0 scale byte per head row (the kv8 format of csrc/decode_attn.hip: half
        the cache memory and stream).  The prefill attends over the exact bf16 K / V of the prompt, so its logits and the first token are those
        of "bf16"; from the second token on the step reads the rounded cache (`hk.decode_attn_kv8`).  Works with every `weights` / `adapters` /
        sampler mode, left padding and beams; needs head_dim 128 and batch x num_beams <= 16, else ValueError.  None (default): "bf16", or
        with `prefix_cache` the kind of that cache.

        `prefix_cache`: a `PrefixCache` of this model (`new_prefix_cache`) that keeps the KV cache of a conversation between calls.  The
        prompt is matched against the cached ids, the common prefix - the image block included when the image embedding is the cached one,
        which is also used when `image_embedding` is None - is not prefilled again, and on return the cache holds the prompt and every new
        token but the last.  The new positions attend each other in exact bf16, as the positions of any prompt do, and the reused ones
        through the cache: bf16 rows, or with an "fp8" cache the e4m3 codes (dequantised exactly by `hk.kv8_dequant_rows`), as the
        single-token step reads them - so behind an "fp8" prefix the first token is no longer the "bf16" one.  Batch 1, no beams, no
        padding mask, one placeholder, prompt + max_new_tokens <= `max_positions`; anything else raises ValueError and leaves the cache as it was.
        Every `weights` / `adapters` / sampler mode works; the cache does not know which produced its rows - `reset()` it when they change.

        `constraint`: a `TokenAutomaton` (`choice_constraint`, or the builders of generation.py) - the answer is a path through it: every
        pick is the best ALLOWED token (`hk.constrain_rows`), rows that reached a final state emit pad_token_id, and the call ends when
        all rows are final (the ids are cut to the longest row, its EOS included) or at max_new_tokens.  The automaton carries its own
        EOS edges, so the "default" `eos_token_id` is None here: the host then looks at the rows only every fourth token.  Greedy only:
        do_sample, num_beams != 1, repetition_penalty != 1 and prefix_cache raise ValueError, as does an automaton of another vocabulary
        size or device.  `return_choices=True` appends (choice [B] int64 - the label of the final state, -1 where max_new_tokens ran out
        first -, score [B] fp32 - the sum of the picked tokens' log-probabilities, normalised over the full vocabulary as HF's scores are)."""
        return generation.run_request(generation.resolve_request(self, {**locals(), "num_return_sequences": _kw.get("num_return_sequences", 1)}))

    # ------------------------------------------------------------------ backward (activation gradients only)
    def backward(self, loss_scale: float = 1.0, need_input_grad: bool = True, on_layer_ready=None):
        """d loss / d image_embedding [B, NI, d] bf16 (None when need_input_grad is False).  With LoRA enabled the adapter
        gradients of layer l are final when its backward finishes; on_layer_ready(l) lets the engine all-reduce them."""
        c = self._ctx
        assert c is not None, "decode(save_ctx=True) must precede backward"
        B, S, desc, LT = c["B"], c["S"], c["desc"], c["LT"]
        d, H, hd, ff, p = self.d, self.heads, self.hd, self.ff, self.p
        base, has = self.base, self._has  # the norm backwards and SwiGLU' hand the 8-bit operand of the next dX product on (None in bf16)
        M = B * S
        dhv = hk.gemm_nt(c["dlogits"], p["lm_headT"], alpha=loss_scale)
        tail = c.get("tail")
        if tail is None:
            dhid = torch.zeros((M, d), device=self.device, dtype=torch.bfloat16)
            hk.scatter_rows(dhv, c["rows"], dhid)
        else:
            dhid = dhv  # x_last holds exactly the supervised rows: the last layer's backward starts compact
        dx, dxq = base.norm_bwd(dhid, c["x_last"], p["norm_w"], self.eps)
        scale = 1.0 / math.sqrt(hd)
        delta = torch.empty((B, H, LT), device=self.device, dtype=torch.float32)
        dqkv = torch.empty((M, 3 * d), device=self.device, dtype=torch.bfloat16)
        nl = len(p["layers"])
        for li in reversed(range(nl)):
            L, s = p["layers"][li], c["layers"][li]
            tl = tail if li == nl - 1 else None  # tail layer: dx, dgu, dh, dx_mid, do below have n rows until they are scattered back
            if self._native_layer(tl):
                dx, _ = hk.llama_layer_backward(dx, s, L, self.cos, self.sin, desc, B, S, LT, H, ff, self.eps, delta, dqkv)
                s.clear()
                if on_layer_ready is not None:
                    on_layer_ready(li)
                continue
            gu, qkv = s["gu"], s["qkv"]
            act = hk.swiglu_fwd(gu, ff) if has("down") else None      # x of the down projection
            dgu, dguq = self._down_bwd(li, dx, L, gu, act, s.get("T_down"), dyq=dxq, drop=self._drop(s, "down"))
            h2 = hk.rmsnorm_fwd(s["x_mid"], L["ln2_w"], self.eps) if has("gu") else None
            dh = self._lin_bwd(li, "gu", dgu, L, h2, s.get("T_gu"), dyq=dguq, drop=self._drop(s, "gu"))
            dx_mid, dmq = base.norm_bwd(dh, s["x_mid"], L["ln2_w"], self.eps, add=dx, out=dh)
            do = self._lin_bwd(li, "o", dx_mid, L, s["o"], s.get("T_o"), dyq=dmq, drop=self._drop(s, "o"))
            adesc, max_q = desc, S
            if tl is not None:
                rows_t, adesc, max_q = tl
                do = hk.scatter_rows(do, rows_t, torch.empty((M, d), device=self.device, dtype=torch.bfloat16))   # only query rows are read
                dx_mid = hk.scatter_rows(dx_mid, rows_t, torch.zeros((M, d), device=self.device, dtype=torch.bfloat16))  # residual path: 0 elsewhere
                dqkv[:, :d].zero_()                                                                                # dq exists for the query rows only
            # delta = rowsum(dO * O) inside the dQ kernel (one launch and one pass over O / dO less), inverse RoPE in the dq / dk stores
            hk.attn_bwd_o(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], do, s["o_full"], s["lse"], delta, dqkv[:, :d], dqkv[:, d:2 * d],
                          dqkv[:, 2 * d:], adesc, B, H, hd, max_q, S, LT, True, scale, rope=(self.cos, self.sin, S, 0))
            h1 = hk.rmsnorm_fwd(s["x_in"], L["ln1_w"], self.eps) if has("qkv") else None
            dh1 = self._lin_bwd(li, "qkv", dqkv, L, h1, s.get("T_qkv"), drop=self._drop(s, "qkv"))
            dx, dxq = base.norm_bwd(dh1, s["x_in"], L["ln1_w"], self.eps, add=dx_mid, out=dh1)
            s.clear()
            if on_layer_ready is not None:
                on_layer_ready(li)
        d_image = None
        if need_input_grad and c.get("img_inv") is not None:      # general splice: rows of the image slots through the inverse map
            inv, n_slots = c["img_inv"]
            if inv.numel() < n_slots * c["NI"]:                    # slots past the last one the batch took: zero gradient
                inv = torch.cat([inv, torch.full((n_slots * c["NI"] - inv.numel(),), -1, device=inv.device, dtype=torch.int32)])
            d_image = hk.splice_map_bwd(dx.view(B, S, d), inv, n_slots, c["NI"])
        elif need_input_grad:
            d_image = hk.splice_bwd(dx.view(B, S, d), c["img_pos"], c["NI"])
        self._ctx = None
        return d_image
