"""Decode throughput of generate() (BASELINE configs[4] shape: 1 image, short prompt, bf16 weights; no EOS: every run produces NEW tokens).

    python tools/decode_bench.py [NEW [WEIGHTS [BATCH]]]                         greedy (the form of before)
    python tools/decode_bench.py 256 bf16 1 --sample device --repeats 3          sampled decode, temperature 0.4, top_k 50, top_p 0.9, drawn by
                                                                                 the HIP sampler (`device`) or by the torch warpers (`torch`)
    python tools/decode_bench.py 256 bf16 8 --sample off,torch,device --repeats 3    A/B: the modes alternate inside every repeat
    python tools/decode_bench.py 256 bf16 1 --num-beams 4 --repeats 3            beam search (batch x 4 rows through the weights), alternating
                                                                                 with greedy at batch 4 x BATCH: the same rows, no beam kernels
    python tools/decode_bench.py 256 bf16,fp8,4bit 1 --repeats 3                 A/B of the weight formats: the entries of WEIGHTS alternate inside
                                                                                 every repeat.  With `4bit` in the list the model is put on the
                                                                                 4-bit base (quantize_base(4, nf4, double_quant)) before the warm-up;
                                                                                 `bf16` then streams the dequantised weights: same bytes, same speed
    python tools/decode_bench.py 256 bf16,fp8,mxfp4 1 --repeats 3                the same with the MXFP4 decode copies (any base; generate builds them
                                                                                 at the warm-up call)
    python tools/decode_bench.py 256 bf16,fp8,int8 1 --repeats 3                 the same with the int8 rows of the LLM.int8 base: with `int8` in the
                                                                                 list the model is put on quantize_base(8, "int8") before the warm-up;
                                                                                 `bf16` then streams the dequantised weights and `fp8` e4m3 copies of them
    python tools/decode_bench.py 256 bf16,4bit 1 --lora-r 8 --lora-targets q,k,v,o --adapters merged,live --repeats 3
                                                                                 un-merged LoRA adapters (random, non-zero B): generate(adapters=...)
                                                                                 modes alternate inside every repeat.  Each mode's FIRST call starts
                                                                                 from a model without derived copies and is timed on its own (merged
                                                                                 pays its merge and re-tiling there), with its peak allocated bytes;
                                                                                 merged + 4bit does not exist and prints "n/a: raises"
    python tools/decode_bench.py 256 bf16,4bit 8 --kv-cache bf16,fp8 --repeats 3   A/B of the KV cache formats (generate(kv_cache=...)): the entries
                                                                                 alternate inside every repeat; each mode's warm-up call is followed
                                                                                 by its peak allocated bytes over one more 4-token call
"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from lhrs_bot_amd.unibind import UniBind

ap = argparse.ArgumentParser()
ap.add_argument("new", nargs="?", type=int, default=64)
ap.add_argument("weights", nargs="?", default="bf16")
ap.add_argument("batch", nargs="?", type=int, default=1)
ap.add_argument("--sample", default="off", help="off = greedy; torch | device = do_sample=True with that sampler; a comma list alternates them")
ap.add_argument("--repetition-penalty", type=float, default=1.0)
ap.add_argument("--repeats", type=int, default=1, help="timed runs (one line each; one model, one warm-up)")
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--num-beams", type=int, default=1, help="> 1: mode `beam` (generate(num_beams=N)) alternates with mode `rows` (greedy at batch N x BATCH)")
ap.add_argument("--beam-only", action="store_true", help="with --num-beams: mode `beam` alone (kernel traces)")
ap.add_argument("--lora-r", type=int, default=0, help="> 0: attach un-merged LoRA adapters of this rank (alpha = 2 r, random A and B)")
ap.add_argument("--lora-targets", default="all", help="q,k,v,o | all (every decoder linear)")
ap.add_argument("--adapters", default="merged", help="merged | live | a comma list that alternates (generate(adapters=...); needs --lora-r)")
ap.add_argument("--kv-cache", default="bf16", help="bf16 | fp8 | a comma list that alternates (generate(kv_cache=...))")
a = ap.parse_args()
new, B = a.new, a.batch
weight_modes = a.weights.split(",")
assert all(w in ("bf16", "fp8", "4bit", "mxfp4", "int8") for w in weight_modes), a.weights
assert not ("4bit" in weight_modes and "int8" in weight_modes), "4bit and int8 need different bases: one run each"
model = UniBind(("rgb", "text"), None, device="cuda", llama_layers=a.layers).init_random(seed=0).eval()
ids = torch.randint(3, 32000, (B, 60)); ids[:, 0] = 1; ids[:, 1] = -200
rgb = torch.randn(B, 3, 224, 224)
modes = a.sample.split(",") if a.num_beams == 1 else ["beam"] if a.beam_only else ["beam", "rows"]
assert all(m in ("off", "torch", "device", "beam", "rows") for m in modes), a.sample
ids_rows, rgb_rows = ids.repeat(a.num_beams, 1), rgb.repeat(a.num_beams, 1, 1, 1)   # mode `rows`: the prompt N times
if "4bit" in weight_modes:
    model.text.quantize_base(4, quant_type="nf4", double_quant=True)
if "int8" in weight_modes:
    model.text.quantize_base(8, "int8")
adapter_modes = a.adapters.split(",") if a.lora_r > 0 else [None]
assert all(m in ("merged", "live", None) for m in adapter_modes), a.adapters
kv_modes = a.kv_cache.split(",")
assert all(m in ("bf16", "fp8") for m in kv_modes), a.kv_cache
if a.lora_r > 0:
    targets = ("q", "k", "v", "o", "gate", "up", "down") if a.lora_targets == "all" else tuple(a.lora_targets.split(","))
    lora = model.enable_lora(r=a.lora_r, alpha=2 * a.lora_r, targets=targets, seed=0)
    g = torch.Generator(device="cuda").manual_seed(1)
    for l in range(a.layers):       # peft starts B at zero: give it values so that the adapters move the logits
        for pr in targets:
            A, Bm = lora.get_adapter(l, pr)
            lora.set_adapter(l, pr, A, torch.randn(Bm.shape, device="cuda", generator=g) * 0.02)
    lora.refresh()


def token_bytes_4bit():
    """bytes of weights one `4bit` token streams, from the tensors generate() reads (after the warm-up has built them): codes + fp32 block
    statistics of every decoder linear, and the bf16 lm_head"""
    def nbytes(t):
        return t.numel() * t.element_size()
    total = nbytes(model.text.p["lm_head"])
    for L in model.text.p["layers"]:
        for k in ("qkv_w", "o_w", "gu_w", "down_w"):
            total += nbytes(L[k + "4p"].codes) + nbytes(L[k + "4p"].absmax)
    return total


def token_bytes_mxfp4():
    """bytes of weights one `mxfp4` token streams, from the tensors generate() reads: the tiled codes and block scales (padding rows included)
    of every decoder linear, and the bf16 lm_head"""
    total = model.text.p["lm_head"].numel() * model.text.p["lm_head"].element_size()
    for L in model.text.p["layers"]:
        for k in ("qkv_w", "o_w", "gu_w", "down_w"):
            total += L[k + "mx4"].nbytes()
    return total


def token_bytes_int8():
    """bytes of weights one `int8` token streams, from the tensors generate() reads: the tiled int8 rows (padding rows included) and fp32 row
    factors of every decoder linear, and the bf16 lm_head"""
    total = model.text.p["lm_head"].numel() * model.text.p["lm_head"].element_size()
    for L in model.text.p["layers"]:
        for k in ("qkv_w", "o_w", "gu_w", "down_w"):
            total += L[k + "i8p"].nbytes() + L[k + "i8s"].numel() * L[k + "i8s"].element_size()
    return total


def kwargs(mode, weights, adapters=None, kv_cache="bf16"):
    # eos_token_id=None in EVERY mode (as bench.py --decode and cli_qa.py --synthetic-prompt time it): with an EOS the host synchronises on every
    # token and torch operators run between the graph replay and decode_emit, whoever picks the token
    kw = dict(do_sample=False, weights=weights, eos_token_id=None)
    if adapters is not None:
        kw.update(adapters=adapters)
    if kv_cache != "bf16":
        kw.update(kv_cache=kv_cache)
    if mode == "beam":
        kw.update(num_beams=a.num_beams)
    elif mode not in ("off", "rows"):
        kw.update(do_sample=True, temperature=0.4, top_k=50, top_p=0.9, sampler=mode, seed=0)
    if a.repetition_penalty != 1.0:
        kw.update(repetition_penalty=a.repetition_penalty)
    return kw


def inputs(mode):
    return (ids_rows, rgb_rows) if mode == "rows" else (ids, rgb)


def drop_derived_copies():
    """forget the merged weights and every derived decode copy (re-tiled bf16, e4m3 and their tiles, the packed 4-bit codes): the next call
    builds what its mode needs.  The quantisation states of the 4-bit base (`q4`) and the int8 rows stay: they ARE the base, not copies of it."""
    model.text._merged_cache = None
    keep = ("q4", "i8", "i8s")
    for L in model.text.p["layers"]:
        for k in ("qkv_w", "o_w", "gu_w", "down_w"):
            for suf in type(model.text).DERIVED_SUFFIXES:
                if suf not in keep:
                    L.pop(k + suf, None)
    for k in ("lm_headp", "lm_head8", "lm_head8s", "lm_head8p"):
        model.text.p.pop(k, None)
    torch.cuda.empty_cache()


runs = []
for mode in modes:
    for weights in weight_modes:
        for ad in adapter_modes:
            if ad == "merged" and weights in ("4bit", "int8"):
                print(f"[{weights}, batch {B}, adapters merged] n/a: raises (merged 16-bit copies have no {weights} form)", flush=True)
                continue
            for kvc in kv_modes:
                runs.append((mode, weights, ad, kvc))
for mode, weights, ad, kvc in runs:
    if ad is not None:               # first call of an adapter mode, from a clean model: merge / re-tiling / capture cost and the peak footprint
        drop_derived_copies()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
    model.generate(inputs(mode)[0], images=inputs(mode)[1], max_new_tokens=4, **kwargs(mode, weights, ad, kvc))
    if ad is not None:
        torch.cuda.synchronize()
        print(f"[{weights}, batch {B}, adapters {ad}] first call (4 new tokens) {time.perf_counter() - t0:.3f}s, peak allocated "
              f"{torch.cuda.max_memory_allocated() / 1e9:.2f} GB", flush=True)
    if len(kv_modes) > 1 and mode != "beam":   # (beam search takes no stopping criteria) the caches of a NEW-token call, on top of what is resident after the warm-up: one more short call with the full context
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        model.generate(inputs(mode)[0], images=inputs(mode)[1], max_new_tokens=new, **kwargs(mode, weights, ad, kvc), stopping_criteria=[lambda *_: True])
        torch.cuda.synchronize()
        print(f"[{weights}, batch {B}, kv_cache {kvc}] a call with room for {new} new tokens: peak allocated {torch.cuda.max_memory_allocated() / 1e9:.3f} GB, "
              f"{(torch.cuda.max_memory_allocated() - base) / 1e9:.3f} GB above the resident {base / 1e9:.3f} GB", flush=True)
if len(adapter_modes) > 1:           # the alternating timed runs keep every mode's copies resident: rebuild them all once, untimed
    for mode, weights, ad, kvc in runs:
        model.generate(inputs(mode)[0], images=inputs(mode)[1], max_new_tokens=4, **kwargs(mode, weights, ad, kvc))
roofline = {"fp8": "6.74 GB/token @ 8 TB/s = 1190 tok/s", "bf16": "13.5 GB/token @ 8 TB/s = 590 tok/s"}
if "4bit" in weight_modes:
    gb = token_bytes_4bit() / 1e9
    roofline["4bit"] = f"{gb:.3g} GB/token @ 8 TB/s = {8000 / gb:.0f} tok/s"
if "mxfp4" in weight_modes and "qkv_wmx4" in model.text.p["layers"][0]:   # with adapters="merged" the copies hang on the merged layers instead
    gb = token_bytes_mxfp4() / 1e9
    roofline["mxfp4"] = f"{gb:.3g} GB/token @ 8 TB/s = {8000 / gb:.0f} tok/s"
if "int8" in weight_modes and "qkv_wi8p" in model.text.p["layers"][0]:
    gb = token_bytes_int8() / 1e9
    roofline["int8"] = f"{gb:.3g} GB/token @ 8 TB/s = {8000 / gb:.0f} tok/s"
if "int8" in weight_modes:
    roofline.setdefault("int8", "n/a (the tiled int8 rows belong to no layer: every int8 run raised)")
roofline.setdefault("mxfp4", "n/a (the MXFP4 copies belong to the merged layers)")
for _ in range(a.repeats):
    for mode, weights, ad, kvc in runs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(inputs(mode)[0], images=inputs(mode)[1], max_new_tokens=new, **kwargs(mode, weights, ad, kvc))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        n_new = out.shape[1]
        name = {"off": "greedy", "beam": f"beam search x{a.num_beams}", "rows": f"greedy, {out.shape[0]} rows"}.get(mode, f"sampled/{mode}")
        if ad is not None:
            name += f", adapters {ad}"
        if len(kv_modes) > 1 or kvc != "bf16":
            name += f", kv_cache {kvc}"
        print(f"[{weights}, batch {B}, {name}] {B}x{n_new} new tokens in {dt:.3f}s = {B*n_new/dt:.1f} tok/s (incl. ViT+pooler+prefill of {60-1+144} positions); HBM roofline " + roofline[weights] + " per sequence", flush=True)
