#!/usr/bin/env python
"""Single-image VQA chat on the gfx950 engine - the reference's `cli_qa.py` surface (/root/reference cli_qa.py:44-202) kept
flag-compatible (`-c Config/multi_modal_eval.yaml --model-path <FINAL.pt dir> --image-file <png> --accelerator gpu`):

    build_model -> custom_load_state_dict -> CLIP preprocess (HIP) -> llava_llama_2 prompt -> tokenizer_image_token ->
    KeywordsStoppingCriteria(["</s>"]) -> model.generate(do_sample=True, temperature=0.4, max_new_tokens=512, streamer=...)

The prefill runs on the GEMM path, the per-token step is one captured hipGraph (lhrs_bot_amd/generation.py `DecodeSession`);
`bits: 8` in the YAML (or `--opts bits 8`) streams e4m3 weights through the MFMA GEMV; `--decode-weights 4bit` with `bits: 4` streams
the NF4 / FP4 codes of the 4-bit base (lhrs_gemv4); `--decode-weights mxfp4` (any base) streams OCP MXFP4 copies on the FP4 MFMA
(lhrs_gemv_mx4); `--decode-weights int8` with `bits: 8` streams the int8 rows of the LLM.int8 base (lhrs_gemv_int8).

Imports and call order follow /root/reference cli_qa.py:10-22, 84-193 over the `lhrs.*` surface.  Weights / tokenizer come from the paths
in the YAML (`text.path`, `rgb_vision.vit_name`); when they are not on disk the towers are random-initialised and the word-hash
stand-in tokenizer is used (both announced).  `--synthetic-prompt T` is the non-interactive BASELINE.json configs[4] run: one 224x224
image, a T-token prompt of random ids with the `<image>` placeholder, `--max-new-tokens` greedy tokens, one JSON line with the rate.
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lhrs.CustomTrainer.utils import ConfigArgumentParser, ConfigDict, str2bool  # noqa: E402
from lhrs.Dataset.build_transform import build_vlp_transform  # noqa: E402
from lhrs.Dataset.conversation import SeparatorStyle, default_conversation  # noqa: E402
from lhrs.models import (DEFAULT_IM_END_TOKEN, DEFAULT_IM_START_TOKEN, DEFAULT_IMAGE_PATCH_TOKEN, DEFAULT_IMAGE_TOKEN, IMAGE_TOKEN_INDEX,  # noqa: E402,F401
                         build_model, tokenizer_image_token)
from lhrs.utils import KeywordsStoppingCriteria, type_dict  # noqa: E402


def parse_option(args=None):
    p = ConfigArgumentParser()
    p.add_argument("--opts", default=None, nargs="+", help="'KEY VALUE' pairs applied on top of the YAML, e.g. --opts bits 8")
    p.add_argument("--image-file", type=str, help="path to image")
    p.add_argument("--model-path", type=str, default=None, help="checkpoint directory / FINAL.pt written by custom_save_checkpoint")
    p.add_argument("--seed", type=int, default=322)
    p.add_argument("--num-gpus", type=int, default=1)
    p.add_argument("--temperature", type=float, default=0.2)
    p.add_argument("--max-new-tokens", type=int, default=512)
    p.add_argument("--debug", action="store_true")
    p.add_argument("--accelerator", default="gpu", type=str, choices=["cpu", "gpu", "mps"])
    p.add_argument("--use-checkpoint", default=False, type=str2bool)
    # knobs of this engine
    p.add_argument("--tokenizer-path", type=str, default=None, help="directory holding the LLaMA-2 tokenizer files")
    p.add_argument("--synthetic-prompt", type=int, default=0, metavar="T", help="non-interactive: T random prompt ids, greedy decode, JSON line")
    p.add_argument("--llama-layers", type=int, default=32)
    p.add_argument("--sampler", default="torch", choices=["torch", "device"],
                   help="who draws the token: HF-style torch warpers + multinomial, or the one-launch HIP sampler (lhrs_sample_rows).  "
                        "device: every turn draws from the Philox stream of --seed starting at step 0, so the same conversation replays to the "
                        "same answers (torch: one global generator runs on across the turns)")
    p.add_argument("--repetition-penalty", type=float, default=1.0, help="HF repetition_penalty over the generated tokens (the web UI uses 1.05)")
    p.add_argument("--num-beams", type=int, default=1, help="HF num_beams: > 1 answers by deterministic beam search on the device (no sampling, no token "
                                                            "stream: the answer is printed when the search ends); batch * num_beams <= 16")
    p.add_argument("--decode-weights", default=None, choices=["bf16", "fp8", "4bit", "mxfp4", "int8"],
                   help="what the single-token step streams (default: fp8 iff `bits: 8`, else bf16); 4bit reads the NF4 / FP4 codes of the `bits: 4` "
                        "base directly and requires it; if the decoder is not on that base yet (an evaluation run has not been through "
                        "prepare_for_training) it is put there first with the YAML's quant_type / double_quant, so the prefill too reads "
                        "the dequantised weights, as every product of the reference's Linear4bit does; mxfp4 (any base, no YAML key) streams OCP MXFP4 "
                        "copies of the decoder linears - e2m1 codes with one e8m0 scale per 32 weights, multiplied by the FP4 MFMA against e4m3 "
                        "activations: lossy like fp8, lm_head and prefill stay bf16; int8 requires `bits: 8` on the LLM.int8 scheme (the reference's "
                        "load_in_8bit) and streams the base's own int8 rows in bitsandbytes' MatMul8bitLt arithmetic, prefill included - if the decoder "
                        "is not on that base yet it is put there first; the default for `bits: 8` stays fp8")
    p.add_argument("--adapters", default="merged", choices=["merged", "live"],
                   help="un-merged LoRA adapters (stage >= 1 with a TextLoRA/ loaded): merged = decode on merged 16-bit copies of the adapted weights; "
                        "live = no copies, the adapters run next to the base weights of whatever --decode-weights streams (4bit included)")
    p.add_argument("--kv-cache", default="bf16", choices=["bf16", "fp8"],
                   help="KV cache of the decode step: bf16, or fp8 = e4m3 codes with one e8m0 scale byte per head row (half the cache memory and "
                        "half the cache stream; the prompt itself is attended in bf16, so the first token is the bf16 one); batch x beams <= 16")
    p.add_argument("--prefix-cache", action="store_true",
                   help="keep the KV cache of the conversation across turns (one PrefixCache of the chosen --kv-cache): a turn encodes no image "
                        "again and prefills only what is new behind the common prefix of its prompt and the cache; not with --num-beams > 1")
    p.add_argument("--length-penalty", type=float, default=1.0, help="HF length_penalty of the beam search: hypotheses score sum(log p) / length ** penalty")
    cfg = ConfigDict(p.parse_args(wandb=True, args=args))
    opts = cfg.get("opts") or []
    if len(opts) % 2:
        p.error("--opts takes KEY VALUE pairs")
    import yaml
    for k, v in zip(opts[0::2], opts[1::2]):
        cfg[k] = yaml.safe_load(v)
    return cfg


class _Streamer:
    """transformers.TextStreamer(skip_prompt=True, skip_special_tokens=True) behaviour for ids that arrive one step at a time."""

    def __init__(self, tokenizer):
        self.tok, self.ids, self.shown = tokenizer, [], 0

    def put(self, ids):
        self.ids.extend(int(i) for i in ids.reshape(-1).tolist())
        text = self.tok.decode(self.ids, skip_special_tokens=True)
        sys.stdout.write(text[self.shown:])
        sys.stdout.flush()
        self.shown = len(text)

    def end(self):
        sys.stdout.write("\n")
        self.ids, self.shown = [], 0


def load_image(path):
    from PIL import Image  # decode only; resize / crop / normalise run in lhrs_clip_preprocess
    return Image.open(path).convert("RGB")


def main(config):
    if config.accelerator != "gpu" or not torch.cuda.is_available():
        raise RuntimeError("cli_qa.py drives the HIP engine: it needs --accelerator gpu and a visible MI355X (there is no CPU path)")
    if config.get("prefix_cache") and int(config.num_beams) > 1:
        raise ValueError("--prefix-cache with --num-beams > 1: beam search starts every turn from an empty cache")
    device = torch.device("cuda", 0)
    torch.manual_seed(int(config.seed))
    # build_model loads the frozen towers + tokenizer from config.text.path / config.rgb_vision.vit_name (random-init with a warning when
    # the paths are not on disk); --model-path adds the trained projector (FINAL.pt, or the directory holding it) and TextLoRA/
    model = build_model(config, activate_modal=("rgb", "text"))
    vision_processor = build_vlp_transform(config, is_train=False)
    dtype = type_dict[config.get("dtype", "bfloat16")]
    model.to(dtype)
    conv = default_conversation.copy()
    roles = conv.roles
    if config.get("model_path") is not None:
        print(model.custom_load_state_dict(config.model_path))
    if config.get("tokenizer_path"):
        import transformers
        model.text.tokenizer = transformers.AutoTokenizer.from_pretrained(config.tokenizer_path, use_fast=False)
    tokenizer = model.text.tokenizer
    model.eval()
    bits = int(config.get("bits", 16) or 16)
    weights = config.get("decode_weights") or ("fp8" if bits == 8 else "bf16")
    adapters = str(config.get("adapters") or "merged")
    kv_cache = str(config.get("kv_cache") or "bf16")
    turn_kw = {"prefix_cache": model.new_prefix_cache(kv_cache)} if config.get("prefix_cache") else {}
    if weights == "4bit":
        if bits != 4:
            raise ValueError("--decode-weights 4bit requires `bits: 4` in the YAML (or --opts bits 4)")
        if not model.text.base4:   # bits: 4 selects the storage in prepare_for_training; an evaluation run has not been through it
            model.text.quantize_base(4, quant_type=str(config.get("quant_type", "nf4")), double_quant=bool(config.get("double_quant", True)))
    if weights == "int8":
        if bits != 8:
            raise ValueError("--decode-weights int8 requires `bits: 8` in the YAML (or --opts bits 8)")
        if model.text.base8:
            raise ValueError("--decode-weights int8 requires the LLM.int8 scheme of `bits: 8`, this decoder is on the e4m3 scheme "
                             "(quantize_base(8, 'e4m3') / LHRS_BASE8=e4m3): use --decode-weights fp8, or load the base with the int8 scheme")
        if not model.text.base_int8:   # an evaluation run has not been through prepare_for_training
            model.text.quantize_base(8, "int8")

    if config.get("image_file"):
        image = load_image(config.image_file)
        image_tensor = vision_processor(image, return_tensors="pt")["pixel_values"]
    elif config.synthetic_prompt:
        g = torch.Generator().manual_seed(int(config.seed))
        image = True
        image_tensor = vision_processor(torch.randint(0, 256, (256, 256, 3), generator=g, dtype=torch.uint8))["pixel_values"]
    else:
        image, image_tensor = None, None

    if config.synthetic_prompt:
        T = int(config.synthetic_prompt)
        g = torch.Generator().manual_seed(int(config.seed))
        ids = torch.randint(3, 32000, (1, T), generator=g)
        ids[0, 0], ids[0, 1] = 1, IMAGE_TOKEN_INDEX
        kw = dict(images=image_tensor, do_sample=False, use_cache=True, weights=weights, eos_token_id=None, num_beams=int(config.num_beams),
                  length_penalty=float(config.length_penalty), adapters=adapters, kv_cache=kv_cache)
        model.generate(ids, max_new_tokens=4, **kw)  # graph capture + allocator warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(ids, max_new_tokens=int(config.max_new_tokens), **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({"metric": "cli_qa greedy generate tokens/s (ViT + projector + prefill included)", "value": round(out.shape[1] / dt, 1),
                          "unit": "tokens/s", "new_tokens": int(out.shape[1]), "prompt_positions": T - 1 + 144, "weights": weights,
                          "adapters": adapters, "seconds": round(dt, 3)}))
        return out

    if getattr(tokenizer, "is_synthetic", False):
        print("WARNING: no tokenizer files (config.text.path / --tokenizer-path): the word-hash stand-in is in use, the answers are not text")
    while True:
        try:
            inp = input(f"{roles[0]}: ")
        except EOFError:
            inp = ""
        if not inp:
            print("exit...")
            break
        print(f"{roles[1]}: ", end="")
        if image is not None:  # first message carries the image
            tok = DEFAULT_IM_START_TOKEN + DEFAULT_IMAGE_TOKEN + DEFAULT_IM_END_TOKEN if config.get("tune_im_start", False) else DEFAULT_IMAGE_TOKEN
            inp, image = tok + "\n" + inp, None
        conv.append_message(conv.roles[0], inp)
        conv.append_message(conv.roles[1], None)
        prompt = conv.get_prompt()
        input_ids = tokenizer_image_token(prompt, tokenizer, IMAGE_TOKEN_INDEX, return_tensors="pt").unsqueeze(0).to(device)
        stop_str = conv.sep if conv.sep_style != SeparatorStyle.TWO else conv.sep2
        stopping_criteria = KeywordsStoppingCriteria([stop_str], tokenizer, input_ids)
        with torch.inference_mode():
            if int(config.num_beams) > 1:   # beam search stops on the tokenizer's EOS, on the device: no streamer, no host stopping criteria
                output_ids = model.generate(input_ids, images=image_tensor, do_sample=False, max_new_tokens=int(config.max_new_tokens), use_cache=True,
                                            weights=weights, num_beams=int(config.num_beams), length_penalty=float(config.length_penalty),
                                            repetition_penalty=float(config.repetition_penalty), adapters=adapters, kv_cache=kv_cache)
                print(tokenizer.decode(output_ids[0], skip_special_tokens=True).strip())
            else:
                output_ids = model.generate(input_ids, images=image_tensor, do_sample=True, max_new_tokens=int(config.max_new_tokens), temperature=0.4,
                                            streamer=_Streamer(tokenizer), use_cache=True, stopping_criteria=[stopping_criteria], weights=weights,
                                            sampler=config.sampler, repetition_penalty=float(config.repetition_penalty), seed=int(config.seed),
                                            adapters=adapters, kv_cache=kv_cache, **turn_kw)
        outputs = tokenizer.decode(output_ids[0]).strip().split("<s>")[-1].strip()
        conv.messages[-1][-1] = outputs
        if config.debug:
            print("\n", {"prompt": prompt, "outputs": outputs}, "\n")
    return conv


if __name__ == "__main__":
    cfg = parse_option()
    cfg.adjust_norm = False
    main(cfg)
