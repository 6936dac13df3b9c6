"""Whole `generate()` calls on a tiny decoder (2 layers, dim 512, 4 heads, ff 512, vocab 128, `init_random(seed=0)`: the model of
tests/decode_plan_cases.py at the narrowest width the row kernels take, columns in multiples of 512), one case per arm of the token loops, shared by tools/record_generate_traces.py (which writes
tests/golden/generate_traces.json) and tests/test_generate_trace_gpu.py (which compares with it for equality).  Only the public model API is
used, so the recording tool runs on any commit.

A case is a function of a model cache -> list of the values its `generate` calls returned, in order; `encode` turns them into what the
golden file holds: integer tensors as lists, every other tensor as the SHA-256 of its bytes."""
import hashlib

import torch

from lhrs_bot_amd import generation as G
from lhrs_bot_amd.text import IMAGE_TOKEN_INDEX, TextModal

BF = torch.bfloat16
NEW, NI, T, V = 6, 5, 6, 128
SHAPES = {"tiny": dict(layers=2, dim=512, ff=512, heads=4), "h16": dict(layers=2, dim=2048, ff=512, heads=16)}   # h16: kv8 under beams moves 16 scale bytes
SAMPLING = dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9)


def make_model(shape="tiny", base=None, lora=False, device="cuda"):
    m = TextModal(device=device, vocab=V, max_pos=512, **SHAPES[shape])
    m.init_random(seed=0)
    if base is not None:
        m.quantize_base(8, base)
    if lora:
        kw = dict(r=8, alpha=16, targets=("q", "k", "v", "o"))
        lo = m.enable_lora(seed=5, **kw)
        g = torch.Generator().manual_seed(11)
        for li in range(SHAPES[shape]["layers"]):
            for proj in kw["targets"]:                                   # B starts at zero in peft: the adapter term must move the logits
                A, B = lo.get_adapter(li, proj)
                lo.set_adapter(li, proj, A.clone(), torch.randn(B.shape, generator=g) * 0.05)
        lo.refresh()
        lo.train_mode = False
    return m


def model_cache():
    cache = {}

    def get(shape="tiny", base=None, lora=False):
        key = (shape, base, lora)
        if key not in cache:
            cache[key] = make_model(*key)
        return cache[key]
    return get


def prompt(m, B, pad=False):
    """-> (ids [B, 6] with one <image> placeholder per row, image embedding [B, 5, d], attention mask or None: row 0 LEFT-padded by two)"""
    g = torch.Generator().manual_seed(17)
    ids = torch.randint(3, V, (B, T), generator=g)
    ids[:, 0], ids[:, 1] = 1, IMAGE_TOKEN_INDEX
    mask = None
    if pad:
        mask = torch.ones(B, T, dtype=torch.int64)
        ids[0, 2:] = ids[0, :4].clone()
        ids[0, :2], mask[0, :2] = 0, 0
    image = (torch.randn(B, NI, m.d, generator=g) * 0.05).to(BF).to(m.device)
    return ids, image, mask


def gen(B, shape="tiny", base=None, lora=False, pad=False, seed=None, **kw):
    def case(models):
        m = models(shape, base, lora)
        ids, image, mask = prompt(m, B, pad)
        if seed is not None:
            torch.manual_seed(seed)
        return [m.generate(ids, image, mask, max_new_tokens=NEW, **{"eos_token_id": None, **kw})]
    return case


def with_eos(B, **kw):
    """greedy first; its third token of row 0 is the EOS of the second call, so that a row finishes and emits pads while another runs on"""
    def case(models):
        first = gen(B, **kw)(models)[0]
        eos = int((first[0] if isinstance(first, tuple) else first)[0, 2])
        return [first] + gen(B, **{**kw, "eos_token_id": eos})(models)
    return case


def constrained(B):
    def case(models):
        m = models()
        a = G.choice_automaton([[5, 6], [5, 7, 8], [9]], 2, 0, V, m.device)
        return gen(B, constraint=a, return_choices=True)(models)
    return case


def prefix_cached(kv_cache):
    def case(models):
        m = models()
        ids, image, _ = prompt(m, 1)
        pc = m.new_prefix_cache(kv_cache, 64)
        first = m.generate(ids, image, max_new_tokens=NEW, eos_token_id=None, prefix_cache=pc)
        longer = torch.cat([ids, first[:, :-1].cpu(), torch.tensor([[7, 9]])], 1)
        second = m.generate(longer, None, max_new_tokens=NEW, eos_token_id=None, prefix_cache=pc)
        return [first, second, torch.tensor([pc.last_reused, pc.last_prefilled, pc.length])]
    return case


class _Streamer:
    def __init__(self):
        self.seen = []

    def put(self, t):
        self.seen.append(t.reshape(-1).tolist())

    def end(self):
        self.seen.append("end")


def streamed(models):
    st = _Streamer()
    out = gen(2, streamer=st, stopping_criteria=[lambda ids, lg: ids.shape[1] >= 4])(models)
    assert st.seen[-1] == "end"
    return out + [torch.tensor(st.seen[:-1])]


def _cases():
    c = {}
    for B in (1, 2, 17):
        c[f"greedy/B{B}"] = gen(B)
        c[f"sampler-device/B{B}"] = gen(B, sampler="device", seed=7, **SAMPLING)
        c[f"constraint/B{B}"] = constrained(B)
    c["eos/B2"], c["eos/B17"] = with_eos(2), with_eos(17)
    c["sampler-torch/B2"], c["sampler-torch/B17"] = gen(2, seed=3, **SAMPLING), gen(17, seed=3, **SAMPLING)
    c["sampler-device-penalty/B2"] = gen(2, sampler="device", seed=7, repetition_penalty=1.3, **SAMPLING)
    c["penalty/B2"], c["penalty/B17"] = gen(2, repetition_penalty=1.3), gen(17, repetition_penalty=1.3)
    c["return-logits/B2"], c["return-logits/B17"] = gen(2, return_logits=True), gen(17, return_logits=True)
    c["left-pad/B2"] = gen(2, pad=True)
    c["kv-fp8/B2"] = gen(2, kv_cache="fp8")
    c["weights-fp8/B2"] = gen(2, weights="fp8")
    c["weights-int8/B2"], c["weights-int8/B17"] = gen(2, base="int8", weights="int8"), gen(17, base="int8", weights="int8")
    for ad in ("merged", "live"):
        c[f"adapters-{ad}/B2"] = gen(2, lora=True, adapters=ad)
    c["adapters-live/B17"] = gen(17, lora=True, adapters="live")
    c["prefix-cache/bf16"], c["prefix-cache/fp8"] = prefix_cached("bf16"), prefix_cached("fp8")
    c["streamer-criteria/B2"] = streamed
    c["beam/B2"] = gen(2, num_beams=2, return_beam_scores=True)
    c["beam-eos/B2"] = with_eos(2, num_beams=2, return_beam_scores=True)
    c["beam-logits-penalty/B2"] = gen(2, num_beams=2, return_logits=True, repetition_penalty=1.3, length_penalty=0.5)
    c["beam-kv-fp8/B2"] = gen(2, shape="h16", num_beams=2, kv_cache="fp8", return_beam_scores=True)
    return c


CASES = _cases()


def encode(values):
    """the golden form of what a case returned"""
    def one(t):
        t = t.detach().cpu().contiguous()
        if t.dtype in (torch.int64, torch.int32):
            return t.tolist()
        return {"sha256": hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest(), "shape": list(t.shape), "dtype": str(t.dtype)}
    return [[one(t) for t in (v if isinstance(v, tuple) else (v,))] for v in values]


def run_case(name, models):
    out = encode(CASES[name](models))
    torch.cuda.synchronize()
    return out
