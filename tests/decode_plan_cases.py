"""The launch plan of single-token decoding, recorded on the CPU: every public function of `lhrs_bot_amd.kernels` is replaced by a recorder
that returns the right KIND of object (a `Packed*` class from the re-tilers, `q_out` from the quantising producers, `out` from whatever takes
one, a slice count from `lora_down`) and launches nothing, so `TextModal._decode_session(...).enqueue()` and `TextModal._layer_step` run on
`device="cpu"`.  One entry per call: the wrapper's name and its bound arguments (defaults applied) - scalars as they are, tensors as a label:

    <owner>+<storage offset>:<shape>:<strides>:<dtype>

`owner` is the key path of the tensor that owns the storage when the model does (`layers[1].qkv_w8p.data`, `lora.shadow`, `cos`), else `#n`, the
ordinal of the storage's first appearance in the trace: the ping-pong of the hidden-state buffers and the `acc[:, :n]` views are pinned
without naming an attribute of the session.  Raw addresses (`copy_2d`) become `<owner>@<byte offset>`.

tests/golden/decode_plan.json holds, per case, the call names and the SHA-256 of the canonical trace (tests/golden/make_golden_decode_plan.py);
tests/test_decode_plan_cpu.py compares.  A host-side refactor of the decode path must leave every digest as it is.

The cases `generate/...` record whole `TextModal.generate` calls: the picks hand back zero-filled int64 (no row ever finishes by accident),
`hk.HipGraph` is a class that launches nothing and records `HipGraph.begin` / `.end` / `.launch` as calls of their own, and the
side-stream bracket of generation.py is a null context.  With max_new_tokens=5 a session loop is one eager step, one capture, replays.
Their golden entries were recorded on the commit before the token loops became one, where the bracket was still inline: there
`_no_side_stream` replaced `torch.cuda.Stream`, `torch.cuda.stream` and `torch.cuda.current_stream` by no-ops instead of `G.side_stream`;
nothing else of this file differed.  The trace holds `hk` calls only: that the prefill's argmax / multinomial token reaches `s.next_ids`
through `copy_` (a torch call) is not seen here - tests/test_generate_trace_gpu.py holds the tokens that depend on it."""
import contextlib
import hashlib
import inspect
import json
import os

import torch

import lhrs_bot_amd.generation as G
import lhrs_bot_amd.kernels as hk
from lhrs_bot_amd.text import IMAGE_TOKEN_INDEX, LORA_ALL, TextModal

# pure functions of shapes: they stay what they are.  `lora_down_splits` asks liblhrs_hip.so, so the BUILT library is required (no GPU is):
# without it every case with an adapter store, and the golden maker, end in the loader's RuntimeError
REAL = ("lora_down_lds_bytes", "lora_down_splits", "pad64")
BF, U8, F32, I8 = torch.bfloat16, torch.uint8, torch.float32, torch.int8


def _E(shape, dtype=BF):
    return torch.empty(shape, dtype=dtype)


def _returns(name, a):
    """what the stub of wrapper `name` hands back for the bound arguments `a`"""
    out = a.get("out")
    if name in ("repack_bf16_mfma", "repack_fp8_mfma"):
        W = a["W"] if name == "repack_bf16_mfma" else a["W8"]
        N, K = W.shape
        cls, dt = (hk.PackedBf16, BF) if name == "repack_bf16_mfma" else (hk.PackedFp8, U8)
        return cls(_E((N + 15) // 16 * 16 * K, dt), N, K)
    if name == "repack_int8_mfma":
        N, K = a["WQ"].shape
        return hk.PackedI8(_E(((N + 15) // 16, max(K // 64, 1), 64, 16), I8), N, K)
    if name == "repack_mx4_mfma":
        N, K = a["codes"].shape[0], a["codes"].shape[1] * 2
        G, S = (N + 15) // 16, K // 128
        return hk.PackedMX4(_E((G, S, 64, 16), U8), _E((G, (S + 3) // 4, 64, 4), U8), N, K)
    if name == "pack4_decode":
        N, K = a["N"], a["K"]
        return hk.Packed4(_E((N, K // 2), U8), _E((N, K // 64), F32), a["states"][0]["quant_type"] == "fp4", N, K)
    if name == "quant4_blocks":
        n = a["W"].numel()
        return {"quant_type": a["quant_type"], "double_quant": bool(a["double_quant"]), "packed": _E(n // 2, U8), "absmax": _E(n // 64, F32)}
    if name in ("quant_fp8_rows", "quant_int8_rows"):
        N, K = a["W"].shape
        return out if out is not None else (_E((N, K), U8 if name == "quant_fp8_rows" else I8), _E(N, F32))
    if name == "quant_mx4_rows":
        N, K = a["W"].shape
        return _E((N, K // 2), U8), _E((N, K // 32), U8)
    if name == "dequant_int8_rows":
        return out if out is not None else _E(tuple(a["Q"].shape))
    if name == "transpose":
        return out if out is not None else _E((a["x"].shape[1], a["x"].shape[0]), a["x"].dtype)
    if name in ("rmsnorm_fwd", "dropout", "cast_f32_to_bf16"):
        return out if out is not None else _E(tuple(a["x"].shape))
    if name in ("rmsnorm_fwd_q", "swiglu_fwd_q"):
        x = a["x"] if name == "rmsnorm_fwd_q" else a["gate_up"]
        M, K = x.shape[0], (x.shape[1] if name == "rmsnorm_fwd_q" else a["F"])
        h = out if out is not None else (_E((M, K)) if a["want_bf16"] else None)
        q = a["q_out"] if a["q_out"] is not None else (_E((M, K), U8), _E(M, F32))
        return (h, q) if name == "rmsnorm_fwd_q" else (h, q[0], q[1])
    if name == "swiglu_fwd":
        return out if out is not None else _E((a["gate_up"].shape[0], a["F"]))
    if name in ("gemm_nt", "gemm_nt_lora"):   # fp32 without `out`: logits the host may read (warp_logits + multinomial) - zeros
        return out if out is not None else (torch.zeros if a["out_f32"] else _E)((a["a"].shape[0], a["b"].shape[0]), dtype=F32 if a["out_f32"] else BF)
    if name == "gemm_nt_skinny":
        return _E((a["a"].shape[0], a["b"].shape[0]))
    if name == "gemm_rope_fwd":
        return out if out is not None else _E((a["x"].shape[0], a["w"].shape[0]))
    if name == "gemm_swiglu_fwd":
        return _E((a["x"].shape[0], 2 * a["ff"])), _E((a["x"].shape[0], a["ff"]))
    if name == "int8_linear":
        return out if out is not None else _E((a["x"].shape[0], a["WQ"].shape[0]))
    if name == "gather_rows":
        return out if out is not None else _E((a["idx"].numel(), a["src"].shape[1]), a["src"].dtype)
    if name == "lora_down":
        return REAL_FNS["lora_down_splits"](a["K"], a["A"].shape[0] if a["R"] is None else int(a["R"]))
    if name in ("argmax_rows", "sample_rows", "constrain_rows"):   # the picks: token 0 for every row
        return out if out is not None else torch.zeros(a["logits_f32"].shape[0], dtype=torch.int64)
    if name == "h2d":
        return a["t"]
    if name == "make_desc":
        return torch.zeros((len(a["entries"]), 8), dtype=torch.int32)
    if name == "kv_cache_table":
        return torch.zeros(sum(len(kv) for kv in a["caches"]), dtype=torch.int64)
    if name == "splice_map_fwd":
        return _E((a["ids"].shape[0], a["S"], a["image"].shape[-1]))
    if name == "splice_fwd":   # -> (embeds, labels, mask, img_pos); the mask is the real one (the image block is visible): it decides the key mask
        ids, mask, S = a["ids"], a["mask"], a["S"]
        B, T = ids.shape
        rows = []
        for b in range(B):
            mrow = torch.ones(T, dtype=U8) if mask is None else mask[b].to(U8)
            pos = (ids[b] == IMAGE_TOKEN_INDEX).nonzero()
            p = int(pos[0]) if len(pos) else T
            rows.append(torch.cat([mrow[:p], torch.ones(S - T + 1 if p < T else 0, dtype=U8), mrow[p + 1:], torch.zeros(0 if p < T else S - T, dtype=U8)]))
        return _E((B, S, a["image"].shape[2])), torch.zeros((B, S), dtype=torch.int64), torch.stack(rows), torch.zeros(B, dtype=torch.int32)
    if "out" in a and out is None:
        raise NotImplementedError(f"decode_plan_cases: no return rule for hk.{name} without `out`")
    return out


REAL_FNS = {n: getattr(hk, n) for n in REAL}
PUBLIC = sorted(n for n, f in vars(hk).items() if inspect.isfunction(f) and f.__module__ == hk.__name__ and not n.startswith("_") and n not in REAL)
SIGNATURES = {n: inspect.signature(getattr(hk, n)) for n in PUBLIC}


class _NoLaunchTranspose:
    """`hk.BatchedTranspose` without its launch (`LoraStore.refresh`)"""

    def __init__(self, pairs):
        self.keep = pairs

    def run(self):
        pass


class Recorder:
    def __init__(self):
        self.calls, self.keep = [], []

    def _graph_class(rec):
        class NoLaunchGraph:
            """`hk.HipGraph` without capture or replay: begin / end / launch are entries of the trace"""
            begin, end, launch = (lambda self, n=n: rec.calls.append((n, {})) for n in ("HipGraph.begin", "HipGraph.end", "HipGraph.launch"))
        return NoLaunchGraph

    def _stub(self, name):
        sig = SIGNATURES[name]

        def stub(*args, **kw):
            b = sig.bind(*args, **kw)
            b.apply_defaults()
            a = dict(b.arguments)
            self.calls.append((name, a))
            r = _returns(name, a)
            self.keep.append(r)
            return r
        stub.__name__ = name
        return stub

    @contextlib.contextmanager
    def installed(self):
        saved = {n: getattr(hk, n) for n in PUBLIC + ["BatchedTranspose", "HipGraph"]}
        for n in PUBLIC:
            setattr(hk, n, self._stub(n))
        hk.BatchedTranspose, hk.HipGraph = _NoLaunchTranspose, self._graph_class()
        try:
            yield self
        finally:
            for n, f in saved.items():
                setattr(hk, n, f)

    def reset(self):
        """forget the calls so far (the storages they touched stay alive: no address is handed out twice within a case)"""
        self.keep.append(self.calls)
        self.calls = []

    # ---------------------------------------------------------------- canonical form
    def canonical(self, model):
        owners = {}

        def own(o, path):
            if torch.is_tensor(o):
                if o.numel():
                    owners.setdefault(o.untyped_storage().data_ptr(), path)
            elif isinstance(o, dict):
                for k, v in o.items():
                    if isinstance(k, tuple):
                        own(v, f"{path}[{','.join(map(str, k))}]")
                    else:
                        own(v, f"{path}.{k}" if path else str(k))
            elif isinstance(o, (list, tuple)):
                for i, v in enumerate(o):
                    own(v, f"{path}[{i}]")
            elif hasattr(o, "__dict__") and type(o).__module__ == hk.__name__:
                for k, v in vars(o).items():
                    own(v, f"{path}.{k}")

        own(model.p, "")
        own(model.cos, "cos")
        own(model.sin, "sin")
        if model._i8ws is not None:
            own(model._i8ws, "i8ws")
        if model.lora is not None:
            for k in ("master", "shadow", "grad"):
                own(getattr(model.lora, k), "lora." + k)
            own(model.lora.derived, "lora.derived")
        ordinals, spans = {}, []

        def owner_of(sp):
            if sp in owners:
                return owners[sp]
            return "#%d" % ordinals.setdefault(sp, len(ordinals))

        def see(o):   # every storage a raw address may point into
            if torch.is_tensor(o) and o.numel():
                st = o.untyped_storage()
                spans.append((st.data_ptr(), st.nbytes()))
            elif isinstance(o, dict):
                for v in o.values():
                    see(v)
            elif isinstance(o, (list, tuple)):
                for v in o:
                    see(v)
            elif hasattr(o, "__dict__") and type(o).__module__ == hk.__name__:
                see(vars(o))

        for name, a in self.calls:
            see(a)
        see(self.keep)
        see(model.p)

        def address(p):
            for sp, n in spans:
                if sp <= p < sp + n:
                    return f"{owner_of(sp)}@{p - sp}"
            raise AssertionError(f"raw address {p:#x} points into no tensor of the trace")

        def canon(o):
            if torch.is_tensor(o):
                if not o.numel():
                    return f"empty:{list(o.shape)}:{o.dtype}"
                return f"{owner_of(o.untyped_storage().data_ptr())}+{o.storage_offset()}:{list(o.shape)}:{list(o.stride())}:{o.dtype}"
            if o is None or isinstance(o, (bool, int, str)):
                return o
            if isinstance(o, float):
                return repr(o)
            if isinstance(o, (torch.dtype, torch.device)):
                return str(o)
            if isinstance(o, dict):
                return {str(k): canon(v) for k, v in sorted(o.items(), key=lambda kv: str(kv[0]))}
            if isinstance(o, (list, tuple)):
                return [canon(v) for v in o]
            if hasattr(o, "__dict__") and (type(o).__module__ == hk.__name__ or isinstance(o, G.TokenAutomaton)):
                return {type(o).__name__: canon({k: v for k, v in vars(o).items() if not k.startswith("_")})}
            raise TypeError(f"decode_plan_cases: cannot canonicalise {type(o)}")

        trace = []
        for name, a in self.calls:
            if name == "copy_2d":
                a = dict(a, dst_ptr=address(a["dst_ptr"]), src_ptr=address(a["src_ptr"]))
            trace.append([name, canon(a)])
        return trace


def digest(trace):
    return hashlib.sha256(json.dumps(trace, sort_keys=True).encode()).hexdigest()


# -------------------------------------------------------------------- models
def model(heads=2, dim=256, ff=512, base=None, lora=None, layers=2, empty=False):
    """dim 256 / heads 2: head_dim 128 and every %128 / %64 rule of the weight formats holds; heads 4: head_dim 64, the `rope_kv_append` arm.
    base: None | "e4m3" | "int8" | "4bit"; lora: None | "r8" (r = 8 on q, k, v, o) | "r4" (r = 4 on all seven: the dense form) | an
    `enable_lora` keyword dict.  empty: parameters are uninitialised storage (a shape too large to fill for a test that only counts calls)."""
    m = TextModal(device="cpu", layers=layers, dim=dim, ff=ff, heads=heads, vocab=128, max_pos=512)
    if empty:
        m.p = {"embed": _E((128, dim)), "norm_w": _E(dim), "lm_head": _E((128, dim)),
               "layers": [{"ln1_w": _E(dim), "qkv_w": _E((3 * dim, dim)), "o_w": _E((dim, dim)), "ln2_w": _E(dim), "gu_w": _E((2 * ff, dim)),
                           "down_w": _E((dim, ff))} for _ in range(layers)]}
        m._finish()
    else:
        m.init_random(seed=0)
    if base == "4bit":
        m.quantize_base(4, quant_type="nf4", double_quant=True)
    elif base is not None:
        m.quantize_base(8, base)
    if lora is not None:
        kw = lora if isinstance(lora, dict) else {"r8": dict(r=8, alpha=16, targets=("q", "k", "v", "o")), "r4": dict(r=4, alpha=8, targets=LORA_ALL)}[lora]
        m.enable_lora(**kw).train_mode = False
    return m


BASE_OF = {"bf16": None, "fp8": None, "4bit": "4bit", "mxfp4": None, "int8": "int8"}
WEIGHTS = tuple(BASE_OF)


def _kmask(B, max_ctx):
    k = torch.ones((B, max_ctx), dtype=U8)
    k[0, :2] = 0
    return k


def run(fn):
    """fn(rec) -> model builds everything under the installed recorder -> the golden entry of the case"""
    rec = Recorder()
    with rec.installed():
        try:
            m = fn(rec)
        except (ValueError, AssertionError, NotImplementedError) as e:
            return {"error": [type(e).__name__, str(e), len(rec.calls)]}
        trace = rec.canonical(m)
    return {"calls": [n for n, _ in trace], "sha256": digest(trace)}


def session_case(weights, B, kv_cache, max_ctx, heads=2, lora=None, kmask=False, base="auto", sessions=1, split=True, **mk):
    def fn(rec):
        m = model(heads=heads, base=BASE_OF.get(weights) if base == "auto" else base, lora=lora, **mk)
        caches = m._alloc_kv(B * max_ctx, kv_cache) if kv_cache in ("bf16", "fp8") else []
        rec.reset()   # from here on: lazy packing, session construction, one step
        saved = os.environ.get("LHRS_DECODE_SPLIT")
        if not split:
            os.environ["LHRS_DECODE_SPLIT"] = "0"
        try:
            for _ in range(sessions):
                s = m._decode_session(B, max_ctx, caches, 4, weights, _kmask(B, max_ctx) if kmask else None, m.lora, kv_cache)
                rec.keep.append(s)
                s.enqueue()
        finally:
            if not split:
                os.environ.pop("LHRS_DECODE_SPLIT")
                if saved is not None:
                    os.environ["LHRS_DECODE_SPLIT"] = saved
        return m
    return fn


def layer_step_case(ctx, S_new, arm, kv_cache, B=2, kmask=False):
    """arm: "plain" (li=None) | "lora" (li, a live store) | "int8" (li, int8=True) | "int8+lora" """
    def fn(rec):
        m = model(base="int8" if "int8" in arm else None, lora="r8" if "lora" in arm else None)
        max_ctx = 16
        caches = m._alloc_kv(B * max_ctx, kv_cache)
        x = _E((B * S_new, m.d))
        desc = torch.zeros((B, 8), dtype=torch.int32)
        rec.keep += [caches, x, desc]
        rec.reset()
        for li, (L, cache) in enumerate(zip(m.p["layers"], caches)):
            x = m._layer_step(L, x, B, S_new, ctx, cache, desc, max_ctx, _kmask(B, max_ctx) if kmask else None,
                              li=None if arm == "plain" else li, int8="int8" in arm)
        return m
    return fn


def generate_reject_case(weights):
    def fn(rec):
        m = model()
        rec.reset()
        m.generate(torch.zeros((1, 4), dtype=torch.int64), weights=weights, max_new_tokens=2)
        return m
    return fn


@contextlib.contextmanager
def _no_side_stream():
    """the side-stream bracket of the token loops as a null context (there is no stream on the CPU)"""
    saved, G.side_stream = G.side_stream, lambda device: contextlib.nullcontext()
    try:
        yield
    finally:
        G.side_stream = saved


class _Streamer:
    put = end = lambda self, *a: None


NEW, NI = 5, 4   # one eager step, one capture, replays; the image block behind the placeholder


def generate_case(B=2, calls=1, pad=False, seed=None, constraint=False, prefix_cache=None, heads=2, dim=256, base=None, lora=None, **kw):
    """`calls` whole generate() calls on a prompt of 6 ids with one <image> placeholder; constraint: a three-choice automaton;
    prefix_cache: the kv_cache of a PrefixCache that the calls share (the second prompt continues the first)"""
    def fn(rec):
        m = model(heads=heads, dim=dim, base=base, lora=lora)
        ids = torch.arange(3, 3 + B * 6).reshape(B, 6) % 100 + 3
        ids[:, 0], ids[:, 1] = 1, IMAGE_TOKEN_INDEX
        mask = None
        if pad:
            mask = torch.ones((B, 6), dtype=torch.int64)
            ids[0, 2:] = ids[0, :4].clone()
            ids[0, :2], mask[0, :2] = 0, 0
        image = torch.zeros((B, NI, dim), dtype=BF)
        opts = {"eos_token_id": None, **kw}
        if constraint:
            opts["constraint"] = G.choice_automaton([[5, 6], [5, 7, 8], [9]], 2, 0, m.vocab)
        if prefix_cache:
            opts["prefix_cache"] = m.new_prefix_cache(prefix_cache, 64)
        rec.keep += [ids, image, mask, opts]
        rec.reset()
        if seed is not None:
            torch.manual_seed(seed)
        with _no_side_stream():
            for i in range(calls):
                out = m.generate(ids, None if prefix_cache and i else image, mask, max_new_tokens=NEW, **opts)   # None: the cached image block
                rec.keep.append(out)
                if prefix_cache:
                    ids = torch.cat([ids, out[:, :-1], torch.tensor([[7, 9]])], 1)
        return m
    return fn


SAMPLING = dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9)
ARMS = ("greedy", "eos", "sampler-torch", "sampler-device", "penalty", "return-logits", "left-pad", "kv-fp8", "weights-fp8", "weights-int8",
        "adapters-merged", "adapters-live", "constraint", "prefix-cache", "beam", "beam-eos", "beam-kv-fp8")
R8 = dict(lora="r8")   # un-merged adapters


def _generate_cases(c):
    for B in (1, 2, 17):   # 1, 2: the session (B >= 2: re-tiled bf16 weights); 17: the GEMM step
        c[f"generate/greedy/B{B}"] = generate_case(B)
        c[f"generate/sampler-device/B{B}"] = generate_case(B, sampler="device", seed=7, **SAMPLING)
        c[f"generate/constraint/B{B}"] = generate_case(B, constraint=True, return_choices=True)
    for B in (2, 17):
        c[f"generate/eos/B{B}"] = generate_case(B, eos_token_id=2)
        c[f"generate/sampler-torch/B{B}"] = generate_case(B, seed=3, sampler="torch", **SAMPLING)
        c[f"generate/penalty/B{B}"] = generate_case(B, repetition_penalty=1.3)
        c[f"generate/return-logits/B{B}"] = generate_case(B, return_logits=True)
        c[f"generate/weights-int8/B{B}"] = generate_case(B, base="int8", weights="int8")
        c[f"generate/adapters-live/B{B}"] = generate_case(B, adapters="live", **R8)
    c["generate/sampler-device-penalty/B2"] = generate_case(2, sampler="device", seed=7, repetition_penalty=1.3, **SAMPLING)
    c["generate/left-pad/B2"] = generate_case(2, pad=True)
    c["generate/kv-fp8/B2"] = generate_case(2, kv_cache="fp8")
    c["generate/weights-fp8/B2"] = generate_case(2, weights="fp8")
    c["generate/adapters-merged/B2"] = generate_case(2, adapters="merged", **R8)
    c["generate/adapters-live/B2/weights-int8"] = generate_case(2, adapters="live", base="int8", weights="int8", **R8)
    c["generate/prefix-cache/bf16"] = generate_case(1, calls=2, prefix_cache="bf16")
    c["generate/prefix-cache/fp8"] = generate_case(1, calls=2, prefix_cache="fp8")
    c["generate/streamer-criteria/B2"] = generate_case(2, streamer=_Streamer(), stopping_criteria=[lambda ids, lg: ids.shape[1] >= 4])
    c["generate/no-graph/B2"] = generate_case(2, use_graph=False)
    # keywords that generate() swallows: neither changes what is launched (the second equals generate/adapters-merged/B2)
    c["generate/greedy/B2/return-sequences-none"] = generate_case(2, num_return_sequences=None)
    c["generate/adapters-merged/B2/stray-live-lora"] = generate_case(2, adapters="merged", live_lora=True, **R8)
    c["generate/beam/B2"] = generate_case(2, num_beams=2, return_beam_scores=True)
    c["generate/beam-eos/B2"] = generate_case(2, num_beams=2, eos_token_id=2, repetition_penalty=1.3, length_penalty=0.5)
    c["generate/beam-kv-fp8/B2"] = generate_case(2, num_beams=2, kv_cache="fp8", heads=16, dim=2048)   # 16 scale bytes of a position per chunk
    c["generate/beam/B2/left-pad/adapters-live"] = generate_case(2, num_beams=2, pad=True, adapters="live", **R8)
    # every rejection of a whole call, in the order they are made: (exception type, message, recorder calls made before it)
    rej = dict(adapters=dict(adapters="fused"), **{"adapters-none": dict(adapters=None), "adapters-none/unmerged-adapters": dict(adapters=None, **R8)}, constraint=dict(constraint=True, do_sample=True), **{
        "return-choices": dict(return_choices=True), "prefix-cache-batch": dict(prefix_cache="bf16"),
        "prefix-cache-kv": dict(B=1, prefix_cache="bf16", kv_cache="fp8"), "kv-cache": dict(kv_cache="int8"),
        "kv-fp8-17-rows": dict(B=17, kv_cache="fp8"), "kv-fp8-beam-heads": dict(num_beams=2, kv_cache="fp8"), "int8-without-base": dict(weights="int8"),
        "sampler": dict(sampler="host"), "sampler/unmerged-adapters": dict(sampler="host", **R8), "beam-count": dict(num_beams=0),
        "beam-sample": dict(num_beams=2, do_sample=True), "beam-streamer": dict(num_beams=2, streamer=_Streamer()),
        "beam-criteria": dict(num_beams=2, stopping_criteria=[]), "beam-sequences": dict(num_beams=2, num_return_sequences=2),
        "beam-early": dict(num_beams=2, early_stopping="never"), "beam-rows": dict(B=9, num_beams=2), "beam-width": dict(B=1, num_beams=9),
        "beam-rows/unmerged-adapters": dict(B=9, num_beams=2, **R8), "4bit-merged": dict(base="4bit", weights="4bit", **R8),
        "int8-merged": dict(base="int8", weights="int8", **R8), "unknown-weights": dict(weights="fp4")})
    for name, kw in rej.items():
        c[f"reject/generate/{name}"] = generate_case(**kw)


def _cases():
    c = {}
    for w in WEIGHTS:
        for B in (1, 2, 3, 4, 16):
            for kv in ("bf16", "fp8"):
                for ctx in (32, 256):
                    c[f"session/{w}/B{B}/kv-{kv}/ctx{ctx}"] = session_case(w, B, kv, ctx)
        for B in (1, 4):
            c[f"session/{w}/B{B}/kv-bf16/ctx32/hd64"] = session_case(w, B, "bf16", 32, heads=4)
        for lora in ("r8", "r4"):
            for B in (1, 2, 4, 16):
                c[f"session/{w}/B{B}/kv-bf16/ctx32/lora-{lora}"] = session_case(w, B, "bf16", 32, lora=lora)
            c[f"session/{w}/B3/kv-fp8/ctx256/lora-{lora}"] = session_case(w, 3, "fp8", 256, lora=lora)
        c[f"session/{w}/B2/kv-bf16/ctx256/kmask"] = session_case(w, 2, "bf16", 256, kmask=True)
        c[f"session/{w}/B2/kv-bf16/ctx32/twice"] = session_case(w, 2, "bf16", 32, sessions=2)
    for kv in ("bf16", "fp8"):
        c[f"session/bf16/B2/kv-{kv}/ctx256/nosplit"] = session_case("bf16", 2, kv, 256, split=False)
        c[f"session/bf16/B2/kv-{kv}/ctx32/kmask"] = session_case("bf16", 2, kv, 32, kmask=True)
        c[f"session/fp8/B4/kv-{kv}/ctx256/kmask"] = session_case("fp8", 4, kv, 256, kmask=True)
    c["session/bf16/B2/kv-bf16/ctx32/hd64/kmask"] = session_case("bf16", 2, "bf16", 32, heads=4, kmask=True)
    c["session/fp8/B2/kv-bf16/ctx32/e4m3-base"] = session_case("fp8", 2, "bf16", 32, base="e4m3")
    c["session/bf16/B2/kv-bf16/ctx32/4bit-base"] = session_case("bf16", 2, "bf16", 32, base="4bit")
    for ctx, S_new in ((0, 3), (5, 1)):
        for arm in ("plain", "lora", "int8", "int8+lora"):
            for kv in ("bf16", "fp8"):
                c[f"layer_step/ctx{ctx}/S{S_new}/{arm}/kv-{kv}"] = layer_step_case(ctx, S_new, arm, kv)
    c["layer_step/ctx0/S3/plain/kv-bf16/kmask"] = layer_step_case(0, 3, "plain", "bf16", kmask=True)
    c["layer_step/ctx0/S3/lora/kv-fp8/kmask"] = layer_step_case(0, 3, "lora", "fp8", kmask=True)
    # every rejection: (exception type, message, recorder calls made before it)
    c["reject/int8-without-base"] = session_case("int8", 1, "bf16", 32, base=None)
    c["reject/4bit-without-base"] = session_case("4bit", 1, "bf16", 32, base=None)
    c["reject/4bit-without-base/B4"] = session_case("4bit", 4, "bf16", 32, base=None)
    c["reject/mxfp4-192-wide"] = session_case("mxfp4", 2, "bf16", 32, heads=3, dim=192, ff=384)
    c["reject/int8-not-64"] = session_case("int8", 2, "bf16", 32, heads=3, dim=96, ff=160)
    c["reject/kv8-head-dim-64"] = session_case("bf16", 2, "fp8", 32, heads=4)
    c["reject/kv8-17-rows"] = session_case("bf16", 17, "fp8", 32)
    c["reject/unknown-weights"] = session_case("fp4", 2, "bf16", 32, base=None)
    c["reject/unknown-kv-cache"] = session_case("bf16", 2, "int8", 32)
    c["reject/lora-over-768-rows"] = session_case("bf16", 2, "bf16", 32, lora=dict(r=264, alpha=16, targets=("q", "k", "v", "o")))
    c["reject/lora-over-768-rows/int8"] = session_case("int8", 2, "bf16", 32, lora=dict(r=264, alpha=16, targets=("q", "k", "v", "o")))
    c["reject/lora-lds"] = session_case("bf16", 16, "bf16", 32, lora=dict(r=8, alpha=16, targets=("down",)), layers=1, empty=True, **LDS_SHAPE)
    c["reject/generate-int8-without-base"] = generate_reject_case("int8")
    _generate_cases(c)
    return c


LDS_SHAPE = dict(dim=256, ff=90112)   # 16 rows of a K-slice of the `down` group's 90112 inputs: past the 160 KiB of a CU (hk.lora_down_lds_bytes)
CASES = _cases()


def record_all():
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return {name: run(fn) for name, fn in CASES.items()}
    finally:
        torch.set_num_threads(threads)
