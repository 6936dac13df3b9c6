"""The one-layer decoder of tests/fp8_base_cases.py::MODEL on a two-sequence batch, under every frozen base, shared by
tests/test_fp8_base_paths_gpu.py (model and batch), tests/test_decoder_trace_gpu.py and tools/record_decoder_traces.py (the cells and the
recorder).  Only the public model API is used (quantize_base, enable_lora, decode, backward), so the recording tool runs on any commit.

A cell is (base, adapter setting, rows, native): `run_cell` does one unrecorded decode + backward (whatever a first call allocates or packs
happens there), then one under a recorder over every public function of lhrs_bot_amd/kernels.py.  One log line per call:
    name(arg=dtype[shape], ...; optional arguments whose value is not the default)
Tensors inside a tuple argument are listed in order; scalars, dicts and lists are not logged."""
import contextlib
import inspect
import os

import torch

from lhrs_bot_amd import kernels as hk
from lhrs_bot_amd.text import IGNORE_INDEX, IMAGE_TOKEN_INDEX, TextModal

import fp8_base_cases as fc

BF = torch.bfloat16
BASES = {"bf16": None, "e4m3": dict(bits=8, scheme="e4m3"), "int8": dict(bits=8, scheme="int8"), "nf4": dict(bits=4, quant_type="nf4")}
ROWS = ("every_row", "tail")
# every base x adapter setting x rows, plus the operator path of the frozen bf16 base (LHRS_NATIVE_LAYER=0; with one layer the compact
# last-layer run never takes the whole-layer entry point, its two cells must be equal)
CELLS = [(b, s, r, True) for b in BASES for s in fc.SETTINGS for r in ROWS] + [("bf16", "none", r, False) for r in ROWS]


def cell_id(cell):
    base, setting, rows, native = cell
    return f"{base}-{setting}-{rows}" + ("" if native else "-native_off")


def batch(device):
    """two sequences of 36 tokens with one <image> placeholder each, 5 image rows: S = 40, M = 80"""
    g = torch.Generator().manual_seed(17)
    B, T, NI = 2, 36, 5
    ids = torch.randint(3, fc.MODEL["vocab"], (B, T), generator=g)
    ids[:, 3] = IMAGE_TOKEN_INDEX
    mask = torch.ones(B, T, dtype=torch.int64)
    mask[1, 26:] = 0                                                      # the second sequence is right-padded: 30 keys after the splice
    labels = torch.full((B, T), IGNORE_INDEX, dtype=torch.int64)
    labels[0, 21:36] = ids[0, 21:36]                                       # labels on a contiguous tail of each sequence
    labels[1, 16:26] = ids[1, 16:26]
    image = (torch.randn(B, NI, fc.MODEL["dim"], generator=g) * 0.05).to(BF).to(device)
    return ids, image, mask, labels


def make_model(setting, seed=3, base="e4m3", device="cuda"):
    m = TextModal(device=device, max_pos=128, **fc.MODEL)
    m.init_random(seed=seed)
    g = torch.Generator().manual_seed(100 + seed)
    for w in (m.p["layers"][0]["ln1_w"], m.p["layers"][0]["ln2_w"], m.p["norm_w"]):      # init_random leaves all three at 1: tell them apart
        w.copy_((1 + 0.1 * torch.randn(w.shape, generator=g)).to(BF))
    if BASES[base] is not None:
        m.quantize_base(**BASES[base])
    kw = fc.SETTINGS[setting]
    if kw is not None:
        lo = m.enable_lora(seed=5, **kw)
        g = torch.Generator().manual_seed(11)
        for proj in kw["targets"]:                                       # B starts at zero in peft: the adapter term must show per element
            A, B = lo.get_adapter(0, proj)
            lo.set_adapter(0, proj, A.clone(), torch.randn(B.shape, generator=g) * 0.05)
        lo.refresh()
        assert lo.train_mode
    return m


def model_cache():
    cache = {}

    def get(base, setting):
        if (base, setting) not in cache:
            cache[(base, setting)] = make_model(setting, base=base)
        return cache[(base, setting)]
    return get


# ------------------------------------------------------------------------------------------------------------------------- the recorder
def _desc(v):
    if torch.is_tensor(v):
        return f"{str(v.dtype).replace('torch.', '')}{list(v.shape)}"
    if isinstance(v, tuple):
        inner = [d for d in map(_desc, v) if d is not None]
        return "(" + ",".join(inner) + ")" if inner else None
    return None


def _is_default(v, default):
    if v is default:
        return True
    if torch.is_tensor(v) or torch.is_tensor(default) or isinstance(v, (tuple, list, dict)):
        return False
    return v == default


def public_functions():
    return sorted(n for n, f in vars(hk).items() if inspect.isfunction(f) and f.__module__ == hk.__name__ and not n.startswith("_"))


@contextlib.contextmanager
def recording():
    """-> list of log lines, one per call of a public function of kernels.py made while the context is open (calls that those functions
    make to each other included); every call is the original's"""
    log, orig = [], {n: getattr(hk, n) for n in public_functions()}

    def wrap(name, fn):
        sig = inspect.signature(fn)

        def rec(*args, **kw):
            b = sig.bind(*args, **kw)
            b.apply_defaults()
            tensors = [f"{k}={d}" for k, d in ((k, _desc(v)) for k, v in b.arguments.items()) if d is not None]
            given = [k for k, v in b.arguments.items() if sig.parameters[k].default is not inspect.Parameter.empty
                     and not _is_default(v, sig.parameters[k].default)]
            log.append(f"{name}({', '.join(tensors)}; {' '.join(given)})")
            return fn(*args, **kw)
        return rec

    try:
        for n, f in orig.items():
            setattr(hk, n, wrap(n, f))
        yield log
    finally:
        for n, f in orig.items():
            setattr(hk, n, f)


@contextlib.contextmanager
def _native_layer(on):
    saved = os.environ.get("LHRS_NATIVE_LAYER")
    os.environ["LHRS_NATIVE_LAYER"] = "1" if on else "0"
    try:
        yield
    finally:
        if saved is None:
            del os.environ["LHRS_NATIVE_LAYER"]
        else:
            os.environ["LHRS_NATIVE_LAYER"] = saved


def run_cell(cell, models):
    """-> (log, dict of the tensors the step produced: loss, d_image, the final-norm hidden rows, the flat adapter gradients or None)"""
    base, setting, rows, native = cell
    m = models(base, setting)
    saved_tail = m.tail_rows_only
    m.tail_rows_only = rows == "tail"
    ids, image, mask, labels = batch(m.device)
    try:
        with _native_layer(native):
            m.decode(ids, image, mask, labels)
            m.backward()
            if m.lora is not None:
                m.lora.grad.zero_()
            with recording() as log:
                loss = m.decode(ids, image, mask, labels)
                hidden = m.last_hidden
                assert hidden.shape[0] == (25 if rows == "tail" else 80)   # the supervised rows only / all B * S
                d_image = m.backward()
        torch.cuda.synchronize()
    finally:
        m.tail_rows_only = saved_tail
    return log, dict(loss=loss, d_image=d_image, hidden=hidden, adapter_grads=None if m.lora is None else m.lora.grad.clone())
