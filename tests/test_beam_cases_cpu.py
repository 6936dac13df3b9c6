"""CPU-only checks of the beam-search test helpers (tests/beam_cases.py) and of the host side of the beam kernels: the float64 reference
against the installed transformers' `generate(num_beams=...)` on a tiny float64 Llama, planted mistakes that must change a result, the
unambiguity of the kernel-test inputs, and the C-ABI / Python surface (rejections happen on the host, before any launch)."""
import inspect
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_cases as BC  # noqa: E402

MAX_NEW = 10
PROMPT = 5
V = 64
GRID = list(itertools.product((2, 3, 4), (0.5, 1.0, 2.0), (False, True), (1.0, 1.3), (1, 2)))   # nb, length_penalty, early_stopping, penalty, B


@pytest.fixture(scope="module")
def llama():
    from transformers import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(vocab_size=V, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                      max_position_embeddings=64, bos_token_id=None, eos_token_id=None, pad_token_id=0)
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).double().eval()
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 2:
                p.mul_(3.0)   # peaked distributions: the beams differ and the scores spread
    return model


def _prompt_embeds(model, B, seed):
    ids = torch.randint(1, V, (B, PROMPT), generator=torch.Generator().manual_seed(seed))
    return model.get_input_embeddings()(ids).detach()


def _hf(model, emb, nb, lp, early, pen, eos):
    with torch.no_grad():
        out = model.generate(inputs_embeds=emb, attention_mask=torch.ones(emb.shape[:2], dtype=torch.long), num_beams=nb, do_sample=False,
                             max_new_tokens=MAX_NEW, length_penalty=lp, early_stopping=early, repetition_penalty=pen, eos_token_id=eos,
                             pad_token_id=0)
    return out.numpy()


def _ref(model, emb, nb, lp, early, pen, eos, mutation=None):
    B = emb.shape[0]
    embed = model.get_input_embeddings()

    def logits_fn(t, seqs):
        x = emb.repeat_interleave(nb, 0)
        if t:
            x = torch.cat([x, embed(torch.tensor(seqs))], 1)
        with torch.no_grad():
            return model(inputs_embeds=x).logits[:, -1].float().numpy()   # HF's beam search takes the logits in fp32

    return BC.ref_beam_search(logits_fn, B, nb, MAX_NEW, lp, early, eos, pen, pad=0, mutation=mutation)


_RESULTS = {}


def _case(model, i):
    """(eos, HF ids, reference result) of grid case i, computed once"""
    if i not in _RESULTS:
        nb, lp, early, pen, B = GRID[i]
        emb = _prompt_embeds(model, B, 100 + i)
        free = _hf(model, emb, nb, lp, early, pen, None)
        eos = int(free[0, 2])   # a token at position >= 2 of the case's own no-EOS result
        _RESULTS[i] = (emb, eos, _hf(model, emb, nb, lp, early, pen, eos), _ref(model, emb, nb, lp, early, pen, eos),
                       free, _ref(model, emb, nb, lp, early, pen, None))
    return _RESULTS[i]


def test_reference_equals_hf_generate(llama):
    n_eos_end = n_early = 0
    for i, (nb, lp, early, pen, B) in enumerate(GRID):
        emb, eos, hf, (ids, scores, n_steps, gaps), hf_free, (ids_free, _, n_free, _) = _case(llama, i)
        what = f"case {i}: nb={nb} lp={lp} early={early} pen={pen} B={B} eos={eos}"
        assert n_free == MAX_NEW and np.array_equal(hf_free, ids_free), what
        ended = False
        for b in range(B):
            want, got = BC.upto_eos(hf[b], eos), BC.upto_eos(ids[b], eos)
            assert want == got, f"{what} row {b}: HF {want} reference {got}"
            ended |= want[-1] == eos
        n_eos_end += ended
        n_early += n_steps < MAX_NEW
    print(f"\nBEAM_HF_PIN cases={len(GRID)} ended_by_eos={n_eos_end} loops_stopped_early={n_early}")
    assert 2 * n_eos_end >= len(GRID), (n_eos_end, len(GRID))
    assert n_early >= 1


@pytest.mark.parametrize("mutation", ("length_exponent", "no_start_neg", "rank_ge_nb_accepted"))
def test_planted_mistake_changes_a_result(llama, mutation):
    changed = 0
    for i, (nb, lp, early, pen, B) in enumerate(GRID):
        emb, eos, hf, (ids, *_), _, _ = _case(llama, i)
        bad = _ref(llama, emb, nb, lp, early, pen, eos, mutation=mutation)[0]
        changed += any(BC.upto_eos(ids[b], eos) != BC.upto_eos(bad[b], eos) for b in range(B))
    print(f"\nBEAM_MUTATION {mutation}: {changed} of {len(GRID)} cases change")
    assert changed >= 1


# ------------------------------------------------------------------------------------------------ kernel-test inputs
def test_band_rule():
    assert BC.SCORE_BOUND <= 1e-4 and BC.BAND == 16 * BC.SCORE_BOUND


@pytest.mark.parametrize("B,nb", BC.STEP_GRID)
def test_kernel_inputs_are_unambiguous(B, nb):
    for Vk in BC.VOCABS:
        for scale in BC.SCALES:
            for pen in BC.PENALTIES:
                before, logits, after, steps = BC.make_step_case(B, nb, Vk, scale, pen)
                for b, s in enumerate(steps):
                    assert s.gap > 1.6e-3 >= BC.BAND, (B, nb, Vk, scale, pen, b, s.gap)
                    assert all(len(q) == BC.STEP_T for q in before[b].seqs) and (np.diff(before[b].run) < 0).all() and before[b].run[0] < 0
                if pen != 1.0:   # the penalty decides: without it another token list comes out
                    plain = BC.make_step_case(B, nb, Vk, scale, 1.0)[3]
                    assert any(list(s.tok) != list(p.tok) or list(s.beam) != list(p.beam) for s, p in zip(steps, plain)), (B, nb, Vk, scale)


# ------------------------------------------------------------------------------------------------ ABI and Python surface
def test_header_declares_and_library_exports_the_beam_entry_points():
    from lhrs_bot_amd import _lib

    protos = _lib.parse_header()
    exported = set(re.findall(r" T (lhrs_\w+)", subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout))
    for name, n_args in (("lhrs_beam_topk_rows", 13), ("lhrs_beam_step", 20), ("lhrs_kv_beam_reorder", 13)):
        assert name in protos and len(protos[name][1]) == n_args and name in exported, name


def _rejected(st, msg):
    from lhrs_bot_amd import _lib

    lib = _lib.load()
    assert st == -1 and msg in lib.lhrs_last_error(), lib.lhrs_last_error()
    with pytest.raises(RuntimeError):
        _lib.check(st, "beam")


@pytest.mark.parametrize("kw,msg", [
    (dict(V=32769), b"V=32769"), (dict(V=3), b"V=3"), (dict(K=18), b"K=18"), (dict(n=0), b"n_rows=0"), (dict(pen=0.0), b"repetition_penalty"),
    (dict(pen=1.3), b"history"), (dict(), b"logits="),
])
def test_rejected_topk_call_reports_error_without_gpu(kw, msg):
    from lhrs_bot_amd import _lib

    a = dict(V=32000, K=8, n=4, pen=1.0)
    a.update(kw)
    # no pointer is touched before the arguments are accepted: NULL everywhere
    _rejected(_lib.load().lhrs_beam_topk_rows(None, a["V"], a["n"], a["V"], a["K"], None, a["pen"], None, 8, None, None, None, None), msg)


@pytest.mark.parametrize("kw,msg", [
    (dict(nb=9), b"num_beams=9"), (dict(nb=1), b"num_beams=1"), (dict(B=5, nb=4), b"B=5"), (dict(V=32769), b"V=32769"), (dict(max_new=0), b"max_new=0"),
    (dict(), b"NULL"),
])
def test_rejected_step_call_reports_error_without_gpu(kw, msg):
    from lhrs_bot_amd import _lib

    a = dict(B=1, nb=4, V=32000, max_new=8)
    a.update(kw)
    _rejected(_lib.load().lhrs_beam_step(None, None, a["B"], a["nb"], a["V"], a["max_new"], -1, 0, *([None] * 12)), msg)


@pytest.mark.parametrize("kw,msg", [
    (dict(nb=9), b"num_beams=9"), (dict(B=9, nb=2), b"B=9"), (dict(d=12), b"d=12"), (dict(t0=10, max_pos=8), b"max_pos=8"), (dict(t1=9), b"t1=9"),
    (dict(n=0), b"n_caches=0"), (dict(), b"table="),
])
def test_rejected_reorder_call_reports_error_without_gpu(kw, msg):
    from lhrs_bot_amd import _lib

    a = dict(n=4, B=1, nb=4, max_ctx=16, d=256, t0=3, t1=5, max_pos=4)
    a.update(kw)
    _rejected(_lib.load().lhrs_kv_beam_reorder(None, a["n"], a["B"], a["nb"], a["max_ctx"], a["d"], None, a["t0"], None, a["t1"], a["max_pos"], None,
                                               None), msg)


def test_generate_signature_has_the_beam_keywords():
    from lhrs_bot_amd.text import TextModal

    for fn in (TextModal.generate, TextModal._generate):
        sig = inspect.signature(fn).parameters
        assert sig["num_beams"].default == 1 and sig["length_penalty"].default == 1.0
        assert sig["early_stopping"].default is False and sig["return_beam_scores"].default is False


def test_cli_has_the_beam_arguments():
    sys.path.insert(0, ROOT)
    import cli_qa

    cfg = cli_qa.parse_option([])
    assert cfg.num_beams == 1 and cfg.length_penalty == 1.0
    cfg = cli_qa.parse_option(["--num-beams", "4", "--length-penalty", "0.5"])
    assert cfg.num_beams == 4 and cfg.length_penalty == 0.5
