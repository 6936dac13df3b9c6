"""lhrs_sample_rows (csrc/sample.hip) on the GPU against the float64 reference of tests/sampling_cases.py, and generate(sampler="device" /
repetition_penalty=...) on small random-init models.  Every rejected-argument check lives in test_sampling_cases_cpu.py (host side)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_cases as SC  # noqa: E402
from lhrs_bot_amd import kernels as hk  # noqa: E402
from lhrs_bot_amd.text import warp_logits  # noqa: E402
from lhrs_bot_amd.unibind import UniBind  # noqa: E402

DEV = "cuda"
SEED = 0xC0FFEE_0123_4567_89
STEP0 = 5   # step_host: the counter is step_host + *step_dev


def _strided(logits, ld):
    n, V = logits.shape
    buf = torch.zeros(n, ld)
    buf[:, :V] = logits
    return buf.to(DEV)[:, :V]


def _bitmap(seen):
    return torch.from_numpy(np.stack([SC.bool_to_bitmap(r) for r in seen])).to(DEV)


def _run_steps(x, params, seen, mode=0):
    n, V = x.shape
    bitmap = _bitmap(seen) if seen is not None else None
    step_dev = torch.zeros(1, device=DEV, dtype=torch.int32)
    toks = torch.full((SC.N_STEPS, n), -1, device=DEV, dtype=torch.int64)
    weights = torch.full((SC.N_STEPS, n, V), -7, device=DEV, dtype=torch.int64)
    for t in range(SC.N_STEPS):
        hk.sample_rows(x, toks[t], mode=mode, temperature=params.temperature, top_k=params.top_k, top_p=params.top_p,
                       repetition_penalty=params.penalty, seen=bitmap, seed=SEED, step_dev=step_dev, step_host=STEP0, weights_out=weights[t])
        step_dev += 1
    return toks, weights, bitmap


# (a) support, (b) distribution, (c) draw, (d) seen bitmap.  (c) runs on all 64 x n draws of every case.  (a) and (b) compare one row's weights
# with the reference: without a penalty the weights of the 64 steps are bit-equal (asserted), so one comparison covers them all; with a penalty
# every draw changes the seen set and with it the row, and the steps of REF_STEPS are compared, each against the bitmap that the draws before
# it left behind.
REF_STEPS = (0, SC.N_STEPS - 1)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("scale", SC.SCALES)
@pytest.mark.parametrize("params", SC.GRID, ids=lambda p: f"t{p.temperature}-k{p.top_k}-p{p.top_p}-r{p.penalty}")
def test_kernel_against_reference(params, scale):
    worst = 0.0
    for V in SC.VOCABS:
        for ld in (V, V + 5):
            for n in SC.ROWS:
                what = f"V={V} ld={ld} n={n}"
                logits = SC.make_logits(n, V, scale, seed=1000 + n)
                x = _strided(logits, ld)
                seen0 = SC.make_seen(n, V, seed=7 + n) if params.penalty != 1.0 else None
                toks, weights, bitmap = _run_steps(x, params, seen0)
                toks_h = toks.cpu().numpy()
                assert toks_h.min() >= 0 and toks_h.max() < V, what
                if seen0 is None:
                    assert bool((weights == weights[:1]).all()), what
                    w_h = weights[:1].cpu().numpy()
                else:
                    w_h = weights.cpu().numpy()
                lg = logits.numpy()
                for r in range(n):
                    for t in range(SC.N_STEPS):
                        w = w_h[t if seen0 is not None else 0, r]
                        if t == 0 or (seen0 is not None and t in REF_STEPS):
                            seen = None
                            if seen0 is not None:
                                seen = seen0[r].copy()
                                seen[toks_h[:t, r]] = True
                            m = SC.check(w, SC.ref_sample64(lg[r], seen, params), toks_h[t, r], SEED, STEP0 + t, r, f"{what} row {r} step {t}")
                            worst = max(worst, m.l1)
                        else:
                            assert toks_h[t, r] == SC.draw_from_weights(w, SEED, STEP0 + t, r), f"{what} row {r} step {t}"
                if seen0 is not None:  # (d)
                    want = seen0.copy()
                    for r in range(n):
                        want[r, toks_h[:, r]] = True
                    words = bitmap.cpu().numpy()
                    got = np.stack([SC.bitmap_to_bool(b, 32 * words.shape[1]) for b in words])
                    assert (got[:, :V] == want).all() and not got[:, V:].any(), what
    print(f"\nSAMPLING_WORST params={tuple(params)} scale={scale} l1={worst:.3e} excused={SC.WORST['n_excused']}")


@pytest.mark.timeout(300)
def test_kernel_is_deterministic():
    for params in (SC.GRID[0], SC.GRID[2], SC.GRID[4], SC.GRID[6]):
        logits = SC.make_logits(16, 32000, 8, seed=3)
        x = _strided(logits, 32000)
        seen0 = SC.make_seen(16, 32000, seed=4) if params.penalty != 1.0 else None
        a = _run_steps(x, params, seen0)
        b = _run_steps(x, params, seen0)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        if seen0 is not None:
            assert torch.equal(a[2], b[2])


@pytest.mark.timeout(300)
def test_mode_1_is_argmax_of_the_penalised_row():
    for V, ld in ((32000, 32000), (32000, 32005), (32003, 32003), (1000, 1000)):
        logits = SC.make_logits(16, V, 1, seed=9)
        logits[1, 17] = logits[1, V - 3] = logits[1].max() + 1     # the maximum twice: the lowest index wins
        logits[2, V - 1] = logits[2, 0] = logits[2].max() + 1
        x = _strided(logits, ld)
        got = hk.sample_rows(x, mode=1, temperature=1.0)
        assert torch.equal(got, hk.argmax_rows(x))
        assert got[1].item() == 17 and got[2].item() == 0
        # penalty 1.3: the float64 argmax of the penalised row, and the picked bit enters the bitmap
        seen0 = SC.make_seen(16, V, seed=10)
        top = logits.argsort(-1, descending=True)[:, :3].numpy()
        for r in range(16):
            seen0[r, top[r, 0]] = True   # the unpenalised maximum has been seen: the penalty decides
        bitmap = _bitmap(seen0)
        got = hk.sample_rows(x, mode=1, temperature=1.0, repetition_penalty=1.3, seen=bitmap).cpu().numpy()
        after = bitmap.cpu().numpy()
        for r in range(16):
            pen = SC.penalised(logits[r].numpy(), seen0[r], 1.3).astype(np.float64)
            assert got[r] == int(np.argmax(pen)), (V, ld, r)
            want = seen0[r].copy()
            want[got[r]] = True
            assert (SC.bitmap_to_bool(after[r], V) == want).all()


# ------------------------------------------------------------------------------------------------ generate
NEW = 12


@pytest.fixture(scope="module")
def model():
    return UniBind(("rgb", "text"), None, device=DEV, llama_layers=2).init_random(seed=1).eval()


def _prompt(B):
    return torch.tensor([[1, 50, 600, 7000, 80, 9], [1, 7, 8000, 31000, 12, 4]][:B])


def _gen(model, B, **kw):
    kw.setdefault("do_sample", True)
    kw.setdefault("eos_token_id", None)
    kw.setdefault("max_new_tokens", NEW)
    return model.generate(_prompt(B), images=None, **kw)


def _replay(logits, params, seed, mode=0):
    """hk.sample_rows over the returned logits [B, n, V], steps 0.. and a fresh bitmap; also the HF support of every step"""
    B, n, V = logits.shape
    bitmap = torch.zeros((B, (V + 31) // 32), device=DEV, dtype=torch.int32) if params.penalty != 1.0 else None
    ids = [hk.sample_rows(logits[:, t].contiguous(), mode=mode, temperature=params.temperature, top_k=params.top_k, top_p=params.top_p,
                          repetition_penalty=params.penalty, seen=bitmap, seed=seed, step_host=t) for t in range(n)]
    return torch.stack(ids, 1)


def _assert_in_hf_support(ids, logits, params):
    ids_h, lg = ids.cpu().numpy(), logits.cpu().numpy()
    for b in range(ids_h.shape[0]):
        for t in range(ids_h.shape[1]):
            seen_ids = ids_h[b, :t]
            seen = np.zeros(lg.shape[-1], dtype=bool)
            seen[seen_ids] = True
            ok = SC.hf_support(lg[b, t], seen_ids, params)[ids_h[b, t]] or SC.ref_sample64(lg[b, t], seen, params).ambiguous[ids_h[b, t]]
            assert ok, (b, t, int(ids_h[b, t]))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("B", (1, 2))
def test_generate_device_sampler(model, B):
    p = SC.Params(0.4, 50, 0.9, 1.0)
    kw = dict(temperature=p.temperature, top_k=p.top_k, top_p=p.top_p, sampler="device")
    a, a_lg = _gen(model, B, seed=11, return_logits=True, **kw)
    b = _gen(model, B, seed=11, **kw)
    assert a.shape == (B, NEW) and torch.equal(a, b)                                  # same seed, same ids
    c, c_lg = _gen(model, B, seed=11, return_logits=True, use_graph=False, **kw)
    assert torch.equal(a, c) and torch.equal(a_lg, c_lg)                              # graph replay == eager launches
    assert torch.equal(_replay(a_lg, p, 11), a)                                       # the ids are the kernel's draws from the returned logits
    _assert_in_hf_support(a, a_lg, p)
    flat = dict(temperature=1.3, top_k=0, top_p=1.0, sampler="device")
    assert not torch.equal(_gen(model, B, seed=1, **flat), _gen(model, B, seed=2, **flat))
    torch.manual_seed(77)                                                             # seed=None: torch.initial_seed()
    d = _gen(model, B, **flat)
    assert torch.equal(d, _gen(model, B, seed=77, **flat))
    greedy = _gen(model, B, do_sample=False)
    assert torch.equal(_gen(model, B, seed=3, temperature=0.7, top_k=1, top_p=1.0, sampler="device"), greedy)


@pytest.mark.timeout(600)
def test_generate_device_sampler_with_penalty_and_fp8(model):
    p = SC.Params(1.0, 50, 0.95, 1.05)
    kw = dict(temperature=p.temperature, top_k=p.top_k, top_p=p.top_p, repetition_penalty=p.penalty, sampler="device")
    a, a_lg = _gen(model, 2, seed=5, return_logits=True, **kw)
    assert torch.equal(_replay(a_lg, p, 5), a)
    _assert_in_hf_support(a, a_lg, p)
    t, t_lg = _gen(model, 2, seed=5, return_logits=True, **dict(kw, sampler="torch"))   # a penalty routes through the kernel whatever the sampler
    assert torch.equal(t, a) and torch.equal(t_lg, a_lg)
    p8 = SC.Params(0.4, 50, 0.9, 1.0)
    f, f_lg = _gen(model, 1, seed=6, return_logits=True, weights="fp8", temperature=p8.temperature, top_k=p8.top_k, top_p=p8.top_p, sampler="device")
    assert f.shape == (1, NEW) and torch.equal(_replay(f_lg, p8, 6), f)


@pytest.mark.timeout(600)
def test_generate_greedy_with_repetition_penalty(model):
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor

    ids, lg = _gen(model, 2, do_sample=False, repetition_penalty=1.3, return_logits=True)
    proc = RepetitionPenaltyLogitsProcessor(1.3)
    ids_h, lg_h = ids.cpu(), lg.cpu()
    for t in range(NEW):
        scores = proc(ids_h[:, :t], lg_h[:, t].clone()) if t else lg_h[:, 0]
        assert torch.equal(scores.argmax(-1), ids_h[:, t]), t
    assert torch.equal(_replay(lg, SC.Params(1.0, 0, 1.0, 1.3), 0, mode=1), ids)


@pytest.mark.timeout(600)
def test_generate_sampled_eos_torch_path_and_bad_sampler(model):
    kw = dict(temperature=0.4, top_k=50, top_p=0.9, sampler="device", seed=21)
    full = _gen(model, 1, **kw)
    toks = full[0].tolist()
    j = max(i for i in range(len(toks)) if toks[i] not in toks[:i])   # as test_sampling_path_runs_and_respects_eos: a token at its first occurrence
    stop = _gen(model, 1, **dict(kw, eos_token_id=int(toks[j])))
    assert stop.shape[1] == j + 1 and torch.equal(stop[0], full[0, :j + 1])
    # sampler="torch", penalty 1: the path of before - HF-style warpers and torch.multinomial from the global generator, unchanged
    tk = dict(temperature=0.4, top_k=50, top_p=0.9)
    torch.manual_seed(0)
    a, a_lg = _gen(model, 2, return_logits=True, sampler="torch", **tk)
    torch.manual_seed(0)
    b = _gen(model, 2, **tk)
    assert torch.equal(a, b)
    torch.manual_seed(0)
    want = torch.stack([torch.multinomial(torch.softmax(warp_logits(a_lg[:, t], 0.4, 50, 0.9), -1), 1).squeeze(1) for t in range(NEW)], 1)
    assert torch.equal(a, want)
    with pytest.raises(ValueError):
        _gen(model, 1, sampler="nope")
