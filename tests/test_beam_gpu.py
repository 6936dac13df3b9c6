"""The beam-search kernels (csrc/beam.hip) on the GPU against the float64 reference of tests/beam_cases.py, and generate(num_beams=...) on small
random-init models, replayed step by step over the logits it returns.  Rejected C-ABI arguments live in test_beam_cases_cpu.py (host side)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_cases as BC  # noqa: E402
from lhrs_bot_amd import kernels as hk  # noqa: E402
from lhrs_bot_amd.unibind import UniBind  # noqa: E402

DEV = "cuda"


def _strided(logits, ld):
    n, V = logits.shape
    buf = torch.zeros(n, ld)
    buf[:, :V] = torch.from_numpy(logits)
    return buf.to(DEV)[:, :V]


def _upload(st, rows, t):
    """reference rows -> the device state before step t"""
    B, nb = st.B, st.nb
    hist = np.zeros((2, B * nb, st.max_new), dtype=np.int32)
    fin_score, fin_len, fin_seq = np.full(B * nb, BC.NEG, dtype=np.float32), np.zeros(B * nb, dtype=np.int32), np.zeros((B * nb, st.max_new), dtype=np.int32)
    for b, r in enumerate(rows):
        for j in range(nb):
            hist[t & 1, b * nb + j, :t] = r.seqs[j]
            if r.fin_seq[j] is not None:
                fin_score[b * nb + j], fin_len[b * nb + j] = r.fin_score[j], len(r.fin_seq[j])
                fin_seq[b * nb + j, :len(r.fin_seq[j])] = r.fin_seq[j]
    st.bstate.copy_(torch.tensor([t, 0, 0, 0], dtype=torch.int32))
    st.run_score.copy_(torch.tensor(np.concatenate([r.run for r in rows]), dtype=torch.float32))
    st.hist.copy_(torch.from_numpy(hist))
    st.fin_score.copy_(torch.from_numpy(fin_score))
    st.fin_len.copy_(torch.from_numpy(fin_len))
    st.fin_seq.copy_(torch.from_numpy(fin_seq))
    st.heur.copy_(torch.tensor([int(r.heur) for r in rows], dtype=torch.int32))


def _near(got, want, what, bound=None):
    err = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))))
    BC.WORST["score"] = max(BC.WORST["score"], err)
    assert err <= (BC.SCORE_BOUND if bound is None else bound), f"{what}: |score - ref64| = {err:.3e}"
    return err


def _check_state(st, next_ids, rows, steps, t, goes_on, what, bound=None):
    """the device state after step t against the reference rows after it; -> worst score error.  bound: SCORE_BOUND for ONE device step from an
    uploaded reference state; a chain of n device steps accumulates n such errors in its scores (the rule of the end-to-end replay)"""
    B, nb = st.B, st.nb
    n = t + 1
    bstate = st.bstate.cpu().tolist()
    assert bstate[0] == n and bstate[1] == int(not goes_on), (what, bstate)
    run, parent, nxt = st.run_score.cpu().numpy(), st.parent.cpu().numpy(), next_ids.cpu().numpy()
    hist = st.hist[n & 1].cpu().numpy()
    fin_score, fin_len, fin_slot, fin_seq = st.fin_score.cpu().numpy(), st.fin_len.cpu().numpy(), st.fin_slot.cpu().numpy(), st.fin_seq.cpu().numpy()
    worst = 0.0
    for b, (r, s) in enumerate(zip(rows, steps)):
        g = slice(b * nb, (b + 1) * nb)
        assert list(parent[g]) == s.parent and list(nxt[g]) == s.next_tok, (what, b, list(parent[g]), s.parent, list(nxt[g]), s.next_tok)
        live = r.run > BC.NEG / 2
        if live.any():   # at t + 1 == max_new every candidate hit: all running scores carry the -1e9
            worst = max(worst, _near(run[g][live], r.run[live], f"{what} row {b} running", bound))
        assert (run[g][~live] <= BC.NEG / 2).all(), (what, b)
        for j in range(nb):
            assert list(hist[b * nb + j, :n]) == r.seqs[j], (what, b, j)
            if r.fin_seq[j] is None:
                assert fin_len[b * nb + j] == 0 and fin_score[b * nb + j] == np.float32(BC.NEG), (what, b, j)
            else:
                assert fin_len[b * nb + j] == len(r.fin_seq[j]), (what, b, j)
                assert list(fin_seq[b * nb + fin_slot[b * nb + j], :len(r.fin_seq[j])]) == r.fin_seq[j], (what, b, j)
                worst = max(worst, _near(fin_score[b * nb + j], r.fin_score[j], f"{what} row {b} finished {j}", bound))
        assert sorted(fin_slot[g]) == list(range(nb)), (what, b)
        assert int(st.heur[b].item()) == int(r.heur), (what, b)
    return worst


# ------------------------------------------------------------------------------------------------ beam_topk_rows + beam_step
@pytest.mark.timeout(300)
@pytest.mark.parametrize("scale", BC.SCALES)
@pytest.mark.parametrize("B,nb", BC.STEP_GRID)
def test_topk_rows_and_step_against_reference(B, nb, scale):
    worst = 0.0
    K, t = 2 * nb, BC.STEP_T
    for V in BC.VOCABS:
        for pen in BC.PENALTIES:
            before, logits, after, steps = BC.make_step_case(B, nb, V, scale, pen)
            for ld in (V, V + 8, V + 5):   # rows that are / are not 16-byte aligned, with and without padding
                what = f"B={B} nb={nb} V={V} ld={ld} scale={scale} pen={pen}"
                st = hk.BeamState(B, nb, V, BC.STEP_MAX_NEW, 1.0, DEV)
                _upload(st, before, t)
                hk.beam_topk_rows(_strided(logits, ld), st, pen)
                cs, ct = st.cand_score.cpu().numpy(), st.cand_tok.cpu().numpy()
                for b, s in enumerate(steps):
                    for j in range(nb):
                        r = b * nb + j
                        worst = max(worst, _near(cs[r], s.row_score[j, :K], f"{what} beam {r} list"))
                        assert (np.diff(cs[r]) <= 0).all() and ct[r].min() >= 0 and ct[r].max() < V and len(set(ct[r])) == K, (what, r)
                        gaps = -np.diff(s.row_score[j])                      # K gaps: below rank k is gaps[k], above it gaps[k - 1]
                        clear = np.array([(k == 0 or gaps[k - 1] > BC.BAND) and gaps[k] > BC.BAND for k in range(K)])
                        assert (ct[r][clear] == s.row_tok[j][clear]).all(), (what, r, ct[r], s.row_tok[j])
                next_ids = torch.full((B * nb,), -1, device=DEV, dtype=torch.int64)
                hk.beam_step(st, next_ids, None, False)
                worst = max(worst, _check_state(st, next_ids, after, steps, t, True, what))
    print(f"\nBEAM_WORST B={B} nb={nb} scale={scale} score={worst:.3e}")


# ------------------------------------------------------------------------------------------------ forced EOS, three chained steps
@pytest.mark.timeout(300)
def test_forced_eos_three_chained_steps_and_launch_after_done():
    B, nb, V = BC.EOS_B, BC.EOS_NB, BC.EOS_V
    lgs, snaps, steps, go = BC.make_eos_case()
    # what the case is for (the reference says so; the device must agree with it below)
    assert all(s.hit[1] and not s.hit[0] for s in steps[0])
    assert all(any(s.hit[k] for k in range(nb)) and any(s.hit[k] for k in range(nb, 2 * nb)) for s in steps[1])     # hits on both sides of rank nb
    assert all(r.full() and min(len(q) for q in r.fin_seq) < 3 for r in snaps[2])   # an EOS hypothesis survives next to those cut at max_new
    assert all(sum(q is not None for q in r.fin_seq) == 2 for r in snaps[1])   # after step 1: one hit per step entered, the rank >= nb ones did not
    assert all(s.all_hit for s in steps[2]) and go == [True, True, False]
    assert min(s.gap for st_ in steps for s in st_) > 1.6e-3 >= BC.BAND
    st = hk.BeamState(B, nb, V, BC.EOS_MAX_NEW, 1.0, DEV)
    next_ids = torch.full((B * nb,), -1, device=DEV, dtype=torch.int64)
    for t in range(BC.EOS_MAX_NEW):
        hk.beam_topk_rows(_strided(lgs[t], V), st, 1.0)
        hk.beam_step(st, next_ids, BC.EOS_TOKEN, False)
        _check_state(st, next_ids, snaps[t], steps[t], t, go[t], f"forced EOS step {t}", bound=BC.SCORE_BOUND * (t + 1))
    # done: a further launch, on other logits, leaves every buffer bit-identical
    frozen = [b.clone() for b in st.buffers()] + [next_ids.clone()]
    hk.beam_topk_rows(_strided(lgs[0], V), st, 1.0)
    hk.beam_step(st, next_ids, BC.EOS_TOKEN, False)
    for a, b in zip(frozen, list(st.buffers()) + [next_ids]):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


# ------------------------------------------------------------------------------------------------ kv_beam_reorder
PARENTS = dict(identity=[0, 1, 2, 3], zero=[0, 0, 0, 0], swap=[1, 0, 2, 3], cycle=[1, 2, 0, 3])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("d", (4096, 256))
def test_kv_beam_reorder_is_index_select_in_place(d):
    B, nb, max_ctx, S0, layers = 2, 4, 16, 3, 2
    g = torch.Generator().manual_seed(d)

    def canary():
        return torch.randint(-32768, 32767, (B * nb * max_ctx, d), generator=g, dtype=torch.int16).to(DEV).view(torch.bfloat16)

    for pa, pb in (("identity", "zero"), ("swap", "cycle"), ("cycle", "identity"), ("zero", "swap")):
        parent = torch.tensor(PARENTS[pa] + PARENTS[pb], dtype=torch.int32, device=DEV)
        src = (parent.view(B, nb) + torch.arange(B, device=DEV, dtype=torch.int32)[:, None] * nb).reshape(-1).long()
        for t0, t1, on_device in ((3, 3, True), (3, 4, True), (3, 9, True), (0, 3, False)):
            caches = [(canary(), canary()) for _ in range(layers)]
            other = canary()                                      # a cache that is not in the table
            before = [c.clone() for kv in caches for c in kv] + [other.clone()]
            table = hk.kv_cache_table(caches, DEV)
            t1_arg = torch.tensor([t1], dtype=torch.int32, device=DEV) if on_device else t1
            hk.kv_beam_reorder(table, B, nb, max_ctx, d, parent, t0, t1_arg, max_ctx - S0 if on_device else S0)
            for got, was in zip([c for kv in caches for c in kv], before):
                want = was.view(B * nb, max_ctx, d).clone()
                want[:, t0:t1] = torch.index_select(was.view(B * nb, max_ctx, d), 0, src)[:, t0:t1]
                assert torch.equal(got.view(torch.int16), want.view(-1, d).view(torch.int16)), (d, pa, pb, t0, t1)
            assert torch.equal(other.view(torch.int16), before[-1].view(torch.int16))
    # a swap with nb = 2, and `done` set: nothing moves
    kc, vc = canary()[:2 * 2 * max_ctx].contiguous(), canary()[:2 * 2 * max_ctx].contiguous()
    was = kc.clone()
    table = hk.kv_cache_table([(kc, vc)], DEV)
    parent = torch.tensor([1, 0, 0, 1], dtype=torch.int32, device=DEV)
    hk.kv_beam_reorder(table, 2, 2, max_ctx, d, parent, 3, 9, 13, done=torch.ones(1, dtype=torch.int32, device=DEV))
    assert torch.equal(kc.view(torch.int16), was.view(torch.int16))
    hk.kv_beam_reorder(table, 2, 2, max_ctx, d, parent, 3, 9, 13, done=torch.zeros(1, dtype=torch.int32, device=DEV))
    want = was.view(4, max_ctx, d).clone()
    want[0, 3:9], want[1, 3:9] = was.view(4, max_ctx, d)[1, 3:9], was.view(4, max_ctx, d)[0, 3:9]
    assert torch.equal(kc.view(torch.int16), want.view(-1, d).view(torch.int16))


# ------------------------------------------------------------------------------------------------ generate
NEW = 12
EXCUSED = {"n": 0}


@pytest.fixture(scope="module")
def model():
    return UniBind(("rgb", "text"), None, device=DEV, llama_layers=2).init_random(seed=1).eval()


def _prompt(B):
    ids = torch.tensor([[1, 50, 600, 7000, 80, 9], [0, 0, 1, 7, 8000, 31000]][:B])   # the second row is left-padded
    return ids, (ids.ne(0) if B > 1 else None)


def _gen(model, B, **kw):
    kw.setdefault("do_sample", False)
    kw.setdefault("eos_token_id", None)
    kw.setdefault("max_new_tokens", NEW)
    ids, mask = _prompt(B)
    return model.generate(ids, images=None, attention_mask=mask, **kw)


def _replays(ids, lg, scores, B, nb, length_penalty=1.0, early_stopping=False, eos=None, pen=1.0):
    """beam_cases over the returned logits [B * nb, n, V], step by step.  True: agrees.  False: disagrees at or after a step whose float64 gap is
    below BAND (excused; more than one such case in this module fails)."""
    lg_h = lg.cpu().numpy()
    want, want_sc, n_steps, gaps = BC.ref_beam_search(lambda t, seqs: lg_h[:, t], B, nb, NEW, length_penalty, early_stopping, eos, pen, pad=0)
    ids_h, sc_h = ids.cpu().numpy(), scores.cpu().numpy()
    same = n_steps == lg_h.shape[1] and ids_h.shape == want.shape and (ids_h == want).all() and \
        float(np.abs(sc_h - want_sc).max()) <= BC.SCORE_BOUND * n_steps
    if same:
        return True
    assert min(gaps) < BC.BAND, f"ids {ids_h.tolist()} vs reference {want.tolist()}, scores {sc_h} vs {want_sc}, no gap below BAND ({min(gaps):.3e})"
    EXCUSED["n"] += 1
    print(f"\nBEAM_E2E excused cases so far: {EXCUSED['n']}")
    assert EXCUSED["n"] <= 1
    return False


def test_num_beams_1_is_the_call_without_the_argument(model):
    a, a_lg = _gen(model, 2, return_logits=True)
    b, b_lg = _gen(model, 2, return_logits=True, num_beams=1, length_penalty=2.0, early_stopping=True)
    assert torch.equal(a, b) and torch.equal(a_lg, b_lg)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("B,nb", ((1, 4), (2, 3)))
def test_generate_beam_replays(model, B, nb):
    ids, lg, sc = _gen(model, B, num_beams=nb, return_logits=True, return_beam_scores=True)
    assert ids.shape == (B, NEW) and lg.shape[:2] == (B * nb, NEW) and sc.shape == (B,)
    _replays(ids, lg, sc, B, nb)
    eager = _gen(model, B, num_beams=nb, use_graph=False)
    assert torch.equal(ids, eager)                                                       # graph replay == eager launches
    print(f"\nBEAM_E2E B={B} nb={nb} excused={EXCUSED['n']} same_as_greedy={torch.equal(ids, _gen(model, B))}")


@pytest.mark.timeout(600)
def test_generate_beam_eos_ends_the_hypothesis(model):
    B, nb = 2, 3
    kw = dict(num_beams=nb, length_penalty=0.5, return_logits=True, return_beam_scores=True)   # 0.5: a short hypothesis beats its continuations
    full, _, _ = _gen(model, B, **kw)
    toks = full[0].tolist()
    j = min(i for i in range(2, NEW) if toks[i] not in toks[:i])   # a token of the no-EOS result, at its first occurrence, position >= 2
    eos = int(toks[j])
    ids, lg, sc = _gen(model, B, eos_token_id=eos, **kw)
    if _replays(ids, lg, sc, B, nb, length_penalty=0.5, eos=eos):
        rows = ids.tolist()
        ended = [r for r in rows if eos in r]
        assert ended, rows
        for r in ended:
            assert all(x == 0 for x in r[r.index(eos) + 1:]), r    # pad_token_id of the synthetic tokenizer
        assert eos in rows[0] and rows[0].index(eos) <= j
    stop, _, _ = _gen(model, B, eos_token_id=eos, early_stopping=True, **kw)
    assert stop.shape[1] <= ids.shape[1]
    print(f"\nBEAM_E2E eos excused={EXCUSED['n']}")


@pytest.mark.timeout(600)
def test_generate_beam_with_repetition_penalty_and_fp8(model):
    ids, lg, sc = _gen(model, 1, num_beams=4, repetition_penalty=1.3, return_logits=True, return_beam_scores=True)
    _replays(ids, lg, sc, 1, 4, pen=1.3)
    ids8, lg8, sc8 = _gen(model, 1, num_beams=4, weights="fp8", return_logits=True, return_beam_scores=True)
    assert ids8.shape == (1, NEW)
    _replays(ids8, lg8, sc8, 1, 4)
    print(f"\nBEAM_E2E penalty/fp8 excused={EXCUSED['n']}")


def test_generate_beam_rejections(model):
    from transformers import StoppingCriteriaList

    for kw, name in ((dict(do_sample=True), "do_sample"), (dict(streamer=object()), "streamer"), (dict(stopping_criteria=StoppingCriteriaList()), "stopping_criteria"),
                     (dict(num_return_sequences=2), "num_return_sequences"), (dict(early_stopping="never"), "early_stopping")):
        with pytest.raises(ValueError, match=name):
            _gen(model, 1, num_beams=2, **kw)
    with pytest.raises(ValueError, match="num_beams"):
        _gen(model, 2, num_beams=9)
