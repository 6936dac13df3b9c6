"""CPU-only checks of the constrained-decoding test helpers (tests/constrain_cases.py) and of the host side of generate(constraint=...):
the numpy reference against HF's own PrefixConstrainedLogitsProcessor, the automaton builders and every ValueError of theirs, the header
and the C entry's rejections, and the comparator against mutants of the reference."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constrain_cases as CC  # noqa: E402
from lhrs_bot_amd import _lib  # noqa: E402
from lhrs_bot_amd import generation as G  # noqa: E402


# ------------------------------------------------------------------------------------------------ the reference against HF
def _hf_walk(a, logits):
    """log_softmax (float64, of the same fp32 logits) -> PrefixConstrainedLogitsProcessor(num_beams=1) -> torch.argmax, the allowed tokens
    found by walking the automaton along the history HF hands over.  A finished row allows the pad token alone (HF's generate pads it);
    its score stops at the EOS, as the reference's does."""
    from transformers.generation.logits_process import PrefixConstrainedLogitsProcessor
    T, n, _ = logits.shape

    def state_of(sent):
        s = 0
        for t in sent.tolist():
            e0, e1 = int(a.off[s]), int(a.off[s + 1])
            if e1 == e0:
                return s
            s = int(a.nxt[e0 + a.tok[e0:e1].tolist().index(t)])
        return s

    def allowed(batch_id, sent):
        s = state_of(sent)
        e0, e1 = int(a.off[s]), int(a.off[s + 1])
        return a.tok[e0:e1].tolist() if e1 > e0 else [a.pad]

    proc = PrefixConstrainedLogitsProcessor(allowed, num_beams=1)
    ids, score = torch.zeros((n, 0), dtype=torch.int64), torch.zeros(n, dtype=torch.float64)
    scores_at = []
    for t in range(T):
        lp = torch.log_softmax(torch.from_numpy(np.array(logits[t])).double(), -1)
        live = torch.tensor([a.off[state_of(row) + 1] > a.off[state_of(row)] for row in ids])
        masked = proc(ids, lp)
        nxt = torch.argmax(masked, -1)
        score = score + torch.where(live, masked.gather(1, nxt[:, None])[:, 0], torch.zeros(n, dtype=torch.float64))
        ids = torch.cat([ids, nxt[:, None]], 1)
        scores_at.append(score.clone())
    return ids.numpy(), torch.stack(scores_at).numpy()


@pytest.mark.parametrize("scale", CC.SCALES)
@pytest.mark.parametrize("V", CC.VOCABS)
def test_reference_is_hf_prefix_constrained_argmax(V, scale):
    a = CC.host(CC.automata(V)["trie"])
    for n in CC.ROWS:
        logits = CC.make_logits(CC.WALK_STEPS, n, V, scale, 100 + n)
        steps = CC.ref_walk(a, logits, fp32_score=False)
        ids, scores = _hf_walk(a, logits)
        for t, rows in enumerate(steps):
            assert (rows.out == ids[:, t]).all(), (V, scale, n, t)
            assert np.abs(rows.score - scores[t]).max() <= 1e-12 * max(1.0, np.abs(scores[t]).max()), (V, scale, n, t)   # fp64 rounding
        last = steps[-1]
        assert last.fin.all() and (last.len <= 5).all()            # 12 steps end every choice (at most 4 tokens + EOS)
        for r in range(n):                                          # ... and the emitted tokens are choice + EOS, pads behind
            c = list(CC.TRIE_CHOICES[int(last.choice[r])]) + [CC.EOS]
            assert ids[r].tolist() == c + [CC.PAD] * (CC.WALK_STEPS - len(c))


def test_reference_planted_cases():
    for V in CC.VOCABS:
        args, x, rows, want_out = CC.planted(V)
        a = CC.host(G.TokenAutomaton.from_edges(*args, CC.PAD, V))
        got = CC.ref_step(a, x, rows)
        assert (got.out == want_out).all()
        assert got.state[:5].tolist() == [2, 2, 2, 1, 2] and got.fin[:5].all() and got.choice[:5].tolist() == [1, 1, 1, 0, 1]
        assert got.score[3] == -np.inf and np.isfinite(got.score[[0, 1, 2, 4]]).all()
        for k in ("state", "fin", "len", "choice", "score"):       # final and out-of-range rows: nothing but `out`
            assert (getattr(got, k)[5:] == getattr(rows, k)[5:]).all(), k
        args, x, rows, want_out = CC.planted(V, nan=True)
        assert (CC.ref_step(a, x, rows, want_score=False).out == want_out).all()


# ------------------------------------------------------------------------------------------------ the builders
def test_choice_automaton_shape_and_labels():
    a = CC.host(G.choice_automaton(CC.TRIE_CHOICES, CC.EOS, CC.PAD, 1000))
    n_nodes = 1 + len({tuple(c[:i]) for c in CC.TRIE_CHOICES for i in range(1, len(c) + 1)})
    assert a.label.size == n_nodes + len(CC.TRIE_CHOICES) and a.tok.size == a.label.size - 1    # a tree: one edge into every state but the start
    assert a.tok[a.off[0]:a.off[1]].tolist() == [5, 7, 11, 20] and a.pad == CC.PAD and a.V == 1000
    for s in range(a.label.size):
        t = a.tok[a.off[s]:a.off[s + 1]]
        assert (np.diff(t) > 0).all()                                # sorted, unique
        assert (a.label[s] >= 0) == (t.size == 0)                    # exactly the final states carry a label
    for i, c in enumerate(CC.TRIE_CHOICES):                          # walking choice i + EOS ends in the final state labelled i
        s = 0
        for t in list(c) + [CC.EOS]:
            e = a.off[s] + a.tok[a.off[s]:a.off[s + 1]].tolist().index(t)
            s = int(a.nxt[e])
        assert a.label[s] == i and a.off[s + 1] == a.off[s]
    # [7, 8] is a strict prefix of [7, 8, 10]: behind 7, 8 both EOS and 10 are allowed
    s = int(a.nxt[a.off[0] + 1])
    s = int(a.nxt[a.off[s] + a.tok[a.off[s]:a.off[s + 1]].tolist().index(8)])
    assert a.tok[a.off[s]:a.off[s + 1]].tolist() == [CC.EOS, 10]


def test_vocab_loop_automaton():
    a = CC.host(G.vocab_loop_automaton(1000))
    assert a.off.tolist() == [0, 1000] and a.tok.tolist() == list(range(1000)) and not a.nxt.any() and a.label.tolist() == [-1]
    b = CC.host(G.vocab_loop_automaton(1000, CC.EOS))
    assert b.off.tolist() == [0, 1000, 1000] and b.nxt[CC.EOS] == 1 and b.nxt.sum() == 1 and b.label.tolist() == [-1, 0]
    with pytest.raises(ValueError, match="outside"):
        G.vocab_loop_automaton(1000, 1000)


def test_builders_reject_what_the_kernel_relies_on():
    ok = dict(off=[0, 2, 2], tok=[3, 4], nxt=[0, 1], label=[-1, 0], pad_token_id=0, V=10)
    G.TokenAutomaton.from_edges(**ok)                                # cycles are allowed
    for change, text in ((dict(off=[1, 2, 2]), "offsets"), (dict(off=[0, 2, 1]), "offsets"), (dict(off=[0, 2, 3]), "offsets"),
                         (dict(off=[0, 1, 0, 2], label=[-1, 0, 1]), "offsets"), (dict(off=[0, 2]), "offsets"),
                         (dict(tok=[3, 10]), "tokens"), (dict(tok=[-1, 4]), "tokens"), (dict(nxt=[0, 2]), "targets"), (dict(nxt=[-1, 0]), "targets"),
                         (dict(tok=[4, 3]), "ascending"), (dict(tok=[3, 3]), "ascending"), (dict(off=[0, 0, 2]), "state 0"),
                         (dict(V=40000), "32768"), (dict(tok=[3.5, 4.0]), "integer"), (dict(nxt=[0]), "target per edge")):
        with pytest.raises(ValueError, match=text):
            G.TokenAutomaton.from_edges(**dict(ok, **change))
    # the order rule is per state: a state may start below the last token of the state before it
    G.TokenAutomaton.from_edges([0, 2, 3, 3], [3, 4, 1], [1, 2, 2], [-1, -1, 0], 0, 10)
    for lists, text in (([[1], [1]], "same token sequence"), ([[1], []], "empty"), ([], "no choices"), ([[1, CC.EOS]], "EOS"), ([[1, 10]], "tokens")):
        with pytest.raises(ValueError, match=text):
            G.choice_automaton(lists, CC.EOS, CC.PAD, 10)


def test_check_constraint_rejections():
    class M:
        vocab, device = 1000, "cpu"
    a = G.vocab_loop_automaton(1000)
    G.check_constraint(M, a, True)
    G.check_constraint(M, None)
    for kw, text in ((dict(do_sample=True), "do_sample"), (dict(num_beams=2), "num_beams"), (dict(repetition_penalty=1.1), "repetition_penalty"),
                     (dict(prefix_cache=object()), "prefix_cache")):
        with pytest.raises(ValueError, match=text):
            G.check_constraint(M, a, **kw)
    with pytest.raises(ValueError, match="vocabulary"):
        G.check_constraint(M, G.vocab_loop_automaton(999))
    with pytest.raises(ValueError, match="return_choices"):
        G.check_constraint(M, None, True)
    with pytest.raises(ValueError, match="TokenAutomaton"):
        G.check_constraint(M, lambda b, s: [1])


# ------------------------------------------------------------------------------------------------ the C entry
def test_header_declares_and_library_exports_constrain_rows():
    restype, args = _lib.parse_header()["lhrs_constrain_rows"]
    assert restype is ctypes.c_int and len(args) == 18 and args[-2] is ctypes.c_void_p and args[1] is ctypes.c_long


def test_c_entry_rejects_before_launching():
    lib = _lib.load()
    one = ctypes.c_void_p(16)   # a non-null pointer that is never dereferenced: every call below is rejected on the host

    def call(n=1, V=1000, out=one, state=one, fin=one, ln=one, choice=one):
        return lib.lhrs_constrain_rows(one, V, out, n, V, one, one, one, one, 1, 1, 0, state, fin, ln, choice, None, None)
    for kw in (dict(V=32769), dict(n=0), dict(out=None), dict(state=None), dict(fin=None), dict(ln=None), dict(choice=None)):
        assert call(**kw) == -1, kw
        assert b"constrain_rows" in lib.lhrs_last_error()


# ------------------------------------------------------------------------------------------------ the comparator against mutants
def _trie_case():
    a = CC.host(CC.automata(1000)["trie"])
    logits = CC.make_logits(CC.WALK_STEPS, 16, 1000, 8, 116)
    return a, logits, CC.ref_walk(a, logits)


def _second_best(a, logits, rows):
    """ref_step with the second-best edge wherever a state has two"""
    x = np.array(logits)
    for r, s in enumerate(rows.state):
        e0, e1 = int(a.off[s]), int(a.off[s + 1])
        if e1 - e0 >= 2:
            x[r, a.tok[e0 + int(np.argmax(x[r, a.tok[e0:e1]]))]] = -np.inf
    return CC.ref_step(a, x, rows)


def test_comparator_accepts_the_reference_and_fp32_noise():
    a, logits, steps = _trie_case()
    for t, rows in enumerate(steps):
        assert CC.compare(rows, rows).score_err == 0.0
        noisy = rows._replace(score=rows.score.astype(np.float32))   # the rounding of the result alone: half an ulp of 64 at most
        assert CC.compare(noisy, rows).score_err <= 4e-6


def test_comparator_rejects_mutants():
    a, logits, steps = _trie_case()
    before = [CC.start_rows(16)] + [s._replace(score=s.score.astype(np.float32).astype(np.float64)) for s in steps[:-1]]
    rejected = {}

    def must_fail(name, got, want):
        with pytest.raises(AssertionError):
            CC.compare(got, want, name)
        rejected[name] = rejected.get(name, 0) + 1

    for t, (b, want) in enumerate(zip(before, steps)):
        live = want.len > b.len
        if not live.any():
            continue
        must_fail("second-best edge", _second_best(a, logits[t], b), want) if any(a.off[s + 1] - a.off[s] >= 2 for s in b.state) else None
        delta = want.score - b.score
        m = logits[t].astype(np.float64).max(-1)
        must_fail("score: the max is not added back", want._replace(score=np.where(live, want.score + m, want.score)), want)
        allowed_lse = np.array([CC.lse64(logits[t][r, a.tok[a.off[s]:a.off[s + 1]]]) if lv else 0.0 for r, (s, lv) in enumerate(zip(b.state, live))])
        full_lse = np.array([CC.lse64(logits[t][r]) for r in range(16)])
        must_fail("score: normalised over the allowed set", want._replace(score=np.where(live, want.score + full_lse - allowed_lse, want.score)), want)
        must_fail("score: not accumulated", want._replace(score=np.where(live, delta, want.score)), want) if t else None
        must_fail("state not advanced", want._replace(state=b.state), want)
        must_fail("len not set", want._replace(len=b.len), want)
        if (want.fin != b.fin).any():
            must_fail("fin not set", want._replace(fin=b.fin), want)
            must_fail("choice not set", want._replace(choice=b.choice), want)
        if not live.all():                                           # a final row that changes
            must_fail("final row: len", want._replace(len=want.len + ~live), want)
            must_fail("final row: state", want._replace(state=np.where(live, want.state, 0)), want)
            must_fail("final row: token", want._replace(out=np.where(live, want.out, CC.EOS)), want)
            must_fail("final row: score", want._replace(score=np.where(live, want.score, want.score - 0.5)), want)
    assert set(rejected) == {"second-best edge", "score: the max is not added back", "score: normalised over the allowed set", "score: not accumulated",
                             "state not advanced", "len not set", "fin not set", "choice not set", "final row: len", "final row: state",
                             "final row: token", "final row: score"}
    # the tie rule, on the planted ties: the higher of the equal tokens is a different token and another final state
    args, x, rows, _ = CC.planted(1000)
    h = CC.host(G.TokenAutomaton.from_edges(*args, CC.PAD, 1000))
    want = CC.ref_step(h, x, rows)
    hi = want._replace(out=want.out.copy(), state=want.state.copy(), choice=want.choice.copy())
    hi.out[0], hi.state[0], hi.choice[0] = 30, 3, 2
    with pytest.raises(AssertionError):
        CC.compare(hi, want, "tie to the higher token")
    # the smallest score error a mutant makes here is far above the bound
    assert CC.SCORE_BOUND <= 1e-4
