"""lhrs_constrain_rows (csrc/constrain.hip) on the GPU against the numpy reference of tests/constrain_cases.py, generate(constraint=...)
on small random-init models, and main_cls.py with `eval.constrained`.  The builders' ValueErrors live in test_constrain_cases_cpu.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import constrain_cases as CC  # noqa: E402
import eval_cases as EC  # noqa: E402
import lhrs_bot_amd.unibind as U  # noqa: E402
from lhrs_bot_amd import generation as G  # noqa: E402
from lhrs_bot_amd import kernels as hk  # noqa: E402

DEV = "cuda"
INTS = ("state", "fin", "len", "choice")


def _strided(logits, ld):
    """fp32 [T, n, V] -> device views [T][n, V] of row stride ld"""
    T, n, V = logits.shape
    buf = torch.zeros(T, n, ld)
    buf[:, :, :V] = torch.from_numpy(np.array(logits))
    return buf.to(DEV)[:, :, :V]


def _to_device(rows):
    st = hk.ConstraintState(len(rows.state), DEV)
    for k in INTS:
        getattr(st, k).copy_(torch.from_numpy(np.asarray(getattr(rows, k)).astype(np.int32)))
    st.score.copy_(torch.from_numpy(np.asarray(rows.score).astype(np.float32)))
    return st


def _to_host(out, st):
    return CC.Rows(out.cpu().numpy(), *(getattr(st, k).cpu().numpy().astype(np.int64) for k in INTS), st.score.cpu().numpy())


def _walk(a_dev, a_host, x_dev, x_host, rows, what, score=True, also=None):
    """T launches from `rows`; every step is compared with the reference's step from the KERNEL's state before it.  -> worst score error"""
    st, worst = _to_device(rows), 0.0
    before = _to_host(torch.zeros(len(rows.state), dtype=torch.int64), st)
    for t in range(x_dev.shape[0]):
        out = torch.full((len(rows.state),), -7, device=DEV, dtype=torch.int64)
        hk.constrain_rows(x_dev[t], a_dev, st, out, score=score)
        got = _to_host(out, st)
        worst = max(worst, CC.compare(got, CC.ref_step(a_host, x_host[t], before, want_score=score), f"{what} step {t}").score_err)
        if also is not None:
            also(t, out)
        before = got
    return worst


@pytest.mark.timeout(600)
@pytest.mark.parametrize("scale", CC.SCALES)
@pytest.mark.parametrize("V", CC.VOCABS)
def test_kernel_against_reference(V, scale):
    worst = 0.0
    autos = CC.automata(V, DEV)
    hosts = {k: CC.host(a) for k, a in autos.items()}
    p_args, p_x, p_rows, p_out = CC.planted(V, scale)
    p_auto = G.TokenAutomaton.from_edges(*p_args, CC.PAD, V, DEV)
    # the NaN case runs at V = 1000 whatever V is: 36 KB, so that no freed block of a megabyte or more is left holding a NaN pattern for a later
    # test's torch.empty() to find
    n_args, n_x, n_rows, n_out = CC.planted(1000, scale, nan=True)
    n_auto = G.TokenAutomaton.from_edges(*n_args, CC.PAD, 1000, DEV)
    for ld in (V, V + 5):
        for n in CC.ROWS:
            x = CC.make_logits(6, n, V, scale, 100 + n)
            xd = _strided(x, ld)
            what = f"V={V} ld={ld} n={n}"
            for k, start in enumerate(CC.sweep_starts(n)):
                for score in (True, False):
                    worst = max(worst, _walk(autos["sweep"], hosts["sweep"], xd[:3], x, CC.start_rows(n, start), f"{what} sweep start {k} score={score}", score))

            def is_argmax(t, out):   # the vocab loop: every token is allowed, the pick is the plain greedy one
                assert torch.equal(out, hk.argmax_rows(xd[t])), f"{what} loop step {t}"
            for score in (True, False):
                worst = max(worst, _walk(autos["trie"], hosts["trie"], xd, x, CC.start_rows(n), f"{what} trie score={score}", score))
                worst = max(worst, _walk(autos["loop"], hosts["loop"], xd[:2], x, CC.start_rows(n), f"{what} loop score={score}", score, is_argmax))
                worst = max(worst, _walk(autos["loop_eos"], hosts["loop_eos"], xd[:2], x, CC.start_rows(n), f"{what} loop_eos score={score}", score))
        # planted: ties, a disallowed maximum, an allowed set of -inf, rows that start final or out of range (they write `out` only)
        pd = _strided(p_x[None], ld)
        for score in (True, False):
            st = _to_device(p_rows)
            out = hk.constrain_rows(pd[0], p_auto, st, score=score)
            got = _to_host(out, st)
            worst = max(worst, CC.compare(got, CC.ref_step(CC.host(p_auto), p_x, p_rows, want_score=score), f"V={V} ld={ld} planted score={score}").score_err)
            assert (got.out == p_out).all()
            for k in INTS + ("score",):
                assert (getattr(got, k)[5:] == np.asarray(getattr(p_rows, k))[5:]).all(), k
        st, nd = _to_device(n_rows), _strided(n_x[None], 1000 + ld - V)   # a NaN on the best allowed token compares as -inf (picks only)
        assert (hk.constrain_rows(nd[0], n_auto, st).cpu().numpy() == n_out).all()
        nd.zero_()
    print(f"\nCONSTRAIN_WORST V={V} scale={scale} score_err={worst:.3e}")


def test_wrapper_rejects_bad_arguments():
    a = CC.automata(1000, DEV)["trie"]
    x = torch.zeros(2, 1000, device=DEV)
    with pytest.raises(TypeError):
        hk.constrain_rows(x.double(), a, hk.ConstraintState(2, DEV))
    with pytest.raises(TypeError):
        hk.constrain_rows(x, a, hk.ConstraintState(2, DEV), torch.zeros(2, device=DEV, dtype=torch.int32))
    with pytest.raises(AssertionError):
        hk.constrain_rows(x, a, hk.ConstraintState(3, DEV))
    with pytest.raises(AssertionError):
        hk.constrain_rows(torch.zeros(2, 999, device=DEV), a, hk.ConstraintState(2, DEV))
    st = hk.ConstraintState(2, DEV)
    assert st.choice.tolist() == [-1, -1] and not any(int(getattr(st, k).abs().sum()) for k in ("state", "fin", "len")) and st.score.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ generate
NEW = 12
CHOICES = [list(c) for c in ([500], [700, 800], [700, 900], [700, 800, 1000], [1100, 1200, 1300, 1400], [1100, 1200, 1500], [2000, 2100, 2200])]
GEN_WORST = {"score_err": 0.0}


@pytest.fixture(scope="module")
def model():
    return U.UniBind(("rgb", "text"), None, device=DEV, llama_layers=2).init_random(seed=1).eval()


@pytest.fixture(scope="module")
def trie(model):
    return model.choice_constraint(CHOICES)


def _prompt(B):
    base = torch.tensor([[1, 50, 600, 7000, 80, 9], [1, 7, 8000, 31000, 12, 4]])
    rows = base[torch.arange(B) % 2].clone()
    rows[:, 2] += 17 * (torch.arange(B) // 2)                      # B = 17: no two rows alike
    return rows


def _gen(model, B, **kw):
    kw.setdefault("do_sample", False)
    kw.setdefault("eos_token_id", None)
    kw.setdefault("max_new_tokens", NEW)
    return model.generate(_prompt(B), images=None, **kw)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("B", (1, 2, 17))
def test_generate_emits_exactly_one_choice(model, trie, B):
    eos, pad = model.text.tokenizer.eos_token_id, model.text.tokenizer.pad_token_id
    ids, lg, choice, score = _gen(model, B, constraint=trie, return_logits=True, return_choices=True)
    assert choice.dtype == torch.int64 and score.dtype == torch.float32 and choice.shape == score.shape == (B,)
    ids_h, choice_h = ids.cpu().tolist(), choice.cpu().tolist()
    longest = 0
    for b in range(B):
        assert 0 <= choice_h[b] < len(CHOICES)
        want = CHOICES[choice_h[b]] + [eos]
        assert ids_h[b] == want + [pad] * (len(ids_h[b]) - len(want)), (b, ids_h[b], want)
        longest = max(longest, len(want))
    assert ids.shape == (B, longest) and longest < NEW and lg.shape[:2] == (B, longest)
    # graph replay == eager launches, bit for bit
    e_ids, e_lg, e_choice, e_score = _gen(model, B, constraint=trie, return_logits=True, return_choices=True, use_graph=False)
    assert torch.equal(ids, e_ids) and torch.equal(lg, e_lg) and torch.equal(choice, e_choice) and torch.equal(score, e_score)
    # the ids are the reference's walk over the returned logits
    steps = CC.ref_walk(CC.host(trie), lg.cpu().numpy().transpose(1, 0, 2))
    assert (np.stack([s.out for s in steps], 1) == ids.cpu().numpy()).all() and (steps[-1].choice == choice.cpu().numpy()).all()
    err = np.abs(score.cpu().numpy().astype(np.float64) - steps[-1].score)
    GEN_WORST["score_err"] = max(GEN_WORST["score_err"], float((err / steps[-1].len).max()))
    print(f"\nCONSTRAIN_GENERATE B={B} score_err_per_step={float((err / steps[-1].len).max()):.3e}")
    assert (err <= CC.SCORE_BOUND * steps[-1].len).all(), err
    # without the scores: the same ids; on the per-token host path (an EOS for the host to look at): the same ids
    assert torch.equal(_gen(model, B, constraint=trie), ids)
    assert torch.equal(_gen(model, B, constraint=trie, eos_token_id=eos), ids)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("B", (1, 2, 17))
def test_generate_vocab_loop_is_plain_greedy(model, B):
    loop = G.vocab_loop_automaton(model.text.vocab, None, 0, model.text.device)
    greedy, g_lg = _gen(model, B, return_logits=True)
    ids, lg, choice, _ = _gen(model, B, constraint=loop, return_logits=True, return_choices=True)
    assert ids.shape == (B, NEW) and torch.equal(ids, greedy) and torch.equal(lg, g_lg)
    assert choice.tolist() == [-1] * B                              # max_new_tokens ran out: no final state was reached


@pytest.mark.timeout(600)
def test_generate_max_new_tokens_inside_a_choice(model, trie):
    ids, choice, _ = _gen(model, 2, constraint=trie, return_choices=True, max_new_tokens=1)
    assert ids.shape == (2, 1) and all(t in (500, 700, 1100, 2000) for t in ids[:, 0].tolist()) and choice.tolist() == [-1, -1]


@pytest.mark.timeout(600)
def test_generate_constrained_fp8_weights_and_cache(model, trie):
    eos = model.text.tokenizer.eos_token_id
    ids, lg, choice, score = _gen(model, 1, constraint=trie, return_logits=True, return_choices=True, weights="fp8", kv_cache="fp8")
    want = CHOICES[int(choice[0])] + [eos]
    assert ids[0].tolist() == want
    steps = CC.ref_walk(CC.host(trie), lg.cpu().numpy().transpose(1, 0, 2))
    assert [int(s.out[0]) for s in steps] == want and abs(float(score[0]) - steps[-1].score[0]) <= CC.SCORE_BOUND * len(want)


@pytest.mark.timeout(600)
def test_generate_rejections_leave_the_allocator_untouched(model, trie):
    _gen(model, 1, constraint=trie)                                 # everything lazy (packed weights, kernel attributes) exists from here on
    torch.cuda.synchronize()
    cpu_loop, small = G.vocab_loop_automaton(model.text.vocab), G.vocab_loop_automaton(1000, None, 0, model.text.device)
    pc = model.new_prefix_cache()
    before = torch.cuda.memory_allocated()
    for kw in (dict(constraint=trie, do_sample=True), dict(constraint=trie, num_beams=2), dict(constraint=trie, repetition_penalty=1.2),
               dict(constraint=trie, prefix_cache=pc), dict(constraint=small), dict(constraint=cpu_loop), dict(return_choices=True),
               dict(constraint=lambda b, s: [1])):
        with pytest.raises(ValueError):
            _gen(model, 1, **kw)
        assert torch.cuda.memory_allocated() == before, kw
    assert pc.caches is None and pc.length == 0


# ------------------------------------------------------------------------------------------------ main_cls.py
class Tok(EC.ToyTok):
    """the fixture's whitespace tokenizer, which here honours add_special_tokens=False, + a decoder of the words it has seen"""

    def __init__(self):
        self.words = {}

    def __call__(self, text, add_special_tokens=True):
        enc = super().__call__(text)
        self.words.update(zip(enc.input_ids[1:], (w for w in text.replace("\n", " \n ").split(" ") if w)))
        if not add_special_tokens:
            enc.input_ids = enc.input_ids[1:]
        return enc

    def decode(self, ids, skip_special_tokens=False):
        ids = [int(i) for i in (ids.tolist() if hasattr(ids, "tolist") else ids)]
        return " ".join(self.words.get(i, f"t{i}") for i in ids if not (skip_special_tokens and i in (0, 1, 2)))

    def batch_decode(self, ids, skip_special_tokens=True):
        return [self.decode(r, skip_special_tokens) for r in ids]


@pytest.mark.timeout(600)
def test_main_cls_constrained(tmp_path, monkeypatch):
    import main_cls
    import transformers
    from lhrs_bot_amd import conversation as conv_lib
    from lhrs_bot_amd import evaluation as EV
    monkeypatch.setattr(conv_lib, "default_conversation", conv_lib.default_conversation)   # put back whatever main() leaves there
    tok = Tok()
    monkeypatch.setattr(transformers.AutoTokenizer, "from_pretrained", staticmethod(lambda *a, **k: tok))
    orig, calls = U.UniBind.generate, []

    def spy(self, input_ids=None, **kw):
        out = orig(self, input_ids=input_ids, **kw)
        calls.append((kw, out))
        return out
    monkeypatch.setattr(U.UniBind, "generate", spy)
    kw = EC.build_case(str(tmp_path / "ucm"), "ucm")
    names = json.load(open(os.path.join(HERE, "golden", "eval.json")))["cls"]["prompts"]["ucm"]["all_classes"]
    args = ["--batch-size", "4", "--data-path", kw["root"], "--llama-layers", "2", "--workers", "0", "--output", str(tmp_path / "o"), "--tokenizer-path", "toy",
            "--opts", "eval.dataset", "UCM"]
    os.makedirs(tmp_path / "o", exist_ok=True)

    res = main_cls.main(main_cls.parse_option(args + ["eval.constrained", "True"]))
    assert [c[1][0].shape[0] for c in calls] == [4, 2] and all(c[0]["return_choices"] and c[0]["max_new_tokens"] == 20 for c in calls)
    choices = [int(v) for c in calls for v in c[1][1].tolist()]
    assert res["classes"] == names and all(p in names for p in res["preds"])          # every prediction is exactly a class name
    assert res["pred_idx"] == choices == [names.index(p) for p in res["preds"]]       # ... and the index is the automaton's choice
    assert all(c[1][0].shape[1] == 2 for c in calls)                                  # one token per UCM class + EOS, not 20 steps
    assert res["trues"] == [c for _, c in EC.UCM_FILES]

    calls.clear()
    res = main_cls.main(main_cls.parse_option(args))                                  # without the key: the call of before, untouched
    assert [set(c[0]) for c in calls] == [{"images", "do_sample", "num_beams", "temperature", "top_p", "max_new_tokens", "weights"}] * 2
    assert all(torch.is_tensor(c[1]) and c[1].shape[1] <= 20 for c in calls)
    assert res["preds"] == [p for c in calls for p in tok.batch_decode(c[1], skip_special_tokens=True)]
    assert res["pred_idx"] == EV.classname_2_idx(res["preds"], {n: i for i, n in enumerate(names)})
