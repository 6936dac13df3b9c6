"""Constrained-decoding cases shared by tests/test_constrain_gpu.py and tests/test_constrain_cases_cpu.py: a numpy reference of what
lhrs_constrain_rows (csrc/constrain.hip) computes - the first maximum among the out-edges of the row's state, the walk along it, and the
picked token's log-probability with a float64 log-sum-exp over the same fp32 logits -, the automata and planted cases of the grid, and a
comparator that returns what it measured.

Bounds.  out, state, fin, len and choice are integers and must be EXACT; no case is excused.  The score is compared per step: the kernel's
fp32 `score + logit - lse` against the float64 value of the same expression from the same incoming fp32 score.  Worst absolute difference
per step measured on an MI355X over all V, ld, n, automata and planted cases of test_constrain_gpu.py, randn scale 1 | scale 8:
    V = 32000    2.8e-6 | 9.8e-6        V = 32003    2.6e-6 | 9.4e-6        V = 1000    1.8e-6 | 5.0e-6
    generate() replays (B = 1, 2, 17; the final score over its steps)    5.1e-7, 5.9e-7, 1.2e-6 per step
    worst 9.8e-6   ->   SCORE_BOUND 4e-5   (~4x; whatever is measured, the bound may not exceed 1e-4 per step)
It is made of: the fp32 sum of V terms exp(x - max), each 1-2 ulp and largely cancelling (relative 1e-7 of the sum, the same absolute in its
log); the rounding of lse = max + log(sum) near 10 (scale 1) or 40 (scale 8): half an ulp is 4.8e-7 or 1.9e-6; and the roundings of
score + (logit - lse) at the size of the running score, which reaches 128-256 in the three-step walks at scale 8 (half an ulp: 7.6e-6) and
stays below 64 at scale 1 (1.9e-6).  The mutants of test_constrain_cases_cpu.py move the score by 0.1 and more."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

SCORE_BOUND = 4e-5
assert SCORE_BOUND <= 1e-4

VOCABS = (32000, 32003, 1000)
ROWS = (1, 3, 16)
SCALES = (1, 8)
EDGE_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, "V")   # out-edges of states 0..8 of the sweep automaton
EOS, PAD = 2, 0
# seven choices of lengths 1-4 with shared prefixes; [7, 8] is a strict prefix of [7, 8, 10]
TRIE_CHOICES = ([5], [7, 8], [7, 9], [7, 8, 10], [11, 12, 13, 14], [11, 12, 15], [20, 21, 22])
WALK_STEPS = 12

Host = namedtuple("Host", "off tok nxt label pad V")            # an automaton as numpy int64 arrays
Rows = namedtuple("Rows", "out state fin len choice score")     # per-row results of one step; score float64 (reference) or float32 (kernel)
Measured = namedtuple("Measured", "score_err")

# worst score error seen by compare() in this process (how SCORE_BOUND was measured)
WORST = {"score_err": 0.0}


def host(a):
    """a generation.TokenAutomaton (any device) -> Host"""
    return Host(*(getattr(a, k).cpu().numpy().astype(np.int64) for k in ("off", "tok", "nxt", "label")), int(a.pad_token_id), int(a.V))


# ------------------------------------------------------------------------------------------------ the reference
def lse64(row):
    x = row.astype(np.float64)
    m = x.max()
    return m + np.log(np.exp(x - m).sum())


def ref_step(a, logits, rows, want_score=True):
    """One launch: a Host, logits fp32 [n, V], rows = Rows before it (out is ignored) -> Rows after it, score in float64"""
    n = logits.shape[0]
    out = np.empty(n, dtype=np.int64)
    state, fin, ln, choice = (np.array(v, dtype=np.int64) for v in (rows.state, rows.fin, rows.len, rows.choice))
    score = np.array(rows.score, dtype=np.float64)
    n_states = a.label.size
    for r in range(n):
        s = int(state[r])
        if not 0 <= s < n_states or a.off[s + 1] == a.off[s]:
            out[r] = a.pad
            continue
        e0, e1 = int(a.off[s]), int(a.off[s + 1])
        vals = logits[r, a.tok[e0:e1]].astype(np.float64)
        vals[np.isnan(vals)] = -np.inf
        e = e0 + int(np.argmax(vals))          # first maximum = lowest token: the edges of a state ascend
        out[r], ln[r], state[r] = a.tok[e], ln[r] + 1, a.nxt[e]
        ns = int(a.nxt[e])
        if a.off[ns + 1] == a.off[ns]:
            fin[r], choice[r] = 1, a.label[ns]
        if want_score:
            with np.errstate(invalid="ignore"):
                score[r] += vals[e - e0] - lse64(logits[r])
    return Rows(out, state, fin, ln, choice, score)


def start_rows(n, state=None):
    return Rows(np.zeros(n, np.int64), np.zeros(n, np.int64) if state is None else np.asarray(state, dtype=np.int64), np.zeros(n, np.int64),
                np.zeros(n, np.int64), np.full(n, -1, np.int64), np.zeros(n, np.float64))


def ref_walk(a, logits, rows=None, want_score=True, fp32_score=True):
    """logits fp32 [T, n, V] -> the Rows after every step.  fp32_score: the incoming score of a step is the reference's own result rounded to
    fp32, as the device holds it."""
    rows = start_rows(logits.shape[1]) if rows is None else rows
    steps = []
    for t in range(logits.shape[0]):
        rows = ref_step(a, logits[t], rows, want_score)
        steps.append(rows)
        if fp32_score:
            rows = rows._replace(score=rows.score.astype(np.float32).astype(np.float64))
    return steps


# ------------------------------------------------------------------------------------------------ the comparator
def measure(got, want):
    g, w = np.asarray(got.score, dtype=np.float64), np.asarray(want.score, dtype=np.float64)
    same_inf = np.isinf(g) & np.isinf(w) & (np.sign(g) == np.sign(w))
    with np.errstate(invalid="ignore"):
        err = np.where(same_inf, 0.0, np.abs(g - w))
    err = np.where(np.isnan(err), np.inf, err)       # NaN, or an infinity on one side only
    return Measured(float(err.max()) if err.size else 0.0)


def compare(got, want, what="", bound=None):
    """Rows of the code under test against the reference's for the same step: the integers exact, the score within SCORE_BOUND"""
    for k in ("out", "state", "fin", "len", "choice"):
        g, w = np.asarray(getattr(got, k), dtype=np.int64), np.asarray(getattr(want, k), dtype=np.int64)
        assert g.shape == w.shape and (g == w).all(), f"{what}: {k} {g.tolist()} != {w.tolist()}"
    m = measure(got, want)
    WORST["score_err"] = max(WORST["score_err"], m.score_err)
    assert m.score_err <= (SCORE_BOUND if bound is None else bound), f"{what}: score off by {m.score_err:.3e}"
    return m


# ------------------------------------------------------------------------------------------------ the cases
@lru_cache(maxsize=None)
def make_logits(T, n, V, scale, seed):
    """finite fp32 logits [T, n, V]; shared between the tests, never written"""
    x = (np.random.default_rng(seed).standard_normal((T, n, V)) * scale).astype(np.float32)
    x.setflags(write=False)
    return x


def sweep_arrays(V, seed=0):
    """states 0..8 with EDGE_COUNTS out-edges each (random ascending tokens, random targets among all 11 states), states 9 and 10 final"""
    rng = np.random.default_rng(seed)
    off, tok, nxt = [0], [], []
    for c in EDGE_COUNTS:
        c = V if c == "V" else c
        tok += np.sort(rng.choice(V, size=c, replace=False)).tolist()
        nxt += rng.integers(0, 11, size=c).tolist()
        off.append(len(tok))
    return off + [len(tok), len(tok)], tok, nxt, [-1] * 9 + [3, 7]


def automata(V, device="cpu"):
    """-> {name: TokenAutomaton} of the grid"""
    from lhrs_bot_amd import generation as G
    return {"sweep": G.TokenAutomaton.from_edges(*sweep_arrays(V), PAD, V, device),
            "trie": G.choice_automaton(TRIE_CHOICES, EOS, PAD, V, device),
            "loop": G.vocab_loop_automaton(V, None, PAD, device),
            "loop_eos": G.vocab_loop_automaton(V, EOS, PAD, device)}


def sweep_starts(n):
    """start states for n rows so that every state of the sweep automaton (the finals included) starts some row: a list of [n] arrays"""
    return [np.array([(k + r) % 11 for r in range(n)]) for k in range(0, 11, n)]


PLANTED_EDGES = (10, 20, 30, 40)
PLANTED_ROWS = 9


def planted(V, scale=1, seed=5, nan=False):
    """-> (from_edges arguments, logits fp32 [9, V], Rows before the step, expected out [9]).  State 0 allows PLANTED_EDGES, each leading to a
    final state of its own.  Rows: 0 an exact tie of two allowed tokens, 1 of three, 2 disallowed tokens (0, 11, V - 1) hold the row's largest
    logits, 3 every allowed logit is -inf, 4 nothing planted - or with `nan` (picks only: the score of such a row is NaN) a NaN on the
    otherwise best allowed token -, 5 starts final, 6-8 states out of range.  The rows that must not change start from len / choice / score
    that a write would disturb."""
    x = np.array(make_logits(1, PLANTED_ROWS, V, scale, seed)[0])
    top = float(np.abs(x).max())
    x[:, list(PLANTED_EDGES)] = [-0.5, 0.25, 0.125, -1.0]
    x[0, [20, 30]] = 1.5
    x[1, [20, 30, 40]] = 1.5
    x[2, [0, 11, V - 1]] = top + 3
    x[3, list(PLANTED_EDGES)] = -np.inf
    if nan:
        x[4, 20] = np.nan
    off, tok, nxt, label = [0, 4, 4, 4, 4, 4], list(PLANTED_EDGES), [1, 2, 3, 4], [-1, 0, 1, 2, 3]
    rows = start_rows(PLANTED_ROWS, [0, 0, 0, 0, 0, 3, -1, 5, 1 << 30])
    rows.len[5:], rows.choice[5:], rows.score[5:] = 7, 2, 1.5
    return (off, tok, nxt, label), x, rows, np.array([20, 20, 20, 10, 30 if nan else 20, PAD, PAD, PAD, PAD])
