"""Beam-search cases shared by tests/test_beam_gpu.py and tests/test_beam_cases_cpu.py: a float64 restatement of what HF
`generate(num_beams=nb, do_sample=False)` (transformers generation/utils.py `_beam_search`) does per step and per batch row, which is what
lhrs_beam_topk_rows / lhrs_beam_step (csrc/beam.hip) compute in fp32, and the inputs of the kernel tests.

Per step, with t tokens generated so far: logp = log_softmax(logits) of each running beam; HF's repetition penalty over the beam's OWN generated
tokens (logp < 0: logp * pen); total = logp + running score (start [0, -1e9, ...]); the top 2 * nb of the nb * V totals, ties to the lower flat
index beam * V + token; a candidate hits if its token is EOS or t + 1 == max_new; next running beams = best nb that did not hit (if fewer exist,
hits follow with -1e9 added); hits of rank < nb enter the finished set with total / (t + 1) ** length_penalty unless (a) early_stopping is True
and the set was full before the step or (b) the row's heuristic is already off; the set keeps its best nb; heuristic (sticky once false):
running[0] / (t + 1) ** length_penalty > worst finished score (-1e9 while a slot is empty); the loop goes on while some row's heuristic holds and
not (all sets full and early_stopping) and not every candidate of every row hit.  Result: the best finished hypothesis, else running beam 0.

Bounds.  |score - ref64| per candidate (the per-row lists, the merged top 2 * nb, the running and finished scores) of ONE device step against
this reference on the same fp32 logits and the same (fp32-rounded) running scores; a chain of n device steps may accumulate n such errors in
its scores.  SCORE_BOUND = 2e-5 comes from the precision of fp32 in total = ((x - max) - log(sum exp)) * pen + running, worst case each:
    x - max, |.| < 16 for a top candidate            half an ulp                     4.8e-7
    sum of <= 32768 exponentials: 32 sequential adds per thread + 10 tree levels, each 2^-24 relative -> log(sum) off by     2.6e-6
    logf itself and the subtraction, |.| < 32        half an ulp each                2.9e-6
    * pen: fp32(1.3) - 1.3 = 4.8e-8 relative on |logp| < 20, and the rounding of the product                               2.9e-6
    + running score, |total| < 64                    half an ulp, and the fp32 rounding of the uploaded running score       5.7e-6
    sum 1.5e-5  ->  SCORE_BOUND 2e-5   (whatever is measured, the bound may not exceed 1e-4)
The same arithmetic carried out in numpy float32 on the inputs of the kernel tests (all of STEP_GRID, VOCABS, SCALES, PENALTIES) is off by at most
1.9e-6; the worst value per case that the GPU test prints (BEAM_WORST) has NOT been recorded on an MI355X yet - when it is, the table belongs
here and SCORE_BOUND becomes about 2.5 x the worst of it.
Ordering: a step may be EXCUSED from the comparison of ids only if two adjacent totals among the reference's top 2 * nb + 1 lie within
BAND = 16 * SCORE_BOUND; the kernel-test inputs are chosen (and asserted on the CPU) to have no such pair."""
import numpy as np

SCORE_BOUND = 2e-5       # fp32 error analysis above (never above 1e-4)
BAND = 16 * SCORE_BOUND
NEG = -1.0e9

STEP_GRID = ((1, 2), (1, 4), (2, 3), (2, 8), (4, 4))   # (B, nb)
VOCABS = (32000, 32003, 1000)
SCALES = (1, 8)
PENALTIES = (1.0, 1.3)
STEP_T = 3               # tokens generated before the step the kernel tests compare
STEP_MAX_NEW = 8

# worst |score - ref| seen by the GPU tests of this process (how SCORE_BOUND was measured)
WORST = {"score": 0.0}


def make_logits(n, V, scale, seed):
    return (np.random.default_rng(seed).standard_normal((n, V), dtype=np.float32) * np.float32(scale)).astype(np.float32)


def log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


class Row:
    """One batch row of a beam search: running beams, finished set, heuristic flag."""

    def __init__(self, nb, start_neg=True):
        self.nb = nb
        self.run = np.array([0.0] + [NEG if start_neg else 0.0] * (nb - 1))
        self.seqs = [[] for _ in range(nb)]
        self.fin_score = [NEG] * nb          # sorted, best first
        self.fin_seq = [None] * nb           # None: empty slot
        self.heur = True

    def full(self):
        return all(s is not None for s in self.fin_seq)

    def best(self):
        """(tokens, score) of the row's result"""
        if self.fin_seq[0] is not None:
            return list(self.fin_seq[0]), self.fin_score[0]
        return list(self.seqs[0]), float(self.run[0])


class Step:
    """What one reference step saw: the merged top 2 * nb (score, beam, token, hit), the per-row top lists, the smallest gap between adjacent
    totals among the top 2 * nb + 1 of the group and among the top K + 1 of each beam's own row."""


def totals64(logits, row, pen):
    logp = log_softmax64(logits)
    if pen != 1.0:
        for j, seq in enumerate(row.seqs):
            if seq:
                idx = np.unique(np.asarray(seq, dtype=np.int64))
                v = logp[j, idx]
                logp[j, idx] = np.where(v < 0, v * pen, v / pen)
    return logp + row.run[:, None]


def ref_step(row, logits, t, max_new, length_penalty=1.0, early_stopping=False, eos=None, pen=1.0, mutation=None):
    """Advance `row` by one step over logits [nb, V] (any float dtype, taken as they are).  -> Step.  mutation: a planted mistake
    ("length_exponent", "rank_ge_nb_accepted") for the tests of the tests."""
    nb = row.nb
    K = 2 * nb
    V = logits.shape[1]
    tot = totals64(logits, row, pen)
    flat = tot.reshape(-1)
    order = np.argsort(-flat, kind="stable")[:K + 1]      # stable: the lower flat index first among equal totals
    st = Step()
    st.gap = float(np.min(-np.diff(flat[order]))) if len(order) > 1 else np.inf
    row_order = np.argsort(-tot, axis=1, kind="stable")[:, :K + 1]
    row_sorted = np.take_along_axis(tot, row_order, 1)
    st.row_gap = float(np.min(-np.diff(row_sorted, axis=1)))
    st.row_tok, st.row_score = row_order[:, :K], row_sorted      # K + 1 scores: the gap below the last rank too
    order = order[:K]
    st.score, st.beam, st.tok = flat[order], order // V, order % V
    n = t + 1
    st.hit = np.array([(eos is not None and int(k) == eos) or n == max_new for k in st.tok])
    lp = length_penalty + 1.0 if mutation == "length_exponent" else length_penalty
    lenp = float(n) ** lp
    # next running beams
    pick = [k for k in range(K) if not st.hit[k]][:nb]
    pick += [k for k in range(K) if st.hit[k]][:nb - len(pick)]
    new_run = np.array([st.score[k] + (NEG if st.hit[k] else 0.0) for k in pick])
    new_seqs = [row.seqs[st.beam[k]] + [int(st.tok[k])] for k in pick]
    st.parent, st.next_tok = [int(st.beam[k]) for k in pick], [int(st.tok[k]) for k in pick]
    # finished set: HF merges the old set with the candidates (blocked ones pushed down by -1e9) and keeps the best nb
    blocked = (row.full() and early_stopping is True) or not row.heur
    ranks = K if mutation == "rank_ge_nb_accepted" else nb
    merged = [(row.fin_score[j], row.fin_seq[j]) for j in range(nb)]
    for k in range(K):
        s = st.score[k] / lenp
        ok = st.hit[k] and k < ranks and not blocked
        merged.append((s if ok else s + NEG, row.seqs[st.beam[k]] + [int(st.tok[k])] if ok else None))
    keep = np.argsort(-np.array([m[0] for m in merged]), kind="stable")[:nb]
    row.fin_score = [merged[i][0] if merged[i][1] is not None else NEG for i in keep]
    row.fin_seq = [merged[i][1] for i in keep]
    row.run, row.seqs = new_run, new_seqs
    worst = row.fin_score[-1] if row.full() else NEG
    row.heur = bool(row.heur and row.run[0] / lenp > worst)
    st.all_hit = bool(st.hit.all())
    return st


def batch_goes_on(rows, steps, early_stopping):
    return any(r.heur for r in rows) and not (all(r.full() for r in rows) and early_stopping is True) and not all(s.all_hit for s in steps)


def ref_beam_search(logits_fn, B, nb, max_new, length_penalty=1.0, early_stopping=False, eos=None, pen=1.0, pad=0, mutation=None):
    """logits_fn(t, seqs) -> [B * nb, V] logits of the running beams (seqs: their B * nb token lists).  -> (ids [B, L] padded with `pad`, scores [B],
    n_steps, min_gap per step)."""
    rows = [Row(nb, start_neg=mutation != "no_start_neg") for _ in range(B)]
    gaps = []
    t = 0
    while True:
        logits = np.asarray(logits_fn(t, [s for r in rows for s in r.seqs]))
        steps = [ref_step(rows[b], logits[b * nb:(b + 1) * nb], t, max_new, length_penalty, early_stopping, eos, pen, mutation) for b in range(B)]
        gaps.append(min(s.gap for s in steps))
        t += 1
        if not batch_goes_on(rows, steps, early_stopping):
            break
    best = [r.best() for r in rows]
    L = max(len(b[0]) for b in best)
    ids = np.full((B, L), pad, dtype=np.int64)
    for b, (seq, _) in enumerate(best):
        ids[b, :len(seq)] = seq
    return ids, np.array([b[1] for b in best]), t, gaps


def upto_eos(seq, eos):
    seq = [int(x) for x in seq]
    return seq[:seq.index(eos) + 1] if eos is not None and eos in seq else seq


# ------------------------------------------------------------------------------------------------ inputs of the kernel tests
# seed per (B, nb, V, scale): chosen so that, with and without the penalty, no two adjacent totals among the top 2 * nb + 1 of a group are
# closer than 1.6e-3, the largest BAND the bound rule allows (test_beam_cases_cpu.py asserts it).  A beam's OWN list of 2 * nb is compared rank by
# rank on the scores, and on the token where the reference's neighbours at that rank are further than BAND away (Step.row_score).
STEP_SEEDS = {(1, 2, 32000, 1): 125, (1, 2, 32003, 1): 128, (1, 4, 32003, 8): 155, (2, 3, 32003, 1): 238, (2, 3, 1000, 1): 238,
              (2, 8, 32000, 1): 286, (2, 8, 32003, 1): 297, (2, 8, 32003, 8): 295, (2, 8, 1000, 1): 294, (4, 4, 32000, 1): 452,
              (4, 4, 32003, 8): 455, (4, 4, 1000, 1): 449}   # where the rule of step_seed() gave an ambiguous case: the next seed that does not


def step_seed(B, nb, V, scale):
    return STEP_SEEDS.get((B, nb, V, scale), 100 * B + 10 * nb + scale + V % 7)


def make_step_case(B, nb, V, scale, pen, seed=None):
    """-> (rows before the step, logits [B * nb, V] fp32, rows after, [Step per row]).  The running scores come from a reference step over other
    logits (negative, unequal); each beam's history is then filled up to STEP_T tokens with its row's 1st and 3rd largest logits, so that the
    penalty decides among the candidates."""
    import copy

    seed = step_seed(B, nb, V, scale) if seed is None else seed
    R = B * nb
    logits0, logits1 = make_logits(R, V, scale, 7919 * seed + 1), make_logits(R, V, scale, 7919 * seed + 2)
    rows = [Row(nb) for _ in range(B)]
    for b, r in enumerate(rows):
        ref_step(r, logits0[b * nb:(b + 1) * nb], 0, STEP_MAX_NEW)
        # a second spread of the running scores: the first step leaves them within the top 2 * nb of ONE row
        r.run = r.run - np.arange(nb) * 0.37
        top = np.argsort(-logits1[b * nb:(b + 1) * nb], axis=1, kind="stable")
        r.seqs = [r.seqs[j] + [int(top[j, 0]), int(top[j, 2])] for j in range(nb)]
    before = copy.deepcopy(rows)
    steps = [ref_step(rows[b], logits1[b * nb:(b + 1) * nb], STEP_T, STEP_MAX_NEW, pen=pen) for b in range(B)]
    return before, logits1, rows, steps


EOS_B, EOS_NB, EOS_V, EOS_MAX_NEW, EOS_TOKEN, EOS_SEED = 2, 3, 1000, 3, 7, 10


def make_eos_case(seed=EOS_SEED):
    """Three chained steps with EOS forced among the candidates: in steps 0 and 1 EOS is the second largest logit of every running beam.  Step 0:
    all candidates come from beam 0, EOS hits at rank 1 and enters the finished set.  Step 1: every beam offers its best token and EOS, so EOS
    candidates land on both sides of rank nb and those of rank >= nb must be dropped.  Step 2: t + 1 == max_new, every candidate hits and the
    top nb finish.
    -> (logits per step [3][B * nb, V], [rows after step t], [[Step per row] per step], [goes_on after step t])"""
    import copy

    R = EOS_B * EOS_NB
    lgs, snaps, steps, go = [], [], [], []
    rows = [Row(EOS_NB) for _ in range(EOS_B)]
    for t in range(EOS_MAX_NEW):
        lg = make_logits(R, EOS_V, 1, 31 * seed + t)
        srt = -np.sort(-lg, axis=1)
        if t < 2:
            lg[:, EOS_TOKEN] = (srt[:, 0] + srt[:, 1]) / 2
        lgs.append(lg)
        st = [ref_step(rows[b], lg[b * EOS_NB:(b + 1) * EOS_NB], t, EOS_MAX_NEW, eos=EOS_TOKEN) for b in range(EOS_B)]
        steps.append(st)
        snaps.append(copy.deepcopy(rows))
        go.append(batch_goes_on(rows, st, False))
    return lgs, snaps, steps, go
