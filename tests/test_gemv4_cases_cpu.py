"""The tools of tests/gemv4_cases.py on the CPU: the float32 emulation of the two 4-bit decode GEMV kernels passes the comparator on every
case with a worst ratio of at most 1/4 (the constants are 4x the emulation's worst ratio and were not taken from the HIP kernels); each named
defect of an emulation is rejected on at least one case; the emulation's dequantisation gives the oracle's bf16 weight bit for bit; the
restated host rule sends every case where the table says and refuses the rejections."""
import pytest
import torch

import gemv4_cases as g4
from oracle import nf4_oracle as N4


@pytest.fixture(scope="module", autouse=True)
def _few_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 4))
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module")
def emu_worst():
    """kind -> (worst ratio at c = 1, where) of the unmutated emulation over every case"""
    worst = {}
    for c in g4.CASES:
        kind = g4.kind_of(c)
        rep = g4.measure(kind, g4.emulate(c), g4.reference(c)[0], "gemv4", c.name)
        if rep.unit >= worst.get(kind, (-1.0, ""))[0]:
            worst[kind] = (rep.unit, rep.where)
    return worst


def test_emulation_passes_with_a_quarter_of_every_bound(emu_worst):
    assert set(emu_worst) == set(g4.BOUNDS), set(g4.BOUNDS) ^ set(emu_worst)
    for kind, (u, where) in sorted(emu_worst.items()):
        print(f"{kind:12s} emulation worst {u:.4g} at c = 1, c = {g4.BOUNDS[kind]:.4g}")
        assert u / g4.BOUNDS[kind] <= 0.25, where


def test_constants_are_4x_the_emulation_ratio_written_next_to_them(emu_worst):
    for kind, (u, where) in emu_worst.items():
        assert g4.BOUNDS[kind] == 4.0 * g4.EMU_WORST[kind]
        assert 0.9 * g4.EMU_WORST[kind] <= u <= g4.EMU_WORST[kind] * 1.0001, (kind, u, g4.EMU_WORST[kind], where)


# defect -> the kernels it exists in
MUTATIONS = {
    "nibbles_swapped": ("valu", "mfma"),                # element 2j from the low nibble
    "absmax_neighbour": ("valu", "mfma"),               # the statistics of the next block of the row
    "weight_not_rounded": ("valu", "mfma"),             # level * absmax kept in fp32: the absmax factored out of the block sum
    "drop_chunk": ("valu", "mfma"),                     # lane 0 skips its last chunk / wave 0 its last step
    "res_last_batch_row": ("valu", "mfma"),             # the residual is not added on the last batch row
    "batch_column_B_live": ("mfma",),                   # the MFMA column after the batch is computed and stored
    "permutation_on_weights_only": ("mfma",),           # the k order inside a step of 128 applied to one operand
}


def _kernels(c):
    return {k for k, _ in g4.plan(c.opt["B"], c.opt["N"], c.opt["K"], c.opt["pro"])}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_comparator_rejects_mutation_by_3x(mutation):
    for kern in MUTATIONS[mutation]:
        best = (0.0, "")
        for c in g4.CASES:
            if _kernels(c) != {kern}:
                continue
            rep = g4.measure(g4.kind_of(c), g4.emulate(c, mutation), g4.reference(c)[0], "gemv4", c.name)
            r = rep.ratio if rep.ratio == rep.ratio else float("inf")
            if r > best[0]:
                best = (r, rep.where)
        print(f"{mutation} on the {kern} kernel: caught at {best[0]:.3g}x the bound: {best[1]}")
        assert best[0] >= 3.0, (mutation, kern, best)


@pytest.mark.parametrize("c", g4.CASES, ids=[c.name.replace(" ", "_") for c in g4.CASES])
def test_emulated_dequantisation_is_the_oracles_bf16_weight(c):
    """N4.dequantize_4bit(N4.quantize_4bit(w)) cast to bf16 == the emulation's level[code] * absmax, bit for bit; and the codes are the
    oracle's packed bytes row by row"""
    i, o = g4.inputs(c), c.opt
    want = torch.from_numpy(N4.dequantize_4bit(N4.quantize_4bit(i["W"].float().numpy(), "fp4" if o["fp4"] else "nf4", o["dq"]))).to(torch.bfloat16)
    got = g4.emu_dequant(i["codes"], i["absmax"], o["fp4"]).to(torch.bfloat16)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)) and torch.equal(want.view(torch.int16), i["Wq"].view(torch.int16))
    assert i["codes"].shape == (o["N"], o["K"] // 2) and i["absmax"].shape == (o["N"], o["K"] // 64)
    assert ("absmax" in i["st"]) == (not o["dq"])


def test_planted_weights_reach_the_special_blocks():
    """an all-zero block (absmax 0), an outlier block, a 1e-4 row and a block on the decision thresholds are in the table"""
    zero = outlier = small = False
    for c in g4.CASES:
        i = g4.inputs(c)
        a = i["absmax"]
        zero |= bool((a == 0).any())
        outlier |= bool((a >= 1.0).any())
        small |= bool(((a > 0) & (a < 2e-5)).any())
    assert zero and outlier and small
    w = g4.weight(16, 192, seed=1).float()
    assert set((w[11, 128:192] * 4).tolist()) >= set(torch.tensor(N4.NF4_THR).to(torch.bfloat16).float().tolist())


def test_host_rule_hand_worked_and_every_branch_in_the_table():
    P = g4.plan
    assert P(1, 4096, 4096, 1) == [("valu", 1)] and P(2, 64, 192, 0) == [("valu", 2)] and P(8, 64, 704, 2) == [("valu", 8)]
    assert P(2, 64, 128, 0) == [("mfma", 2)] and P(16, 64, 11008, 0) == [("mfma", 16)] and P(3, 4096, 11008, 2) == [("mfma", 3)]
    assert P(8, 35, 11008, 1) == [("mfma", 7), ("valu", 1)] and P(16, 35, 4096, 1) == [("mfma", 16)]
    assert 8 * 11008 * 2 + g4.MFMA_STATIC_LDS > g4.LDS_BYTES >= 7 * 11008 * 2 + g4.MFMA_STATIC_LDS
    for name, o in g4.REJECTS.items():
        with pytest.raises(g4.Rejected):
            P(o["B"], o["N"], o["K"], 0, o.get("absmax", True), o.get("ldc"))
    seen = set()
    for c in g4.CASES:
        o = c.opt
        launches = P(o["B"], o["N"], o["K"], o["pro"])
        for kern, nb in launches:
            seen |= {f"{kern}/pro{o['pro']}", f"{kern}/{'f32' if o['f32'] else 'bf16'}", f"{kern}/{'res' if o['res'] else 'no_res'}",
                     f"{kern}/{'fp4' if o['fp4'] else 'nf4'}", f"{kern}/{'dq' if o['dq'] else 'plain_absmax'}", f"{kern}/{'strided' if o['strided'] else 'dense'}"}
            if kern == "valu":
                seen.add(f"valu/NB{nb}")
                nch = o["K"] // 32
                seen.add("valu/chunks<lanes" if nch < 64 else "valu/partial_trip" if nch % 64 else "valu/full_trip")
                seen.add("valu/tall" if nb == 1 and o["N"] > 4096 else "valu/short" if nb == 1 else "valu/batch")
            else:
                steps = [e - b for b, e in g4.mfma4_waves(o["K"])]
                seen |= {f"mfma/steps{min(max(steps), 9)}", "mfma/B16" if nb == 16 else "mfma/dead_columns", "mfma/ragged_rows" if o["N"] % 16 else "mfma/full_rows"}
                if 0 in steps:
                    seen.add("mfma/idle_waves")
                if len(set(steps)) > 1 and min(steps) > 0:
                    seen.add("mfma/short_last_wave")
        if len(launches) > 1:
            seen.add("chunked")
    want = ({f"{k}/{x}" for k in ("valu", "mfma") for x in ("pro0", "pro1", "pro2", "f32", "bf16", "res", "no_res", "fp4", "nf4", "dq", "plain_absmax",
                                                          "strided", "dense")}
            | {f"valu/NB{n}" for n in range(1, 9)} | {"valu/chunks<lanes", "valu/partial_trip", "valu/full_trip", "valu/tall", "valu/short", "valu/batch"}
            | {"mfma/steps1", "mfma/steps2", "mfma/steps4", "mfma/steps9", "mfma/B16", "mfma/dead_columns", "mfma/ragged_rows", "mfma/full_rows",
               "mfma/idle_waves", "mfma/short_last_wave", "chunked"})
    assert seen == want, (sorted(want - seen), sorted(seen - want))


def test_wave_split_of_the_mfma_kernel_covers_every_step_once():
    for K in sorted({c.opt["K"] for c in g4.CASES if c.opt["K"] % 128 == 0}) + [256, 1024, 2176]:
        waves = g4.mfma4_waves(K)
        steps = [s for b, e in waves for s in range(b, e)]
        assert steps == list(range(K // 128)) and all(0 <= b <= e <= K // 128 for b, e in waves), K
        # the two loads a wave issues before its prologue stay inside its own steps, and an idle wave re-reads the row's last step
        for b, e in waves:
            nst = e - b
            for u in range(2):
                s = min(b + min(u, max(nst - 1, 0)), K // 128 - 1)
                assert (b <= s < e) if nst else s == K // 128 - 1


def test_comparator_sees_a_written_guard_row_and_names_the_element():
    want = torch.ones(2, 16, dtype=torch.float64)
    got = torch.full((3, 16), float("nan"), dtype=torch.bfloat16)
    got[:2] = 1
    ref = g4.gc.R(want, want, 16)
    assert g4.measure("bf16_plain", got, ref).ratio == 0.0
    got[1, 11] = 1.5
    rep = g4.measure("bf16_plain", got, ref, "gemv4", "x")
    assert rep.ratio > 3 and rep.where.startswith("gemv4 [x] bf16_plain: row 1 col 11 "), rep.where
    got[1, 11], got[2, 0] = 1, 0
    assert g4.measure("bf16_plain", got, ref).ratio == float("inf")
