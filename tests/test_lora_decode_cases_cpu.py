"""The tools of tests/lora_decode_cases.py on the CPU: the float32 emulations of lhrs_lora_down / lhrs_lora_up pass the comparator on every case
with at most a quarter of each bound (the constants are 4x the emulation's worst ratio and were not taken from the HIP kernels); every named
defect of an emulation breaks the bound; the allowances stay small; the restated host rules hold over the shapes of the table and of the model."""
import pytest
import torch

import gemv_cases as gc
import lora_decode_cases as lc


@pytest.fixture(scope="module", autouse=True)
def _few_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 4))
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module")
def refs():
    """case -> (inputs, reference): computed once, shared by every test of the module and left unchanged"""
    out = {}
    for c in lc.DOWN_CASES:
        i = lc.down_inputs(c)
        out[c] = (i, lc.down_reference(c, i)[0])
    for c in lc.UP_CASES:
        i = lc.up_inputs(c)
        out[c] = (i, lc.up_reference(c, i)[0])
    return out


def _kind(c):
    return lc.down_kind(c) if isinstance(c, lc.Down) else "up"


def _emulate(c, i, mut=None):
    return lc.emu_down(c, i, mut) if isinstance(c, lc.Down) else lc.emu_up(c, i, mut)


@pytest.fixture(scope="module")
def emu_worst(refs):
    worst = {}
    for c, (i, ref) in refs.items():
        rep = lc.measure(_kind(c), _emulate(c, i), ref, op=type(c).__name__, case=str(tuple(c)))
        if rep.unit >= worst.get(_kind(c), (-1.0, ""))[0]:
            worst[_kind(c)] = (rep.unit, rep.where)
    return worst


def test_emulation_passes_with_a_quarter_of_every_bound(emu_worst):
    assert set(emu_worst) == set(lc.BOUNDS)
    for kind, (u, where) in sorted(emu_worst.items()):
        print(f"{kind:12s} emulation worst {u:.4g} at c = 1, c = {lc.BOUNDS[kind]:.4g}")
        assert lc.BOUNDS[kind] >= 4.0 * u, where


def test_constants_are_4x_the_emulation_ratio_written_next_to_them(emu_worst):
    """the written figures are the emulation's, not padded: the recomputed ratio is at least 0.9 of each (that c >= 4 x the recomputed ratio is the
    test above; a torch build that sums in another order may move the ratio a little either way without failing here)"""
    for kind, (u, where) in emu_worst.items():
        assert lc.BOUNDS[kind] == 4.0 * lc.EMU_WORST[kind]
        assert u >= 0.9 * lc.EMU_WORST[kind], (kind, u, lc.EMU_WORST[kind], where)


# defect -> the cases it is tried on: it must break the bound on EVERY one of them
MUTATIONS = {
    "drop_slice": lambda c: not getattr(c, "zero", False),                                  # the last K-slice is left out (down: written as zeros; up: not summed)
    "drop_chunk": lambda c: not getattr(c, "zero", False),                                  # lane 0 skips its last 16-B chunk
    "neighbour_block": lambda c: isinstance(c, lc.Up) and not c.zero,                       # Bw read at the next block's columns
    "t_not_rounded": lambda c: isinstance(c, lc.Up) and not c.zero and not c.exact,         # t kept in fp32
    "res_last_batch_row": lambda c: isinstance(c, lc.Up) and c.res,                         # the residual is not added on the last batch row
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_comparator_rejects_mutation(refs, mutation):
    tried = 0
    for c, (i, ref) in refs.items():
        if not MUTATIONS[mutation](c):
            continue
        rep = lc.measure(_kind(c), _emulate(c, i, mutation), ref, op=type(c).__name__, case=str(tuple(c)))
        ratio = rep.ratio if rep.ratio == rep.ratio else float("inf")
        print(f"{mutation} on {tuple(c)}: {ratio:.3g}x the bound")
        assert ratio > 1.0, (mutation, tuple(c), rep.where)
        tried += 1
    assert tried >= 3


def test_guards_are_checked(refs):
    """a write into the guard slice, the guard batch row or the guard column tail fails whatever the live values are"""
    c = lc.DOWN_CASES[1]
    i, ref = refs[c]
    got = lc.emu_down(c, i)
    assert lc.measure(lc.down_kind(c), got, ref).ratio <= 0.25
    for row in (ref.want.shape[0], got.shape[0] - 1):
        bad = got.clone()
        bad[row, 3] = 0.0
        assert lc.measure(lc.down_kind(c), bad, ref).ratio == float("inf")
    c = lc.UP_CASES[0]
    i, ref = refs[c]
    got = lc.emu_up(c, i)
    for row, col in ((c.B, 0), (0, i["N"])):
        bad = got.clone()
        bad[row, col] = 0.0
        assert lc.measure("up", bad, ref).ratio == float("inf")


def test_allowances_are_small_and_absent_where_t_is_exact(refs):
    for c, (i, ref) in refs.items():
        if isinstance(c, lc.Down):
            act = gc.ref_prologue(i["x"], c.pro, i["norm_w"], lc.EPS)
            assert gc.marked_fraction(act) <= 0.01, (tuple(c), gc.marked_fraction(act))   # the cap of tests/test_gemv_cases_cpu.py
            assert c.pro != 0 or float(ref.extra.abs().max()) == 0.0
        else:
            _, marked = lc.up_reference(c, i)
            assert marked <= 0.03 * c.B * i["R"] + 1, (c.name, marked)   # a t near zero sits between closely spaced bf16 values: marked, with a tiny ulp
            if c.exact or c.zero:
                assert marked == 0 and float(ref.extra.abs().max()) == 0.0, c.name


def test_t_zero_case_is_exactly_the_rounded_sum(refs):
    c = next(c for c in lc.UP_CASES if c.zero)
    i, _ = refs[c]
    got = lc.emu_up(c, i)
    want = (i["acc"] + i["res"].float()).to(torch.bfloat16)
    assert torch.equal(got[:c.B, :i["N"]], want)


def test_host_rules():
    """the slice rule: 1..16 slices, whole 64-element chunks, none empty, together exactly K; R / 8 row blocks x slices reach the 256 CUs where K allows"""
    shapes = [(c.K, c.R) for c in lc.DOWN_CASES] + [(K, R) for K in (4096, 11008) for R in (8, 16, 24, 64, 128, 256, 384, 768)]
    for K, R in shapes:
        nsl = lc.splits(K, R)
        b = lc.slice_bounds(K, nsl)
        assert 1 <= nsl <= lc.MAX_SLICES and b[0][0] == 0 and b[-1][1] == K
        assert all(k1 > k0 and (k1 - k0) % 64 == 0 for k0, k1 in b) and all(b[j][1] == b[j + 1][0] for j in range(nsl - 1))
        assert nsl == min(lc.MAX_SLICES, K // 64) or nsl * (R // 8) >= 200, (K, R, nsl)
    assert lc.splits(64, 8) == 1 and lc.splits(4096, 24) == 16 and lc.splits(4096, 384) == 6 and lc.splits(11008, 128) == 16
    assert [lc.lanes_per_row(r) for r in (8, 16, 24, 64, 128, 768)] == [1, 2, 4, 8, 16, 64]


def test_rejection_table_names_every_rule():
    down = {tuple(o.items()) for e, o in lc.REJECTS if e == "down"}
    up = {tuple(o.items()) for e, o in lc.REJECTS if e == "up"}
    assert len(down) == 8 and len(up) == 11
    for entry, o in lc.REJECTS:
        assert set(o) <= set(lc.REJECT_BASE[entry])
