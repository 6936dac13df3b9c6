"""The tools of tests/rowwise_cases.py on the CPU: the float32 emulation of every arithmetic row-wise kernel passes the comparator on every
CPU-sized case with a worst ratio of at most 1/4 (the constants are 4x the emulation's worst ratio, and were not taken from the HIP kernels);
each named defect of the emulation is rejected by at least 3x the bound on at least one case; the old whole-matrix rel_err check would not
notice one wrong LayerNorm row; cells_of's host rules agree with the ones the library exports."""
import math

import pytest
import torch

import rowwise_cases as rc

BF = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _few_threads():
    """thousands of tiny tensor operations: a thread pool sized by the machine only slows them down"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 4))
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module")
def emu_worst():
    """kind -> (worst ratio at c = 1, where) of the unmutated emulation over every CPU-sized case"""
    worst = {}
    for c in rc.CASES:
        if c.op not in rc.EMULATED or rc.case_elems(c) > rc.CPU_MAX_ELEMS:
            continue
        for kind, what, got, ref in rc.emulate(c):
            rep = rc.measure(kind, got, ref, c.op, c.name + " " + what)
            if rep.unit >= worst.get(kind, (-1.0, ""))[0]:
                worst[kind] = (rep.unit, rep.where)
    return worst


def test_emulation_passes_with_a_quarter_of_every_bound(emu_worst):
    assert set(emu_worst) == set(rc.BOUNDS), set(rc.BOUNDS) ^ set(emu_worst)
    for kind, (u, where) in sorted(emu_worst.items()):
        print(f"{kind:12s} emulation worst {u:.4g} at c = 1, c = {rc.BOUNDS[kind]:.4g}")
        assert u / rc.BOUNDS[kind] <= 0.25, where


def test_constants_are_4x_the_emulation_ratio_written_next_to_them(emu_worst):
    for kind, (u, where) in emu_worst.items():
        assert rc.BOUNDS[kind] == 4.0 * rc.EMU_WORST[kind]
        assert 0.9 * rc.EMU_WORST[kind] <= u <= rc.EMU_WORST[kind] * 1.0001, (kind, u, rc.EMU_WORST[kind], where)   # the recorded ratio is the measured one (3 digits, rounded up)


# defect -> the operations whose cases it is tried on
MUTATIONS = {
    "mean_over_cols_minus_1": ("layernorm_fwd",),
    "eps_omitted": ("layernorm_fwd", "rmsnorm_fwd"),
    "add_dropped": ("layernorm_bwd", "rmsnorm_bwd"),
    "last_row_missing_from_dgamma": ("layernorm_bwd",),
    "dbeta_dgamma_swapped": ("layernorm_bwd",),
    "accumulate_ignored": ("layernorm_bwd", "pooler_query_grad"),
    "sin_sign_flipped_on_second_half": ("rope",),
    "position_off_by_one": ("rope",),
    "du_dg_swapped": ("swiglu_bwd",),
    "gelu_bwd_tanh_form": ("map",),
    "grad_scaled_by_1_over_n_minus_1": ("ce",),
    "onehot_at_t_plus_1": ("ce",),
    "no_max_subtraction": ("ce",),
    "last_row_of_one_split_dropped": ("colsum",),
    "tail_beyond_multiple_of_256_dropped": ("sqnorm",),
    "bias_correction_with_step_minus_1": ("adan",),
    "pre_grad_not_updated": ("adan",),
    "coupled_l2": ("adamw",),
    "clip_applied_when_coef_above_1": ("adan", "adamw"),
}


def _worst_ratio(op, mut, only=None):
    best = (0.0, "")
    for c in rc.cases_of(op, cpu=True):
        if only is not None and not only(c):
            continue
        for kind, what, got, ref in rc.emulate(c, mut):
            rep = rc.measure(kind, got, ref, c.op, c.name + " " + what)
            r = rep.ratio if rep.ratio == rep.ratio else float("inf")
            if r > best[0]:
                best = (r, rep.where)
    return best


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_comparator_rejects_mutation_by_3x(mutation):
    for op in MUTATIONS[mutation]:
        ratio, where = _worst_ratio(op, mutation)
        assert ratio >= 3.0, (mutation, op, ratio, where)


def test_ce_without_max_subtraction_overflows_on_the_offset_rows():
    """a +200 row without the max subtraction: exp(200) is inf in fp32 - the loss comes out inf or NaN and the comparator rejects it"""
    c = next(c for c in rc.cases_of("ce") if c.shape == dict(n=77, V=2040) and c.opt["grad"] and c.opt["inplace"])
    i = rc.ce_inputs(c)
    got = rc.emu_ce(i["x"], i["t"], "no_max_subtraction")
    offset_rows = i["x"].float().amin(1) > 150
    assert bool(offset_rows.any()) and not bool(torch.isfinite(got["row_loss"][offset_rows]).any())
    assert rc.measure("ce_loss", got["row_loss"], rc.ref_ce(i["x"], i["t"])["row_loss"]).ratio == float("inf")


def test_adan_bias_correction_with_step_minus_1_is_rejected_at_a_finite_step_too():
    """step 1 divides by 1 - b^0 = 0 (inf: rejected, the parametrised test above); a step 3 taken from the state of two correct steps gives finite
    wrong values, rejected as well"""
    c = next(c for c in rc.cases_of("adan") if not c.opt["clip"])
    i, kw = rc.opt_inputs(c), rc.opt_args(c)
    st = rc.opt_state0(c, i["p"])
    for k in (1, 2):
        new = rc.emu_adan(st, i["grads"][k - 1], k, **kw)
        st = {name: new[name] for name in st}
    ref = rc.ref_adan(st, i["grads"][2], 3, **kw)
    good, bad = rc.emu_adan(st, i["grads"][2], 3, **kw), rc.emu_adan(st, i["grads"][2], 3, mut="bias_correction_with_step_minus_1", **kw)
    assert bool(torch.isfinite(bad["p"]).all())
    assert rc.measure("adan", good["p"], ref["p"]).ratio <= 0.25 and rc.measure("adan", bad["p"], ref["p"]).ratio >= 3.0


def test_rmsnorm_xhat_not_rounded_before_the_weight():
    """y = bf16(w * xhat) instead of bf16(w * bf16(xhat)).  The defect moves an element by at most half a bf16 ulp of xhat times w - LESS than
    the whole ulp of `pre` the bound grants (fp32 and fp64 rstd may round xhat to different neighbours), so the bound alone cannot see it:
    its worst ratio over the grid stays below 1.  What rejects it is the reference's pair of admissible bf16 values per element (Ref.alts):
    away from a rounding tie of xhat there is ONE value the kernel can store, and bf16(w * xhat) is another one on many elements."""
    c = next(c for c in rc.cases_of("rmsnorm_fwd") if c.shape == dict(rows=9, cols=1024))
    i = rc.norm_inputs(c)
    ref = rc.ref_rmsnorm_fwd(i["x"], i["gamma"], 1e-5)["y"]
    bad = rc.emu_rmsnorm_fwd(i["x"], i["gamma"], 1e-5, "xhat_not_rounded")["y"]
    assert rc.measure("rms_y", bad, ref._replace(alts=None)).ratio < 1.0
    assert rc.measure("rms_y", bad, ref).ratio == float("inf")
    lo, hi = ref.alts
    assert float((lo != hi).double().mean()) < 1e-3                          # two admissible values: only next to a tie
    ratio, where = _worst_ratio("rmsnorm_fwd", "xhat_not_rounded")
    assert ratio >= 3.0, where


def test_old_whole_matrix_check_misses_one_wrong_layernorm_row_at_2057x1024():
    """rel_err(out, ref) < 4e-3 (tests/test_kernels_gpu.py) over 2057 rows of unit RMS: a row normalised with a mean that is off by 5 % of a
    standard deviation carries an error of 0.05 in every one of its elements (25x the bf16 rounding of a value near 1) and moves the
    whole-matrix figure by 0.05 / sqrt(2057) = 1.1e-3: accepted.  Any row-local error below 4e-3 * sqrt(2057) = 0.18 RMS is.  The comparator
    rejects the same row and names it."""
    assert 0.05 / math.sqrt(2057) < 4e-3
    c = next(c for c in rc.cases_of("layernorm_bwd") if c.shape == dict(rows=2057, cols=1024))
    i = rc.norm_inputs(c)
    ref = rc.ref_layernorm_fwd(i["x"], i["gamma"], i["beta"], 1e-5)
    good = rc.emu_layernorm_fwd(i["x"], i["gamma"], i["beta"], 1e-5)["y"]
    bad = good.clone()
    r = 1500
    bad[r] = (good[r].float() + 0.05 * i["gamma"].float()).to(BF)                       # the row's mean off by 0.05 sigma
    old = ((bad.float() - ref["y"].want.float()).norm() / ref["y"].want.float().norm()).item()
    assert old < 4e-3, old                                                              # the old check accepts it
    assert rc.measure("ln_y", good, ref["y"]).ratio <= 0.25
    rep = rc.measure("ln_y", bad, ref["y"])
    assert rep.ratio >= 3.0 and f"row {r} " in rep.where, rep.where


def test_comparator_names_operation_case_row_and_column():
    want = torch.ones(5, 16, dtype=torch.float64)
    got = want.clone().to(BF)
    got[3, 11] = float("nan")
    rep = rc.measure("map", got, rc.R(want, want), "map", "n=80")
    assert rep.ratio == float("inf") and rep.where.startswith("map [n=80] map: row 3 col 11 "), rep.where


def test_sentinel_check_sees_one_element_past_a_vector_slice():
    buf = torch.full((20,), -1, dtype=torch.int32)
    buf[4:12] = 7
    mark = torch.zeros(20, dtype=torch.bool)
    mark[4:12] = True
    assert bool((buf[~mark] == -1).all())
    buf[12] = 0
    assert not bool((buf[~mark] == -1).all())


def test_cells_of_hand_worked():
    f = rc.cells_of
    assert f("layernorm_bwd", dict(rows=1024, cols=512), dict(add=None)) >= {"layernorm_bwd/one_trip", "layernorm_bwd/NCH=1", "layernorm_bwd/no_add"}
    assert "layernorm_bwd/grid_stride" in f("layernorm_bwd", dict(rows=1025, cols=1024), dict(add="alias", need_dx=True))
    assert "layernorm_bwd/no_dx" in f("layernorm_bwd", dict(rows=3, cols=512), dict(add=None, need_dx=False))
    assert "ce/idle_threads" in f("ce", dict(n=1, V=2040), {}) and "ce/one_trip" in f("ce", dict(n=1, V=2048), {}) and "ce/multi_trip" in f("ce", dict(n=1, V=2056), {})
    assert "swiglu_bwd/grid_stride" in f("swiglu_bwd", dict(rows=1525, F=11008), {}) and "swiglu_bwd/one_trip" in f("swiglu_bwd", dict(rows=1524, F=11008), {})
    assert "rope/grid_stride" in f("rope", dict(rows=4097, nheads=64, D=128), dict(pos_mod=5)) and "rope/one_trip" in f("rope", dict(rows=4096, nheads=64, D=128), dict(pos_mod=5))
    assert "map/grid_stride" in f("map", dict(n=16777232), dict(op=0)) and "map/one_trip" in f("map", dict(n=16777216), dict(op=0))
    assert "colsum/nsplit_cap" in f("colsum", dict(rows=16385, cols=1), {}) and "colsum/nsplit>1" in f("colsum", dict(rows=16384, cols=1), {})
    assert "colsum/nsplit=1" in f("colsum", dict(rows=256, cols=1), {}) and "colsum/nsplit>1" in f("colsum", dict(rows=257, cols=1), {})
    assert "sqnorm/grid_stride" in f("sqnorm", dict(n=1048577), {}) and "sqnorm/blocks" in f("sqnorm", dict(n=1048576), {})
    assert "adan/prox" in f("adan", dict(n=8), dict(no_prox=False)) and "adan/no_clip" in f("adan", dict(n=8), dict(clip=True, max_norm=0.0))
    assert "accum_f32/grid_stride" in f("accum_f32", dict(n=4194312), {}) and "accum_f32/one_trip" in f("accum_f32", dict(n=4194304), {})
    reached = set().union(*(f(c.op, c.shape, c.opt) for c in rc.CASES))
    assert reached == rc.paths, (sorted(rc.paths - reached), sorted(reached - rc.paths))


def test_cells_of_agrees_with_the_exported_host_rules():
    from lhrs_bot_amd import _lib
    lib = _lib.load()
    for rows in (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2057, 16384, 16385, 100000):
        assert lib.lhrs_layernorm_bwd_nblk(rows) == rc.layernorm_bwd_nblk(rows), rows
        assert lib.lhrs_colsum_nsplit(rows) == rc.colsum_nsplit(rows), rows
        assert (rows > 4 * 256) == ("layernorm_bwd/grid_stride" in rc.cells_of("layernorm_bwd", dict(rows=rows, cols=512), dict(add=None))), rows
        assert (lib.lhrs_colsum_nsplit(rows) * 256 < rows) == ("colsum/nsplit_cap" in rc.cells_of("colsum", dict(rows=rows, cols=8), {})), rows
    for n in (1, 255, 256, 257, 10007, 1048576, 1048577, 1048576 + 257, 5000000):
        assert lib.lhrs_sqnorm_nblk(n) == rc.sqnorm_nblk(n), n
        assert (lib.lhrs_sqnorm_nblk(n) * 256 < n) == ("sqnorm/grid_stride" in rc.cells_of("sqnorm", dict(n=n), {})), n
        assert (lib.lhrs_sqnorm_nblk(n) * 256 < n) == ("adan/grid_stride" in rc.cells_of("adan", dict(n=n), {})), n
