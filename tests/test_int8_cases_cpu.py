"""The tools of tests/int8_cases.py on the CPU: the references agree with oracle/int8_oracle.py, the torch emulation of the device pipeline
passes every comparison the GPU tests make, and every mutant of the emulation fails a named case (so each case's inputs matter)."""
import numpy as np
import pytest
import torch

from oracle import int8_oracle as I8

import gemm_cases as gc
import int8_cases as ic


def _w_for(case):
    return ic.make_w(100 + case.N + case.K, case.N, case.K)


def _run_emu_prepare(x, wq, wscale, ws=None, mut=()):
    M, K = x.shape
    N = wq.shape[0]
    ws = ws or ic.EmuWorkspace(K)
    kpad = ic.ceil64(K)
    A2 = torch.full((M, kpad), ic.NAN, dtype=torch.bfloat16)
    B2 = torch.full((N, kpad), ic.NAN, dtype=torch.bfloat16)
    XQ, sx, mask = ic.emu_prepare(x, wq, wscale, ws, A2, B2, mut=mut)
    mask8 = torch.from_numpy(np.packbits(mask.numpy().reshape(K // 8, 8), axis=1, bitorder="little").reshape(-1).copy())
    return dict(meta=ws.meta, idx=ws.idx, sx=sx, XQ=XQ, A2=A2, B2=B2, mask8=mask8)


@pytest.fixture(scope="module")
def prep():
    """name -> (x, wq, wscale, ref_prepare), computed once"""
    out = {}
    for c in ic.PREPARE:
        x = c.build()
        wq, wscale, _ = ic.ref_quant_rows(_w_for(c))
        out[c.name] = (x, wq, wscale, ic.ref_prepare(x, wq, wscale))
    return out


@pytest.fixture(scope="module")
def lin():
    """name -> (x, operands, ref_linear), computed once"""
    out = {}
    for c in ic.LINEAR:
        x, o = c.build(), ic.lin_operands(c)
        out[c.name] = (x, o, ic.ref_linear(x, o["wq"], o["wscale"], a2=o["a2"], b2=o["b2"], residual=o["residual"], alpha=c.alpha))
    return out


def _emu_lin(c, x, o, mut=()):
    return ic.emu_linear(x, o["wq"], o["wscale"], ic.EmuWorkspace(c.K), a2=o["a2"], b2=o["b2"], residual=o["residual"], alpha=c.alpha, mut=mut)


# ------------------------------------------------------------------------------------------------------------- the tables themselves

@pytest.mark.parametrize("case", ic.PREPARE, ids=[c.name for c in ic.PREPARE])
def test_prepare_case_has_the_edge_it_names(case, prep):
    x, _, _, ref = prep[case.name]
    assert x.shape == (case.M, case.K) and x.dtype == torch.bfloat16
    assert ref.n == case.n and ref.n_pad == ic.ceil64(case.n)
    hit = x.float().abs() >= ic.THR
    if case.n and case.name not in ("thr_edges", "row_rules", "m33_k264_nK"):
        per_col = hit.sum(0)
        only = per_col == 1
        assert bool(hit[case.M - 1][only].any())                                     # the only outlier of a column in row M - 1 ...
        assert case.n == 1 or bool(hit[0][only].any())                               # ... and of another in row 0
    if case.n >= 5 and case.n < case.K:
        assert {0, 1, 31, 32, case.K - 1} <= set(ref.cols)
    if case.name.endswith("nK"):
        assert ref.n == case.K and ref.n_pad > case.K and bool((ref.sx == 0).any()) and not bool(ref.XQ.any())
    if case.name == "thr_edges":
        assert ref.cols == [40, 41] and float(ref.sx[case.M // 2]) == float(np.float32(ic.BELOW_THR) / np.float32(127.0))
    if case.name == "row_rules":
        assert ref.cols == [100] and float(ref.sx[3]) == 0.0 and not bool(ref.XQ[3].any())
        assert float(ref.sx[4]) == float(np.float32(5.75) / np.float32(127.0)) and int(ref.XQ[4, 100]) == 0
        for r in (5, 6):
            assert ic.count_ties(x[r:r + 1]) >= 1, r                                  # each tie row has at least one entry decided by the tie rule
        assert ic.count_ties(x[7:8], even=False) >= 1                                 # ... and one that needs the correctly rounded inverse
    if case.name == "m5_k24832_stream":
        ax = x.float().abs()
        counted = torch.where(ax < ic.THR, ax, torch.zeros_like(ax))
        assert bool((counted.argmax(1) >= ic.QCH_K).all()) and max(ref.cols) >= ic.QCH_K
        assert bool((counted[:, :ic.QCH_K].amax(1) < counted.amax(1)).all())


def test_tie_values_exist_for_exact_and_inexact_inverses():
    for a in ic.TIE_ABSMAX:
        t = ic.tie_values(a)
        assert t.size >= 1, a
        inv = np.float32(127.0) / np.float32(a)
        p = (t * inv).astype(np.float32)
        assert bool(np.all(p - np.floor(p) == 0.5))
    assert [float(np.float32(127.0) / np.float32(a)) for a in ic.TIE_ABSMAX] == [32.0, 128.0]
    inv = np.float32(127.0) / np.float32(ic.HALF_ABSMAX)
    assert 127.0 / ic.HALF_ABSMAX != float(inv)                                                    # an inexact inverse ...
    assert float(np.float32(ic.HALF_ABSMAX / 2) * inv) == 63.5                                     # ... whose product is still exactly 63.5
    assert float(np.float32(ic.HALF_ABSMAX / 2) * np.nextafter(inv, np.float32(0))) < 63.5         # and not one ulp lower


@pytest.mark.parametrize("case", ic.WEIGHTS, ids=[c.name for c in ic.WEIGHTS])
def test_weight_reference_equals_the_oracle(case):
    w = case.build()
    assert w.shape == (case.N, case.K)
    q, scale, deq = ic.ref_quant_rows(w)
    cb, scb = I8.quantize_rows_int8(w.float())
    assert torch.equal(q, cb)
    zero = w.float().abs().amax(1) == 0
    want_scale = torch.from_numpy(scb.numpy().astype(np.float32) / np.float32(127.0))
    assert torch.equal(ic.bits32(scale[~zero]), ic.bits32(want_scale[~zero])) and bool((scale[zero] == 0).all())
    assert torch.equal(ic.bits16(deq), ic.bits16(I8.dequantize_rows_int8(cb, torch.where(zero, torch.zeros_like(scb), scb)).to(torch.bfloat16)))
    assert bool(torch.isfinite(deq.float()).all()) and not bool(deq[zero].float().any()) and not bool(q[zero].any())
    if "ties" in case.edge:
        assert ic.count_ties(w, mask_outliers=False) >= 1
    if case.name == "n5_k264_rows":
        assert ic.count_ties(w[4:5], mask_outliers=False, even=False) >= 1
        assert bool(zero[1]) and int(q[2].ne(0).sum()) == 1 and int(q[2, 3]) == -127
    if case.K > ic.QCH_K:
        assert int(w[0].float().abs().argmax()) >= ic.QCH_K


# ------------------------------------------------------------------------------------------------------------- reference against oracle

def _oracle_codes(x, thr=ic.THR):
    """the activation codes as oracle/int8_oracle.py::_MatMul8bitLt.forward forms them"""
    x2 = x.float()
    outlier = (x2.abs() >= thr).any(dim=0)
    sca = x2.abs().masked_fill(x2.abs() >= thr, 0.0).amax(dim=1).clamp_min(1e-30)
    return outlier, sca, I8._codes(x2, sca).masked_fill(outlier[None, :], 0.0)


@pytest.mark.parametrize("case", ic.PREPARE, ids=[c.name for c in ic.PREPARE])
def test_ref_prepare_equals_the_oracle(case, prep):
    x, wq, wscale, ref = prep[case.name]
    outlier, sca, ca = _oracle_codes(x)
    assert ref.cols == outlier.nonzero().flatten().tolist()
    assert torch.equal(ref.XQ.float(), ca)
    live = sca > 1e-30                   # rows without a counted non-zero entry: the kernel writes 0.0 where the oracle clamps to 1e-30
    want_sx = torch.from_numpy(sca.numpy().astype(np.float32) / np.float32(127.0))
    assert torch.equal(ic.bits32(ref.sx[live]), ic.bits32(want_sx[live])) and bool((ref.sx[~live] == 0).all())
    assert ref.idx[:ref.n].tolist() == ref.cols and bool((ref.idx[ref.n:] == -1).all()) and ref.idx.numel() == ref.n_pad
    assert torch.equal(ref.A2[:, :ref.n], x[:, ref.cols]) and not bool(ref.A2[:, ref.n:].float().any())


@pytest.mark.parametrize("case", ic.LINEAR, ids=[c.name for c in ic.LINEAR])
def test_ref_linear_equals_the_oracle(case, lin):
    x, o, ref = lin[case.name]
    w8 = I8.Int8Weight(o["w"].float())
    assert torch.equal(w8.cb, o["wq"])
    y = I8.linear(x.float(), w8).double()
    if case.KP:
        y = y + o["a2"].double() @ o["b2"].double().t()
    y = case.alpha * y
    if case.res:
        y = y + o["residual"].double()
    # The oracle multiplies the outlier columns with the fp32 dequantised weight; the device operand B2 is that weight rounded to bf16
    # (ref_prepare).  Undo that one rounding in the reference, then only the oracle's own fp32 error is left: a K_eff-term fp32
    # product-sum has at most K_eff roundings of 2^-24 relative to the sum of magnitudes S.
    p = ic.ref_prepare(x, o["wq"], o["wscale"])
    exact_b2 = o["wq"][:, p.cols].double() * o["wscale"].double()[:, None]
    want = ref.want + case.alpha * (p.A2[:, :p.n].double() @ (exact_b2 - p.B2[:, :p.n].double()).t())
    bound = 2.0 ** -24 * ref.K_eff * ref.S + 2.0 ** -23 * want.abs()
    assert bool(((y - want).abs() <= bound).all()), float(((y - want).abs() / bound.clamp_min(1e-300)).max())
    # and the rounding of B2 itself (half a bf16 ulp: at most 2^-8 relative) is bounded by the outlier term's magnitudes
    s_out = abs(case.alpha) * (p.A2.double().abs() @ p.B2.double().abs().t())
    assert bool(((want - ref.want).abs() <= 2.0 ** -8 * s_out).all())


# ------------------------------------------------------------------------------------------------------------- emulation against reference

@pytest.mark.parametrize("case", ic.PREPARE, ids=[c.name for c in ic.PREPARE])
def test_emulated_prepare_is_bit_equal_to_the_reference(case, prep):
    x, wq, wscale, ref = prep[case.name]
    got = _run_emu_prepare(x, wq, wscale)
    assert ic.prepare_mismatches(got, ref) == []
    assert bool(torch.isnan(got["A2"][:, ref.n_pad:].float()).all())         # nothing past n_pad is written


@pytest.mark.parametrize("case", ic.LINEAR, ids=[c.name for c in ic.LINEAR])
def test_emulated_linear_passes_the_gpu_comparator(case, lin):
    x, o, ref = lin[case.name]
    rep = gc.measure("bf16", _emu_lin(case, x, o), ref)
    assert rep.ratio <= 1.0, rep.where


def _reuse(mut=(), fresh=False):
    M, N, K = ic.REUSE_LINEAR
    o = ic.lin_operands((M, N, K, 0, False))
    ws = ic.EmuWorkspace(K)
    out = []
    for x in ic.reuse_inputs(M, K):
        if fresh:
            ws = ic.EmuWorkspace(K)
        y = ic.emu_linear(x, o["wq"], o["wscale"], ws, mut=mut)
        out.append((y, ic.ref_linear(x, o["wq"], o["wscale"]), list(ws.meta)))
    return out


def test_emulated_workspace_reuse_equals_fresh_workspaces():
    for (y, ref, meta), (y0, _, meta0), n in zip(_reuse(), _reuse(fresh=True), ic.REUSE_N):
        assert meta == meta0 == [n, ic.ceil64(n)]
        assert torch.equal(ic.bits16(y), ic.bits16(y0))
        rep = gc.measure("bf16", y, ref)
        assert rep.ratio <= 1.0, rep.where


def _pure_int8_case(residual):
    """synthetic codes, no pair: the product has one correctly rounded value per element"""
    g = torch.Generator().manual_seed(77)
    M, N, K = 40, 72, 256
    A8 = torch.randint(-127, 128, (M, K), generator=g).to(torch.int8)
    B8 = torch.randint(-127, 128, (N, K), generator=g).to(torch.int8)
    sa, sb = (0.5 + torch.rand(M, generator=g)) / 127, (0.5 + torch.rand(N, generator=g)) * 0.02 / 127
    res = (torch.randn(M, N, generator=g) * 0.3).to(torch.bfloat16) if residual else None
    return A8, sa, B8, sb, res


def test_emulated_product_holds_the_derived_bound_without_pair():
    A8, sa, B8, sb, _ = _pure_int8_case(False)
    y = ic.emu_product(A8, sa, B8, sb, None, None, 0, alpha=0.5)
    ok, ratio = ic.tight_bound_ok(y, ic.ref_int8(A8, sa, B8, sb, alpha=0.5).want)
    assert ok, ratio


# ------------------------------------------------------------------------------------------------------------- mutants

PREPARE_MUTANTS = {          # mutant -> the prepare cases it must fail, and a product that must be among the wrong ones
    "absmax_counts_outlier_entries": (("m31_k264_n1_last_row", "m33_k264_n63", "m5_k24832_stream"), "sx"),
    "absmax_skips_outlier_columns": (("row_rules",), "sx"),
    "outlier_columns_not_zeroed": (("m31_k264_n1_last_row", "m70_k520_n65", "row_rules"), "XQ"),
    "gt_instead_of_ge": (("thr_edges", "m33_k264_n63"), "idx"),
    "round_half_away_from_zero": (("row_rules",), "XQ"),
    "last_row_skipped_by_column_scan": (("m31_k264_n1_last_row", "m33_k264_n63", "m70_k520_n65", "thr_edges", "m5_k24832_stream"), "idx"),
    "idx_pad_zero": (("m31_k264_n1_last_row", "m33_k264_n63", "m70_k520_n65", "m1_k8_nK", "m33_k264_nK"), "idx"),
    "n_pad_is_n": (("m31_k264_n1_last_row", "m33_k264_n63", "m70_k520_n65", "m1_k8_nK", "m33_k264_nK"), "A2"),
}


@pytest.mark.parametrize("mutant", sorted(PREPARE_MUTANTS))
def test_prepare_mutant_fails_its_named_cases(mutant, prep):
    names, product = PREPARE_MUTANTS[mutant]
    for name in names:
        x, wq, wscale, ref = prep[name]
        bad = ic.prepare_mismatches(_run_emu_prepare(x, wq, wscale, mut=(mutant,)), ref)
        assert any(b.startswith(product) for b in bad) or (product == "idx" and any(b.startswith("meta") for b in bad)), (mutant, name, bad)


def test_round_half_away_also_fails_the_weight_ties():
    for case in ic.WEIGHTS:
        if "ties" not in case.edge:
            continue
        w = case.build()
        q, _, _ = ic.ref_quant_rows(w)
        p = w.float() * ic._f32_div(torch.tensor(127.0), w.float().abs().amax(1).clamp_min(1e-38))[:, None]
        away = (torch.sign(p) * torch.floor(p.abs() + 0.5)).clamp(-127, 127).to(torch.int8)
        assert not torch.equal(away, q), case.name


LINEAR_MUTANTS = {           # mutant -> the linear cases whose element / cell comparison it must fail
    "outlier_columns_not_zeroed": ("m70_n520_k384_n65_lora", "m5_n64_k24832_n3"),
    "idx_pad_zero": ("m70_n520_k384_n65_lora", "m5_n64_k24832_n3"),
    "n_pad_is_n": ("m70_n520_k384_n65_lora", "m5_n64_k24832_n3"),
    "bf16_stage_dropped": ("m70_n520_k384_n65_lora", "m5_n64_k24832_n3"),
    "bf16_stage_doubled": ("m70_n520_k384_n65_lora", "m5_n64_k24832_n3"),
    "k_half_of_a_fragment_dropped": ("m33_n264_k256_n0", "m70_n520_k384_n65_lora"),
    "last_row_skipped_by_column_scan": ("m70_n520_k384_n65_lora",),
    "absmax_counts_outlier_entries": ("m70_n520_k384_n65_lora",),
}


@pytest.mark.parametrize("mutant", sorted(LINEAR_MUTANTS))
def test_linear_mutant_fails_its_named_cases(mutant, lin):
    by_name = {c.name: c for c in ic.LINEAR}
    for name in LINEAR_MUTANTS[mutant]:
        x, o, ref = lin[name]
        rep = gc.measure("bf16", _emu_lin(by_name[name], x, o, mut=(mutant,)), ref)
        assert rep.ratio > 1.0, (mutant, name, rep)


def test_stale_meta_fails_the_reuse_sequence():
    """130 -> 0 -> 1 outlier columns through one workspace: the second call would read 192 columns nobody wrote, the third would drop its one
    outlier column."""
    ratios = [gc.measure("bf16", y, ref).ratio for y, ref, _ in _reuse(mut=("stale_meta",))]
    assert ratios[1] > 1.0 and ratios[2] > 1.0, ratios


def test_residual_before_the_store_fails_bit_equality_without_pair():
    """The element bound grants the residual's operand half an ulp, so both orders pass it; without a pair the product has ONE value, and the
    GPU test compares it bit for bit with emu_product."""
    A8, sa, B8, sb, res = _pure_int8_case(True)
    y = ic.emu_product(A8, sa, B8, sb, None, None, 0, residual=res)
    wrong = ic.emu_product(A8, sa, B8, sb, None, None, 0, residual=res, mut=("residual_before_bf16_store",))
    assert not torch.equal(ic.bits16(y), ic.bits16(wrong))
    assert gc.measure("bf16", y, ic.ref_int8(A8, sa, B8, sb, residual=res)).ratio <= 1.0


def test_every_mutant_is_covered():
    covered = set(PREPARE_MUTANTS) | set(LINEAR_MUTANTS) | {"stale_meta", "residual_before_bf16_store"}
    assert covered == set(ic.MUTANTS)
