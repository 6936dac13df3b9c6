"""CPU-only checks of tests/fp8_base_cases.py: the inputs keep the e4m3 code comparison sharp (few elements within FLIP of a rounding
boundary), every SwiGLU case reaches the branch it is named for, the comparisons of tests/test_fp8_base_paths_gpu.py reject each error
planted into the plain-torch emulations, and the two entry points of csrc/fp8.hip reject what they cannot run (on the host, before any
launch)."""
import pytest
import torch

import fp8_base_cases as fc
import gemm_cases as gc
import gemv_cases as gv

INPUTS = {c.name: fc.swiglu_q_inputs(c) for c in fc.SWIGLU}
IDS = [c.name for c in fc.SWIGLU]


def _out64(c):
    return fc.swiglu_q_ref(c, INPUTS[c.name])[1].want.to(fc.BF)


# ------------------------------------------------------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize("c", fc.SWIGLU, ids=IDS)
def test_border_share_of_every_swiglu_case_stays_under_the_cap(c):
    share = fc.border_share(c, INPUTS[c.name])
    print(f"\n{c.name}: {100 * share:.4f} % of the elements within FLIP of an e4m3 rounding boundary")
    assert share <= fc.BORDER_CAP, (c.name, share)


@pytest.mark.parametrize("c", fc.SWIGLU, ids=IDS)
def test_every_swiglu_case_reaches_the_branch_it_is_named_for(c):
    out = _out64(c)
    n, F = out.shape[1], c.F
    assert out.shape[0] == c.rows == len(c.kinds) and F % 16 == 0 and F <= fc.F_MAX
    lo, hi = fc.chunks_per_thread(F)
    nch = F // 8
    held = [len(range(t, nch, 256)) for t in range(256)]                # chunks of thread t: t, t + 256, ...
    assert (min(held), max(held)) == (lo, hi) and hi <= fc.FCH
    a = out.float().abs()
    col = a.argmax(1)
    q = gv.ref_quant(out)
    for r, kind in enumerate(c.kinds):
        m = float(a[r].max())
        if kind == "zero":
            assert m == 0 and float(q.scale[r]) == 1.0 and not bool(q.codes[r].any())
            continue
        assert int((a[r] == m).sum()) == 1, (c.name, r, "the maximum is planted once")
        assert int(out[r, col[r]].view(torch.int16)) & 1, (c.name, r, "the maximum's bf16 significand is odd")
        if kind == "last_chunk":
            assert int(col[r]) >= n - 8                                 # forward: of F, backward: of all 2F columns (the up half)
            assert int(col[r]) % F // 8 % 256 == (nch - 1) % 256        # held by the thread of the last chunk
        if kind == "max_gate":
            assert int(col[r]) < F
        if kind == "max_up":
            assert F <= int(col[r]) < n - 8
        if kind == "dominant":
            val = gv.e4m3_values(q.codes[r]).abs()
            assert float((val < 2.0 ** -6).double().mean()) > 0.9       # subnormal or zero codes
            assert float((val == 0).double().mean()) > 0.25             # below half the smallest subnormal
            assert int((val > 0).sum()) > 8
        if kind == "large":
            assert m > 448 * 64 and fc._above_448(m)
    if c.op == "swiglu_bwd_q":                                           # the gate-half maximum alone would give another scale
        for r, kind in enumerate(c.kinds):
            if kind in ("max_up", "last_chunk"):
                assert float(a[r, :F].max()) < 0.5 * float(a[r].max())


def test_paths_table_is_reached_by_the_case_tables():
    reached = fc.reached()
    assert not fc.paths - reached, sorted(fc.paths - reached)
    assert not reached - fc.paths, sorted(reached - fc.paths)
    for op, variants in (("swiglu_fwd_q", fc.FWD_VARIANTS), ("swiglu_bwd_q", fc.BWD_VARIANTS)):
        shapes = sorted((c.rows, c.F) for c in fc.SWIGLU if c.op == op)
        assert shapes == [(1, 16), (2, 12288), (3, 2048), (3, 11008), (5, 2064)]
        assert all(c.variants == variants for c in fc.SWIGLU if c.op == op)
    assert fc.MODEL["dim"] // fc.MODEL["heads"] == 128 and fc.MODEL["dim"] % 512 == 0 and fc.M_ROWS == 80 and fc.M_ROWS % 64


# ------------------------------------------------------------------------------------------------------------------------- the emulations pass
@pytest.mark.parametrize("c", fc.SWIGLU, ids=IDS)
def test_unmutated_swiglu_emulation_passes_the_gpu_comparisons(c):
    inp = INPUTS[c.name]
    e = fc.emulate_swiglu(c, inp)
    share = fc.compare_swiglu_q(c, inp, e["out"], e["scale"], e["codes"], "emulation")
    assert share <= fc.BORDER_CAP


# ------------------------------------------------------------------------------------------------------------------------- planted errors
def _caught(c, mut):
    inp = INPUTS[c.name]
    e = fc.emulate_swiglu(c, inp, mut)
    try:
        fc.compare_swiglu_q(c, inp, e["out"], e["scale"], e["codes"], mut)
    except AssertionError:
        return True
    return False


def _with(op, *kinds):
    return [c for c in fc.SWIGLU if c.op == op and any(k in c.kinds for k in kinds)]


def test_comparison_catches_truncation_instead_of_rne():
    for c in fc.SWIGLU:
        assert _caught(c, "trunc"), c.name


def test_comparison_catches_missing_saturation_at_448():
    cs = _with("swiglu_fwd_q", "large")
    assert cs
    for c in cs:
        assert _caught(c, "no_sat"), c.name


def test_comparison_catches_backward_scale_over_the_gate_half_only():
    cs = _with("swiglu_bwd_q", "max_up", "last_chunk")
    assert len(cs) == 5
    for c in cs:
        assert _caught(c, "scale_gate_only"), c.name


def test_comparison_catches_scale_0_for_a_zero_row():
    cs = _with("swiglu_fwd_q", "zero") + _with("swiglu_bwd_q", "zero")
    assert len(cs) >= 4
    for c in cs:
        assert _caught(c, "zero_scale_0"), c.name


def test_comparison_catches_the_max_taken_before_the_bf16_rounding():
    """the scale then differs by up to half a bf16 ulp of the maximum, 2^14 fp32 ulps: every case whose maximum is not an exact product"""
    hit = [c.name for c in fc.SWIGLU if _caught(c, "max_before_round")]
    assert len(hit) >= len(fc.SWIGLU) - 2, hit
    assert any(n.startswith("fwd") for n in hit) and any(n.startswith("bwd") for n in hit)


def _lin_caught(o, mut, **kw):
    args = dict(residual=o["residual"], a2=o["a2"], b2=o["b2"])
    args.update(kw)
    y = fc.emu_fp8_linear(o["a8"], o["sa"], o["b8"], o["sb"], mut=mut, **args)
    try:
        fc.check_fp8_gemm(y, o["a8"], o["sa"], o["b8"], o["sb"], what=str(mut), **args)
    except AssertionError:
        return True
    return False


def test_linear_comparison_passes_the_emulation_and_catches_planted_errors():
    o = fc.linear_operands()
    assert not _lin_caught(o, None)
    assert not _lin_caught(o, None, a2=None, b2=None, residual=None)
    assert not _lin_caught(o, None, alpha=0.5)
    for mut in fc.LINEAR_MUTATIONS:
        assert _lin_caught(o, mut), mut
    assert _lin_caught(o, "sa_sb_swapped", a2=None, b2=None, residual=None)


def test_wiring_check_catches_forward_scales_on_transposed_codes():
    """W8's scales used with WT8's codes: the product is wrong per element, but the per-call check (float64 of the call's OWN operands) cannot
    see a wrong operand - the wiring check does"""
    o = fc.linear_operands()
    L = {"w8": o["b8"], "w8s": o["sb"], "wT8": o["bT8"], "wT8s": o["sbT"]}
    fc.check_weight_operand(o["bT8"], o["sbT"], L, "wT")
    fc.check_weight_operand(o["b8"], o["sb"], L, "w")
    assert o["sb"].shape == o["sbT"].shape and not torch.equal(o["sb"], o["sbT"])
    for b8, sb, key in ((o["bT8"], o["sb"], "wT"), (o["b8"], o["sbT"], "w"), (o["b8"], o["sb"], "wT")):
        with pytest.raises(AssertionError):
            fc.check_weight_operand(b8, sb, L, key)
    # and the dequantised product with the wrong scales is far from the right one: the error is not one a tolerance could hide
    y = fc.emu_fp8_linear(o["a8"], o["sa"], o["bT8"], o["sb"])
    with pytest.raises(AssertionError):
        fc.check_fp8_gemm(y, o["a8"], o["sa"], o["bT8"], o["sbT"])


def test_drop_branch_comparisons_pass_the_emulation_and_catch_the_mask_on_the_base_product():
    o = fc.linear_operands()
    p, seed = 0.05, 0x1234ABCD
    U, AT = o["a2"], o["b2"]

    def run(mut):
        base, dx = fc.emu_drop_branch(o["a8"], o["sa"], o["bT8"], o["sbT"], U, AT, p, seed, mut)
        fc.check_fp8_gemm(base, o["a8"], o["sa"], o["bT8"], o["sbT"], what="base")
        gc.check("bf16", dx, fc.ref_dropmask(U, AT, p, seed, base), what="dropmask call")
        gc.check("bf16", dx, fc.ref_drop_branch(o["a8"], o["sa"], o["bT8"], o["sbT"], U, AT, p, seed), what="branch")

    run(None)
    with pytest.raises(AssertionError):
        run("mask_on_base")
    dropped = 1.0 - float((gc.drop_mask(256, 256, seed, p, "cpu") > 0).double().mean())
    assert 0.02 < dropped < 0.09                                           # the mask drops something at these sizes


def test_blockdiag_reference():
    g = torch.arange(1, 1 + 64 * 24, dtype=torch.float32).reshape(64, 24)
    out = fc.ref_blockdiag(g, 8, 8, 0b101)
    assert torch.equal(out[:8, :8], g[:8, :8]) and torch.equal(out[16:24, 16:24], g[16:24, 16:24])
    out[:8, :8] = 0
    out[16:24, 16:24] = 0
    assert not bool(out.any())


# ------------------------------------------------------------------------------------------------------------------------- rejections
def _lib():
    from lhrs_bot_amd import _lib as L
    return L


@pytest.mark.parametrize("bad", fc.SWIGLU_REJECTS, ids=lambda b: f"rows{b['rows']}_F{b['F']}")
def test_swiglu_q_entry_points_reject_on_the_host(bad):
    """F % 16 != 0, F above the 6 x 256 x 8 columns a block keeps in registers, rows = 0: -1 and a message, nothing is launched (the pointers
    are never dereferenced)"""
    L = _lib()
    lib = L.load()
    rows, F = bad["rows"], bad["F"]
    buf = torch.zeros(64, dtype=torch.uint8)
    p = buf.data_ptr()
    st = lib.lhrs_swiglu_fwd_q(p, p, p, p, rows, F, None)
    assert st == -1 and f"swiglu_fwd_q: rows={rows} F={F}".encode() in lib.lhrs_last_error(), lib.lhrs_last_error()
    with pytest.raises(RuntimeError, match="swiglu_fwd_q"):
        L.check(st, "swiglu_fwd_q")
    st = lib.lhrs_swiglu_bwd_q(p, p, p, p, p, rows, F, None)
    assert st == -1 and f"swiglu_bwd_q: rows={rows} F={F}".encode() in lib.lhrs_last_error(), lib.lhrs_last_error()


def test_swiglu_q_entry_points_reject_missing_outputs():
    lib = _lib().load()
    buf = torch.zeros(64, dtype=torch.uint8)
    p = buf.data_ptr()
    assert lib.lhrs_swiglu_fwd_q(p, p, None, p, 1, 16, None) == -1 and lib.lhrs_swiglu_fwd_q(p, p, p, None, 1, 16, None) == -1
    assert lib.lhrs_swiglu_bwd_q(p, p, p, None, p, 1, 16, None) == -1 and lib.lhrs_swiglu_bwd_q(p, p, p, p, None, 1, 16, None) == -1
