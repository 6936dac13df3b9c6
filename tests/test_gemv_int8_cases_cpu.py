"""The tools of tests/gemv_int8_cases.py on the CPU: the plain-torch emulation of the int8 decode GEMV passes every comparison of the GPU
test with a worst ratio of at most 1/4 of the measure() bound (the constants are 4x the emulation's worst ratio against float64, not taken
from the HIP kernel); each named defect fails a named case; the emulated prepare equals int8_cases.ref_prepare bit for bit on every prepare
case; the restated host rules refuse what the library refuses - asked of the library itself, loaded without a GPU: the entry points are
exported and each rejection returns -1 with its message before anything is enqueued."""
import ctypes

import pytest
import torch

import gemv_int8_cases as g8
import int8_cases as ic


@pytest.fixture(scope="module", autouse=True)
def _few_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 4))
    yield
    torch.set_num_threads(n)


def _reuse_reports():
    xs, wq, wscale = g8.reuse_operands()
    ws = g8.EmuWorkspace(g8.REUSE[0], g8.REUSE[2])
    out = []
    for x in xs:
        p, ref = g8.make_ref(x, wq, wscale, None, False)
        XQ, sx = g8.emu_prepare(x, ws)
        assert ws.meta == p.n and torch.equal(XQ, p.XQ)
        out.append(g8.measure("bf16", g8.emu_gemv(XQ, sx, wq, wscale, ws), ref, "reuse", f"n={p.n}"))
    return out


@pytest.fixture(scope="module")
def emu_worst():
    worst = {}
    reps = [(g8.kind_of(c), g8.measure(g8.kind_of(c), g8.emulate(c), g8.reference(c)[1], "emu", c.name)) for c in g8.GEMV + [g8.STRIDED]]
    reps += [("bf16", r) for r in _reuse_reports()]
    for kind, rep in reps:
        if rep.unit >= worst.get(kind, (-1.0, ""))[0]:
            worst[kind] = (rep.unit, rep.where)
    return worst


def test_emulation_passes_every_comparison_of_the_gpu_test():
    for c in g8.GEMV + [g8.STRIDED]:
        assert g8.verdict(c, g8.emulate(c), g8.reference(c)[0]) == [], c.name


def test_constants_are_4x_the_emulation_ratio_written_next_to_them(emu_worst):
    assert set(emu_worst) == set(g8.BOUNDS)
    for kind, (u, where) in sorted(emu_worst.items()):
        print(f"{kind:5s} emulation worst {u:.4g} at c = 1, c = {g8.BOUNDS[kind]:.4g}")
        assert g8.BOUNDS[kind] == 4.0 * g8.EMU_WORST[kind]
        assert u / g8.BOUNDS[kind] <= 0.25, where
        assert 0.9 * g8.EMU_WORST[kind] <= u <= g8.EMU_WORST[kind] * 1.0001, (kind, u, g8.EMU_WORST[kind], where)


# defect -> the GEMV case that must fail with it
GEMV_MUTANT_CASE = {
    "k_half_of_a_fragment_dropped": "b1_n16_k128_n0_f32",
    "outlier_term_dropped": "b3_n40_k1152_n1_res",
    "outlier_term_doubled": "b2_n32_k256_nK",
    "stale_meta": "b5_n64_k1152_n65_res",
    "residual_after_bf16_store": "b5_n64_k1152_n65_res",
    "factor_product_wrong_order": "b1_n16_k128_n0_f32",
}
# defect of the activation side -> the prepare case whose outputs must differ from int8_cases.ref_prepare
PREPARE_MUTANT_CASE = {
    "gt_instead_of_ge": "b3_k1152_thr_edges",
    "absmax_counts_outlier_entries": "b16_k128_row_rules",
    "outlier_columns_not_zeroed": "b3_k1152_cols5",
    "round_half_away_from_zero": "b16_k1152_row_rules",
}


def test_every_named_mutant_has_a_case():
    assert set(GEMV_MUTANT_CASE) | set(PREPARE_MUTANT_CASE) == set(g8.MUTANTS)


@pytest.mark.parametrize("mutant", sorted(GEMV_MUTANT_CASE))
def test_gemv_mutant_fails_its_case(mutant):
    c = {c.name: c for c in g8.GEMV}[GEMV_MUTANT_CASE[mutant]]
    bad = g8.verdict(c, g8.emulate(c, (mutant,)), g8.reference(c)[0])
    print(mutant, "->", bad)
    assert bad, (mutant, c.name)


def _emu_prepared(h, mut=()):
    ws = g8.EmuWorkspace(*h.shape)
    XQ, sx = g8.emu_prepare(h, ws, mut)
    return dict(n=ws.meta, idx=ws.idx, sx=sx, XQ=XQ, xo=ws.xo)


@pytest.mark.parametrize("mutant", sorted(PREPARE_MUTANT_CASE))
def test_prepare_mutant_fails_its_case(mutant):
    c = {c.name: c for c in g8.PREPARE}[PREPARE_MUTANT_CASE[mutant]]
    h = c.build()
    ref = ic.ref_prepare(h, torch.zeros(1, c.K, dtype=torch.int8), torch.zeros(1))
    assert g8.prepare_mismatches(_emu_prepared(h), ref) == []
    bad = g8.prepare_mismatches(_emu_prepared(h, (mutant,)), ref)
    print(mutant, "->", bad)
    assert bad, (mutant, c.name)


@pytest.mark.parametrize("c", g8.PREPARE, ids=[c.name for c in g8.PREPARE])
def test_emulated_prepare_is_the_reference_and_the_case_has_its_edge(c):
    h = c.build()
    ref = ic.ref_prepare(h, torch.zeros(1, c.K, dtype=torch.int8), torch.zeros(1))
    assert ref.n == c.n, (c.name, ref.n)
    assert g8.prepare_mismatches(_emu_prepared(h), ref) == []
    if c.name.endswith("_nK"):
        assert bool((ref.sx == 0).any()) and bool((ref.XQ == 0).all())
    if c.name.endswith("_last_row"):
        assert ref.cols == [c.K - 1] and (c.B == 1 or float(h[:-1].float().abs().max()) < g8.THR)
    if c.name.endswith("_cols5"):
        assert ref.cols == sorted({0, 1, 31, 32, c.K - 1})
    if c.name.endswith("_row_rules"):
        assert ic.count_ties(h) > 0 and float(ref.sx[3]) == 0.0


def test_gemv_cases_have_their_edges():
    by = {c.name: c for c in g8.GEMV}
    for c in g8.GEMV + [g8.STRIDED]:
        p, _ = g8.reference(c)
        assert p.n == c.n and c.K % g8.KSTEP == 0
    assert g8.reference(by["b3_n40_k1152_n1_res"])[0].cols == [1151]
    assert set(g8.reference(by["b5_n64_k1152_n65_res"])[0].cols) >= {0, 1, 63, 64, 127, 128, 1151}
    p = g8.reference(by["b2_n32_k256_nK"])[0]
    assert float(p.sx[1]) == 0.0 and bool((p.XQ == 0).all())
    i, p = g8.inputs(by["b4_n32_k256_n0_zero_rows"]), g8.reference(by["b4_n32_k256_n0_zero_rows"])[0]
    assert float(i["wscale"][5]) == 0.0 and float(p.sx[1]) == 0.0
    assert [e - b for b, e in g8.wave_steps(1152)] == [3, 3, 3, 3, 3, 3, 0, 0] and [e - b for b, e in g8.wave_steps(384)] == [1] * 6 + [0, 0]
    assert [e - b for b, e in g8.wave_steps(11008)] == [22] * 7 + [18]
    for K in (128, 384, 1152, 4096, 11008):
        assert [s for b, e in g8.wave_steps(K) for s in range(b, e)] == list(range(K // 64))
    xs, _, _ = g8.reuse_operands()
    assert tuple(ic.ref_prepare(x, torch.zeros(1, x.shape[1], dtype=torch.int8), torch.zeros(1)).n for x in xs) == ic.REUSE_N


def test_repack_restatement_places_every_byte():
    wq = torch.arange(40 * 128).reshape(40, 128).remainder(251).sub(125).to(torch.int8)
    t = g8.repack(wq)
    assert t.shape == (3, 2, 64, 16)
    for n, k in ((0, 0), (17, 63), (39, 64), (39, 127), (16, 15), (16, 16)):
        assert int(t[n // 16, k // 64, 16 * ((k // 16) & 3) + n % 16, k % 16]) == int(wq[n, k])
    assert bool((t[2, :, [r + 16 * g for g in range(4) for r in range(8, 16)]] == 0).all())      # rows 40..47 do not exist


def test_host_rules_restated():
    for name, (what, kw, _) in g8.REJECTS.items():
        with pytest.raises(g8.Rejected):
            g8.RULES[what](**kw)
    for what, kw in g8.ACCEPTS:
        g8.RULES[what](**kw)


# ------------------------------------------------------------------------------------------------ the library itself, without a GPU
P = 1 << 20          # a 16-byte aligned address nothing dereferences: every call below is refused before anything is enqueued


def _call(lib, what, kw):
    al = kw.get("align", True)
    ptr = P if al else P + 8
    if what == "gemv":
        B, N, K = kw["B"], kw["N"], kw["K"]
        return lib.lhrs_gemv_int8(ptr, kw.get("ldw", K), int(kw.get("packed", False)), P, P, kw.get("ldq", K), P, P, P, P, kw.get("ldo", K), None, 0, P,
                                  kw.get("ldy", N), B, N, K, 0, None)
    if what == "prepare":
        B, K, pro = kw["B"], kw["K"], kw.get("pro", 0)
        return lib.lhrs_int8_decode_prepare(ptr, kw.get("ldx", 2 * K if pro == 2 else K), pro, P if kw.get("norm_w", True) else None, 1e-5,
                                            kw.get("thr", g8.THR), None, 0, P, kw.get("ldq", K), P, P, P, P, kw.get("ldo", K), B, K, None)
    return lib.lhrs_repack_int8_mfma(ptr, kw.get("ldw", kw["K"]), P, kw["N"], kw["K"], None)


def test_library_exports_the_entry_points_and_refuses_bad_shapes():
    from lhrs_bot_amd import _lib

    protos = _lib.parse_header()
    for name in ("lhrs_gemv_int8", "lhrs_int8_decode_prepare", "lhrs_repack_int8_mfma"):
        assert name in protos, name
    lib = _lib.load()
    assert lib.lhrs_gemv_int8.argtypes[-1] is ctypes.c_void_p and len(lib.lhrs_gemv_int8.argtypes) == 20
    for name, (what, kw, msg) in g8.REJECTS.items():
        st = _call(lib, what, kw)
        err = lib.lhrs_last_error().decode()
        assert st == -1 and msg in err, (name, st, err)
