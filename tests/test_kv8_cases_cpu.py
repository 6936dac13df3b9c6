"""tests/kv8_cases.py against itself and against plain torch, without a GPU: the restated kv8 quantiser on planted rows, its error bound,
the float64 attention against a torch.softmax formulation, and a float32 emulation of the kernel's order of operations inside the derived
bound on EVERY case - so the case table cannot hide a failure: each case must pass for the reference alone."""
import pytest
import torch

import kv8_cases as kv

F64, U8 = torch.float64, torch.uint8


def _rows():
    g = torch.Generator().manual_seed(3)
    rnd = (torch.randn(4096, kv.D, generator=g).double() * torch.exp2(torch.randint(-30, 31, (4096, 1), generator=g).double())).to(kv.BF)
    return torch.cat((kv.planted(), rnd))


def test_planted_rows_quantise_as_the_format_says():
    R = kv.planted()
    codes, byte = kv.quant(R)
    val = kv.code_values(codes)
    assert byte[0] == 127 and not bool(codes[0].any())                                   # zero row: byte 127, +0 codes, the -0.0 included
    assert byte[1] == 127 - 3 and val[1, 17] == 448.0                                     # maximum exactly 448 * 2^-3: e = -3
    assert byte[2] == 127 - 2 and val[2, 100] == -224.0                                   # just above: e = -2, 450 / 2 = 225 -> 224 (step 16 in [128, 256))
    want3 = [256.0, 0.0, 2 * 2.0 ** -9, -2 * 2.0 ** -9, 16.0, 20.0, -20.0, 1.0, 1.25, -0.0, 0.0, 0.0, 0.0]
    assert byte[3] == 127 and val[3, :len(want3)].tolist() == want3
    assert codes[3, 9] == 0x80 and codes[3, 12] == 0x80 and codes[3, 11] == 0            # signs of zeros are kept in a non-zero row
    assert byte[4] == 0 and bool(codes[4].any())                                          # the clamp at byte 0
    assert byte[5] == 247 and val[5, 64] == 256.0                                         # 1.9921875 * 2^127 / 2^120 = 255 -> 256
    assert byte[7] == 127 - 12 and val[7, 127] == 256.0                                   # a power of two: 2^-4 / 2^-12


def test_scaled_maximum_lies_in_224_448_and_nothing_is_nan():
    R = _rows()
    codes, byte = kv.quant(R)
    assert not bool(((codes & 0x7F) == 0x7F).any())
    m = R.double().abs().amax(-1)
    nz = (m > 0) & (byte > 0)                                                             # byte 0 is the clamp: the scaled maximum may be below 224 there
    sm = m[nz] / torch.exp2(byte[nz].double() - 127)
    assert bool((sm > 224).all()) and bool((sm <= 448).all())
    assert bool((m[byte == 0] / 2.0 ** -127 <= 448).all())


def test_dequant_of_quant_is_within_a_sixteenth_of_the_row_maximum():
    R = _rows()
    codes, byte = kv.quant(R)
    err = (kv.dequant(codes, byte) - R.double()).abs().amax(-1)
    m = R.double().abs().amax(-1)
    assert bool((err <= 2.0 ** -4 * m).all()), float((err / m.clamp_min(1e-300)).max())
    print(f"largest |dequant - v| / row max: {float((err / m.clamp_min(1e-300)).max()):.4f}")


def test_restated_rounding_agrees_with_torch_float8():
    """every bf16 value of [2^-12, 448] and its negative: the restated round-to-nearest-even equals torch's conversion to float8_e4m3fn"""
    bits = torch.arange(0x3980, 0x43E1, dtype=torch.int32).to(torch.int16)              # bf16 2^-12 .. 448
    v = torch.cat((bits.view(kv.BF), -bits.view(kv.BF))).double()
    assert torch.equal(kv.e4m3_rne(v).float(), v.float().to(kv.E4).float())


@pytest.mark.parametrize("c", kv.CASES, ids=[c.name.replace(" ", "_") for c in kv.CASES])
def test_float64_attention_equals_a_plain_softmax(c):
    caches = kv.emulate(c)[1] if c.real else kv.expected_caches(c)
    ref = kv.reference(c, caches)
    q, _ = kv.rotated(c)
    i = kv.inputs(c)
    for b, p in enumerate(c.pos):
        rows = slice(b * kv.MAX_CTX, b * kv.MAX_CTX + p + 1)
        K = kv.dequant(caches["kc"][rows].reshape(p + 1, kv.H, kv.D), caches["ks"][rows])        # [n, H, D], NaN where the filler is
        V = kv.dequant(caches["vc"][rows].reshape(p + 1, kv.H, kv.D), caches["vs"][rows])
        vis = kv.visible(c, b)
        s = kv.SCALE * torch.einsum("nhd,hd->hn", torch.nan_to_num(K, nan=0.0, posinf=0.0, neginf=0.0), q[b])
        s = s.masked_fill(~vis[None], float("-inf"))
        want = torch.einsum("hn,nhd->hd", torch.softmax(s, -1), torch.nan_to_num(V, nan=0.0, posinf=0.0, neginf=0.0)).reshape(-1)
        assert torch.allclose(want, ref.want[b], rtol=1e-10, atol=1e-13), (c.name, b)
        assert i["kmask"] is None or not bool(vis.all())


@pytest.mark.parametrize("c", kv.CASES, ids=[c.name.replace(" ", "_") for c in kv.CASES])
def test_float32_emulation_stays_within_the_bound(c):
    out, caches = kv.emulate(c)
    if c.real:
        kv.check_real_append(c, caches["kc"], caches["ks"])
        ref = kv.reference(c, caches)
    else:
        want = kv.expected_caches(c)
        assert all(torch.equal(caches[k], want[k]) for k in want), c.name
        ref = kv.case_reference(c)
    r = kv.ratio(out, ref)
    print(f"{c.name}: float32 emulation at {r:.4f} x the bound")
    assert r <= 1.0, (c.name, r)


def test_emulated_split_counts_agree_within_twice_the_bound():
    c = kv.CASES[5]
    ref = kv.case_reference(c)
    outs = [kv.emulate(c, ns)[0].double() for ns in (1, 2, 3)]
    for o in outs[1:]:
        assert bool(((o - outs[0]).abs() <= 2 * ref.bound).all())


def test_the_case_table_covers_what_it_claims():
    i = kv.inputs(kv.CASES[7])
    used = i["ks"][i["ks"] != 0xFF]
    assert int(used.min()) <= 104 and int(used.max()) >= 136, (int(used.min()), int(used.max()))
    assert any(c.mask for c in kv.CASES) and any(c.real for c in kv.CASES) and {c.nsplit for c in kv.CASES} == {1, 2, 3}
    for c in kv.CASES:
        i = kv.inputs(c)
        for b, p in enumerate(c.pos):                                    # everything from pos[b] on is NaN filler before the call
            rows = slice(b * kv.MAX_CTX + p, (b + 1) * kv.MAX_CTX)
            assert bool(((i["kc"][rows] & 0x7F) == 0x7F).all()) and bool((i["ks"][rows] == 0xFF).all()) and bool((i["vs"][rows] == 0xFF).all())
