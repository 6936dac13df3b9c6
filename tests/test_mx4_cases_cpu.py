"""The MXFP4 restatement of tests/mx4_cases.py checked against the format's definition, without a GPU: the quantiser's rounding rules on
random and planted blocks, the tiled index maps as bijections, the wave split, and the float32 emulation of the GEMV against the float64
reference inside the derived bound on every case of the table."""
import pytest
import torch

import mx4_cases as mx

BF, U8 = mx.BF, mx.U8


def _scaled(W, scales):
    """v / 2^(byte - 127) per element, float64"""
    return W.double() / torch.exp2(scales.double() - 127).repeat_interleave(32, 1)


@pytest.mark.parametrize("N,K", [(16, 128), (24, 640), (5, 11008)])
def test_every_code_is_a_nearest_level(N, K):
    W = mx.weight(N, K, seed=N + K)
    codes, scales = mx.quant(W)
    q = _scaled(W, scales)
    lv = mx.levels_of(codes)
    dist = (q.abs().clamp_max(6.0)[..., None] - mx.LEVELS).abs().amin(-1)     # saturating: a value past 6 is nearest to 6
    assert torch.equal((q.abs().clamp_max(6.0) - lv.abs()).abs(), dist)
    assert bool((torch.signbit(lv) == torch.signbit(W.double())).all())
    m = W.double().reshape(N, -1, 32).abs().amax(-1)
    e = scales.double() - 127
    assert bool(((m >= 4 * torch.exp2(e)) & (m < 8 * torch.exp2(e))).all())    # floor(log2 m) - 2 == e
    assert int(scales.max()) < 255


def test_planted_blocks():
    W = mx.planted()
    codes, scales = mx.quant(W)
    c = mx.unpack(codes)
    lv = mx.levels_of(codes)
    # a zero block: byte 127, +0 codes, the -0.0 in it included
    assert int(scales[0, 0]) == 127 and not bool(c[0, :32].any())
    # the outlier fixes the scale; everything 2^10 below it rounds to zero and keeps its sign
    assert int(scales[1, 0]) == 127 + 4 - 2 and float(lv[1, 7]) == 4.0
    rest = torch.arange(32) != 7
    assert bool((lv[1, :32][rest] == 0).all()) and bool((torch.signbit(lv[1, :32]) == torch.signbit(W[1, :32].double())).all())
    assert 0 < int(scales[2, 0]) < 10
    # ties to the even code: .25 -> 0, .75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4
    assert int(scales[3, 0]) == 127
    assert lv[3, :15].tolist() == [4.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, -0.0, -1.0, -1.0, -2.0, -2.0, -4.0, 0.0, 0.5]
    assert c[3, 1:7].tolist() == [0, 2, 2, 4, 4, 6] and c[3, 7:13].tolist() == [8, 10, 10, 12, 12, 14]
    # (6, 8) 2^e saturates; 5 is the tie 4 | 6 -> the even code 4
    assert int(scales[4, 0]) == 127 - 3
    assert lv[4, :8].tolist() == [6.0, -6.0, 6.0, 4.0, -4.0, 6.0, 6.0, 4.0]
    # the sign of a negative value that rounds to zero is kept
    assert c[5, 1:4].tolist() == [8, 8, 8] and float(lv[5, 4]) == 0.0 and int(c[5, 4]) == 0
    # bf16 subnormals: floor(log2 m) - 2 + 127 < 0 clamps to byte 0; the largest finite bf16: byte 252, never 255
    assert int(scales[6, 0]) == 0 and int(scales[7, 0]) == 252
    assert lv[7, :4].tolist() == [6.0, -6.0, 1.0, 0.0]


def test_requantising_the_dequantised_weight_is_the_identity():
    for W in (mx.weight(24, 640, seed=3), mx.planted()):
        codes, scales = mx.quant(W)
        Wd = mx.dequant(codes, scales)
        assert torch.equal(Wd.to(BF).double(), Wd)              # exact in bf16, the clamp at byte 0 included (multiples of 2^-133)
        c2, s2 = mx.quant(Wd.to(BF))
        # a block whose codes are all zero has lost its maximum: it re-quantises as a zero block (byte 127, +0)
        lost = (mx.levels_of(codes).reshape(W.shape[0], -1, 32) == 0).all(-1)
        assert torch.equal(s2[~lost], scales[~lost])
        keep = (~lost).repeat_interleave(16, 1)
        assert torch.equal(c2[keep], codes[keep])
        assert bool((s2[lost] == 127).all())
        assert not bool(lost[:, 1:].any())


@pytest.mark.parametrize("N", [16, 24, 40])
@pytest.mark.parametrize("K", [128, 512, 640, 1152, 4096, 11008])
def test_tiled_maps_are_bijections_onto_the_used_bytes(N, K):
    G, S = mx.groups_of(N), K // 128
    nd = -(-S // 4)
    n = torch.arange(N)[:, None]
    ci = mx.code_byte_index(n, torch.arange(K // 2)[None], K).reshape(-1)
    si = mx.scale_byte_index(n, torch.arange(K // 32)[None], K).reshape(-1)
    assert ci.unique().numel() == ci.numel() and int(ci.min()) >= 0 and int(ci.max()) < G * S * 1024
    assert si.unique().numel() == si.numel() and int(si.min()) >= 0 and int(si.max()) < G * nd * 256
    codes = torch.randint(1, 256, (N, K // 2), dtype=torch.int64).to(U8)
    scales = torch.randint(1, 127, (N, K // 32), dtype=torch.int64).to(U8)
    ct, st = mx.tile(codes, scales, N, K)
    used_c = torch.zeros(ct.numel(), dtype=torch.bool)
    used_c[ci] = True
    used_s = torch.zeros(st.numel(), dtype=torch.bool)
    used_s[si] = True
    assert bool((ct.reshape(-1)[~used_c] == 0).all()) and bool((st.reshape(-1)[~used_s] == 127).all())
    assert int((~used_c).sum()) == (16 * G - N) * K // 2
    assert int((~used_s).sum()) == G * nd * 256 - N * (K // 32)
    # lane (r, g) of a step holds 32 consecutive k of one row, and its scale byte sits at [step / 4][lane][step % 4]
    for row, blk in ((0, 0), (N - 1, K // 32 - 1), (N // 2, (K // 32) // 2)):
        step, g = blk // 4, blk % 4
        lane = row % 16 + 16 * g
        assert torch.equal(ct[row // 16, step, lane], codes[row, blk * 16:blk * 16 + 16])
        assert int(st[row // 16, step // 4, lane, step % 4]) == int(scales[row, blk])


@pytest.mark.parametrize("K", [128, 512, 640, 1152, 4096, 11008])
def test_every_wave_starts_on_a_multiple_of_four_steps(K):
    ws = mx.wave_steps(K)
    assert len(ws) == 8 and ws[0][0] == 0
    covered = [s for b, e in ws for s in range(b, e)]
    assert covered == list(range(K // 128))
    assert all(b % 4 == 0 for b, e in ws if e > b)
    if K == 11008:
        assert [e - b for b, e in ws] == [12] * 7 + [2]


def test_case_table_covers_what_the_gpu_file_promises():
    x8 = [c for c in mx.CASES if c.op == "x8"]
    fu = [c for c in mx.CASES if c.op == "fused"]
    assert {c.B for c in x8} == {1, 3, 5, 16} and {(c.B, c.pro) for c in fu} == {(b, p) for b in (1, 2) for p in (0, 1, 2)}
    for cs in (x8, fu):
        assert {c.K for c in cs} == set(mx.KS) | {11008} and {c.N for c in cs} == set(mx.NS)
        for K in mx.KS:
            assert {(c.f32, c.res) for c in cs if c.K == K} == set(mx.OUT), K
            assert {c.N for c in cs if c.K == K} == set(mx.NS), K
    assert len({c.name for c in mx.CASES}) == len(mx.CASES)


@pytest.mark.parametrize("c", mx.CASES, ids=[c.name.replace(" ", "_") for c in mx.CASES])
def test_emulation_stays_inside_the_bound(c):
    i = mx.inputs(c)
    ref, act, xs = mx.case_reference(c)
    if c.op == "fused":
        assert mx.marked_fraction(act) < mx.MARKED_MAX            # the FLIP allowance touches a handful of activations, not the case
    got = mx.emulate(act.a, xs, i["codes"], i["scales"], i["res"], c.f32)
    w = mx.check(got, ref, "emulation " + c.op + (" f32" if c.f32 else " bf16"), c.name)
    if c.op == "x8":                                              # (one marked activation of a fused batch-1 row excuses the tiny fp32 error of all its outputs)
        assert w > 0 or c.K == 128                                # the reference is float64: a float32 emulation that matches it exactly compares nothing


def test_emulation_worst_ratios():
    """after the cases: what the emulation reached per entry point and output type (c = 1 units; allowed 2)"""
    for k in sorted(mx.WORST):
        if k.startswith("emulation"):
            print(f"WORST {k:22s} {mx.WORST[k]:.3f}")
