"""Every template instance, grid-stride trip and option of the row-wise kernels (csrc/norm.hip, elementwise.hip, optim.hip, the layout kernels
of pooler.hip, cross-entropy / gather / scatter of text.hip) against the float64 references of tests/rowwise_cases.py, element by element.

The cases are rowwise_cases.CASES: the smallest shapes that reach each cell of rowwise_cases.paths (not the workload's shapes).  Inputs are
seeded; every strided input carries NaN in the columns the kernel must not read (vectors: NaN past their end, RoPE tables: NaN in the rows of
unused positions); every output lies inside a larger buffer prefilled with a sentinel bit pattern (0xFFFF / 0xFFFFFFFF, NaNs no kernel
computes) that must come back unchanged: pad columns, rows beyond `rows`, the elements around a vector slice.  References are computed in
float64 on the device.  Layout kernels and the casts are compared bit for bit (torch.equal), arithmetic kernels by rowwise_cases.check.

Dropout: element indices beyond 2^32 (the high word of drop_keep's counter) would need an 8 GB activation and are not run here; the
restatement of that word is pinned on the CPU (tests/test_gemm_cases_cpu.py)."""
import pytest
import torch

from lhrs_bot_amd import _lib
from lhrs_bot_amd import kernels as hk

import rowwise_cases as rc

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
SENT = -1
BF, F32 = torch.bfloat16, torch.float32
_INT = {BF: torch.int16, F32: torch.int32, torch.uint8: torch.int8}


def L():
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def dev(t):
    return None if t is None else t.to(DEV)


def nanpad(t, pad=8, off=0):
    """[rows, cols] -> the same values as a view at column `off` of a [rows, cols + pad] device buffer that holds NaN elsewhere"""
    rows, cols = t.shape
    buf = torch.full((rows, cols + pad), NAN, dtype=t.dtype)
    buf[:, off:off + cols] = t
    return buf.to(DEV)[:, off:off + cols]


def nanvec(t, pad=8):
    buf = torch.full((t.numel() + pad,), NAN, dtype=t.dtype)
    buf[:t.numel()] = t
    return buf.to(DEV)[:t.numel()]


def sent_buf(rows, cols, dtype=BF, pad=8, extra=3):
    """sentinel buffer [rows + extra, cols + pad] and its [rows, cols] view"""
    buf = torch.full((rows + extra, cols + pad), SENT, dtype=_INT[dtype], device=DEV).view(dtype)
    return buf, buf[:rows, :cols]


def sent_vec(n, dtype=F32, off=4, pad=8):
    buf = torch.full((n + off + pad,), SENT, dtype=_INT[dtype], device=DEV).view(dtype)
    return buf, buf[off:off + n]


def untouched(buf, view, what):
    """every element of buf outside view (a basic slice of it) still holds the sentinel"""
    b = buf.view(_INT[buf.dtype])
    mark = torch.zeros(b.shape, dtype=torch.bool, device=DEV)
    esz = buf.element_size()
    o = (view.data_ptr() - buf.data_ptr()) // esz
    if buf.dim() == 1:
        mark[o:o + view.numel()] = True
    else:
        r0, c0 = divmod(o, buf.stride(0))
        mark[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = True
    assert bool((b[~mark] == SENT).all()), f"{what}: an element outside the result was written"


def ok(st, what):
    _lib.check(st, what)


def chk(c, kind, got, ref, what=""):
    return rc.check(kind, got, ref, c.op, c.name + (" " + what if what else ""))


# ------------------------------------------------------------------------------------------------------------------------- norms
def run_layernorm_fwd(c):
    i, (rows, cols), o = rc.norm_inputs(c), (c.shape["rows"], c.shape["cols"]), c.opt
    x = nanpad(i["x"], 8) if o["strided"] else dev(i["x"])
    gamma, beta = nanvec(i["gamma"]), nanvec(i["beta"])
    buf, y = sent_buf(rows, cols, pad=16 if o["strided"] else 0)
    mbuf, mean = sent_vec(rows)
    rbuf, rstd = sent_vec(rows)
    ok(L().lhrs_layernorm_fwd(x.data_ptr(), x.stride(0), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), y.stride(0),
                              ptr(mean) if o["stats"] else None, ptr(rstd) if o["stats"] else None, rows, cols, 1e-5, stream()), "layernorm_fwd")
    ref = rc.ref_layernorm_fwd(x, gamma, beta, 1e-5)
    chk(c, "ln_y", y, ref["y"])
    untouched(buf, y, c.name)
    if o["stats"]:
        chk(c, "ln_stats", mean, ref["mean"], "mean")
        chk(c, "ln_stats", rstd, ref["rstd"], "rstd")
        untouched(mbuf, mean, c.name + " mean")
        untouched(rbuf, rstd, c.name + " rstd")
    else:
        untouched(mbuf, mbuf[:0], c.name + " mean")


def run_layernorm_bwd(c):
    i, (rows, cols), o = rc.norm_inputs(c), (c.shape["rows"], c.shape["cols"]), c.opt
    mean, rstd = (nanvec(t) for t in rc.ln_stats_f32(i))
    pad = 8 if o["strided"] else 0
    x, dy = (nanpad(i["x"], 8), nanpad(i["dy"], 24)) if o["strided"] else (dev(i["x"]), dev(i["dy"]))
    gamma = nanvec(i["gamma"])
    buf = dx = add = None
    if o["need_dx"]:
        buf, dx = sent_buf(rows, cols, pad=pad)
        if o["add"] == "alias":
            dx.copy_(i["add"])
            add = dx
        elif o["add"] == "separate":
            add = nanpad(i["add"], pad) if pad else dev(i["add"])
            assert add.stride(0) == dx.stride(0)
    dgb = dbb = dg = db = part = None
    if o["dgamma"]:
        (dgb, dg), (dbb, db) = sent_vec(cols), sent_vec(cols)
        if o["accumulate"]:
            dg.copy_(i["old"][0])
            db.copy_(i["old"][1])
        part = torch.full((L().lhrs_layernorm_bwd_nblk(rows) * 2 * cols,), NAN, device=DEV, dtype=F32)     # the workspace handed in full of NaN
    ok(L().lhrs_layernorm_bwd(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ptr(add), ptr(dx),
                              dx.stride(0) if dx is not None else 0, ptr(dg), ptr(db), ptr(part), int(o["accumulate"]), rows, cols, stream()), "layernorm_bwd")
    ref = rc.ref_layernorm_bwd(dy, x, gamma, mean, rstd, add=dev(i["add"]) if o["add"] else None, old=[dev(t) for t in i["old"]] if o["accumulate"] else None,
                               need_dx=o["need_dx"], need_dg=o["dgamma"])
    if o["need_dx"]:
        chk(c, "ln_dx", dx, ref["dx"])
        untouched(buf, dx, c.name)
    if o["dgamma"]:
        chk(c, "ln_dgamma", dg, ref["dgamma"], "dgamma")
        chk(c, "ln_dgamma", db, ref["dbeta"], "dbeta")
        untouched(dgb, dg, c.name + " dgamma")
        untouched(dbb, db, c.name + " dbeta")


def run_rmsnorm_fwd(c):
    i, (rows, cols), o = rc.norm_inputs(c), (c.shape["rows"], c.shape["cols"]), c.opt
    x = nanpad(i["x"], 8) if o["strided"] else dev(i["x"])
    w = nanvec(i["gamma"])
    buf, y = sent_buf(rows, cols, pad=16 if o["strided"] else 0)
    rbuf, rstd = sent_vec(rows)
    ok(L().lhrs_rmsnorm_fwd(x.data_ptr(), x.stride(0), w.data_ptr(), y.data_ptr(), y.stride(0), ptr(rstd) if o["rstd"] else None, rows, cols, 1e-5, stream()),
       "rmsnorm_fwd")
    ref = rc.ref_rmsnorm_fwd(x, w, 1e-5)
    chk(c, "rms_y", y, ref["y"])
    untouched(buf, y, c.name)
    if o["rstd"]:
        chk(c, "rms_rstd", rstd, ref["rstd"], "rstd")
    untouched(rbuf, rstd if o["rstd"] else rbuf[:0], c.name + " rstd")


def _quant_rows(y):
    """lhrs_quant_fp8_rows of a contiguous bf16 matrix -> (bytes, scales)"""
    return hk.quant_fp8_rows(y.contiguous())


def run_rmsnorm_fwd_q(c):
    """the bf16 output is bit-identical to the plain entry point, y == NULL is accepted, the e4m3 bytes and scales are bit-identical to
    lhrs_quant_fp8_rows of the bf16 rows, an all-zero row has scale 1"""
    i, (rows, cols), o = rc.norm_inputs(c), (c.shape["rows"], c.shape["cols"]), c.opt
    x, w = nanpad(i["x"], 8), nanvec(i["gamma"])
    plain = hk.rmsnorm_fwd(x, w, out=torch.empty(rows, cols, device=DEV, dtype=BF))
    chk(c, "rms_y", plain, rc.ref_rmsnorm_fwd(x, w, 1e-5)["y"])
    buf, y = sent_buf(rows, cols, pad=16)
    b8, y8 = sent_buf(rows, cols, dtype=torch.uint8, pad=0)
    sbuf, sc = sent_vec(rows)
    ok(L().lhrs_rmsnorm_fwd_q(x.data_ptr(), x.stride(0), w.data_ptr(), ptr(y) if o["y"] else None, y.stride(0) if o["y"] else 0, y8.data_ptr(), sc.data_ptr(),
                              rows, cols, 1e-5, stream()), "rmsnorm_fwd_q")
    if o["y"]:
        assert torch.equal(y, plain), c.name
    untouched(buf, y if o["y"] else buf[:0, :0], c.name)
    q8, qs = _quant_rows(plain)
    assert torch.equal(y8, q8) and torch.equal(sc, qs), c.name
    untouched(b8, y8, c.name + " bytes")
    untouched(sbuf, sc, c.name + " scales")
    zero = (i["x"].float().abs().amax(1) == 0).to(DEV)
    assert bool((sc[zero] == 1.0).all()), c.name


def _rms_bwd_args(c, i):
    rows, cols, o = c.shape["rows"], c.shape["cols"], c.opt
    x, dy0, w = dev(i["x"]), dev(i["dy"]), nanvec(i["gamma"])
    rstd = nanvec(rc.ref_rmsnorm_fwd(i["x"], i["gamma"], 1e-5)["rstd"].want.float()) if o["rstd"] else None
    buf = torch.full((rows + 3, cols), SENT, dtype=torch.int16, device=DEV).view(BF)
    dx, dy, add = buf[:rows], dy0.clone(), None
    if o.get("dy_alias"):
        dx.copy_(dy0)
        dy = dx
    if o["add"] == "alias":
        dx.copy_(i["add"])
        add = dx
    elif o["add"] == "separate":
        add = dev(i["add"])
    ref = rc.ref_rmsnorm_bwd(dy0, x, w, rstd=rstd, add=dev(i["add"]) if o["add"] else None)
    return x, dy, w, rstd, add, buf, dx, ref


def run_rmsnorm_bwd(c):
    """rstd given and NULL: the cases come in pairs over the same inputs, both held to the same reference and bound"""
    i = rc.norm_inputs(c)
    x, dy, w, rstd, add, buf, dx, ref = _rms_bwd_args(c, i)
    got = hk.rmsnorm_bwd(dy, x, w, rstd, add=add, out=dx)
    assert got.data_ptr() == dx.data_ptr()
    chk(c, "rms_dx", dx, ref["dx"])
    untouched(buf, dx, c.name)


def run_rmsnorm_bwd_q(c):
    i = rc.norm_inputs(c)
    x, dy, w, rstd, add, buf, dx, ref = _rms_bwd_args(c, i)
    plain = hk.rmsnorm_bwd(dy, x, w, rstd, add=add)
    got, (d8, sc) = hk.rmsnorm_bwd_q(dy, x, w, rstd, add=add, out=dx)
    chk(c, "rms_dx", dx, ref["dx"])
    assert torch.equal(dx, plain), c.name
    untouched(buf, dx, c.name)
    q8, qs = _quant_rows(plain)
    assert torch.equal(d8, q8) and torch.equal(sc, qs), c.name


# ------------------------------------------------------------------------------------------------------------------------- element-wise
def _rope_run(c, i, x0, pos_ids):
    rows, nheads, D, o = c.shape["rows"], c.shape["nheads"], c.shape["D"], c.opt
    used = torch.zeros(i["cos"].shape[0], dtype=torch.bool)
    used[i["pos"]] = True
    cos_t, sin_t = i["cos"].clone(), i["sin"].clone()
    cos_t[~used], sin_t[~used] = NAN, NAN                                   # rows of positions the call must not read
    buf, x = sent_buf(rows, nheads * D, pad=16 if o.get("strided") else 0)
    x.copy_(x0)
    hk.rope_(x, rows, nheads, D, dev(cos_t), dev(sin_t), 1 if pos_ids else o["pos_mod"], 0 if pos_ids else o.get("pos0", 0), bool(o.get("inverse")),
             pos_ids=dev(i["pos"].to(torch.int32)) if pos_ids else None)
    untouched(buf, x, c.name)
    return x


def run_rope(c):
    i = rc.rope_inputs(c)
    x = _rope_run(c, i, i["x"], bool(c.opt.get("pos_ids")))
    ref = rc.ref_rope(dev(i["x"]), dev(i["cos"]), dev(i["sin"]), dev(i["pos"]), c.shape["nheads"], c.shape["D"], bool(c.opt.get("inverse")))
    chk(c, "rope", x, ref["x"])
    if not c.opt.get("pos_ids") and c.shape["rows"] < 1000:        # the same positions handed in as pos_ids: bit for bit
        assert torch.equal(x, _rope_run(c, i, i["x"], True)), c.name


def run_swiglu_fwd(c):
    i, rows, F = rc.swiglu_inputs(c), c.shape["rows"], c.shape["F"]
    gu = dev(i["gu"])
    buf, act = sent_buf(rows, F, pad=0)
    hk.swiglu_fwd(gu, F, out=act)
    chk(c, "swiglu_act", act, rc.ref_swiglu_fwd(gu, F)["act"])
    assert bool(torch.isfinite(act.float()).all())
    untouched(buf, act, c.name)


def run_swiglu_bwd(c):
    i, rows, F = rc.swiglu_inputs(c), c.shape["rows"], c.shape["F"]
    gu0, dact = dev(i["gu"]), dev(i["dact"])
    buf, dgu = sent_buf(rows, 2 * F, pad=0)
    if c.opt.get("alias"):
        dgu.copy_(gu0)
        hk.swiglu_bwd(dact, dgu, F, out=dgu)
    else:
        hk.swiglu_bwd(dact, gu0, F, out=dgu)
    chk(c, "swiglu_dgu", dgu, rc.ref_swiglu_bwd(dact, gu0, F)["dgu"])
    assert bool(torch.isfinite(dgu.float()).all())
    untouched(buf, dgu, c.name)


def run_map(c):
    i, n, o = rc.map_inputs(c), c.shape["n"], c.opt
    a0, b = dev(i["a"]), nanvec(i["b"])
    buf, out = sent_vec(n, dtype=BF, off=8, pad=64)
    a = a0
    if o["alias"]:
        out.copy_(a0)
        a = out
    hk.map_(o["op"], a, b if o["op"] in (1, 2) else None, out=out)
    chk(c, "map", out, rc.ref_map(o["op"], a0, b)["out"])
    untouched(buf, out, c.name)


def run_dropout(c):
    g = torch.Generator().manual_seed(rc.seed_of(c))
    rows, cols, p = c.shape["rows"], c.shape["cols"], c.opt["p"]
    x0 = torch.randn(rows, cols, generator=g).to(BF)
    x = nanpad(x0, 8) if c.opt.get("strided") else dev(x0)
    buf, out = sent_buf(rows, cols, pad=16 if c.opt.get("strided") else 0)
    hk.dropout(x, p, 0x9E3779B97F4A7C15, out=out)                      # the wrapper keeps the low 32 bits of the seed
    want, keep = rc.ref_dropout(x, p, 0x9E3779B97F4A7C15 & 0xFFFFFFFF)
    assert torch.equal(out.view(torch.int16), want.view(torch.int16)), c.name             # bits: dropped elements are +0
    if p == 0:
        assert torch.equal(out.view(torch.int16), x.contiguous().view(torch.int16))
    else:
        frac = 1.0 - float(keep.double().mean())
        assert abs(frac - p) < 4 * (p * (1 - p) / keep.numel()) ** 0.5 + 1e-9, (c.name, frac)
    untouched(buf, out, c.name)


def run_colsum(c):
    rows, cols, o = c.shape["rows"], c.shape["cols"], c.opt
    x0, old = rc.mat_inputs(c, rows, cols)
    x = nanpad(x0, 8, off=3) if o["strided"] else dev(x0)                # a column slice of a wider matrix
    buf, out = sent_vec(cols)                                            # a slice of a longer vector
    if o["accumulate"]:
        out.copy_(old)
    hk.colsum(x, out, accumulate=o["accumulate"])
    chk(c, "colsum", out, rc.ref_colsum(x, dev(old) if o["accumulate"] else None)["out"])
    untouched(buf, out, c.name)


def run_transpose(c):
    rows, cols, rp, extra = (c.shape[k] for k in ("rows", "cols", "rows_pad", "extra"))
    x0, _ = rc.mat_inputs(c, rows, cols)
    x = nanpad(x0, 8)
    buf, out = sent_buf(cols, rp, pad=extra)
    hk.transpose(x, rows_pad=rp, out=out)
    assert torch.equal(out[:, :rows], x.t()) and bool((out[:, rows:].view(torch.int16) == 0).all()), c.name
    untouched(buf, out, c.name)


def run_transpose_batched(c):
    pairs, bufs = [], []
    for k, (r, cc) in enumerate(c.shape["shapes"]):
        g = torch.Generator().manual_seed(rc.seed_of(c) + k)
        src = nanpad(torch.randn(r, cc, generator=g).to(BF), 8)
        buf, dst = sent_buf(cc, r, pad=8)
        pairs.append((src, dst))
        bufs.append(buf)
    hk.BatchedTranspose(pairs).run()
    for (src, dst), buf in zip(pairs, bufs):
        assert torch.equal(dst, src.t()), (c.name, tuple(src.shape))
        untouched(buf, dst, c.name)


def _bits32(v):
    return torch.tensor([x - (1 << 32) if x >= 2 ** 31 else x for x in v], dtype=torch.int32).view(F32)


def run_cast_f32_bf16(c):
    """round to nearest even: exact ties to the even and the odd side, NaN, +-inf, subnormals, the largest finite fp32 (rounds up to inf)"""
    n = c.shape["n"]
    g = torch.Generator().manual_seed(rc.seed_of(c))
    x = torch.randn(n, generator=g) * 10
    special = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F800000, 0xFF800000,
               0x7FC00000, 0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80018000, 0x00000000, 0x80000000]
    want_bits = [0x3F80, 0x3F82, 0x3F81, 0x3F80, 0xBF80, 0xBF82, 0x7F80, 0xFF80, 0x7F80, 0x7F80, 0xFF80,
                 None, 0x0000, 0x0000, 0x0002, 0x0080, 0x8002, 0x0000, 0x8000]
    x[:len(special)] = _bits32(special)
    src = nanvec(x)
    buf, out = sent_vec(n, dtype=BF, off=8)
    hk.cast_f32_to_bf16(src, out=out)
    got = out.view(torch.int16).cpu().to(torch.int32) & 0xFFFF
    for k, wb in enumerate(want_bits):
        if wb is None:
            assert bool(torch.isnan(out[k]))
        else:
            assert int(got[k]) == wb, (hex(special[k]), hex(int(got[k])), hex(wb))
    assert torch.equal(out[len(special):].cpu(), x[len(special):].to(BF))
    untouched(buf, out, c.name)


def run_cast_bf16_f32(c):
    n = c.shape["n"]
    bits = (torch.arange(n, dtype=torch.int32) * 64 + 1).to(torch.int16)            # every exponent, subnormals, infs and NaNs among them
    src = bits.view(BF).to(DEV)
    buf, out = sent_vec(n, dtype=F32)
    ok(L().lhrs_cast_bf16_to_f32(src.data_ptr(), out.data_ptr(), n, stream()), "cast_bf16_to_f32")
    assert torch.equal(out.view(torch.int32), src.view(torch.int16).to(torch.int32) << 16), c.name                  # exact: the bits, shifted
    untouched(buf, out, c.name)


def run_patchify(c):
    B, img, P, KP = (c.shape[k] for k in ("B", "img", "P", "KP"))
    g = torch.Generator().manual_seed(rc.seed_of(c))
    rgb = torch.randn(B, 3, img, img, generator=g).to(DEV)
    out = hk.patchify(rgb, P, KP)
    GP, K = img // P, 3 * P * P
    want = rgb.reshape(B, 3, GP, P, GP, P).permute(0, 2, 4, 1, 3, 5).reshape(B * GP * GP, K).to(BF)
    assert out.shape == (B * GP * GP, KP) and torch.equal(out[:, :K], want) and bool((out[:, K:].view(torch.int16) == 0).all())


def run_vit_assemble(c):
    i, s = rc.assemble_inputs(c), c.shape
    patch, cls, pos = nanvec(i["patch"].reshape(-1)).reshape(i["patch"].shape), nanvec(i["cls"]), nanvec(i["pos"].reshape(-1)).reshape(i["pos"].shape)
    rows = s["B"] * (s["NP"] + 1)
    buf, out = sent_buf(rows, s["dim"], pad=0)
    ok(L().lhrs_vit_assemble(patch.data_ptr(), cls.data_ptr(), pos.data_ptr(), out.data_ptr(), s["B"], s["NP"], s["dim"], stream()), "vit_assemble")
    chk(c, "assemble", out, rc.ref_assemble(patch, cls, pos, s["B"], s["NP"])["out"])
    untouched(buf, out, c.name)


def run_gather_rows(c):
    n, sr, dim = c.shape["n"], c.shape["src_rows"], c.shape["dim"]
    src0, _ = rc.mat_inputs(c, sr, dim)
    src = nanpad(src0, 8)
    idx = torch.tensor([(3 * k) % sr for k in range(n)], dtype=torch.int32)          # repeats: n > src_rows
    buf, out = sent_buf(n, dim, pad=16)
    hk.gather_rows(src, dev(idx), out=out)
    assert torch.equal(out, src[idx.long().to(DEV)]), c.name
    untouched(buf, out, c.name)


def run_scatter_rows(c):
    n, dr, dim = c.shape["n"], c.shape["dst_rows"], c.shape["dim"]
    src0, _ = rc.mat_inputs(c, n, dim)
    src = nanpad(src0, 8)
    idx = torch.tensor([(5 * k + 2) % dr for k in range(n)], dtype=torch.int32)      # 5 and 13 coprime: no repeats
    assert len(set(idx.tolist())) == n
    buf, dst = sent_buf(dr, dim, pad=16)
    hk.scatter_rows(src, dev(idx), dst)
    assert torch.equal(dst[idx.long().to(DEV)], src), c.name
    keep = torch.ones(dr, dtype=torch.bool)
    keep[idx.long()] = False
    assert bool((dst[keep.to(DEV)].view(torch.int16) == SENT).all()), c.name             # untouched rows keep the sentinel
    untouched(buf, dst, c.name)


# ------------------------------------------------------------------------------------------------------------------------- pooler layout
def run_pooler_build(c):
    s = c.shape
    nq, ni, dim, B = s["nq"], s["ni"], s["dim"], s["B"]
    NQ, NI = sum(nq), sum(ni)
    g = torch.Generator().manual_seed(rc.seed_of(c))
    query, img = dev(torch.randn(NQ, dim, generator=g).to(BF)), dev(torch.randn(B * NI, dim, generator=g).to(BF))
    tb, t = sent_buf(B * NQ, dim, pad=0)
    kb, kv = sent_buf(B * (NQ + NI), dim, pad=0)
    ok(L().lhrs_pooler_build(query.data_ptr(), img.data_ptr(), t.data_ptr(), kv.data_ptr(), B, *nq, *ni, dim, stream()), "pooler_build")
    wt, wkv = rc.ref_pooler_build(query, img, B, nq, ni)
    assert torch.equal(t, wt) and torch.equal(kv, wkv), c.name
    untouched(tb, t, c.name + " t")
    untouched(kb, kv, c.name + " kv")


def run_pooler_query_grad(c):
    s, o = c.shape, c.opt
    i = rc.qgrad_inputs(c)
    dt0, dkv = dev(i["dt0"]), dev(i["dkv"]) if o["dkv"] else None
    NQ = sum(s["nq"])
    buf, dq = sent_buf(NQ, s["dim"], dtype=F32, pad=0)
    if o["accumulate"]:
        dq.copy_(i["old"])
    hk.pooler_query_grad(dt0, dkv, dq, s["B"], s["nq"], s["ni"], accumulate=o["accumulate"])
    chk(c, "qgrad", dq, rc.ref_query_grad(dt0, dkv, s["B"], s["nq"], s["ni"], dev(i["old"]) if o["accumulate"] else None)["out"])
    untouched(buf, dq, c.name)


# ------------------------------------------------------------------------------------------------------------------------- loss
def _ce_call(x, t, dl, n, V):
    rb, row = sent_vec(n)
    lb, loss = sent_vec(1)
    ok(L().lhrs_cross_entropy(x.data_ptr(), x.stride(0), t.data_ptr(), row.data_ptr(), loss.data_ptr(), ptr(dl), dl.stride(0) if dl is not None else 0, n, V,
                              stream()), "cross_entropy")
    untouched(rb, row, "ce row_loss")
    untouched(lb, loss, "ce loss")
    return row, loss


def run_ce(c):
    """preconditions of lhrs_cross_entropy (its header comment): finite rows, 0 <= target < V - nothing else is fed here"""
    i, n, V, o = rc.ce_inputs(c), c.shape["n"], c.shape["V"], c.opt
    pad = 8 if o["strided"] else 0
    full = torch.full((n, V + pad), NAN, dtype=BF)
    full[:, :V] = i["x"]
    full = full.to(DEV)
    x, t = full[:, :V], dev(i["t"])
    before = full.view(torch.int16).clone()
    ref = rc.ref_ce(dev(i["x"]), t)
    if not o["grad"]:
        row, loss = _ce_call(x, t, None, n, V)
        assert torch.equal(full.view(torch.int16), before), c.name
    elif o["inplace"]:
        row, loss = _ce_call(x, t, x, n, V)
        chk(c, "ce_grad", x, ref["grad"], "grad")
        assert torch.equal(full.view(torch.int16)[:, V:], before[:, V:]), c.name                         # the pad columns: neither read nor written
    else:
        buf, dl = sent_buf(n, V, pad=16)
        row, loss = _ce_call(x, t, dl, n, V)
        assert torch.equal(full.view(torch.int16), before), c.name
        chk(c, "ce_grad", dl, ref["grad"], "grad")
        untouched(buf, dl, c.name)
        row2, loss2 = _ce_call(x, t, x, n, V)                                                            # in place: the same bits
        assert torch.equal(x, dl) and torch.equal(row2, row) and torch.equal(loss2, loss), c.name
    chk(c, "ce_loss", row, ref["row_loss"], "row_loss")
    chk(c, "ce_loss", loss, ref["loss"], "loss")


# ------------------------------------------------------------------------------------------------------------------------- optimizer
def run_sqnorm(c):
    i, n, o = rc.sqnorm_inputs(c), c.shape["n"], c.opt
    g = nanvec(i["g"])
    buf, out = sent_vec(1)
    if o["accumulate"]:
        out.copy_(i["old"])
    hk.sqnorm(g, out, accumulate=o["accumulate"])
    chk(c, "sqnorm", out, rc.ref_sqnorm(g, dev(i["old"]) if o["accumulate"] else None)["out"])
    untouched(buf, out, c.name)


def run_accum_f32(c):
    n, copy = c.shape["n"], c.opt["copy"]
    g = torch.Generator().manual_seed(rc.seed_of(c))
    x, y0 = nanvec(torch.randn(n, generator=g)), dev(torch.randn(n, generator=g) * 100)
    buf, y = sent_vec(n)
    y.copy_(y0)
    hk.accum_f32(y, x, copy_only=copy)
    assert torch.equal(y, x if copy else y0 + x), c.name                  # one IEEE fp32 add per element: torch's own
    untouched(buf, y, c.name)


def run_opt(c):
    """four steps; before each the state is cloned, the reference advances THAT state by one step in float64 and every state array is compared"""
    i, n, o = rc.opt_inputs(c), c.shape["n"], c.opt
    adan = c.op == "adan"
    names = ("p", "m", "v", "n", "pre") if adan else ("p", "m", "v")
    bufs = {k: sent_vec(n) for k in names}
    st = {k: v for k, (_, v) in bufs.items()}
    st["p"].copy_(i["p"])
    for k in names[1:]:
        st[k].zero_()
    sb, shadow = sent_vec(n, dtype=BF, off=8) if o["shadow"] else (None, None)
    gn = torch.empty(1, device=DEV, dtype=F32)
    for step, g0 in enumerate(i["grads"], 1):
        g = nanvec(g0)
        if o["clip"]:
            hk.sqnorm(g, gn)
        prev = {k: st[k].clone() for k in names}
        if adan and step == 1:
            prev["pre"] = None
        kw = dict(eps=rc.OPT_EPS, wd=o["wd"], gnorm_sq=gn if o["clip"] else None, max_norm=o["max_norm"], grad_scale=o["grad_scale"])
        if adan:
            hk.adan_step(st["p"], g, st["m"], st["v"], st["n"], st["pre"], shadow, step, rc.OPT_LR, betas=rc.ADAN_BETAS, no_prox=o["no_prox"], **kw)
            ref = rc.ref_adan(prev, g, step, **rc.opt_args(c))
        else:
            hk.adamw_step(st["p"], g, st["m"], st["v"], shadow, step, rc.OPT_LR, betas=rc.ADAMW_BETAS, **kw)
            ref = rc.ref_adamw(prev, g, step, **rc.opt_args(c))
        for k in names:
            chk(c, c.op, st[k], ref[k], f"step {step} {k}")
            untouched(bufs[k][0], st[k], f"{c.name} {k}")
        if shadow is not None:
            assert torch.equal(shadow, st["p"].to(BF)), (c.name, step)
            untouched(sb, shadow, c.name + " shadow")
    if o["clip"] and o["max_norm"] > 0:                    # the clip was off, on, off, off: ||g|| * grad_scale = 0.3, 30, 0.3, 0.3 against max_norm 1
        norms = [float(g0.double().norm()) * o["grad_scale"] for g0 in i["grads"]]
        assert [x > o["max_norm"] for x in norms] == [False, True, False, False], norms


RUNNERS = dict(layernorm_fwd=run_layernorm_fwd, layernorm_bwd=run_layernorm_bwd, rmsnorm_fwd=run_rmsnorm_fwd, rmsnorm_fwd_q=run_rmsnorm_fwd_q,
               rmsnorm_bwd=run_rmsnorm_bwd, rmsnorm_bwd_q=run_rmsnorm_bwd_q, rope=run_rope, swiglu_fwd=run_swiglu_fwd, swiglu_bwd=run_swiglu_bwd, map=run_map,
               dropout=run_dropout, colsum=run_colsum, transpose=run_transpose, transpose_batched=run_transpose_batched, cast_f32_bf16=run_cast_f32_bf16,
               cast_bf16_f32=run_cast_bf16_f32, patchify=run_patchify, vit_assemble=run_vit_assemble, gather_rows=run_gather_rows, scatter_rows=run_scatter_rows,
               pooler_build=run_pooler_build, pooler_query_grad=run_pooler_query_grad, ce=run_ce, sqnorm=run_sqnorm, accum_f32=run_accum_f32, adan=run_opt,
               adamw=run_opt)


@pytest.mark.parametrize("op", sorted(RUNNERS))
def test_rowwise_cases(op):
    cases = rc.cases_of(op)
    assert cases, op
    for c in cases:
        RUNNERS[op](c)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------- rejections
def test_map_rejects_unknown_op_and_ragged_n():
    a = torch.zeros(16, device=DEV, dtype=BF)
    with pytest.raises(RuntimeError, match="unknown op 7"):
        hk.map_(7, a)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        _lib.check(L().lhrs_map(0, a.data_ptr(), None, a.data_ptr(), 12, stream()), "map")


def test_norm_backward_wrappers_assert_the_strides_the_kernels_assume():
    """layernorm_bwd reads `add` with dx's row stride; rmsnorm_bwd(_q) read `add` and write `out` with row stride cols"""
    rows, cols = 3, 512
    z = lambda *s, dt=BF: torch.zeros(*s, device=DEV, dtype=dt)
    x, dy, w, st = z(rows, cols), z(rows, cols), z(cols), z(rows, dt=F32)
    wide = z(rows, cols + 8)[:, :cols]
    with pytest.raises(AssertionError, match="row stride"):
        hk.layernorm_bwd(dy, x, w, st, st, add=wide)
    hk.layernorm_bwd(dy, x, w, st, st, add=wide, out=z(rows, cols + 8)[:, :cols])
    for fn in (hk.rmsnorm_bwd, hk.rmsnorm_bwd_q):
        with pytest.raises(AssertionError, match="row stride"):
            fn(dy, x, w, add=wide)
        with pytest.raises(AssertionError, match="row stride"):
            fn(dy, x, w, out=wide)
        fn(dy, x, w, add=x, out=z(rows, cols))
    torch.cuda.synchronize()


def test_rowwise_table_reaches_every_cell():
    """The union of the cells of the cases that have a runner equals rowwise_cases.paths; prints the worst kernel / (bound at c = 1) ratios
    of this process next to the constants."""
    print("\nrow-wise worst |err| / (bound at c = 1) on this device, and c:", {k: (round(v, 4), rc.BOUNDS[k]) for k, v in sorted(rc.WORST.items())})
    reached = set().union(*(rc.cells_of(c.op, c.shape, c.opt) for c in rc.CASES if c.op in RUNNERS))
    assert not rc.paths - reached, sorted(rc.paths - reached)
    assert not reached - rc.paths, sorted(reached - rc.paths)
    assert not {c.op for c in rc.CASES} - set(RUNNERS)
