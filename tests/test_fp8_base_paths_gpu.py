"""The e4m3 base (quantize_base(8, "e4m3")) per element, in four parts (tests/fp8_base_cases.py holds the cases, the comparisons and `paths`;
tests/test_fp8_base_cases_cpu.py shows what the comparisons catch):

1. lhrs_swiglu_fwd_q / lhrs_swiglu_bwd_q through the C ABI on sentinel-filled buffers: the bf16 output against float64 (rowwise_cases), codes
   and scales against gemv_cases.ref_quant of that output, NULL and aliased outputs bit-equal to the plain run, nothing written elsewhere.
2. the e4m3 linears of TextModal call by call (_lin, _gu_fwd, _lin_bwd, _down_bwd under three adapter settings) on a small model: the hk
   entry points the base8 path calls are wrapped by recorders (operands cloned before, results after; they replace nothing), every recorded
   call is held per element to float64 of ITS OWN operands, and a restatement of the linear asserts which recorded tensor is which operand.
3. one decoder layer, forward and backward, every row and on the compact last-layer path: every recorded call per element as in 2, and a
   restatement of the HF decoder layer with the quantisation points of DESIGN.md walks the recorded calls and asserts, bit for bit, that
   each operand is the recorded result it must come from and that each product reads the right stored copy of the right weight.  The
   layer's output is NOT compared with a float64 layer: chained quantisation turns one bf16 ulp upstream into another e4m3 code downstream.
4. the stored copies: W8 / WT8 / lm_head8 against ref_quant of the bf16 weights, and again after merge_lora on the merged weights.

Nothing measured here is asserted as a number; the last test prints the worst ratios seen next to the bounds."""
import inspect
from collections import deque, namedtuple

import pytest
import torch

from lhrs_bot_amd import _lib
from lhrs_bot_amd import kernels as hk

import decoder_trace_cases as dc
import fp8_base_cases as fc
import gemm_cases as gc
import rowwise_cases as rc

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -1
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
_INT = {BF: torch.int16, F32: torch.int32, U8: torch.int8}
BORDER = {}          # case / call -> share of elements whose code the reference left open (printed, never asserted here)


def L():
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ok(st, what):
    _lib.check(st, what)


def sent(rows, cols, dtype, pre=2, extra=3):
    """sentinel buffer [pre + rows + extra, cols] and its [rows, cols] view: the rows in front of and behind the result must come back"""
    buf = torch.full((pre + rows + extra, cols), SENT, dtype=_INT[dtype], device=DEV).view(dtype)
    return buf, buf[pre:pre + rows]


def sent_vec(n, off=4, pad=8):
    buf = torch.full((n + off + pad,), SENT, dtype=torch.int32, device=DEV).view(F32)
    return buf, buf[off:off + n]


def untouched(buf, view, what):
    """every element of buf outside view (a row range / slice of it) still holds the sentinel"""
    b = buf.view(_INT[buf.dtype])
    mark = torch.zeros(b.shape, dtype=torch.bool, device=DEV)
    o = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    if buf.dim() == 1:
        mark[o:o + view.numel()] = True
    else:
        r0 = o // buf.stride(0)
        mark[r0:r0 + view.shape[0]] = True
    assert bool((b[~mark] == SENT).all()), f"{what}: an element outside the result was written"


def same(a, b, what):
    """bit for bit (a recorded clone against the tensor it must be); NaNs of never-written rows compare equal to themselves"""
    assert torch.is_tensor(a) and torch.is_tensor(b), what
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}"
    assert torch.equal(a.contiguous().view(U8), b.contiguous().view(U8)), f"{what}: not the same tensor"


# ------------------------------------------------------------------------------------------------------------------------- 1. SwiGLU
def run_swiglu_fwd_q(c):
    inp = fc.swiglu_q_inputs(c)
    rows, F = c.rows, c.F
    gu = inp["gu"].to(DEV)
    gu0 = gu.clone()
    abuf, act = sent(rows, F, BF)
    cbuf, codes = sent(rows, F, U8)
    sbuf, sc = sent_vec(rows)
    ok(L().lhrs_swiglu_fwd_q(gu.data_ptr(), act.data_ptr(), codes.data_ptr(), sc.data_ptr(), rows, F, stream()), c.name)
    BORDER[c.name] = fc.compare_swiglu_q(c, inp, act, sc, codes, "act given")
    for buf, view, what in ((abuf, act, "act"), (cbuf, codes, "codes"), (sbuf, sc, "scales")):
        untouched(buf, view, f"{c.name} {what}")
    assert torch.equal(gu, gu0), c.name
    c2buf, codes2 = sent(rows, F, U8)
    s2buf, sc2 = sent_vec(rows)
    ok(L().lhrs_swiglu_fwd_q(gu.data_ptr(), None, codes2.data_ptr(), sc2.data_ptr(), rows, F, stream()), c.name)           # act == NULL
    assert torch.equal(codes2, codes) and torch.equal(sc2.view(torch.int32), sc.view(torch.int32)), f"{c.name}: act == NULL changes the codes"
    untouched(c2buf, codes2, f"{c.name} codes (NULL)")
    untouched(s2buf, sc2, f"{c.name} scales (NULL)")


def run_swiglu_bwd_q(c):
    inp = fc.swiglu_q_inputs(c)
    rows, F = c.rows, c.F
    gu0, dact = inp["gu"].to(DEV), inp["dact"].to(DEV)
    dact0 = dact.clone()

    def call(gu, dgu):
        cbuf, codes = sent(rows, 2 * F, U8)
        sbuf, sc = sent_vec(rows)
        ok(L().lhrs_swiglu_bwd_q(dact.data_ptr(), gu.data_ptr(), None if dgu is None else dgu.data_ptr(), codes.data_ptr(), sc.data_ptr(), rows, F,
                                 stream()), c.name)
        untouched(cbuf, codes, f"{c.name} codes")
        untouched(sbuf, sc, f"{c.name} scales")
        return codes, sc

    gu = gu0.clone()                                                       # dgu in a buffer of its own: gate_up stays
    dbuf, dgu = sent(rows, 2 * F, BF)
    codes, sc = call(gu, dgu)
    BORDER[c.name] = fc.compare_swiglu_q(c, inp, dgu, sc, codes, "dgu separate")
    untouched(dbuf, dgu, f"{c.name} dgu")
    assert torch.equal(gu, gu0) and torch.equal(dact, dact0), f"{c.name}: an input was written"
    gbuf, gua = sent(rows, 2 * F, BF)                                      # dgu over gate_up, what hk.swiglu_bwd_q(want_bf16=True) does
    gua.copy_(gu0)
    codes_a, sc_a = call(gua, gua)
    assert torch.equal(gua.view(torch.int16), dgu.view(torch.int16)), f"{c.name}: dgu over gate_up differs"
    assert torch.equal(codes_a, codes) and torch.equal(sc_a.view(torch.int32), sc.view(torch.int32)), f"{c.name}: aliasing changes the codes"
    untouched(gbuf, gua, f"{c.name} dgu (alias)")
    codes_n, sc_n = call(gu, None)                                         # dgu == NULL
    assert torch.equal(codes_n, codes) and torch.equal(sc_n.view(torch.int32), sc.view(torch.int32)), f"{c.name}: dgu == NULL changes the codes"
    assert torch.equal(gu, gu0), c.name


@pytest.mark.parametrize("c", fc.SWIGLU, ids=[c.name for c in fc.SWIGLU])
def test_swiglu_q_cases(c):
    (run_swiglu_fwd_q if c.op == "swiglu_fwd_q" else run_swiglu_bwd_q)(c)
    torch.cuda.synchronize()


def test_swiglu_q_wrappers_hand_the_outputs_the_cases_cover():
    """hk.swiglu_fwd_q / hk.swiglu_bwd_q: want_bf16 picks act given / NULL and dgu over gate_up / NULL"""
    c = next(c for c in fc.SWIGLU if c.name == "bwd_5x2064")
    inp = fc.swiglu_q_inputs(c)
    gu, dact = inp["gu"].to(DEV), inp["dact"].to(DEV)
    act, a8, sa = hk.swiglu_fwd_q(gu, c.F, want_bf16=True)
    none, b8, sb = hk.swiglu_fwd_q(gu, c.F)
    assert none is None and torch.equal(a8, b8) and torch.equal(sa, sb)
    rc.check("swiglu_act", act, rc.ref_swiglu_fwd(gu, c.F)["act"], "swiglu_fwd_q", "wrapper")
    fc.check_quant(act, sa, a8, "hk.swiglu_fwd_q")
    g1, g2 = gu.clone(), gu.clone()
    none, d8, sd = hk.swiglu_bwd_q(dact, g1, c.F)
    dgu, e8, se = hk.swiglu_bwd_q(dact, g2, c.F, want_bf16=True)
    assert none is None and torch.equal(g1, gu) and dgu.data_ptr() == g2.data_ptr() and torch.equal(d8, e8) and torch.equal(sd, se)
    fc.compare_swiglu_q(c, inp, dgu, se, e8, "wrapper")


# ------------------------------------------------------------------------------------------------------------------------- recorders
Call = namedtuple("Call", "i name a out after ptr")
LINKS = ("attn_fwd", "attn_bwd_o", "gather_rows", "scatter_rows", "rmsnorm_fwd", "swiglu_fwd")       # recorded for the dataflow only
WRITES = {"rope_": ("x",), "gemm_tn_skinny": ("out",), "blockdiag_mask": ("g",), "attn_fwd": ("o",), "attn_bwd_o": ("dq", "dk", "dv"),
          "scatter_rows": ("dst",)}


def _clone(v):
    if torch.is_tensor(v):
        return v.detach().clone()
    if isinstance(v, (tuple, list)):
        return tuple(_clone(x) for x in v)
    return v


class Recorder:
    """wraps hk entry points: operands are cloned before the call, results (and the arguments a call writes) after it; the call itself is
    the original's"""

    def __init__(self, monkeypatch, names=fc.RECORDED + LINKS):
        self.calls, self.orig = [], {}
        for n in names:
            self.orig[n] = getattr(hk, n)
            monkeypatch.setattr(hk, n, self._wrap(n))

    def _wrap(self, name):
        orig = self.orig[name]
        sig = inspect.signature(orig)

        def rec(*args, **kw):
            b = sig.bind(*args, **kw)
            b.apply_defaults()
            a = {k: _clone(v) for k, v in b.arguments.items()}
            ptr = {k: v.data_ptr() for k, v in b.arguments.items() if torch.is_tensor(v)}
            res = orig(*args, **kw)
            after = {k: _clone(b.arguments[k]) for k in WRITES.get(name, ())}
            self.calls.append(Call(len(self.calls), name, a, _clone(res), after, ptr))
            return res
        return rec


def check_call(c, orig):
    """one recorded call per element against float64 of its own recorded operands"""
    a, n = c.a, c.name
    what = f"call {c.i} {n}"
    if n == "quant_fp8_rows":
        BORDER[what] = fc.check_quant(a["W"], c.out[1], c.out[0], what)
    elif n == "gemm_fp8_nt":
        assert (a["a2"] is None) == (a["b2"] is None), what
        fc.check_fp8_gemm(c.out, a["a8"], a["sa"], a["b8"], a["sb"], a["residual"], a["a2"], a["b2"], a["alpha"], what)
    elif n == "gemm_nt_skinny":
        gc.check("bf16", c.out, gc.ref_nt(a["a"], a["b"], alpha=a["alpha"]), what=what)
    elif n == "gemm_nt_dropmask":
        gc.check("bf16", c.out, fc.ref_dropmask(a["a"], a["b"], a["p"], a["seed"], a["residual"], a["alpha"]), what=what)
    elif n == "gemm_tn_skinny":
        assert not a["accumulate"], what
        gc.check("f32", c.after["out"], gc.ref_tn(a["p"], a["q"]), what=what)
    elif n == "blockdiag_mask":
        same(c.after["g"], fc.ref_blockdiag(a["g"], a["r"], a["w"], a["active_mask"]), what)
    elif n == "dropout":
        same(c.out, rc.ref_dropout(a["x"], a["p"], a["seed"])[0], what)
    elif n == "rope_":
        rows, nh, D = a["rows"], a["nheads"], a["D"]
        assert a["pos_ids"] is None and not a["inverse"] and rows == a["x"].shape[0], what
        pos = torch.arange(rows, device=DEV) % a["pos_mod"] + a["pos0"]
        x0, x1 = a["x"], c.after["x"]
        rc.check("rope", x1[:, :nh * D], rc.ref_rope(x0[:, :nh * D], a["cos_t"], a["sin_t"], pos, nh, D)["x"], n, what)
        same(x1[:, nh * D:], x0[:, nh * D:], what + " (the columns behind the rotated heads)")
    elif n == "rmsnorm_fwd_q":
        y, (y8, sc) = c.out
        plain = orig["rmsnorm_fwd"](a["x"], a["w"], a["eps"])
        rc.check("rms_y", plain, rc.ref_rmsnorm_fwd(a["x"], a["w"], a["eps"])["y"], n, what)
        assert (y is None) == (not a["want_bf16"]), what
        if y is not None:
            same(y, plain, what + " bf16 output")
        BORDER[what] = fc.check_quant(plain, sc, y8, what)
    elif n == "rmsnorm_bwd_q":
        dx, (d8, sc) = c.out
        rc.check("rms_dx", dx, rc.ref_rmsnorm_bwd(a["dy"], a["x"], a["w"], rstd=a["rstd"], add=a["add"], eps=a["eps"])["dx"], n, what)
        BORDER[what] = fc.check_quant(dx, sc, d8, what)
    elif n == "swiglu_fwd_q":
        act, a8, sc = c.out
        full = orig["swiglu_fwd_q"](a["gate_up"], a["F"], want_bf16=True)          # the run WITH the bf16 output
        rc.check("swiglu_act", full[0], rc.ref_swiglu_fwd(a["gate_up"], a["F"])["act"], n, what)
        same(a8, full[1], what + " codes")
        same(sc, full[2], what + " scales")
        assert (act is None) == (not a["want_bf16"]), what
        if act is not None:
            same(act, full[0], what + " bf16 output")
        BORDER[what] = fc.check_quant(full[0], sc, a8, what)
    elif n == "swiglu_bwd_q":
        dgu, d8, sc = c.out
        full = orig["swiglu_bwd_q"](a["dact"], a["gate_up"].clone(), a["F"], want_bf16=True)
        rc.check("swiglu_dgu", full[0], rc.ref_swiglu_bwd(a["dact"], a["gate_up"], a["F"])["dgu"], n, what)
        same(d8, full[1], what + " codes")
        same(sc, full[2], what + " scales")
        assert (dgu is None) == (not a["want_bf16"]), what
        if dgu is not None:
            same(dgu, full[0], what + " bf16 output")
        BORDER[what] = fc.check_quant(full[0], sc, d8, what)
    else:
        raise AssertionError(f"no check for {n}")


def check_calls(rec):
    n = 0
    for c in rec.calls:
        if c.name in fc.RECORDED:
            check_call(c, rec.orig)
            n += 1
    return n


# ------------------------------------------------------------------------------------------------------------------------- the linear, restated
class Walk:
    """Walks the recorded calls (first unconsumed call of a name) along the formulas of the e4m3 linear:
        forward   y  = dq(x8) dq(W8)^T + T Bfull^T (+ residual),  T = s dropout(x) A^T,   x8 the producer's codes or quant_fp8_rows(x)
        backward  dx = dq(dy8) dq(WT8)^T + [mask] U AT^T,         U = s dy BD^T,  dA = U^T dropout(x),  dBD = blockdiag(T^T dy)
    and asserts for every call that each operand IS the recorded tensor it must be."""

    def __init__(self, calls, m):
        self.q = {}
        for c in calls:
            self.q.setdefault(c.name, deque()).append(c)
        self.m, self.L, self.lo = m, m.p["layers"][0], m.lora
        self.T, self.seed = {}, {}

    def nxt(self, name):
        assert self.q.get(name), f"the path made no (further) {name} call"
        return self.q[name].popleft()

    def done(self):
        left = {n: len(q) for n, q in self.q.items() if q}
        assert not left, f"calls nobody accounts for: {left}"

    def has(self, g):
        return self.lo is not None and g in self.lo.groups

    def pd(self):
        return self.lo.active_dropout() if self.lo is not None else 0.0

    def adapter_down(self, g, x):
        lo, xa = self.lo, x
        if self.pd() > 0:
            d = self.nxt("dropout")
            same(d.a["x"], x, f"{g}: dropout input")
            assert d.a["p"] == lo.dropout and d.a["seed"] == lo.seed_for(0, g), g
            xa, self.seed[g] = d.out, d.a["seed"]
        k = self.nxt("gemm_nt_skinny")
        same(k.a["a"], xa, f"{g}: adapter input")
        same(k.a["b"], lo.view(lo.shadow, 0, g, "A"), f"{g}: A")
        assert k.a["alpha"] == lo.s, g
        self.T[g] = k.out
        return k.out

    def lin(self, g, x, xq, residual=None, rope=None):
        T = self.adapter_down(g, x) if self.has(g) else None
        if xq is None:
            qc = self.nxt("quant_fp8_rows")
            same(qc.a["W"], x, f"{g}: the quantised activation")
            xq = qc.out
        p = self.nxt("gemm_fp8_nt")
        same(p.a["a8"], xq[0], f"{g}: a8")
        same(p.a["sa"], xq[1], f"{g}: sa")
        fc.check_weight_operand(p.a["b8"], p.a["sb"], self.L, g + "_w", f"{g} forward")
        assert p.a["alpha"] == 1.0, g
        if residual is None:
            assert p.a["residual"] is None, f"{g}: a residual nobody asked for"
        else:
            same(p.a["residual"], residual, f"{g}: residual")
        if T is None:
            assert p.a["a2"] is None and p.a["b2"] is None, f"{g}: an adapter pair without adapters"
        else:
            same(p.a["a2"], T, f"{g}: a2")
            same(p.a["b2"], self.lo.derived[(0, g, "Bfull")], f"{g}: b2")
        y = p.out
        if rope is not None:
            r = self.nxt("rope_")
            same(r.a["x"], y, f"{g}: RoPE input")
            assert (r.a["rows"], r.a["nheads"], r.a["D"], r.a["pos_mod"], r.a["pos0"]) == (y.shape[0], 2 * self.m.heads, self.m.hd, rope[0], rope[1]), g
            same(r.a["cos_t"], self.m.cos, "cos")
            same(r.a["sin_t"], self.m.sin, "sin")
            y = r.after["x"]
        return y

    def gu_fwd(self, h, hq):
        gu = self.lin("gu", h, hq)
        s = self.nxt("swiglu_fwd_q")
        same(s.a["gate_up"], gu, "SwiGLU input")
        assert s.a["F"] == self.m.ff and s.a["want_bf16"] == self.has("down")
        act, a8, sc = s.out
        return gu, act, (a8, sc)

    def lin_bwd(self, g, dy, dyq, x):
        lo, key = self.lo, g + "_wT"
        if dyq is None:
            qc = self.nxt("quant_fp8_rows")
            same(qc.a["W"], dy, f"{g} backward: the quantised gradient")
            dyq = qc.out
        U = None
        if self.has(g):
            k = self.nxt("gemm_nt_skinny")
            same(k.a["a"], dy, f"{g} backward: U input")
            same(k.a["b"], lo.view(lo.shadow, 0, g, "BD"), f"{g} backward: BD")
            assert k.a["alpha"] == lo.s, g
            U = k.out
        p = self.nxt("gemm_fp8_nt")
        same(p.a["a8"], dyq[0], f"{g} backward: a8")
        same(p.a["sa"], dyq[1], f"{g} backward: sa")
        fc.check_weight_operand(p.a["b8"], p.a["sb"], self.L, key, f"{g} backward")
        assert p.a["alpha"] == 1.0 and p.a["residual"] is None, g
        if U is None:
            assert p.a["a2"] is None and p.a["b2"] is None, g
            return p.out
        G, AT, pd = lo.groups[g], lo.derived[(0, g, "AT")], self.pd()
        if pd > 0:                                                                      # the unfused branch: base in bf16, then the masked pair
            assert p.a["a2"] is None and p.a["b2"] is None, f"{g} backward: the pair must not ride on the base product under dropout"
            dm = self.nxt("gemm_nt_dropmask")
            same(dm.a["a"], U, f"{g} backward: masked pair a")
            same(dm.a["b"], AT, f"{g} backward: masked pair b")
            same(dm.a["residual"], p.out, f"{g} backward: the base product")
            assert dm.a["p"] == lo.dropout and dm.a["seed"] == self.seed[g] and dm.a["alpha"] == 1.0, g
            dx = dm.out
            gc.check("bf16", dx, fc.ref_drop_branch(dyq[0], dyq[1], p.a["b8"], p.a["sb"], U, AT, pd, self.seed[g]), what=f"{g} backward: drop branch")
            d = self.nxt("dropout")
            same(d.a["x"], x, f"{g} backward: dropout input")
            assert d.a["p"] == lo.dropout and d.a["seed"] == self.seed[g], g
            xa = d.out
        else:
            same(p.a["a2"], U, f"{g} backward: a2")
            same(p.a["b2"], AT, f"{g} backward: b2")
            dx, xa = p.out, x
        tA = self.nxt("gemm_tn_skinny")
        same(tA.a["p"], U, f"{g}: dA p")
        same(tA.a["q"], xa, f"{g}: dA q")
        tB = self.nxt("gemm_tn_skinny")
        same(tB.a["p"], self.T[g], f"{g}: dBD p")
        same(tB.a["q"], dy, f"{g}: dBD q")
        bm = self.nxt("blockdiag_mask")
        same(bm.a["g"], tB.after["out"], f"{g}: masked gradient")
        assert (bm.a["r"], bm.a["w"], bm.a["active_mask"]) == (lo.r, G["fout"], G["mask"]), g
        gA, gB = lo.view(lo.grad, 0, g, "A"), lo.view(lo.grad, 0, g, "BD")
        assert tA.ptr["out"] == gA.data_ptr() and tB.ptr["out"] == gB.data_ptr() and bm.ptr["g"] == gB.data_ptr(), f"{g}: gradients outside lora.grad"
        same(gA, tA.after["out"], f"{g}: dA in lora.grad")
        same(gB, bm.after["g"], f"{g}: dBD in lora.grad")
        return dx

    def down_bwd(self, dy, dyq, gu, act):
        dact = self.lin_bwd("down", dy, dyq, act)
        s = self.nxt("swiglu_bwd_q")
        same(s.a["dact"], dact, "SwiGLU' d_act")
        same(s.a["gate_up"], gu, "SwiGLU' gate|up")
        assert s.a["F"] == self.m.ff and s.a["want_bf16"] == self.has("gu")
        dgu, d8, sc = s.out
        return dgu, (d8, sc)


# ------------------------------------------------------------------------------------------------------------------------- the model
make_model = dc.make_model          # the e4m3 base by default; shared with test_decoder_trace_gpu.py


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(setting):
        if setting not in cache:
            cache[setting] = make_model(setting)
        return cache[setting]
    return get


def rnd(seed, rows, cols, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, cols, generator=g) * scale).to(BF).to(DEV)


# ------------------------------------------------------------------------------------------------------------------------- 2. call by call
def _drive(m, rec_factory, cell, opt):
    """-> (rec, walk function): prepares operands with the plain entry points, then runs ONE method of the model under the recorders"""
    Lw, lo, M, d, ff = m.p["layers"][0], m.lora, fc.M_ROWS, m.d, m.ff
    has = lambda g: lo is not None and g in lo.groups
    if cell.startswith("lin_xq") or cell == "gu_fwd":
        g = opt.get("group", "gu")
        x = rnd(21, M, d)
        residual = rnd(22, M, d) if opt.get("residual") else None
        rope = (40, 0) if opt.get("rope") else None
        if cell == "gu_fwd" or opt["xq"]:
            h, hq = hk.rmsnorm_fwd_q(x, Lw["ln1_w"], m.eps)                   # a producer's bf16 output and e4m3 operand
        else:
            h, hq = x, None
        save = {}
        rec = rec_factory()
        if cell == "gu_fwd":
            out = m._gu_fwd(0, h, Lw, save, xq=hq)
        else:
            out = m._lin(0, g, h, Lw, residual=residual, save=save, xq=hq, rope=rope)

        def walk(w):
            if cell == "gu_fwd":
                gu, act, actq = w.gu_fwd(h, hq)
                same(out[0], gu, "gate|up")
                assert (out[1] is None) == (act is None)
                if act is not None:
                    same(out[1], act, "act")
                same(out[2][0], actq[0], "act8")
                same(out[2][1], actq[1], "act scales")
            else:
                same(out, w.lin(g, h, hq, residual, rope), f"{g}: result")
            if has(g):
                same(save["T_" + g], w.T[g], f"{g}: saved T")
                assert save.get("seed_" + g) == w.seed.get(g)
        return rec, walk
    g = opt.get("group", "down")
    fin, fout = (ff, d) if g == "down" else (d, {"qkv": 3 * d, "gu": 2 * ff}[g])
    dy = rnd(31, M, fout, 0.1)
    gu = rnd(32, M, 2 * ff) if g == "down" else None
    x = (hk.swiglu_fwd(gu, ff) if g == "down" else rnd(33, M, fin)) if has(g) else None
    save = {}
    if has(g):                                                            # the forward of this group: T and the dropout seed the backward needs
        m._lin(0, g, x, Lw, save=save)
    dyq = hk.quant_fp8_rows(dy) if (cell == "down_bwd" or opt["dyq"]) else None
    gu0 = None if gu is None else gu.clone()
    rec = rec_factory()
    if cell == "down_bwd":
        out = m._down_bwd(0, dy, Lw, gu, x, save.get("T_down"), dyq=dyq, drop=m._drop(save, "down"))
    else:
        out = m._lin_bwd(0, g, dy, Lw, x, save.get("T_" + g), dyq=dyq, drop=m._drop(save, g))

    def walk(w):
        if has(g):
            w.T[g], w.seed[g] = save["T_" + g], save.get("seed_" + g)
        if cell == "down_bwd":
            dgu, dguq = w.down_bwd(dy, dyq, gu0, x)
            assert (out[0] is None) == (dgu is None)
            if dgu is not None:
                same(out[0], dgu, "dgu")
                assert out[0].data_ptr() == gu.data_ptr()                 # written over gate|up
            same(out[1][0], dguq[0], "dgu8")
            same(out[1][1], dguq[1], "dgu scales")
        else:
            same(out, w.lin_bwd(g, dy, dyq, x), f"{g}: dx")
    return rec, walk


@pytest.mark.parametrize("cell", [c for c, _, _ in fc.LIN_CALLS])
@pytest.mark.parametrize("setting", list(fc.SETTINGS))
def test_e4m3_linear_call_by_call(setting, cell, models, monkeypatch):
    m = models(setting)
    opt = next(o for c, _, o in fc.LIN_CALLS if c == cell)
    rec, walk = _drive(m, lambda: Recorder(monkeypatch), cell, opt)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert check_calls(rec) >= 1
    w = Walk(rec.calls, m)
    walk(w)
    w.done()
    names = [c.name for c in rec.calls]
    drop = setting == "all_drop"
    if cell in ("lin_xq_given_rope", "gu_fwd", "lin_bwd_dyq_given", "down_bwd"):
        assert "quant_fp8_rows" not in names, "a producer handed the e4m3 operand over: nothing is quantised again"
    else:
        assert names.count("quant_fp8_rows") == 1
    g = opt.get("group", "gu" if cell == "gu_fwd" else "down")
    adapted = m.lora is not None and g in m.lora.groups
    assert ("gemm_nt_skinny" in names) == adapted and ("gemm_nt_dropmask" in names) == (adapted and drop and "bwd" in cell)
    assert ("dropout" in names) == (adapted and drop)


# ------------------------------------------------------------------------------------------------------------------------- 3. one layer
def _batch():
    return dc.batch(DEV)


def walk_layer(calls, m, x_in, rows, S):
    """The HF decoder layer (x + o_proj(attn(rope(qkv(norm1 x)))), then + down(silu(gate) up) of norm2) with e4m3 operands emitted by the
    producers (both norms, the SwiGLU and its derivative, both norm backwards) and quantised on the fly behind attention (o, dqkv)."""
    w, d = Walk(calls, m), m.d
    Lw, has = w.L, w.has
    n1 = w.nxt("rmsnorm_fwd_q")
    same(n1.a["x"], x_in, "norm1 input")
    same(n1.a["w"], Lw["ln1_w"], "norm1 weight")
    assert n1.a["eps"] == m.eps and n1.a["want_bf16"] == has("qkv")
    h1, h1q = n1.out
    qkv = w.lin("qkv", h1, h1q, rope=(S, 0))
    at = w.nxt("attn_fwd")
    for k, c0 in (("q", 0), ("k", d), ("v", 2 * d)):
        same(at.a[k], qkv[:, c0:c0 + d], f"attention {k}")
    o_full = at.after["o"]
    if rows is None:
        o, x_res = o_full, x_in
    else:
        g1, g2 = w.nxt("gather_rows"), w.nxt("gather_rows")
        same(g1.a["src"], o_full, "gathered attention rows")
        same(g2.a["src"], x_in, "gathered residual rows")
        same(g1.a["idx"], rows, "tail rows")
        same(g2.a["idx"], rows, "tail rows")
        o, x_res = g1.out, g2.out
        same(o, o_full[rows.long()], "o rows")
        same(x_res, x_in[rows.long()], "x rows")
    x_mid = w.lin("o", o, None, residual=x_res)
    n2 = w.nxt("rmsnorm_fwd_q")
    same(n2.a["x"], x_mid, "norm2 input")
    same(n2.a["w"], Lw["ln2_w"], "norm2 weight")
    assert n2.a["eps"] == m.eps and n2.a["want_bf16"] == has("gu")
    h2, h2q = n2.out
    gu, act, actq = w.gu_fwd(h2, h2q)
    x_out = w.lin("down", act, actq, residual=x_mid)
    fn = w.nxt("rmsnorm_fwd")
    same(fn.a["x"], x_out, "final norm input")
    same(fn.a["w"], m.p["norm_w"], "final norm weight")
    if rows is None:                                                       # every row: the supervised rows are picked behind the final norm
        same(w.nxt("gather_rows").a["src"], fn.out, "rows handed to lm_head")
    # ---- backward
    r0 = w.nxt("rmsnorm_bwd_q")
    if rows is None:
        same(r0.a["dy"], w.nxt("scatter_rows").after["dst"], "d hidden")
    same(r0.a["x"], x_out, "final norm backward x")
    same(r0.a["w"], m.p["norm_w"], "final norm backward weight")
    assert r0.a["add"] is None and r0.a["rstd"] is None and r0.a["eps"] == m.eps
    dx, dxq = r0.out
    act_b = None
    if has("down"):
        sf = w.nxt("swiglu_fwd")
        same(sf.a["gate_up"], gu, "recomputed act input")
        act_b = sf.out
        same(act_b, act, "recomputed act")
    dgu, dguq = w.down_bwd(dx, dxq, gu, act_b)
    h2b = None
    if has("gu"):
        rf = w.nxt("rmsnorm_fwd")
        same(rf.a["x"], x_mid, "recomputed norm2 input")
        same(rf.a["w"], Lw["ln2_w"], "recomputed norm2 weight")
        h2b = rf.out
        same(h2b, h2, "recomputed norm2")
    dh = w.lin_bwd("gu", dgu, dguq, h2b)
    r2 = w.nxt("rmsnorm_bwd_q")
    same(r2.a["dy"], dh, "norm2 backward dy")
    same(r2.a["x"], x_mid, "norm2 backward x")
    same(r2.a["w"], Lw["ln2_w"], "norm2 backward weight")
    same(r2.a["add"], dx, "norm2 backward add: the residual stream's gradient")
    assert r2.a["rstd"] is None and r2.a["eps"] == m.eps
    dx_mid, dmq = r2.out
    do = w.lin_bwd("o", dx_mid, dmq, o if has("o") else None)
    ab = w.nxt("attn_bwd_o")
    add1 = dx_mid
    if rows is None:
        same(ab.a["dout"], do, "attention dO")
    else:
        s1, s2 = w.nxt("scatter_rows"), w.nxt("scatter_rows")
        same(s1.a["src"], do, "scattered dO")
        same(s2.a["src"], dx_mid, "scattered dx_mid")
        same(ab.a["dout"], s1.after["dst"], "attention dO")
        same(ab.a["dout"][rows.long()], do, "attention dO rows")
        add1 = s2.after["dst"]
        want = torch.zeros_like(add1)
        want[rows.long()] = dx_mid
        same(add1, want, "dx_mid scattered into zeros")
    same(ab.a["o"], o_full, "attention backward O")
    for k, c0 in (("q", 0), ("k", d), ("v", 2 * d)):
        same(ab.a[k], qkv[:, c0:c0 + d], f"attention backward {k}")
    dqkv = torch.cat([ab.after["dq"], ab.after["dk"], ab.after["dv"]], 1)
    h1b = None
    if has("qkv"):
        rf = w.nxt("rmsnorm_fwd")
        same(rf.a["x"], x_in, "recomputed norm1 input")
        same(rf.a["w"], Lw["ln1_w"], "recomputed norm1 weight")
        h1b = rf.out
        same(h1b, h1, "recomputed norm1")
    dh1 = w.lin_bwd("qkv", dqkv, None, h1b)
    r1 = w.nxt("rmsnorm_bwd_q")
    same(r1.a["dy"], dh1, "norm1 backward dy")
    same(r1.a["x"], x_in, "norm1 backward x")
    same(r1.a["w"], Lw["ln1_w"], "norm1 backward weight")
    same(r1.a["add"], add1, "norm1 backward add: dx_mid")
    w.done()
    return r1.out[0]


@pytest.mark.parametrize("run", fc.LAYER_RUNS)
@pytest.mark.parametrize("setting", list(fc.SETTINGS))
def test_one_decoder_layer_forward_and_backward(setting, run, models, monkeypatch):
    m = models(setting)
    ids, image, mask, labels = _batch()
    monkeypatch.setattr(m, "tail_rows_only", run == "tail")
    if m.lora is not None:
        m.lora.grad.zero_()
    rec = Recorder(monkeypatch)
    loss = m.decode(ids, image, mask, labels)
    ctx = m._ctx
    x_in = ctx["layers"][0]["x_in"].clone()
    rows = None if ctx["tail"] is None else ctx["tail"][0].clone()
    S = ctx["S"]
    assert (rows is not None) == (run == "tail") and x_in.shape == (2 * S, m.d) and S == 40
    if rows is not None:
        assert rows.tolist() == list(range(24, 39)) + list(range(40 + 19, 40 + 29))
    m.backward(need_input_grad=False)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert bool(torch.isfinite(loss))
    n = check_calls(rec)
    dx = walk_layer(rec.calls, m, x_in, rows, S)
    assert dx.shape == x_in.shape and bool(torch.isfinite(dx.float()).all())
    print(f"\n{setting} / {run}: {n} recorded calls held per element, {len(rec.calls)} walked")


# ------------------------------------------------------------------------------------------------------------------------- 4. stored copies
WEIGHTS = ("qkv_w", "o_w", "gu_w", "down_w")


def check_copies(m, what):
    for Lw in m.p["layers"]:
        for k in WEIGHTS:
            same(Lw[k + "T"], Lw[k].t().contiguous(), f"{what}: {k}T")
            fc.check_quant(Lw[k], Lw[k + "8s"], Lw[k + "8"], f"{what}: {k}8")
            fc.check_quant(Lw[k + "T"], Lw[k + "T8s"], Lw[k + "T8"], f"{what}: {k}T8")
            assert Lw[k + "8"].dtype == U8 and Lw[k + "8s"].shape == (Lw[k].shape[0],) and Lw[k + "T8s"].shape == (Lw[k].shape[1],)
    fc.check_quant(m.p["lm_head"], m.p["lm_head8s"], m.p["lm_head8"], f"{what}: lm_head8")


def test_stored_e4m3_copies_are_the_reference_quantisation_of_the_weights(models):
    m = models("none")
    assert m.base8 and not m.base_int8
    check_copies(m, "quantize_base")


def test_merge_lora_requantises_the_merged_weights():
    m = make_model("qkvo_r8", seed=4)
    lo, Lw = m.lora, m.p["layers"][0]
    before = {k: Lw[k].clone() for k in WEIGHTS}
    codes = {k: (Lw[k + "8"].clone(), Lw[k + "T8"].clone()) for k in WEIGHTS}
    pairs = {g: (lo.derived[(0, g, "Bfull")].clone(), lo.derived[(0, g, "AT")].clone()) for g in lo.groups}
    s = lo.s
    m.merge_lora()
    torch.cuda.synchronize()
    assert m.lora is None and m.base8 and not m.base_int8
    for g, (Bfull, AT) in pairs.items():                                   # the merged weight itself: W + s Bfull AT^T per element
        gc.check("bf16", Lw[g + "_w"], gc.ref_nt(Bfull, AT, alpha=s, residual=before[g + "_w"]), what=f"merged {g}_w")
        assert not torch.equal(Lw[g + "_w"], before[g + "_w"])
        assert not torch.equal(Lw[g + "_w8"], codes[g + "_w"][0]) and not torch.equal(Lw[g + "_wT8"], codes[g + "_w"][1]), f"{g}: stale codes"
    for k in ("gu_w", "down_w"):
        assert torch.equal(Lw[k], before[k]) and torch.equal(Lw[k + "8"], codes[k][0])
    check_copies(m, "merge_lora")


# ------------------------------------------------------------------------------------------------------------------------- the table
def test_fp8_base_table_reaches_every_cell():
    """every entry of fp8_base_cases.paths is reached by a case that the tests above run; prints what this process measured"""
    print("\nrow-wise worst |err| / (bound at c = 1), and c:", {k: (round(v, 4), rc.BOUNDS[k]) for k, v in sorted(rc.WORST.items())})
    print("GEMM worst (element ratio at c = 1, cell rel-L2):", {k: (round(e, 4), float(f"{c:.3g}")) for k, (e, c) in sorted(gc.WORST.items())})
    if BORDER:
        worst = max(BORDER, key=BORDER.get)
        print(f"largest share of codes left open by the reference: {100 * BORDER[worst]:.3f} % ({worst}); SwiGLU cases:",
              {c.name: round(100 * BORDER[c.name], 4) for c in fc.SWIGLU if c.name in BORDER})
    reached = fc.reached()
    assert not fc.paths - reached, sorted(fc.paths - reached)
    assert not reached - fc.paths, sorted(reached - fc.paths)
