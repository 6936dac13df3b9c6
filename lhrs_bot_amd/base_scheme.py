"""The arithmetic of the frozen decoder linears, one object per format (`TextModal.base`, chosen by `TextModal.quantize_base`).

    Bf16Base   bf16 weights on the bf16 GEMMs.  storage4 = (quant_type, double_quant): the weights are bitsandbytes 4-bit storage (`bits: 4`)
               - codes and statistics beside each weight, the bf16 weight IS their dequantisation, so the same kernels run.
    E4m3Base   OCP e4m3 copies of W and W^T (one fp32 scale per row) on the block-scaled MFMA; norms, SwiGLU and SwiGLU' emit the e4m3
               operand of the next product, activations without such a producer are quantised per row on the fly.
    Int8Base   LLM.int8 (bitsandbytes MatMul8bitLt): int8 rows + absmax factors in the forward (`hk.int8_linear`), the backward multiplies
               with the dequantised weight in bf16 - Bf16Base's, inherited.

Every scheme answers the same questions with the same shape of value; a member its format does not have is None.  `L` is a layer dict, `name`
the key of a weight in it ("qkv_w" forward, "qkv_wT" for dX): a scheme finds its own stored copies beside it (`name + "8"`, `name + "i8"`).
`m` is the TextModal; (a2, b2) / (U, AT) an adapter pair riding on the product's accumulators, or (None, None).  Kernels are looked up on
`hk` at call time (tests wrap them)."""
from . import kernels as hk

WEIGHTS = ("qkv_w", "o_w", "gu_w", "down_w")
W4_PARTS = {"qkv_w": 3, "o_w": 1, "gu_w": 2, "down_w": 1}   # reference Linears per fused weight (row-concatenated): 4-bit statistics are per Linear


def _rope(m, y, rope):
    """RoPE of the q / k heads as a launch of its own behind an 8-bit product (the bf16 GEMM has it in its epilogue)"""
    if rope is not None:
        hk.rope_(y, y.shape[0], 2 * m.heads, m.hd, m.cos, m.sin, pos_mod=rope[0], pos0=rope[1])
    return y


class Bf16Base:
    native_layer = True   # the whole-layer entry points (lhrs_llama_layer_forward / _backward) run this arithmetic
    ws = None             # Int8Base: its hk.Int8Workspace

    def __init__(self, storage4=None):
        self.storage4 = storage4

    def install(self, m) -> None:
        """Build the stored copies from the CURRENT weights of `m` (quantize_base; again after merge_lora, as peft re-quantises a merged Linear4bit)."""
        if self.storage4 is None:
            return
        for L in m.p["layers"]:
            m._drop_derived(L)
            for k, parts in W4_PARTS.items():
                W = L[k]
                rows = W.shape[0] // parts
                states = []
                for i in range(parts):
                    sub = W[i * rows:(i + 1) * rows]
                    st = hk.quant4_blocks(sub, *self.storage4)
                    hk.dequant4_blocks(st, out=sub)              # from here on the 16-bit weight IS the 4-bit one
                    states.append(st)
                L[k + "q4"] = states
                L[k + "T"] = hk.transpose(W)

    def norm_fwd(self, x, w, eps, want_bf16, out=None):
        """-> (h, hq): RMSNorm and the 8-bit operand of the product behind it"""
        return hk.rmsnorm_fwd(x, w, eps, out=out), None

    def norm_bwd(self, dy, x, w, eps, add=None, out=None):
        """-> (dx, dxq)"""
        return hk.rmsnorm_bwd(dy, x, w, None, add=add, eps=eps, out=out), None

    def operand(self, x, xq):
        """the 8-bit operand of x for `product` / `dx`: the producer's `xq`, or made here"""
        return None

    def product(self, m, L, name, x, xq, residual, a2, b2, rope):
        """y = x W^T (+ a2 b2^T) (+ residual), rope = (pos_mod, pos0): RoPE of the q / k heads of the qkv projection"""
        if rope is not None:
            return hk.gemm_rope_fwd(x, L[name], m.cos, m.sin, pos_mod=rope[0], pos0=rope[1], rope_cols=2 * m.d, head_dim=m.hd, a2=a2, b2=b2)
        if a2 is None:
            return hk.gemm_nt(x, L[name], residual=residual)
        return hk.gemm_nt_lora(x, L[name], a2, b2, residual=residual)

    def gu_fwd(self, m, li, h, hq, L, save):
        """gate|up projection + SwiGLU -> (gu [M, 2ff], act [M, ff], actq); here both in one launch"""
        return hk.gemm_swiglu_fwd(h, L["gu_w"], m.ff, *m._adapter_down(li, "gu", h, save)) + (None,)

    def dx(self, L, name, dy, dyq, U=None, AT=None, drop=None, **fused):
        """dx = dy W (+ U AT^T); drop = (p, seed): dx = dy W + mask * (U AT^T) / (1 - p) - the adapter term cannot share the base product's accumulators"""
        if drop is not None:
            return hk.gemm_nt_dropmask(U, AT, drop[0], drop[1], residual=self._dx(L, name, dy, dyq, None, None))
        return self._dx(L, name, dy, dyq, U, AT, **fused)

    def _dx(self, L, name, dy, dyq, U, AT, gu=None, ff=None):
        if gu is not None:   # the down projection: dgu (written over gu) = swiglu'(gu) * d_act, d_act never leaving the GEMM epilogue
            return hk.gemm_swiglu_bwd(dy, L[name], gu, ff, U, AT)
        if U is None:
            return hk.gemm_nt(dy, L[name])
        return hk.gemm_nt_lora(dy, L[name], U, AT)

    def down_bwd(self, m, li, dy, dyq, L, gu, act, T, drop):
        """down projection's dX + SwiGLU' -> (dgu over gu, dguq); `m._lin_bwd` adds the adapter gradients of `down`"""
        if drop is not None:  # masked adapter term: unfused sequence
            return hk.swiglu_bwd(m._lin_bwd(li, "down", dy, L, act, T, drop=drop), gu, m.ff, out=gu), None
        return m._lin_bwd(li, "down", dy, L, act, T, gu=gu, ff=m.ff), None


class E4m3Base(Bf16Base):
    native_layer = False

    def install(self, m) -> None:
        m.quantize_fp8()
        for L in m.p["layers"]:
            for k in WEIGHTS:
                L[k + "T8"], L[k + "T8s"] = hk.quant_fp8_rows(L[k + "T"])

    def norm_fwd(self, x, w, eps, want_bf16, out=None):
        return hk.rmsnorm_fwd_q(x, w, eps, want_bf16=want_bf16)   # the bf16 copy only if an adapter reads it

    def norm_bwd(self, dy, x, w, eps, add=None, out=None):
        return hk.rmsnorm_bwd_q(dy, x, w, None, add=add, eps=eps, out=out)

    def operand(self, x, xq):
        return xq if xq is not None else hk.quant_fp8_rows(x)

    def product(self, m, L, name, x, xq, residual, a2, b2, rope):
        x8, sx = self.operand(x, xq)
        return _rope(m, hk.gemm_fp8_nt(x8, sx, L[name + "8"], L[name + "8s"], residual=residual, a2=a2, b2=b2), rope)

    def gu_fwd(self, m, li, h, hq, L, save):
        gu = m._lin(li, "gu", h, L, save=save, xq=hq)
        act, act8, sact = hk.swiglu_fwd_q(gu, m.ff, want_bf16=m._has("down"))   # bf16 act only if an adapter on `down` needs it
        return gu, act, (act8, sact)

    def _dx(self, L, name, dy, dyq, U, AT):
        return hk.gemm_fp8_nt(dyq[0], dyq[1], L[name + "8"], L[name + "8s"], a2=U, b2=AT)

    def down_bwd(self, m, li, dy, dyq, L, gu, act, T, drop):
        dact = m._lin_bwd(li, "down", dy, L, act, T, dyq=dyq, drop=drop)
        dgu, dgu8, sdgu = hk.swiglu_bwd_q(dact, gu, m.ff, want_bf16=m._has("gu"))   # bf16 d(gate|up) only if an adapter on `gu` needs it
        return dgu, (dgu8, sdgu)


class Int8Base(Bf16Base):
    native_layer = False

    def install(self, m) -> None:
        for L in m.p["layers"]:
            m._drop_derived(L)
            for k in WEIGHTS:
                L[k + "i8"], L[k + "i8s"] = hk.quant_int8_rows(L[k])
                hk.dequant_int8_rows(L[k + "i8"], L[k + "i8s"], out=L[k])     # from here on the 16-bit weight IS the int8 one
                L[k + "T"] = hk.transpose(L[k])
        self.ws = hk.Int8Workspace(m.device, kmax=max(m.d, m.ff))

    def product(self, m, L, name, x, xq, residual, a2, b2, rope):   # int8 product + 16-bit outlier columns, adapters on top
        return _rope(m, hk.int8_linear(x, L[name + "i8"], L[name + "i8s"], self.ws, residual=residual, a2=a2, b2=b2), rope)

    def gu_fwd(self, m, li, h, hq, L, save):
        gu = m._lin(li, "gu", h, L, save=save)
        return gu, hk.swiglu_fwd(gu, m.ff), None
