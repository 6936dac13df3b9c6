"""Thin host wrappers: torch tensors (device memory + streams only) -> raw pointers -> the C ABI.

No arithmetic happens here and nothing falls back to torch: every function enqueues one or two HIP kernels
of liblhrs_hip.so on the current HIP stream.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch

from . import _lib

ACT_NONE, ACT_QUICK_GELU, ACT_GELU, ACT_SILU = 0, 1, 2, 3
MAP_GELU, MAP_GELU_BWD, MAP_ADD, MAP_QUICK_GELU = 0, 1, 2, 3


def _L():
    return _lib.load()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _req(t: torch.Tensor, dtype, name: str):
    if t.dtype != dtype or not t.is_cuda:
        raise TypeError(f"{name}: expected cuda {dtype}, got {t.device} {t.dtype}")


# --------------------------------------------------------------------------------------------- GEMM
_GEMM_WS = {}


def ensure_gemm_workspace(device) -> None:
    """Give the library its GEMM workspace on `device` (caller-owned, 64 MiB + 4 KiB: include/lhrs_hip.h) - once per device and process;
    the towers call this when they are built.  One user inside the library: the split-K launch for the tail rows of a row-split product
    with a long k-loop.  LHRS_GEMM_WORKSPACE=0: nothing is registered (those tail rows then run whole-K small tiles)."""
    dev = torch.device(device)
    if dev.type != "cuda" or os.environ.get("LHRS_GEMM_WORKSPACE", "1") == "0":
        return
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx in _GEMM_WS:
        return
    with torch.cuda.device(idx):
        n = int(_L().lhrs_gemm_workspace_bytes())
        ws = torch.empty(n, device=f"cuda:{idx}", dtype=torch.uint8)
        torch.cuda.synchronize()
        _lib.check(_L().lhrs_gemm_set_workspace(ws.data_ptr(), n), "gemm_set_workspace")
    _GEMM_WS[idx] = ws


def gemm_set_u4(on: bool) -> None:
    """The four-wave gemm_u4_kernel (csrc/gemm_u4.hip) for the plain long-k products and the fused-epilogue products it covers (default on; LHRS_GEMM_U4=0:
    the 16-wave kernels everywhere - kernel A/B tests)."""
    _L().lhrs_gemm_set_u4(int(bool(on)))


def gemm_u4_takes(M, N, K, lda=None, ldb=None, ldc=None, ldr=0, has_bias=False, act=0, out_f32=False, accumulate=False, alpha=1.0) -> bool:
    """The shape rule of lhrs_gemm_bf16_nt: True when that problem runs on gemm_u4_kernel (a pure function of the arguments)."""
    return bool(_L().lhrs_gemm_u4_takes(int(M), int(N), int(K), int(K if lda is None else lda), int(K if ldb is None else ldb), int(N if ldc is None else ldc),
                                        int(ldr), int(has_bias), int(act), int(out_f32), int(accumulate), float(alpha)))


GEMM_KIND_NAMES = ("gemm_nt_256s_kernel plain", "gemm_nt_256s_kernel SwiGLU-fwd", "gemm_nt_256s_kernel SwiGLU-bwd", "gemm_nt_256s_kernel RoPE", "gemm_nt_144s_kernel plain",
                   "gemm_u4_kernel<0, true> plain + residual", "gemm_u4_kernel<0, false> plain", "gemm_u4_kernel<1, false> SwiGLU-fwd", "gemm_u4_kernel<2, false> SwiGLU-bwd",
                   "gemm_u4_kernel<3, false> RoPE")


class gemm_kernel_census:
    """with gemm_kernel_census() as c: ...  -> c.counts = {kernel instantiation: timed launches} of the persistent GEMM kernels that ran inside the block (the library's live
    profile counters, include/lhrs_hip.h: lhrs_gemm_profile_*): which kernel the shape rules gave each product - the parity tests record it next to their numbers.
    c.launches = every GEMM launch inside the block, timed or not (lhrs_gemm_profile_read out[3]: small tiles, split-K tails and e4m3 kernels included)."""

    def __enter__(self):
        _lib.check(_L().lhrs_gemm_profile_stride(1), "gemm_profile_stride")
        _lib.check(_L().lhrs_gemm_profile_enable(20000), "gemm_profile_enable")
        self.counts, self.launches = {}, 0
        return self

    def __exit__(self, *exc):
        kinds = (ctypes.c_double * 30)()
        totals = (ctypes.c_double * 5)()
        torch.cuda.synchronize()
        _lib.check(_L().lhrs_gemm_profile_read_kinds(ctypes.addressof(kinds)), "gemm_profile_read_kinds")
        _lib.check(_L().lhrs_gemm_profile_read(ctypes.addressof(totals)), "gemm_profile_read")
        _L().lhrs_gemm_profile_enable(0)
        self.counts = {GEMM_KIND_NAMES[k]: int(kinds[3 * k]) for k in range(10) if kinds[3 * k] > 0}
        self.launches = int(totals[3])
        return False


def gemm_u4_nt(a, b, out, residual=None, a2=None, b2=None) -> bool:
    """The raw launch of gemm_u4_kernel (tests, tools): True when launched, False when the problem is not its kind.  a2 / b2: the fused LoRA pair."""
    ldr = residual.stride(0) if residual is not None else 0
    if a2 is not None:
        st = _L().lhrs_gemm_u4_nt_lora(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), a2.data_ptr(), a2.stride(0), b2.data_ptr(), b2.stride(0),
                                       a2.shape[1], out.data_ptr(), out.stride(0), a.shape[0], b.shape[0], a.shape[1], _p(residual), ldr, _stream())
    else:
        st = _L().lhrs_gemm_u4_nt(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0), a.shape[0], b.shape[0], a.shape[1],
                                  _p(residual), ldr, _stream())
    if st < 0:
        _lib.check(st, "gemm_u4_nt")
    return st == 0


def gemm_nt(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None, *, bias=None, residual=None,
            act: int = ACT_NONE, out_f32: bool = False, accumulate: bool = False, alpha: float = 1.0,
            M: Optional[int] = None, N: Optional[int] = None, K: Optional[int] = None) -> torch.Tensor:
    """out[M,N] = act(alpha * a[M,K] @ b[N,K]^T + bias) + residual.  a/b/out may be strided row views."""
    _req(a, torch.bfloat16, "a"); _req(b, torch.bfloat16, "b")
    assert a.dim() == 2 and b.dim() == 2 and a.stride(1) == 1 and b.stride(1) == 1
    M = a.shape[0] if M is None else M
    N = b.shape[0] if N is None else N
    K = a.shape[1] if K is None else K
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    assert out.stride(1) == 1 and out.dtype == (torch.float32 if out_f32 else torch.bfloat16)
    ldr = residual.stride(0) if residual is not None else 0
    st = _L().lhrs_gemm_bf16_nt(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0), M, N, K,
                                _p(bias), _p(residual), ldr, act, int(out_f32), int(accumulate), float(alpha), _stream())
    _lib.check(st, "gemm_bf16_nt")
    return out


def gemm_nt_lora(a, b, a2, b2, out=None, *, bias=None, residual=None, out_f32=False, accumulate=False, alpha=1.0):
    """out = alpha * (a @ b^T + a2 @ b2^T) + bias + residual  (rank-K2 LoRA update fused into the base GEMM's k-loop)."""
    M, K = a.shape
    N, K2 = b.shape[0], a2.shape[1]
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    ldr = residual.stride(0) if residual is not None else 0
    st = _L().lhrs_gemm_bf16_nt_lora(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), a2.data_ptr(), a2.stride(0), b2.data_ptr(),
                                     b2.stride(0), K2, out.data_ptr(), out.stride(0), M, N, K, _p(bias), _p(residual), ldr,
                                     int(out_f32), int(accumulate), float(alpha), _stream())
    _lib.check(st, "gemm_bf16_nt_lora")
    return out


def gemm_swiglu_fwd(x, w_gu, ff, a2=None, b2=None):
    """(gu [M, 2ff], act [M, ff]) = LLaMA MLP first half in ONE launch: gu = x @ w_gu^T (+ a2 @ b2^T), act = silu(gate) * up."""
    M, K = x.shape
    assert w_gu.shape[0] == 2 * ff
    gu = torch.empty((M, 2 * ff), device=x.device, dtype=torch.bfloat16)
    act = torch.empty((M, ff), device=x.device, dtype=torch.bfloat16)
    K2 = a2.shape[1] if a2 is not None else 0
    st = _L().lhrs_gemm_swiglu_fwd(x.data_ptr(), x.stride(0), w_gu.data_ptr(), w_gu.stride(0), _p(a2), a2.stride(0) if K2 else 0, _p(b2),
                                   b2.stride(0) if K2 else 0, K2, gu.data_ptr(), gu.stride(0), act.data_ptr(), act.stride(0), M, ff, K,
                                   _stream())
    _lib.check(st, "gemm_swiglu_fwd")
    return gu, act


def gemm_rope_fwd(x, w, cos_t, sin_t, *, pos_mod, pos0=0, rope_cols, head_dim, a2=None, b2=None, out=None):
    """out [M, N] = x @ w^T (+ a2 @ b2^T) with RoPE applied to the heads in columns [0, rope_cols) inside the GEMM epilogue (one launch;
    bit-identical to gemm_nt(+lora) followed by rope_)."""
    M, K = x.shape
    N = w.shape[0]
    out = torch.empty((M, N), device=x.device, dtype=torch.bfloat16) if out is None else out
    K2 = a2.shape[1] if a2 is not None else 0
    st = _L().lhrs_gemm_rope_fwd(x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), _p(a2), a2.stride(0) if K2 else 0, _p(b2),
                                 b2.stride(0) if K2 else 0, K2, out.data_ptr(), out.stride(0), M, N, K, cos_t.data_ptr(), sin_t.data_ptr(),
                                 int(pos_mod), int(pos0), int(rope_cols), int(head_dim), _stream())
    _lib.check(st, "gemm_rope_fwd")
    return out


def gemm_swiglu_bwd(dy, w_down_t, gu, ff, a2=None, b2=None, out=None):
    """dgu [M, 2ff] = swiglu'(gu) * (dy @ w_down_t^T (+ a2 @ b2^T)) in ONE launch; out defaults to gu (in place)."""
    M, K = dy.shape
    assert w_down_t.shape[0] == ff and gu.shape == (M, 2 * ff)
    dgu = gu if out is None else out
    K2 = a2.shape[1] if a2 is not None else 0
    L = _L()
    scratch = None
    if not L.lhrs_gemm_swiglu_fusable(M, ff, K, K, K2):
        scratch = torch.empty((M, ff), device=dy.device, dtype=torch.bfloat16)
    st = L.lhrs_gemm_swiglu_bwd(dy.data_ptr(), dy.stride(0), w_down_t.data_ptr(), w_down_t.stride(0), _p(a2), a2.stride(0) if K2 else 0,
                                _p(b2), b2.stride(0) if K2 else 0, K2, gu.data_ptr(), dgu.data_ptr(), gu.stride(0), _p(scratch), M, ff, K,
                                _stream())
    _lib.check(st, "gemm_swiglu_bwd")
    return dgu


def gemm_fp8_nt(a8, sa, b8, sb, out=None, *, residual=None, alpha=1.0, a2=None, b2=None):
    """out[M, N] bf16 = alpha * (sa[:, None] * sb[None, :] * (a8 @ b8^T) + a2 @ b2^T) (+ residual); a8 [M, K], b8 [N, K] uint8 e4m3 with
    per-row fp32 scales; the optional bf16 pair a2 [M, K2], b2 [N, K2] (LoRA update) is accumulated by the same launch."""
    M, K = a8.shape
    N = b8.shape[0]
    assert a8.dtype == torch.uint8 and b8.dtype == torch.uint8 and sa.dtype == torch.float32 and sb.dtype == torch.float32
    if out is None:
        out = torch.empty((M, N), device=a8.device, dtype=torch.bfloat16)
    ldr = residual.stride(0) if residual is not None else 0
    if a2 is None:
        st = _L().lhrs_gemm_fp8_nt(a8.data_ptr(), a8.stride(0), sa.data_ptr(), b8.data_ptr(), b8.stride(0), sb.data_ptr(), out.data_ptr(),
                                   out.stride(0), M, N, K, _p(residual), ldr, float(alpha), _stream())
    else:
        st = _L().lhrs_gemm_fp8_nt_lora(a8.data_ptr(), a8.stride(0), sa.data_ptr(), b8.data_ptr(), b8.stride(0), sb.data_ptr(), a2.data_ptr(),
                                        a2.stride(0), b2.data_ptr(), b2.stride(0), a2.shape[1], out.data_ptr(), out.stride(0), M, N, K,
                                        _p(residual), ldr, float(alpha), _stream())
    _lib.check(st, "gemm_fp8_nt")
    return out


def gemm_nt_skinny(a, b, alpha=1.0):
    """out[M, N] bf16 = alpha * a[M, K] @ b[N, K]^T for a skinny N (64..384): split-K launch + reduction (LoRA down-projections)."""
    M, K = a.shape
    N = b.shape[0]
    if N > 256 or N % 64 or M < 1024 or K < 1024:  # N = 384 at K = 4096: 54.5 us here against 42.8 us on the plain path (M = 8190)
        return gemm_nt(a, b, alpha=alpha)
    out = torch.empty((M, N), device=a.device, dtype=torch.bfloat16)
    ws = torch.empty(_L().lhrs_gemm_skinny_splits(K, N) * M * N, device=a.device, dtype=torch.float32)
    st = _L().lhrs_gemm_bf16_nt_skinny(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0), M, N, K,
                                       float(alpha), ws.data_ptr(), _stream())
    _lib.check(st, "gemm_bf16_nt_skinny")
    return out


def gemm_nt_splitk_f32(a, b, out):
    """out[M, N] fp32 = a[M, K] @ b[N, K]^T for a long K and few output tiles (weight gradients): split-K launch + ordered reduction."""
    M, K = a.shape
    N = b.shape[0]
    L = _L()
    splits = L.lhrs_gemm_splitk_splits(M, N, K)
    ws = torch.empty(splits * M * N, device=a.device, dtype=torch.float32) if splits > 1 else None
    st = L.lhrs_gemm_bf16_nt_splitk_f32(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0), M, N, K,
                                        _p(ws), _stream())
    _lib.check(st, "gemm_bf16_nt_splitk_f32")
    return out


def gemm_tn_f32(p, q, out):
    """out[Mo, No] fp32 = p[T, Mo]^T @ q[T, No] - weight gradients dW = dY^T X from the token-major operands as they lie (no transposes).
    Mo, No multiples of 128; row strides free (multiples of 8)."""
    T, Mo = p.shape
    No = q.shape[1]
    L = _L()
    splits = L.lhrs_gemm_tn_splits(T, Mo, No)
    ws = torch.empty(splits * Mo * No, device=p.device, dtype=torch.float32) if splits > 1 else None
    st = L.lhrs_gemm_tn_f32(p.data_ptr(), p.stride(0), q.data_ptr(), q.stride(0), out.data_ptr(), out.stride(0), T, Mo, No, _p(ws), _stream())
    _lib.check(st, "gemm_tn_f32")
    return out


class BatchedTranspose:
    """out_i = in_i^T for a fixed list of (in, out) bf16 matrix pairs, refreshed by ONE launch (lhrs_transpose_batched)."""

    def __init__(self, pairs):
        rows, tiles = [], 0
        for src, dst in pairs:
            r, c = src.shape
            assert dst.shape == (c, r) and src.stride(1) == 1 and dst.stride(1) == 1
            rows.append([src.data_ptr(), dst.data_ptr(), src.stride(0), dst.stride(0), r, c, tiles])
            tiles += ((r + 63) // 64) * ((c + 63) // 64)
        self.keep = pairs
        self.n, self.tiles = len(rows), tiles
        self.desc = torch.tensor(rows, dtype=torch.int64).to(pairs[0][0].device)

    def run(self):
        _lib.check(_L().lhrs_transpose_batched(self.desc.data_ptr(), self.n, self.tiles, _stream()), "transpose_batched")


def dropout(x, p, seed, out=None):
    """peft lora_dropout on the adapter input: out = x * mask / (1 - p), mask regenerated from (seed, element index)."""
    rows, cols = x.shape
    out = torch.empty((rows, cols), device=x.device, dtype=torch.bfloat16) if out is None else out
    _lib.check(_L().lhrs_dropout_bf16(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), rows, cols, float(p), int(seed) & 0xFFFFFFFF,
                                      _stream()), "dropout")
    return out


def gemm_nt_dropmask(a, b, p, seed, residual=None, alpha=1.0):
    """out = mask * (alpha * a @ b^T) / (1 - p) + residual with the same counter-based mask as dropout() over the [M, N] result."""
    M, K = a.shape
    N = b.shape[0]
    out = torch.empty((M, N), device=a.device, dtype=torch.bfloat16)
    st = _L().lhrs_gemm_bf16_nt_dropmask(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0), M, N, K,
                                         _p(residual), residual.stride(0) if residual is not None else 0, float(alpha), float(p),
                                         int(seed) & 0xFFFFFFFF, _stream())
    _lib.check(st, "gemm_bf16_nt_dropmask")
    return out


def gemm_tn_skinny(p, q, out, accumulate=False):
    """out[KP, N] (+)= p[M, KP]^T @ q[M, N]  (fp32 out; p, q token-major bf16, row strides free)."""
    M, KP = p.shape
    N = q.shape[1]
    ns = _L().lhrs_tn_skinny_splits(M, N)
    part = torch.empty(ns * KP * N, device=p.device, dtype=torch.float32)
    st = _L().lhrs_gemm_tn_skinny(p.data_ptr(), p.stride(0), q.data_ptr(), q.stride(0), out.data_ptr(), out.stride(0), part.data_ptr(),
                                  M, N, KP, int(accumulate), _stream())
    _lib.check(st, "gemm_tn_skinny")
    return out


def blockdiag_mask(g, r, w, active_mask):
    rows, cols = g.shape
    _lib.check(_L().lhrs_blockdiag_mask(g.data_ptr(), g.stride(0), rows, cols, r, w, active_mask, _stream()), "blockdiag_mask")
    return g


# --------------------------------------------------------------------------------------------- norms
def layernorm_fwd(x, gamma, beta, eps=1e-5, save_stats=False, out=None):
    rows, cols = x.shape
    y = torch.empty_like(x) if out is None else out
    mean = rstd = None
    if save_stats:
        mean = torch.empty(rows, device=x.device, dtype=torch.float32)
        rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    st = _L().lhrs_layernorm_fwd(x.data_ptr(), x.stride(0), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), y.stride(0),
                                 _p(mean), _p(rstd), rows, cols, eps, _stream())
    _lib.check(st, "layernorm_fwd")
    return (y, mean, rstd) if save_stats else y


def layernorm_bwd(dy, x, gamma, mean, rstd, dgamma=None, dbeta=None, accumulate=False, need_dx=True, add=None, out=None):
    rows, cols = x.shape
    dx = (torch.empty_like(x) if out is None else out) if need_dx else None
    assert add is None or dx is None or add.stride(0) == dx.stride(0), "layernorm_bwd: add is read with dx's row stride"
    part = None
    if dgamma is not None:
        nblk = _L().lhrs_layernorm_bwd_nblk(rows)
        part = torch.empty(nblk * 2 * cols, device=x.device, dtype=torch.float32)
    st = _L().lhrs_layernorm_bwd(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), gamma.data_ptr(), mean.data_ptr(),
                                 rstd.data_ptr(), _p(add), _p(dx), dx.stride(0) if dx is not None else 0, _p(dgamma), _p(dbeta),
                                 _p(part), int(accumulate), rows, cols, _stream())
    _lib.check(st, "layernorm_bwd")
    return dx


def rmsnorm_fwd(x, w, eps=1e-5, save_rstd=False, out=None):
    rows, cols = x.shape
    y = torch.empty_like(x) if out is None else out
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32) if save_rstd else None
    st = _L().lhrs_rmsnorm_fwd(x.data_ptr(), x.stride(0), w.data_ptr(), y.data_ptr(), y.stride(0), _p(rstd), rows, cols, eps,
                               _stream())
    _lib.check(st, "rmsnorm_fwd")
    return (y, rstd) if save_rstd else y


def rmsnorm_bwd(dy, x, w, rstd=None, add=None, eps=1e-5, out=None):
    rows, cols = x.shape
    assert dy.is_contiguous() and x.is_contiguous()
    dx = torch.empty_like(x) if out is None else out
    assert dx.is_contiguous() and (add is None or add.is_contiguous()), "rmsnorm_bwd: add and out are read / written with row stride cols"
    st = _L().lhrs_rmsnorm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), _p(rstd), _p(add), dx.data_ptr(), rows, cols, eps,
                               _stream())
    _lib.check(st, "rmsnorm_bwd")
    return dx


def rmsnorm_fwd_q(x, w, eps=1e-5, want_bf16=True, out=None, q_out=None):
    """-> (y bf16 or None, (y8 uint8 [rows, cols], scale fp32 [rows])): RMSNorm + per-row e4m3 copy of its output in one pass."""
    rows, cols = x.shape
    y = (torch.empty_like(x) if out is None else out) if want_bf16 else None
    y8, sc = q_out if q_out is not None else (torch.empty((rows, cols), device=x.device, dtype=torch.uint8),
                                              torch.empty(rows, device=x.device, dtype=torch.float32))
    st = _L().lhrs_rmsnorm_fwd_q(x.data_ptr(), x.stride(0), w.data_ptr(), _p(y), y.stride(0) if y is not None else 0, y8.data_ptr(),
                                 sc.data_ptr(), rows, cols, eps, _stream())
    _lib.check(st, "rmsnorm_fwd_q")
    return y, (y8, sc)


def rmsnorm_bwd_q(dy, x, w, rstd=None, add=None, eps=1e-5, out=None):
    """-> (dx bf16, (dx8, scale)): RMSNorm backward (+ residual add) + per-row e4m3 copy of dx."""
    rows, cols = x.shape
    assert dy.is_contiguous() and x.is_contiguous()
    dx = torch.empty_like(x) if out is None else out
    assert dx.is_contiguous() and (add is None or add.is_contiguous()), "rmsnorm_bwd_q: add and out are read / written with row stride cols"
    d8 = torch.empty((rows, cols), device=x.device, dtype=torch.uint8)
    sc = torch.empty(rows, device=x.device, dtype=torch.float32)
    st = _L().lhrs_rmsnorm_bwd_q(dy.data_ptr(), x.data_ptr(), w.data_ptr(), _p(rstd), _p(add), dx.data_ptr(), d8.data_ptr(), sc.data_ptr(),
                                 rows, cols, eps, _stream())
    _lib.check(st, "rmsnorm_bwd_q")
    return dx, (d8, sc)


# --------------------------------------------------------------------------------------------- attention
def h2d(t: torch.Tensor, device) -> torch.Tensor:
    """Small host tensor -> device without stalling the host: a pageable source makes the copy wait for everything already queued on
    the stream (the launch queue drains, the GPU then idles until new work arrives); a pinned source with non_blocking=True is just
    another item in the queue."""
    if t.is_cuda:
        return t
    return t.pin_memory().to(device, non_blocking=True)


def make_desc(entries, device) -> torch.Tensor:
    """entries: list of (q_off, q_len, kv_off, kv_len[, kv_rows[, causal_off]]) -> int32 [n, 8] on device."""
    rows = []
    for e in entries:
        e = list(e)
        if len(e) == 4:
            e.append(e[3])
        if len(e) == 5:
            e.append(0)
        rows.append(e + [0, 0])
    return h2d(torch.tensor(rows, dtype=torch.int32), device)


def pad64(n: int) -> int:
    return (n + 63) // 64 * 64


def seq_transpose(x, cols, LT, desc, nseq, which: str):
    """x: [tokens, ld] view (first `cols` columns used) -> [nseq, cols, LT] zero padded.  which: 'q' | 'kv' | 'kv_rows'."""
    out = torch.empty((nseq, cols, LT), device=x.device, dtype=torch.bfloat16)
    use = {"q": 0, "kv": 1, "kv_rows": 2}[which]
    st = _L().lhrs_seq_transpose(x.data_ptr(), x.stride(0), out.data_ptr(), cols, LT, desc.data_ptr(), nseq, use, _stream())
    _lib.check(st, "seq_transpose")
    return out


def attn_fwd(q, k, v, o, lse, desc, nseq, H, D, max_q, max_kv, LTq, causal, scale, key_mask=None):
    """key_mask: optional uint8 [nseq, >= kv_len] HF-style attention_mask over the keys (left-padded batched generate)."""
    if key_mask is None:
        st = _L().lhrs_attn_fwd(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), o.data_ptr(),
                                o.stride(0), _p(lse), desc.data_ptr(), nseq, H, D, max_q, max_kv, LTq, int(causal), float(scale),
                                _stream())
    else:
        assert key_mask.dtype == torch.uint8 and key_mask.dim() == 2 and key_mask.shape[0] == nseq and key_mask.stride(1) == 1
        st = _L().lhrs_attn_fwd_kmask(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), o.data_ptr(),
                                      o.stride(0), _p(lse), desc.data_ptr(), nseq, H, D, max_q, max_kv, LTq, int(causal),
                                      float(scale), key_mask.data_ptr(), key_mask.stride(0), _stream())
    _lib.check(st, "attn_fwd")


def attn_delta(o, dout, delta, desc, nseq, H, D, max_q, LTq):
    st = _L().lhrs_attn_delta(o.data_ptr(), o.stride(0), dout.data_ptr(), dout.stride(0), delta.data_ptr(), desc.data_ptr(),
                              nseq, H, D, max_q, LTq, _stream())
    _lib.check(st, "attn_delta")


def attn_bwd(q, k, v, dout, lse, delta, dq, dk, dv, desc, nseq, H, D, max_q, max_kv, LTq, causal, scale, rope=None):
    """rope = (cos_t, sin_t, pos_mod, pos0): q / k were rotated before the scores - dq / dk are returned as gradients of the UN-rotated
    projections (inverse rotation inside the stores of the resident kernels; a separate pass for long sequences), rows = dq.shape[0]."""
    if rope is None:
        st = _L().lhrs_attn_bwd(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), dout.data_ptr(),
                                dout.stride(0), lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), dq.stride(0), dk.data_ptr(),
                                dk.stride(0), dv.data_ptr(), dv.stride(0), desc.data_ptr(), nseq, H, D, max_q, max_kv, LTq,
                                int(causal), float(scale), _stream())
    else:
        cos_t, sin_t, pos_mod, pos0 = rope
        st = _L().lhrs_attn_bwd_rope(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), dout.data_ptr(),
                                     dout.stride(0), lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), dq.stride(0), dk.data_ptr(),
                                     dk.stride(0), dv.data_ptr(), dv.stride(0), desc.data_ptr(), nseq, H, D, max_q, max_kv, LTq,
                                     int(causal), float(scale), cos_t.data_ptr(), sin_t.data_ptr(), int(pos_mod), int(pos0), dq.shape[0],
                                     _stream())
    _lib.check(st, "attn_bwd")


def attn_bwd_o(q, k, v, dout, o, lse, delta, dq, dk, dv, desc, nseq, H, D, max_q, max_kv, LTq, causal, scale, rope=None):
    """attn_delta + attn_bwd in one call: `o` are the forward output rows, `delta` [nseq, H, LTq] fp32 is WRITTEN (the resident dQ kernel
    computes rowsum(dO * O) for the rows it loads anyway; longer sequences launch the delta kernel inside)."""
    cos_t, sin_t, pos_mod, pos0 = rope if rope is not None else (None, None, 1, 0)
    st = _L().lhrs_attn_bwd_o(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), dout.data_ptr(),
                              dout.stride(0), o.data_ptr(), o.stride(0), lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), dq.stride(0),
                              dk.data_ptr(), dk.stride(0), dv.data_ptr(), dv.stride(0), desc.data_ptr(), nseq, H, D, max_q, max_kv, LTq,
                              int(causal), float(scale), _p(cos_t), _p(sin_t), int(pos_mod), int(pos0), dq.shape[0], _stream())
    _lib.check(st, "attn_bwd_o")


# --------------------------------------------------------------------------------------------- whole decoder layer (module-level ABI)
def llama_layer_forward(x, L, cos_t, sin_t, desc, B, S, LT, heads, ff, eps, h_scratch):
    """One frozen bf16 decoder layer in ONE library call (lhrs_llama_layer_forward): -> (x_out, saved dict like TextModal._layer_fwd's)."""
    M, d = x.shape
    dev, bf = x.device, torch.bfloat16
    qkv = torch.empty((M, 3 * d), device=dev, dtype=bf)
    o = torch.empty((M, d), device=dev, dtype=bf)
    lse = torch.empty((B, heads, LT), device=dev, dtype=torch.float32)
    x_mid = torch.empty((M, d), device=dev, dtype=bf)
    gu = torch.empty((M, 2 * ff), device=dev, dtype=bf)
    act = torch.empty((M, ff), device=dev, dtype=bf)
    x_out = torch.empty((M, d), device=dev, dtype=bf)
    st = _L().lhrs_llama_layer_forward(x.data_ptr(), L["ln1_w"].data_ptr(), L["qkv_w"].data_ptr(), L["o_w"].data_ptr(), L["ln2_w"].data_ptr(),
                                       L["gu_w"].data_ptr(), L["down_w"].data_ptr(), cos_t.data_ptr(), sin_t.data_ptr(), desc.data_ptr(), B, S, LT, d,
                                       heads, ff, float(eps), h_scratch.data_ptr(), qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), x_mid.data_ptr(),
                                       gu.data_ptr(), act.data_ptr(), x_out.data_ptr(), _stream())
    _lib.check(st, "llama_layer_forward")
    return x_out, dict(x_in=x, qkv=qkv, o=o, o_full=o, lse=lse, x_mid=x_mid, gu=gu)


def vit_layer_forward(x, L, desc, B, n, LT, heads, ff, h, qkv, o, f):
    """One frozen CLIP ViT encoder layer IN PLACE on x, in one library call (lhrs_vit_layer_forward)."""
    d = x.shape[1]
    st = _L().lhrs_vit_layer_forward(x.data_ptr(), L["ln1_w"].data_ptr(), L["ln1_b"].data_ptr(), L["qkv_w"].data_ptr(), L["qkv_b"].data_ptr(),
                                     L["o_w"].data_ptr(), L["o_b"].data_ptr(), L["ln2_w"].data_ptr(), L["ln2_b"].data_ptr(), L["fc1_w"].data_ptr(),
                                     L["fc1_b"].data_ptr(), L["fc2_w"].data_ptr(), L["fc2_b"].data_ptr(), desc.data_ptr(), B, n, LT, d, heads, ff,
                                     h.data_ptr(), qkv.data_ptr(), o.data_ptr(), f.data_ptr(), _stream())
    _lib.check(st, "vit_layer_forward")
    return x


def llama_layer_backward(dx_out, s, L, cos_t, sin_t, desc, B, S, LT, heads, ff, eps, delta, dqkv):
    """d loss / d x_out -> d loss / d x of one frozen bf16 decoder layer in ONE library call (lhrs_llama_layer_backward); s = the saved dict."""
    M, d = dx_out.shape
    dev, bf = dx_out.device, torch.bfloat16
    dh = torch.empty((M, d), device=dev, dtype=bf)
    d_o = torch.empty((M, d), device=dev, dtype=bf)
    dx_in = torch.empty((M, d), device=dev, dtype=bf)
    lib = _L()
    dact = None if lib.lhrs_gemm_swiglu_fusable(M, ff, d, d, 0) else torch.empty((M, ff), device=dev, dtype=bf)
    st = lib.lhrs_llama_layer_backward(dx_out.data_ptr(), s["x_in"].data_ptr(), s["x_mid"].data_ptr(), s["qkv"].data_ptr(), s["o_full"].data_ptr(),
                                       s["lse"].data_ptr(), s["gu"].data_ptr(), L["ln1_w"].data_ptr(), L["ln2_w"].data_ptr(), L["qkv_wT"].data_ptr(),
                                       L["o_wT"].data_ptr(), L["gu_wT"].data_ptr(), L["down_wT"].data_ptr(), cos_t.data_ptr(), sin_t.data_ptr(),
                                       desc.data_ptr(), B, S, LT, d, heads, ff, float(eps), dh.data_ptr(), d_o.data_ptr(), dqkv.data_ptr(),
                                       delta.data_ptr(), _p(dact), dx_in.data_ptr(), _stream())
    _lib.check(st, "llama_layer_backward")
    return dx_in, dh          # (d loss / d x, d loss / d x_mid)


# --------------------------------------------------------------------------------------------- element-wise
def patchify(rgb, P=14, KP=640):
    B, C, H, W = rgb.shape
    assert C == 3 and H == W
    _req(rgb, torch.float32, "rgb")
    rgb = rgb.contiguous()
    out = torch.empty((B * (H // P) ** 2, KP), device=rgb.device, dtype=torch.bfloat16)
    _lib.check(_L().lhrs_patchify(rgb.data_ptr(), out.data_ptr(), B, H, P, KP, _stream()), "patchify")
    return out


def vit_assemble(patch, cls, pos, B, NP, dim):
    out = torch.empty((B * (NP + 1), dim), device=patch.device, dtype=torch.bfloat16)
    _lib.check(_L().lhrs_vit_assemble(patch.data_ptr(), cls.data_ptr(), pos.data_ptr(), out.data_ptr(), B, NP, dim, _stream()),
               "vit_assemble")
    return out


def rope_(x, rows, nheads, D, cos_t, sin_t, pos_mod, pos0=0, inverse=False, pos_ids=None):
    st = _L().lhrs_rope(x.data_ptr(), x.stride(0), rows, nheads, D, cos_t.data_ptr(), sin_t.data_ptr(), _p(pos_ids), pos_mod,
                        pos0, int(inverse), _stream())
    _lib.check(st, "rope")


def swiglu_fwd(gate_up, F, out=None):
    rows = gate_up.shape[0]
    act = torch.empty((rows, F), device=gate_up.device, dtype=torch.bfloat16) if out is None else out
    _lib.check(_L().lhrs_swiglu_fwd(gate_up.data_ptr(), act.data_ptr(), rows, F, _stream()), "swiglu_fwd")
    return act


def swiglu_fwd_q(gate_up, F, want_bf16=False, q_out=None):
    """-> (act bf16 or None, act8 uint8 [rows, F], scale fp32 [rows]): SwiGLU + per-row e4m3 quantisation in one pass."""
    rows = gate_up.shape[0]
    act = torch.empty((rows, F), device=gate_up.device, dtype=torch.bfloat16) if want_bf16 else None
    act8, sc = q_out if q_out is not None else (torch.empty((rows, F), device=gate_up.device, dtype=torch.uint8),
                                                torch.empty(rows, device=gate_up.device, dtype=torch.float32))
    _lib.check(_L().lhrs_swiglu_fwd_q(gate_up.data_ptr(), _p(act), act8.data_ptr(), sc.data_ptr(), rows, F, _stream()), "swiglu_fwd_q")
    return act, act8, sc


def swiglu_bwd_q(dact, gate_up, F, want_bf16=False):
    """-> (dgu bf16 written over gate_up or None, dgu8 uint8 [rows, 2F], scale fp32 [rows])."""
    rows = gate_up.shape[0]
    dgu8 = torch.empty((rows, 2 * F), device=gate_up.device, dtype=torch.uint8)
    sc = torch.empty(rows, device=gate_up.device, dtype=torch.float32)
    _lib.check(_L().lhrs_swiglu_bwd_q(dact.data_ptr(), gate_up.data_ptr(), gate_up.data_ptr() if want_bf16 else None, dgu8.data_ptr(),
                                      sc.data_ptr(), rows, F, _stream()), "swiglu_bwd_q")
    return (gate_up if want_bf16 else None), dgu8, sc


def swiglu_bwd(dact, gate_up, F, out=None):
    rows = gate_up.shape[0]
    dgu = torch.empty_like(gate_up) if out is None else out
    _lib.check(_L().lhrs_swiglu_bwd(dact.data_ptr(), gate_up.data_ptr(), dgu.data_ptr(), rows, F, _stream()), "swiglu_bwd")
    return dgu


def map_(op, a, b=None, out=None):
    out = torch.empty_like(a) if out is None else out
    assert a.is_contiguous() and out.is_contiguous()
    _lib.check(_L().lhrs_map(op, a.data_ptr(), _p(b), out.data_ptr(), a.numel(), _stream()), "map")
    return out


def colsum(x, out, accumulate=False):
    rows, cols = x.shape
    ns = _L().lhrs_colsum_nsplit(rows)
    part = torch.empty(ns * cols, device=x.device, dtype=torch.float32)
    _lib.check(_L().lhrs_colsum(x.data_ptr(), x.stride(0), out.data_ptr(), part.data_ptr(), rows, cols, int(accumulate),
                                _stream()), "colsum")
    return out


def cast_f32_to_bf16(x, out=None):
    out = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16) if out is None else out
    _lib.check(_L().lhrs_cast_f32_to_bf16(x.data_ptr(), out.data_ptr(), x.numel(), _stream()), "cast")
    return out


def transpose(x, rows_pad=None, out=None):
    """x [rows, cols] (strided rows ok) -> [cols, rows_pad] with zero padding."""
    rows, cols = x.shape
    rows_pad = rows if rows_pad is None else rows_pad
    out = torch.empty((cols, rows_pad), device=x.device, dtype=torch.bfloat16) if out is None else out
    _lib.check(_L().lhrs_transpose(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), rows, cols, rows_pad, _stream()),
               "transpose")
    return out


# --------------------------------------------------------------------------------------------- pooler layout
def pooler_build(query, img, B, nq=(64, 48, 32), ni=(256, 256, 256)):
    dim = query.shape[1]
    NQ, KV = sum(nq), sum(nq) + sum(ni)
    t = torch.empty((B * NQ, dim), device=query.device, dtype=torch.bfloat16)
    kv = torch.empty((B * KV, dim), device=query.device, dtype=torch.bfloat16)
    _lib.check(_L().lhrs_pooler_build(query.data_ptr(), img.data_ptr(), t.data_ptr(), kv.data_ptr(), B, *nq, *ni, dim, _stream()),
               "pooler_build")
    return t, kv


def pooler_query_grad(dt0, dkv, dquery, B, nq=(64, 48, 32), ni=(256, 256, 256), accumulate=False):
    dim = dquery.shape[1]
    _lib.check(_L().lhrs_pooler_query_grad(dt0.data_ptr(), _p(dkv), dquery.data_ptr(), B, *nq, *ni, dim, int(accumulate),
                                           _stream()), "pooler_query_grad")
    return dquery


def copy_2d(dst_ptr, dst_pitch, src_ptr, src_pitch, width_bytes, height):
    _lib.check(_L().lhrs_copy_2d(dst_ptr, dst_pitch, src_ptr, src_pitch, width_bytes, height, _stream()), "copy_2d")


# --------------------------------------------------------------------------------------------- token side
def splice_fwd(ids, labels, mask, image, embed, S):
    B, T = ids.shape
    NI, dim = image.shape[1], image.shape[2]
    _req(ids, torch.int64, "input_ids")
    dev = ids.device
    out = torch.empty((B, S, dim), device=dev, dtype=torch.bfloat16)
    out_labels = torch.empty((B, S), device=dev, dtype=torch.int64)
    out_mask = torch.empty((B, S), device=dev, dtype=torch.uint8)
    img_pos = torch.empty(B, device=dev, dtype=torch.int32)
    m8 = None if mask is None else mask.to(torch.uint8).contiguous()
    st = _L().lhrs_splice_fwd(ids.contiguous().data_ptr(), _p(None if labels is None else labels.contiguous()), _p(m8),
                              image.data_ptr(), embed.data_ptr(), out.data_ptr(), out_labels.data_ptr(), out_mask.data_ptr(),
                              img_pos.data_ptr(), B, T, NI, dim, S, embed.shape[0], _stream())
    _lib.check(st, "splice_fwd")
    return out, out_labels, out_mask, img_pos


def splice_bwd(d_embeds, img_pos, NI):
    B, S, dim = d_embeds.shape
    d_image = torch.empty((B, NI, dim), device=d_embeds.device, dtype=torch.bfloat16)
    _lib.check(_L().lhrs_splice_bwd(d_embeds.data_ptr(), img_pos.data_ptr(), d_image.data_ptr(), B, NI, dim, S, _stream()),
               "splice_bwd")
    return d_image


def splice_map_fwd(ids, src_tok, src_img, image, embed, S):
    """General splice (several <image> placeholders per sample): ids int64 [B, T], src_tok / src_img int32 [B, S] from TextModal.splice_plan_host,
    image bf16 [n_slots, NI, dim] -> embeds bf16 [B, S, dim]."""
    B, T = ids.shape
    dim = image.shape[-1]
    _req(ids, torch.int64, "input_ids")
    _req(src_tok, torch.int32, "src_tok")
    _req(src_img, torch.int32, "src_img")
    out = torch.empty((B, S, dim), device=ids.device, dtype=torch.bfloat16)
    _lib.check(_L().lhrs_splice_map_fwd(ids.contiguous().data_ptr(), src_tok.contiguous().data_ptr(), src_img.contiguous().data_ptr(), image.data_ptr(),
                                        embed.data_ptr(), out.data_ptr(), B, T, dim, S, embed.shape[0], _stream()), "splice_map_fwd")
    return out


def splice_map_bwd(d_embeds, inv, n_slots, NI):
    """d_image [n_slots, NI, dim] = rows inv[r] of d_embeds [B, S, dim] (inv int32 [n_slots * NI], < 0 -> zeros)."""
    dim = d_embeds.shape[-1]
    _req(inv, torch.int32, "inv")
    d_image = torch.empty((n_slots, NI, dim), device=d_embeds.device, dtype=torch.bfloat16)
    _lib.check(_L().lhrs_splice_map_bwd(d_embeds.data_ptr(), inv.data_ptr(), d_image.data_ptr(), n_slots * NI, dim, _stream()), "splice_map_bwd")
    return d_image


def gather_rows(src, idx, out=None):
    n, dim = idx.numel(), src.shape[1]
    out = torch.empty((n, dim), device=src.device, dtype=torch.bfloat16) if out is None else out
    _lib.check(_L().lhrs_gather_rows(src.data_ptr(), src.stride(0), idx.data_ptr(), out.data_ptr(), out.stride(0), n, dim,
                                     _stream()), "gather_rows")
    return out


def scatter_rows(src, idx, dst):
    n, dim = idx.numel(), src.shape[1]
    _lib.check(_L().lhrs_scatter_rows(src.data_ptr(), src.stride(0), idx.data_ptr(), dst.data_ptr(), dst.stride(0), n, dim,
                                      _stream()), "scatter_rows")
    return dst


def argmax_rows(logits_f32, out=None):
    n, V = logits_f32.shape
    out = torch.empty(n, device=logits_f32.device, dtype=torch.int64) if out is None else out
    _lib.check(_L().lhrs_argmax_rows(logits_f32.data_ptr(), logits_f32.stride(0), out.data_ptr(), n, V, _stream()), "argmax_rows")
    return out


def sample_rows(logits_f32, out=None, *, mode=0, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, seen=None, seed=0,
                step_dev=None, step_host=0, weights_out=None):
    """lhrs_sample_rows: HF's repetition penalty -> temperature -> top-k -> top-p -> one Philox draw per row of fp32 logits [n, V], in one launch
    (mode 1: first maximum of the penalised row).  `seen` [n, (V+31)//32] int32 bitmap (read for the penalty, the picked token's bit is set);
    `step_dev` a 1-element int32 device tensor added to `step_host` (the draw's counter); `weights_out` [n, V] int64, tests only.
    top_k None / 0 and top_p None / >= 1 switch the filter off."""
    n, V = logits_f32.shape
    _req(logits_f32, torch.float32, "logits")
    assert logits_f32.stride(1) == 1
    out = torch.empty(n, device=logits_f32.device, dtype=torch.int64) if out is None else out
    _req(out, torch.int64, "out")
    if seen is not None:
        _req(seen, torch.int32, "seen")
        assert seen.is_contiguous() and tuple(seen.shape) == (n, (V + 31) // 32), f"seen {tuple(seen.shape)} for n={n} V={V}"
    if step_dev is not None:
        _req(step_dev, torch.int32, "step_dev")
    if weights_out is not None:
        _req(weights_out, torch.int64, "weights_out")
        assert weights_out.is_contiguous() and tuple(weights_out.shape) == (n, V)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    st = _L().lhrs_sample_rows(logits_f32.data_ptr(), logits_f32.stride(0), out.data_ptr(), n, V, int(mode), float(temperature),
                               int(top_k or 0), 1.0 if top_p is None else float(top_p), float(repetition_penalty), _p(seen),
                               seed - (1 << 64) if seed >= (1 << 63) else seed, _p(step_dev), int(step_host), _p(weights_out), _stream())
    _lib.check(st, "sample_rows")
    return out


class ConstraintState:
    """Per-row device state of a walk over a token automaton (include/lhrs_hip.h: lhrs_constrain_rows): `state` (0 = the start), `fin`
    (1 once the row reached a final state), `len` (tokens picked so far, the EOS included), `choice` (the final state's label, -1 before)
    all int32 [n], and `score` fp32 [n], the sum of the picked tokens' log-probabilities (only moved when the pick is asked to)."""

    def __init__(self, n, device):
        i32 = dict(device=device, dtype=torch.int32)
        self.n = int(n)
        self.state, self.fin, self.len = torch.zeros(n, **i32), torch.zeros(n, **i32), torch.zeros(n, **i32)
        self.choice = torch.full((n,), -1, **i32)
        self.score = torch.zeros(n, device=device, dtype=torch.float32)


def constrain_rows(logits_f32, automaton, st: ConstraintState, out=None, *, score=False):
    """lhrs_constrain_rows: per row of fp32 logits [n, V] the first maximum among the out-edges of the row's state in `automaton` (a
    generation.TokenAutomaton: off / tok / nxt / label int32 on the device, pad_token_id, V), the walk along that edge in `st`, and with
    `score` the picked token's log-probability over the whole row added to st.score.  Rows in a final or invalid state get pad_token_id."""
    n, V = logits_f32.shape
    _req(logits_f32, torch.float32, "logits")
    assert logits_f32.stride(1) == 1
    out = torch.empty(n, device=logits_f32.device, dtype=torch.int64) if out is None else out
    _req(out, torch.int64, "out")
    a = automaton
    for name in ("off", "tok", "nxt", "label"):
        _req(getattr(a, name), torch.int32, "automaton." + name)
        assert getattr(a, name).is_contiguous(), f"automaton.{name} is not contiguous"
    for name in ("state", "fin", "len", "choice"):
        _req(getattr(st, name), torch.int32, "ConstraintState." + name)
    _req(st.score, torch.float32, "ConstraintState.score")
    n_states, n_edges = a.label.numel(), a.tok.numel()
    assert V == a.V, f"logits of {V} columns for an automaton validated for V={a.V}"
    assert a.off.numel() == n_states + 1 and a.nxt.numel() == n_edges, "automaton arrays disagree in length"
    assert st.n == n and out.numel() == n and out.is_contiguous(), f"ConstraintState of {st.n} rows / out of {out.numel()} for {n} rows of logits"
    _lib.check(_L().lhrs_constrain_rows(logits_f32.data_ptr(), logits_f32.stride(0), out.data_ptr(), n, V, a.off.data_ptr(), a.tok.data_ptr(),
                                        a.nxt.data_ptr(), a.label.data_ptr(), n_states, n_edges, int(a.pad_token_id), st.state.data_ptr(),
                                        st.fin.data_ptr(), st.len.data_ptr(), st.choice.data_ptr(), st.score.data_ptr() if score else None,
                                        _stream()), "constrain_rows")
    return out


class BeamState:
    """Device state of one beam search over B rows x nb beams (include/lhrs_hip.h: lhrs_beam_step), initialised as HF's _beam_search does."""

    def __init__(self, B, nb, V, max_new, length_penalty, device):
        R = B * nb
        i32, f32 = dict(device=device, dtype=torch.int32), dict(device=device, dtype=torch.float32)
        self.B, self.nb, self.V, self.max_new, self.K = B, nb, V, max_new, 2 * nb
        self.bstate = torch.zeros(4, **i32)                       # {t, done, -, -}
        run = torch.full((B, nb), -1.0e9, dtype=torch.float32)
        run[:, 0] = 0.0
        self.run_score = h2d(run.reshape(-1), device)
        self.parent = torch.zeros(R, **i32)
        self.hist = torch.zeros((2, R, max_new), **i32)
        self.fin_score = torch.full((R,), -1.0e9, **f32)
        self.fin_len = torch.zeros(R, **i32)
        self.fin_slot = h2d(torch.arange(nb, dtype=torch.int32).repeat(B), device)
        self.fin_seq = torch.zeros((R, max_new), **i32)
        self.heur = torch.ones(B, **i32)
        self.cand_score = torch.zeros((R, self.K), **f32)
        self.cand_tok = torch.zeros((R, self.K), **i32)
        # n ** length_penalty as HF forms it (a Python float) and as its fp32 division sees it
        self.len_pow = h2d(torch.tensor([1.0] + [float(n) ** float(length_penalty) for n in range(1, max_new + 1)], dtype=torch.float64).to(torch.float32),
                           device)

    def buffers(self):
        return (self.bstate, self.run_score, self.parent, self.hist, self.fin_score, self.fin_len, self.fin_slot, self.fin_seq, self.heur,
                self.cand_score, self.cand_tok)


def beam_topk_rows(logits_f32, st: BeamState, repetition_penalty=1.0):
    """lhrs_beam_topk_rows: per running beam the top 2 * nb of log_softmax(logits) (+ penalty over the beam's history) + running score
    -> st.cand_score / st.cand_tok [B * nb, K]"""
    n, V = logits_f32.shape
    _req(logits_f32, torch.float32, "logits")
    assert logits_f32.stride(1) == 1 and n == st.B * st.nb and V == st.V, f"logits {tuple(logits_f32.shape)} for B={st.B} nb={st.nb} V={st.V}"
    _lib.check(_L().lhrs_beam_topk_rows(logits_f32.data_ptr(), logits_f32.stride(0), n, V, st.K, st.run_score.data_ptr(), float(repetition_penalty),
                                        st.hist.data_ptr(), st.max_new, st.bstate.data_ptr(), st.cand_score.data_ptr(), st.cand_tok.data_ptr(),
                                        _stream()), "beam_topk_rows")
    return st.cand_score, st.cand_tok


def beam_step(st: BeamState, next_ids, eos_token_id=None, early_stopping=False):
    """lhrs_beam_step: merge st.cand_*, advance the running beams / finished set / flags of every row; next_ids int64 [B * nb] is where
    decode_emit reads the tokens of the new running beams"""
    _req(next_ids, torch.int64, "next_ids")
    assert next_ids.is_contiguous() and next_ids.numel() == st.B * st.nb
    _lib.check(_L().lhrs_beam_step(st.cand_score.data_ptr(), st.cand_tok.data_ptr(), st.B, st.nb, st.V, st.max_new,
                                   -1 if eos_token_id is None else int(eos_token_id), int(bool(early_stopping)), st.len_pow.data_ptr(),
                                   st.run_score.data_ptr(), st.parent.data_ptr(), next_ids.data_ptr(), st.hist.data_ptr(), st.fin_score.data_ptr(),
                                   st.fin_len.data_ptr(), st.fin_slot.data_ptr(), st.fin_seq.data_ptr(), st.heur.data_ptr(), st.bstate.data_ptr(),
                                   _stream()), "beam_step")


def kv_cache_table(caches, device):
    """int64 device array of the base pointers of every K and V cache (built once per session) for kv_beam_reorder"""
    return h2d(torch.tensor([c.data_ptr() for kv in caches for c in kv], dtype=torch.int64), device)


def kv_beam_reorder(table, B, nb, max_ctx, d, parent, t0, t1, max_pos, done=None):
    """lhrs_kv_beam_reorder: cache row [b * nb + j] takes positions [t0, t1) of row [b * nb + parent[b * nb + j]], in place, in every cache of
    `table`.  t1: an int, or a 1-element int32 device tensor (the session's context length: the captured launch stays valid for every step)."""
    _req(table, torch.int64, "table")
    _req(parent, torch.int32, "parent")
    assert parent.is_contiguous() and parent.numel() == B * nb
    t1_dev = t1 if isinstance(t1, torch.Tensor) else None
    if t1_dev is not None:
        _req(t1_dev, torch.int32, "t1")
    _lib.check(_L().lhrs_kv_beam_reorder(table.data_ptr(), table.numel(), B, nb, max_ctx, d, parent.data_ptr(), int(t0), _p(t1_dev),
                                         0 if t1_dev is not None else int(t1), int(max_pos), _p(done), _stream()), "kv_beam_reorder")


def cross_entropy(logits, target, want_grad=True, inplace=True):
    n, V = logits.shape
    row_loss = torch.empty(n, device=logits.device, dtype=torch.float32)
    loss = torch.empty((), device=logits.device, dtype=torch.float32)
    dl = None
    if want_grad:
        dl = logits if inplace else torch.empty_like(logits)
    st = _L().lhrs_cross_entropy(logits.data_ptr(), logits.stride(0), target.data_ptr(), row_loss.data_ptr(), loss.data_ptr(),
                                 _p(dl), dl.stride(0) if dl is not None else 0, n, V, _stream())
    _lib.check(st, "cross_entropy")
    return loss, dl


# --------------------------------------------------------------------------------------------- decode
def gemv(W, x, out, residual=None, out_f32=False):
    """out[B, N] = x[B, K] @ W[N, K]^T (+ residual): weight-streaming kernels of the decode step (batch 1: VALU dot products, batch 2..16: MFMA with the batch as N)."""
    B, K = x.shape
    N = W.shape[0]
    st = _L().lhrs_gemv_bf16(W.data_ptr(), W.stride(0), x.data_ptr(), x.stride(0), _p(residual),
                             residual.stride(0) if residual is not None else 0, out.data_ptr(), out.stride(0), B, N, K, int(out_f32),
                             _stream())
    _lib.check(st, "gemv_bf16")
    return out


PRO_NONE, PRO_RMSNORM, PRO_SWIGLU = 0, 1, 2


class PackedBf16:
    """bf16 weight [N, K] re-tiled by `repack_bf16_mfma` into the operand order of the batched MFMA GEMV (batch >= 2 decode)."""

    def __init__(self, data, N, K):
        self.data, self.N, self.K = data, N, K
        self.shape = (N, K)


def repack_bf16_mfma(W) -> PackedBf16:
    N, K = W.shape
    out = torch.empty((N + 15) // 16 * 16 * K, device=W.device, dtype=torch.bfloat16)
    _lib.check(_L().lhrs_repack_bf16_mfma(W.data_ptr(), W.stride(0), out.data_ptr(), N, K, _stream()), "repack_bf16_mfma")
    return PackedBf16(out, N, K)


def gemv_fused(W, x, out, K, *, wscale=None, prologue=PRO_NONE, norm_w=None, eps=1e-5, residual=None, out_f32=False):
    """out[B, N] = pro(x)[B, K] @ W[N, K]^T (+ residual).  W: bf16 [N, K], (wscale given) e4m3 bytes [N, K] with per-row scales, or a
    PackedBf16 (batch >= 2)."""
    B, N = x.shape[0], W.shape[0]
    if isinstance(W, PackedBf16):
        wp, ldw, fmt = W.data.data_ptr(), 0, 2
    else:
        wp, ldw, fmt = W.data_ptr(), W.stride(0), int(wscale is not None)
    st = _L().lhrs_gemv(wp, ldw, _p(wscale), fmt, x.data_ptr(), x.stride(0), prologue, _p(norm_w),
                        float(eps), _p(residual), residual.stride(0) if residual is not None else 0, out.data_ptr(), out.stride(0), B, N, K,
                        int(out_f32), _stream())
    _lib.check(st, "gemv")
    return out


class PackedFp8:
    """e4m3 weight [N, K] re-tiled by `repack_fp8_mfma` into the operand order of the MFMA GEMV (decode weight stream)."""

    def __init__(self, data, N, K):
        self.data, self.N, self.K = data, N, K
        self.shape = (N, K)


def repack_fp8_mfma(W8) -> PackedFp8:
    N, K = W8.shape
    out = torch.empty((N + 15) // 16 * 16 * K, device=W8.device, dtype=torch.uint8)
    _lib.check(_L().lhrs_repack_fp8_mfma(W8.data_ptr(), W8.stride(0), out.data_ptr(), N, K, _stream()), "repack_fp8_mfma")
    return PackedFp8(out, N, K)


def _w8(W8):  # -> (ptr, ldw, N, packed)
    if isinstance(W8, PackedFp8):
        return W8.data.data_ptr(), 0, W8.N, 1
    return W8.data_ptr(), W8.stride(0), W8.shape[0], 0


def gemv_fp8_mfma(W8, wscale, x8, xscale, out, *, residual=None, out_f32=False):
    """out[B, N] = xscale[:, None] * wscale[None, :] * (x8 @ W8^T) (+ residual): e4m3 weights and activations on the scaled MFMA.
    W8: uint8 [N, K] rows or a PackedFp8."""
    B, K = x8.shape
    wp, ldw, N, pk = _w8(W8)
    st = _L().lhrs_gemv_fp8_mfma(wp, ldw, wscale.data_ptr(), x8.data_ptr(), x8.stride(0), xscale.data_ptr(),
                                 _p(residual), residual.stride(0) if residual is not None else 0, out.data_ptr(), out.stride(0), B, N, K,
                                 int(out_f32), pk, _stream())
    _lib.check(st, "gemv_fp8_mfma")
    return out


def gemv_fp8_mfma_fused(W8, wscale, x, out, K, *, prologue=PRO_NONE, norm_w=None, eps=1e-5, residual=None, out_f32=False):
    """batch <= 2: out = (e4m3(pro(x)) @ W8^T) * scales (+ residual), prologue and activation quantisation inside the kernel."""
    B = x.shape[0]
    wp, ldw, N, pk = _w8(W8)
    st = _L().lhrs_gemv_fp8_mfma_fused(wp, ldw, wscale.data_ptr(), x.data_ptr(), x.stride(0), prologue, _p(norm_w),
                                       float(eps), _p(residual), residual.stride(0) if residual is not None else 0, out.data_ptr(),
                                       out.stride(0), B, N, K, int(out_f32), pk, _stream())
    _lib.check(st, "gemv_fp8_mfma_fused")
    return out


def quant_fp8_rows(W, out=None):
    """bf16 [N, K] -> (uint8 e4m3 [N, K], fp32 per-row scale [N]); out = preallocated (W8, scale) for graph-captured callers."""
    N, K = W.shape
    W8, sc = out if out is not None else (torch.empty((N, K), device=W.device, dtype=torch.uint8),
                                          torch.empty(N, device=W.device, dtype=torch.float32))
    _lib.check(_L().lhrs_quant_fp8_rows(W.data_ptr(), W.stride(0), W8.data_ptr(), W8.stride(0), sc.data_ptr(), N, K, _stream()), "quant_fp8_rows")
    return W8, sc


def rope_kv_append(qkv, kc, vc, cos_t, sin_t, pos, B, H, D, max_ctx):
    _lib.check(_L().lhrs_rope_kv_append(qkv.data_ptr(), qkv.stride(0), kc.data_ptr(), vc.data_ptr(), cos_t.data_ptr(), sin_t.data_ptr(),
                                        pos.data_ptr(), B, H, D, max_ctx, _stream()), "rope_kv_append")


def _key_mask_args(key_mask):
    """pointer and row stride of the HF attention_mask bytes the decode attention entry points take (NULL, 0 without a mask)"""
    return _p(key_mask), key_mask.stride(0) if key_mask is not None else 0


def _check_split_buffers(part, tickets, B, H, nsplit):
    assert part.dtype == torch.float32 and part.numel() >= B * H * nsplit * 132 and tickets.dtype == torch.int32 and tickets.numel() >= B * H


def decode_attn(qkv, kc, vc, cos_t, sin_t, pos, out, B, H, D, max_ctx, scale, key_mask=None):
    """RoPE(new q, k) + KV append + attention over the cache for one new token per sequence, one launch (lhrs_decode_attn)."""
    st = _L().lhrs_decode_attn(qkv.data_ptr(), qkv.stride(0), kc.data_ptr(), vc.data_ptr(), cos_t.data_ptr(), sin_t.data_ptr(), pos.data_ptr(),
                               *_key_mask_args(key_mask), out.data_ptr(), out.stride(0), B, H, D, max_ctx, float(scale), _stream())
    _lib.check(st, "decode_attn")
    return out


def decode_attn_split(qkv, kc, vc, cos_t, sin_t, pos, out, B, H, D, max_ctx, scale, nsplit, part, tickets, key_mask=None, cs=None):
    """decode_attn with the context split over `nsplit` workgroups per head (lhrs_decode_attn_split); part fp32 [B, H, nsplit, 132],
    tickets int32 [B, H] (zero before the first call)."""
    _check_split_buffers(part, tickets, B, H, nsplit)
    st = _L().lhrs_decode_attn_split(qkv.data_ptr(), qkv.stride(0), kc.data_ptr(), vc.data_ptr(), cos_t.data_ptr(), sin_t.data_ptr(),
                                     pos.data_ptr(), *_key_mask_args(key_mask), out.data_ptr(), out.stride(0), B, H, D, max_ctx, float(scale),
                                     int(nsplit), part.data_ptr(), tickets.data_ptr(), _p(cs), _stream())
    _lib.check(st, "decode_attn_split")
    return out


def kv8_quant_rows(src, codes, scales, row0, H):
    """lhrs_kv8_quant_rows: bf16 rows src [n, H * 128] (any row stride: a column block of a qkv buffer in place) -> the codes and scale
    bytes of the cache rows row0 .. row0 + n - 1"""
    _req(src, torch.bfloat16, "src")
    _req(codes, torch.uint8, "codes")
    _req(scales, torch.uint8, "scales")
    n = src.shape[0]
    assert src.shape[1] == H * 128 and src.stride(1) == 1 and codes.is_contiguous() and scales.is_contiguous()
    assert codes.shape[1] == H * 128 and scales.shape[1] == H and 0 <= row0 and row0 + n <= codes.shape[0] and codes.shape[0] == scales.shape[0]
    _lib.check(_L().lhrs_kv8_quant_rows(src.data_ptr(), src.stride(0), codes.data_ptr(), scales.data_ptr(), int(row0), n, H, _stream()),
               "kv8_quant_rows")


def kv8_dequant_rows(codes, scales, row0, n, H, out):
    """lhrs_kv8_dequant_rows: the cache rows row0 .. row0 + n - 1 (codes uint8 [rows, H * 128], scales uint8 [rows, H]) -> the first n rows
    of `out`, bf16 [>= n, H * 128] with any row stride: e4m3(code) * 2^(byte - 127), exact in bf16"""
    _req(codes, torch.uint8, "codes")
    _req(scales, torch.uint8, "scales")
    _req(out, torch.bfloat16, "out")
    row0, n = int(row0), int(n)
    assert out.dim() == 2 and out.shape[1] == H * 128 and out.stride(1) == 1 and out.shape[0] >= n and codes.is_contiguous() and scales.is_contiguous()
    assert codes.shape[1] == H * 128 and scales.shape[1] == H and 0 <= row0 and row0 + n <= codes.shape[0] and codes.shape[0] == scales.shape[0]
    _lib.check(_L().lhrs_kv8_dequant_rows(codes.data_ptr(), scales.data_ptr(), row0, n, H, out.data_ptr(), out.stride(0), _stream()),
               "kv8_dequant_rows")
    return out


def decode_attn_kv8(qkv, kc8, vc8, ks, vs, cos_t, sin_t, pos, out, B, H, D, max_ctx, scale, nsplit=1, part=None, tickets=None, key_mask=None,
                    cs=None):
    """decode_attn / decode_attn_split on the kv8 caches (lhrs_decode_attn_kv8): kc8 / vc8 uint8 [B * max_ctx, H * 128], ks / vs uint8
    [B * max_ctx, H]; nsplit > 1 needs part fp32 [B, H, nsplit, 132] and tickets int32 [B, H] (zero before the first call)."""
    for t, name in ((kc8, "kc8"), (vc8, "vc8"), (ks, "ks"), (vs, "vs")):
        _req(t, torch.uint8, name)
        assert t.is_contiguous() and t.shape[0] >= B * max_ctx and t.shape[1] == (H * D if t is kc8 or t is vc8 else H), name
    if nsplit > 1:
        _check_split_buffers(part, tickets, B, H, nsplit)
    st = _L().lhrs_decode_attn_kv8(qkv.data_ptr(), qkv.stride(0), kc8.data_ptr(), vc8.data_ptr(), ks.data_ptr(), vs.data_ptr(), cos_t.data_ptr(),
                                   sin_t.data_ptr(), pos.data_ptr(), *_key_mask_args(key_mask), out.data_ptr(), out.stride(0), B, H, D, max_ctx,
                                   float(scale), int(nsplit), _p(part), _p(tickets), _p(cs), _stream())
    _lib.check(st, "decode_attn_kv8")
    return out


def decode_advance(state, desc, pos, B, max_ctx, inc=1, cos_t=None, sin_t=None, cs=None):
    """cs (float32 [B, 128]) with the tables: also leave the cos | sin rows of the new position there (lhrs_decode_advance_cs)"""
    if cs is not None:
        _lib.check(_L().lhrs_decode_advance_cs(state.data_ptr(), desc.data_ptr(), pos.data_ptr(), cos_t.data_ptr(), sin_t.data_ptr(), cs.data_ptr(),
                                               B, max_ctx, inc, _stream()), "decode_advance_cs")
        return
    _lib.check(_L().lhrs_decode_advance(state.data_ptr(), desc.data_ptr(), pos.data_ptr(), B, max_ctx, inc, _stream()), "decode_advance")


def kv_append(qkv, kc, vc, pos, B, d, max_ctx):
    _lib.check(_L().lhrs_kv_append(qkv.data_ptr(), qkv.stride(0), kc.data_ptr(), vc.data_ptr(), pos.data_ptr(), B, d, max_ctx, _stream()),
               "kv_append")


def decode_emit(next_ids, tok32, out_ids, state, B, max_new):
    _lib.check(_L().lhrs_decode_emit(next_ids.data_ptr(), tok32.data_ptr(), out_ids.data_ptr(), state.data_ptr(), B, max_new, _stream()),
               "decode_emit")


class HipGraph:
    """hipGraph capture / replay of the launches enqueued on the current (non-default) HIP stream."""

    def __init__(self):
        self.exec = None

    def begin(self):
        _lib.check(_L().lhrs_graph_begin(_stream()), "graph_begin")

    def end(self):
        import ctypes
        h = ctypes.c_void_p()
        _lib.check(_L().lhrs_graph_end(_stream(), ctypes.byref(h)), "graph_end")
        self.exec = h.value

    def launch(self):
        _lib.check(_L().lhrs_graph_launch(self.exec, _stream()), "graph_launch")

    def __del__(self):
        try:
            if self.exec:
                _L().lhrs_graph_destroy(self.exec)
        except Exception:
            pass


# --------------------------------------------------------------------------------------------- optimizer
def sqnorm(g, out, accumulate=False):
    nb = _L().lhrs_sqnorm_nblk(g.numel())
    part = torch.empty(nb, device=g.device, dtype=torch.float32)
    _lib.check(_L().lhrs_sqnorm(g.data_ptr(), g.numel(), part.data_ptr(), out.data_ptr(), int(accumulate), _stream()), "sqnorm")
    return out


def accum_f32(y, x, copy_only=False):
    """y = x (copy_only) or y += x on flat fp32 buffers (gradient accumulation)."""
    assert y.dtype == torch.float32 and x.dtype == torch.float32 and y.numel() == x.numel()
    _lib.check(_L().lhrs_accum_f32(y.data_ptr(), x.data_ptr(), y.numel(), int(copy_only), _stream()), "accum_f32")
    return y


def adan_step(p, g, m, v, n, pre, shadow, step, lr, betas=(0.98, 0.92, 0.99), eps=1e-8, wd=0.0, no_prox=True,
              gnorm_sq=None, max_norm=0.0, grad_scale=1.0):
    st = _L().lhrs_adan_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n.data_ptr(), pre.data_ptr(), _p(shadow),
                             p.numel(), step, lr, betas[0], betas[1], betas[2], eps, wd, int(no_prox), _p(gnorm_sq), max_norm,
                             grad_scale, _stream())
    _lib.check(st, "adan_step")


def adamw_step(p, g, m, v, shadow, step, lr, betas=(0.9, 0.95), eps=1e-8, wd=0.0, gnorm_sq=None, max_norm=0.0, grad_scale=1.0):
    st = _L().lhrs_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _p(shadow), p.numel(), step, lr, betas[0],
                              betas[1], eps, wd, _p(gnorm_sq), max_norm, grad_scale, _stream())
    _lib.check(st, "adamw_step")


# --------------------------------------------------------------------------------------------- data boundary (images)
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def image_preprocess(img_u8: torch.Tensor, out: torch.Tensor = None, short_edge: int = 224, crop_round: int = 0, rescale_mode: int = 0,
                     mean=CLIP_MEAN, std=CLIP_STD) -> torch.Tensor:
    """uint8 [H, W, 3] device tensor -> float32 [3, 224, 224]: Pillow-BICUBIC resize of the short edge to `short_edge`, centre crop,
    byte -> float, (x - mean) / std (lhrs_image_preprocess; the defaults are CLIPImageProcessor, bit-exact)."""
    assert img_u8.dtype == torch.uint8 and img_u8.dim() == 3 and img_u8.shape[2] == 3 and img_u8.is_cuda and img_u8.stride(2) == 1 \
        and img_u8.stride(1) == 3, "image_preprocess: uint8 [H, W, 3] device tensor with packed pixels"
    H, W = int(img_u8.shape[0]), int(img_u8.shape[1])
    if out is None:
        out = torch.empty((3, 224, 224), device=img_u8.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == 3 * 224 * 224
    nbytes = _L().lhrs_image_preprocess_workspace(H, W, short_edge)
    if nbytes < 0:
        raise ValueError(f"image_preprocess: H={H} W={W} short_edge={short_edge} (short_edge must be >= 224)")
    ws = torch.empty(nbytes, device=img_u8.device, dtype=torch.uint8)
    m, sd = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    st = _L().lhrs_image_preprocess(img_u8.data_ptr(), H, W, img_u8.stride(0), out.data_ptr(), ws.data_ptr(), nbytes, short_edge, crop_round,
                                    rescale_mode, ctypes.cast(m, ctypes.c_void_p), ctypes.cast(sd, ctypes.c_void_p), _stream())
    _lib.check(st, "image_preprocess")
    return out


def clip_preprocess(img_u8: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """uint8 [H, W, 3] device tensor -> float32 [3, 224, 224] pixel_values, bit-exact with CLIPImageProcessor."""
    return image_preprocess(img_u8, out)


# ------------------------------------------------------------------------------------------------ LLM.int8 base (csrc/int8.hip)
def quant_int8_rows(W):
    """bf16 [N, K] -> (int8 [N, K], fp32 [N] dequantisation factor absmax / 127): bitsandbytes' vector-wise weight quantisation."""
    N, K = W.shape
    Q = torch.empty((N, K), device=W.device, dtype=torch.int8)
    sc = torch.empty(N, device=W.device, dtype=torch.float32)
    _lib.check(_L().lhrs_quant_int8_rows(W.data_ptr(), W.stride(0), Q.data_ptr(), Q.stride(0), sc.data_ptr(), N, K, _stream()), "quant_int8_rows")
    return Q, sc


def dequant_int8_rows(Q, sc, out=None):
    N, K = Q.shape
    out = torch.empty((N, K), device=Q.device, dtype=torch.bfloat16) if out is None else out
    _lib.check(_L().lhrs_dequant_int8_rows(Q.data_ptr(), Q.stride(0), sc.data_ptr(), out.data_ptr(), out.stride(0), N, K, _stream()), "dequant_int8_rows")
    return out


# --------------------------------------------------------------------------------------------- 4-bit base storage (bits: 4)
def dynamic_map_8bit() -> torch.Tensor:
    """The sorted 256-entry table of bitsandbytes' signed "dynamic" 8-bit data type (functional.create_dynamic_map(signed=True,
    max_exponent_bits=7, total_bits=8)) that `double_quant` stores the absmax statistics in: for i = 0..6 the 2^i midpoints of
    linspace(0.1, 1, 2^i + 1) scaled by 10^(i - 6), both signs, plus 0 and 1.  fp32 CPU tensor."""
    data = []
    for i in range(7):
        b = torch.linspace(0.1, 1, 2 ** i + 1)
        means = (b[:-1] + b[1:]) / 2.0
        data += ((10 ** (-6 + i)) * means).tolist()
        data += (-(10 ** (-6 + i)) * means).tolist()
    data += [0.0, 1.0]
    assert len(data) == 256
    return torch.tensor(sorted(data), dtype=torch.float32)


_DYN_MAP = {}


def _dyn_map(device) -> torch.Tensor:
    key = str(device)
    if key not in _DYN_MAP:
        _DYN_MAP[key] = dynamic_map_8bit().to(device)
    return _DYN_MAP[key]


def quant4_blocks(W, quant_type: str = "nf4", double_quant: bool = True):
    """bitsandbytes quantize_4bit of ONE weight (a contiguous bf16 [N, K] tensor or row range, N*K % 64 == 0) -> state dict:
    packed uint8 [N*K/2], and either absmax fp32 [N*K/64] or (double_quant) its 8-bit form: qabsmax uint8, absmax2 fp32, offset."""
    if quant_type not in ("nf4", "fp4"):
        raise ValueError(f"quant_type {quant_type!r}: 'nf4' or 'fp4' (bitsandbytes bnb_4bit_quant_type)")
    _req(W, torch.bfloat16, "quant4_blocks weight")
    if not W.is_contiguous():
        raise ValueError("quant4_blocks: the weight (row range) must be contiguous")
    n = W.numel()
    packed = torch.empty(n // 2, device=W.device, dtype=torch.uint8)
    absmax = torch.empty(n // 64, device=W.device, dtype=torch.float32)
    _lib.check(_L().lhrs_quant4_blocks(W.data_ptr(), n, int(quant_type == "fp4"), packed.data_ptr(), absmax.data_ptr(), _stream()), "quant4_blocks")
    st = dict(packed=packed, quant_type=quant_type, shape=tuple(W.shape))
    if not double_quant:
        st["absmax"] = absmax
        return st
    nb = absmax.numel()
    offset = float(absmax.double().mean().float())   # the package: absmax.mean() in fp32; the fp64 sum makes the value independent of the reduction order
    rest = absmax - offset
    q = torch.empty(nb, device=W.device, dtype=torch.uint8)
    absmax2 = torch.empty((nb + 255) // 256, device=W.device, dtype=torch.float32)
    _lib.check(_L().lhrs_quant8_dynamic(rest.data_ptr(), nb, _dyn_map(W.device).data_ptr(), q.data_ptr(), absmax2.data_ptr(), _stream()), "quant8_dynamic")
    st.update(qabsmax=q, absmax2=absmax2, offset=offset)
    return st


def absmax_of(st) -> torch.Tensor:
    """The fp32 block absmax a 4-bit state dequantises with (double_quant: code[q] * absmax2 + offset)."""
    if "absmax" in st:
        return st["absmax"]
    q = st["qabsmax"]
    out = torch.empty(q.numel(), device=q.device, dtype=torch.float32)
    _lib.check(_L().lhrs_dequant8_dynamic(q.data_ptr(), st["absmax2"].data_ptr(), q.numel(), _dyn_map(q.device).data_ptr(), float(st["offset"]),
                                          out.data_ptr(), _stream()), "dequant8_dynamic")
    return out


def dequant4_blocks(st, out=None):
    """bitsandbytes dequantize_4bit: table[code] * absmax -> bf16, into `out` (contiguous, same element count) or a new tensor of the stored shape."""
    packed = st["packed"]
    n = packed.numel() * 2
    out = torch.empty(st["shape"], device=packed.device, dtype=torch.bfloat16) if out is None else out
    if out.numel() != n or not out.is_contiguous() or out.dtype != torch.bfloat16:
        raise ValueError("dequant4_blocks: `out` must be a contiguous bf16 tensor with the element count of the state")
    a = absmax_of(st)
    _lib.check(_L().lhrs_dequant4_blocks(packed.data_ptr(), a.data_ptr(), n, int(st["quant_type"] == "fp4"), out.data_ptr(), _stream()), "dequant4_blocks")
    return out


class Packed4:
    """One fused decoder weight [N, K] as the decode GEMV reads it from the 4-bit base: `codes` uint8 [N, K/2] (two codes per byte, even element
    in the high nibble), `absmax` fp32 [N, K/64], `fp4` (False: NF4 levels).  Made by `pack4_decode`."""

    def __init__(self, codes, absmax, fp4, N, K):
        self.codes, self.absmax, self.fp4 = codes, absmax, bool(fp4)
        self.N, self.K = N, K
        self.shape = (N, K)


def pack4_decode(states, N: int, K: int) -> Packed4:
    """The per-Linear 4-bit states of ONE fused weight (`L[name + "q4"]`: row-concatenated parts, each a contiguous row range) -> Packed4.
    The codes are the stored ones, concatenated; the block statistics are `absmax_of` of each part, so `double_quant` statistics are expanded
    to fp32 once, here.  Nothing is quantised anew."""
    if K % 64 or not states:
        raise ValueError(f"pack4_decode: K={K} must be a multiple of the block size 64 and the state list non-empty")
    kinds = {st["quant_type"] for st in states}
    if len(kinds) != 1:
        raise ValueError(f"pack4_decode: the parts of one weight mix quant types {sorted(kinds)}")
    codes = torch.cat([st["packed"].reshape(-1) for st in states]).reshape(-1, K // 2)
    absmax = torch.cat([absmax_of(st).reshape(-1) for st in states]).reshape(-1, K // 64)
    if codes.shape[0] != N or absmax.shape[0] != N:
        raise ValueError(f"pack4_decode: the states hold {codes.shape[0]} rows of {K}, expected {N}")
    return Packed4(codes.contiguous(), absmax.contiguous(), kinds.pop() == "fp4", N, K)


def gemv4(W4: Packed4, x, out, K, *, prologue=PRO_NONE, norm_w=None, eps=1e-5, residual=None, out_f32=False):
    """out[B, N] = pro(x)[B, K] @ w[N, K]^T (+ residual), w = bf16(level[code] * absmax) formed in registers from the 4-bit codes: what
    `gemv_fused` computes on `dequant4_blocks` of the same states, up to the order of the fp32 sums.  Keywords as `gemv_fused`."""
    if K != W4.K:
        raise ValueError(f"gemv4: K={K} but the packed weight has K={W4.K}")
    _req(W4.codes, torch.uint8, "gemv4 codes")
    _req(W4.absmax, torch.float32, "gemv4 absmax")
    _req(x, torch.bfloat16, "gemv4 x")
    _req(out, torch.float32 if out_f32 else torch.bfloat16, "gemv4 out")
    B = x.shape[0]
    if x.dim() != 2 or x.shape[1] != (2 * K if prologue == PRO_SWIGLU else K) or x.stride(1) != 1:
        raise ValueError(f"gemv4: x {tuple(x.shape)} for K={K}, prologue {prologue} (SwiGLU reads [B, 2K]); rows must be dense")
    if tuple(out.shape) != (B, W4.N) or out.stride(1) != 1:
        raise ValueError(f"gemv4: out {tuple(out.shape)}, expected ({B}, {W4.N}) with dense rows")
    if residual is not None:
        _req(residual, torch.bfloat16, "gemv4 residual")
        if tuple(residual.shape) != (B, W4.N) or residual.stride(1) != 1:
            raise ValueError(f"gemv4: residual {tuple(residual.shape)}, expected ({B}, {W4.N}) with dense rows")
    if prologue == PRO_RMSNORM:
        if norm_w is None or norm_w.numel() != K or not norm_w.is_contiguous():
            raise ValueError(f"gemv4: the RMSNorm prologue needs a contiguous norm_w of {K} elements")
        _req(norm_w, torch.bfloat16, "gemv4 norm_w")
    if tuple(W4.codes.shape) != (W4.N, K // 2) or tuple(W4.absmax.shape) != (W4.N, K // 64) or W4.codes.stride(1) != 1 or W4.absmax.stride(1) != 1:
        raise ValueError(f"gemv4: codes {tuple(W4.codes.shape)} / absmax {tuple(W4.absmax.shape)} for a weight of shape {W4.shape}")
    st = _L().lhrs_gemv4(W4.codes.data_ptr(), W4.codes.stride(0), W4.absmax.data_ptr(), W4.absmax.stride(0), int(W4.fp4), x.data_ptr(), x.stride(0),
                         prologue, _p(norm_w), float(eps), _p(residual), residual.stride(0) if residual is not None else 0, out.data_ptr(),
                         out.stride(0), B, W4.N, K, int(out_f32), _stream())
    _lib.check(st, "gemv4")
    return out


# --------------------------------------------------------------------------------------------- decode from MXFP4 weights
def quant_mx4_rows(W, out=None):
    """bf16 [N, K] (K % 32 == 0) -> (codes uint8 [N, K/2], scales uint8 [N, K/32]): OCP MXFP4.  Element k of a row sits in byte k/2, even k in
    the low nibble; a code is `s m m m` (sign, index into {0, .5, 1, 1.5, 2, 3, 4, 6}); a block of 32 consecutive k shares the e8m0 scale
    2^(byte - 127) with byte = clamp(floor(log2 max|v|) - 2 + 127, 0, 254) (OCP MX v1.0; a zero block: 127 and +0 codes).  Elements round to
    the nearest level, ties to the even code, saturating at +-6.  out = preallocated (codes, scales), rows may be strided."""
    _req(W, torch.bfloat16, "quant_mx4_rows W")
    N, K = W.shape
    codes, scales = out if out is not None else (torch.empty((N, K // 2), device=W.device, dtype=torch.uint8),
                                                 torch.empty((N, max(K // 32, 1)), device=W.device, dtype=torch.uint8))
    if W.stride(1) != 1 or codes.stride(1) != 1 or scales.stride(1) != 1:
        raise ValueError("quant_mx4_rows: rows must be dense")
    _lib.check(_L().lhrs_quant_mx4_rows(W.data_ptr(), W.stride(0), codes.data_ptr(), codes.stride(0), scales.data_ptr(), scales.stride(0), N, K,
                                        _stream()), "quant_mx4_rows")
    return codes, scales


def dequant_mx4_rows(codes, scales, out=None):
    """(codes [N, K/2], scales [N, K/32]) of `quant_mx4_rows` -> bf16 [N, K] = level * 2^(byte - 127), exact in bf16."""
    _req(codes, torch.uint8, "dequant_mx4_rows codes")
    _req(scales, torch.uint8, "dequant_mx4_rows scales")
    N, K = codes.shape[0], codes.shape[1] * 2
    if out is None:
        out = torch.empty((N, K), device=codes.device, dtype=torch.bfloat16)
    _req(out, torch.bfloat16, "dequant_mx4_rows out")
    if tuple(out.shape) != (N, K) or tuple(scales.shape) != (N, K // 32) or out.stride(1) != 1 or codes.stride(1) != 1 or scales.stride(1) != 1:
        raise ValueError(f"dequant_mx4_rows: codes {tuple(codes.shape)}, scales {tuple(scales.shape)}, out {tuple(out.shape)} with dense rows")
    _lib.check(_L().lhrs_dequant_mx4_rows(codes.data_ptr(), codes.stride(0), scales.data_ptr(), scales.stride(0), out.data_ptr(), out.stride(0), N, K,
                                          _stream()), "dequant_mx4_rows")
    return out


class PackedMX4:
    """MXFP4 weight [N, K] in the operand order of the decode GEMV (`repack_mx4_mfma`): `codes_t` uint8 [ceil(N/16), K/128, 64, 16] - lane
    (r, g) of a 128-k step holds the 16 code bytes of block 4 step + g of row 16 rg + r - and `scales_t` uint8 [ceil(N/16), ceil(K/512), 64, 4] -
    byte j of a lane's dword t is the scale of its block in step 4 t + j.  Rows past N: zero codes, scale byte 127."""

    def __init__(self, codes_t, scales_t, N, K):
        self.codes_t, self.scales_t, self.N, self.K = codes_t, scales_t, N, K
        self.shape = (N, K)

    def nbytes(self) -> int:
        return self.codes_t.numel() + self.scales_t.numel()


def repack_mx4_mfma(codes, scales, out=None) -> PackedMX4:
    """row-major (codes, scales) -> PackedMX4 (K % 128 == 0); out = preallocated (codes_t, scales_t) of exactly the tiled sizes."""
    _req(codes, torch.uint8, "repack_mx4_mfma codes")
    _req(scales, torch.uint8, "repack_mx4_mfma scales")
    N, K = codes.shape[0], codes.shape[1] * 2
    if tuple(scales.shape) != (N, K // 32) or codes.stride(1) != 1 or scales.stride(1) != 1:
        raise ValueError(f"repack_mx4_mfma: codes {tuple(codes.shape)} / scales {tuple(scales.shape)}: expected [N, K/2] and [N, K/32] with dense rows")
    G, S = (N + 15) // 16, K // 128
    if out is None:
        out = (torch.empty((G, S, 64, 16), device=codes.device, dtype=torch.uint8), torch.empty((G, (S + 3) // 4, 64, 4), device=codes.device, dtype=torch.uint8))
    ct, st = out
    if K % 128 == 0 and (ct.numel() != G * S * 1024 or st.numel() != G * ((S + 3) // 4) * 256 or not ct.is_contiguous() or not st.is_contiguous()):
        raise ValueError(f"repack_mx4_mfma: out of {ct.numel()} + {st.numel()} bytes for N={N}, K={K}")
    _lib.check(_L().lhrs_repack_mx4_mfma(codes.data_ptr(), codes.stride(0), scales.data_ptr(), scales.stride(0), ct.data_ptr(), st.data_ptr(), N, K,
                                         _stream()), "repack_mx4_mfma")
    return PackedMX4(ct, st, N, K)


def _mx4_out(what, W, B, out, residual, out_f32):
    _req(W.codes_t, torch.uint8, what + " codes_t")
    _req(W.scales_t, torch.uint8, what + " scales_t")
    _req(out, torch.float32 if out_f32 else torch.bfloat16, what + " out")
    G, S = (W.N + 15) // 16, W.K // 128
    if W.K % 128 == 0 and (W.codes_t.numel() != G * S * 1024 or W.scales_t.numel() != G * ((S + 3) // 4) * 256):
        raise ValueError(f"{what}: the tiled buffers do not belong to a weight of shape {W.shape}")
    if tuple(out.shape) != (B, W.N) or out.stride(1) != 1:
        raise ValueError(f"{what}: out {tuple(out.shape)}, expected ({B}, {W.N}) with dense rows")
    if residual is not None:
        _req(residual, torch.bfloat16, what + " residual")
        if tuple(residual.shape) != (B, W.N) or residual.stride(1) != 1:
            raise ValueError(f"{what}: residual {tuple(residual.shape)}, expected ({B}, {W.N}) with dense rows")


def gemv_mx4(W: PackedMX4, x8, xscale, out, *, residual=None, out_f32=False):
    """out[B, N] = xscale[:, None] * (x8 @ w^T) (+ residual), w = the MXFP4 weight, dequantised by the block-scaled MFMA itself; x8 / xscale are
    the per-row e4m3 activations of `quant_fp8_rows` / `rmsnorm_fwd_q` / `swiglu_fwd_q`.  1 <= B <= 16, K % 128 == 0."""
    _req(x8, torch.uint8, "gemv_mx4 x8")
    _req(xscale, torch.float32, "gemv_mx4 xscale")
    B, K = x8.shape
    if K != W.K or x8.stride(1) != 1 or xscale.numel() < B:
        raise ValueError(f"gemv_mx4: x8 {tuple(x8.shape)} / xscale {tuple(xscale.shape)} for a weight of shape {W.shape}; rows must be dense")
    _mx4_out("gemv_mx4", W, B, out, residual, out_f32)
    st = _L().lhrs_gemv_mx4(W.codes_t.data_ptr(), W.scales_t.data_ptr(), x8.data_ptr(), x8.stride(0), xscale.data_ptr(), _p(residual),
                            residual.stride(0) if residual is not None else 0, out.data_ptr(), out.stride(0), B, W.N, K, int(out_f32), _stream())
    _lib.check(st, "gemv_mx4")
    return out


def gemv_mx4_fused(W: PackedMX4, x, out, K, *, prologue=PRO_NONE, norm_w=None, eps=1e-5, residual=None, out_f32=False):
    """batch <= 2: out = xscale * (e4m3(pro(x)) @ w^T) (+ residual), prologue and per-row activation quantisation inside the kernel, as in
    `gemv_fp8_mfma_fused`."""
    _req(x, torch.bfloat16, "gemv_mx4_fused x")
    B = x.shape[0]
    if K != W.K or x.dim() != 2 or x.shape[1] != (2 * K if prologue == PRO_SWIGLU else K) or x.stride(1) != 1:
        raise ValueError(f"gemv_mx4_fused: x {tuple(x.shape)} for a weight of shape {W.shape}, prologue {prologue} (SwiGLU reads [B, 2K]); rows must be dense")
    if prologue == PRO_RMSNORM:
        if norm_w is None or norm_w.numel() != K or not norm_w.is_contiguous():
            raise ValueError(f"gemv_mx4_fused: the RMSNorm prologue needs a contiguous norm_w of {K} elements")
        _req(norm_w, torch.bfloat16, "gemv_mx4_fused norm_w")
    _mx4_out("gemv_mx4_fused", W, B, out, residual, out_f32)
    st = _L().lhrs_gemv_mx4_fused(W.codes_t.data_ptr(), W.scales_t.data_ptr(), x.data_ptr(), x.stride(0), prologue, _p(norm_w), float(eps),
                                  _p(residual), residual.stride(0) if residual is not None else 0, out.data_ptr(), out.stride(0), B, W.N, K,
                                  int(out_f32), _stream())
    _lib.check(st, "gemv_mx4_fused")
    return out


class PackedI8:
    """int8 weight rows [N, K] of `quant_int8_rows` re-tiled by `repack_int8_mfma` into the operand order of `gemv_int8`: int8
    [ceil(N/16), K/64, 64, 16] - lane (r, g) of a 64-k step holds WQ[16 rg + r][64 step + 16 g .. +16]; rows past N are zero."""

    def __init__(self, data, N, K):
        self.data, self.N, self.K = data, N, K
        self.shape = (N, K)

    def nbytes(self) -> int:
        return self.data.numel()


def repack_int8_mfma(WQ) -> PackedI8:
    """int8 [N, K] rows -> PackedI8 (K % 64 == 0)."""
    _req(WQ, torch.int8, "repack_int8_mfma WQ")
    if WQ.dim() != 2 or WQ.stride(1) != 1:
        raise ValueError(f"repack_int8_mfma: WQ {tuple(WQ.shape)}: expected [N, K] with dense rows")
    N, K = WQ.shape
    out = torch.empty(((N + 15) // 16, max(K // 64, 1), 64, 16), device=WQ.device, dtype=torch.int8)
    _lib.check(_L().lhrs_repack_int8_mfma(WQ.data_ptr(), WQ.stride(0), out.data_ptr(), N, K, _stream()), "repack_int8_mfma")
    return PackedI8(out, N, K)


class Int8DecodeWorkspace:
    """Static buffers of the activation side of the int8 decode linears (`int8_decode_prepare` writes them, `gemv_int8` reads them), for up to
    `B` rows of up to `kmax` columns: codes, row factors, the outlier column list, the gathered 16-bit activations and meta = [n]."""

    def __init__(self, device, B: int, kmax: int, threshold: float = 6.0):
        self.threshold, self.B, self.kmax = float(threshold), B, (kmax + 63) // 64 * 64
        self.xq = torch.zeros((B, self.kmax), device=device, dtype=torch.int8)
        self.sx = torch.zeros(B, device=device, dtype=torch.float32)
        self.idx = torch.zeros(self.kmax, device=device, dtype=torch.int32)
        self.xo = torch.zeros((B, self.kmax), device=device, dtype=torch.bfloat16)
        self.meta = torch.zeros(2, device=device, dtype=torch.int32)


def int8_decode_prepare(x, K, ws: Int8DecodeWorkspace, *, prologue=PRO_NONE, norm_w=None, eps=1e-5, h_out=None):
    """The activation side of one decode linear on the LLM.int8 base in one launch (1 <= B <= 16): h = pro(x) (x is [B, 2K] for the SwiGLU
    prologue), then what `lhrs_int8_prepare` computes on h, into `ws`: ws.xq[:B, :K], ws.sx[:B], ws.idx[:n], ws.xo[:B, :n], ws.meta[0] = n.
    h_out: optional bf16 [B, K] that receives h."""
    _req(x, torch.bfloat16, "int8_decode_prepare x")
    if x.dim() != 2:
        raise ValueError(f"int8_decode_prepare: x {tuple(x.shape)}: expected [B, K] ([B, 2K] for the SwiGLU prologue)")
    B = x.shape[0]
    if x.shape[1] != (2 * K if prologue == PRO_SWIGLU else K) or x.stride(1) != 1:
        raise ValueError(f"int8_decode_prepare: x {tuple(x.shape)} for K={K}, prologue {prologue} (SwiGLU reads [B, 2K]); rows must be dense")
    if B > ws.B or K > ws.kmax:
        raise ValueError(f"int8_decode_prepare: {B} rows x {K} columns, the workspace holds {ws.B} x {ws.kmax}")
    if prologue == PRO_RMSNORM:
        if norm_w is None or norm_w.numel() != K or not norm_w.is_contiguous():
            raise ValueError(f"int8_decode_prepare: the RMSNorm prologue needs a contiguous norm_w of {K} elements")
        _req(norm_w, torch.bfloat16, "int8_decode_prepare norm_w")
    if h_out is not None:
        _req(h_out, torch.bfloat16, "int8_decode_prepare h_out")
        if tuple(h_out.shape) != (B, K) or h_out.stride(1) != 1:
            raise ValueError(f"int8_decode_prepare: h_out {tuple(h_out.shape)}, expected ({B}, {K}) with dense rows")
    st = _L().lhrs_int8_decode_prepare(x.data_ptr(), x.stride(0), int(prologue), _p(norm_w), float(eps), ws.threshold, _p(h_out),
                                       h_out.stride(0) if h_out is not None else 0, ws.xq.data_ptr(), ws.xq.stride(0), ws.sx.data_ptr(),
                                       ws.idx.data_ptr(), ws.meta.data_ptr(), ws.xo.data_ptr(), ws.xo.stride(0), B, K, _stream())
    _lib.check(st, "int8_decode_prepare")
    return ws


def gemv_int8(WQ, wscale, ws: Int8DecodeWorkspace, out, K, *, residual=None, out_f32=False):
    """out[B, N] = f32(ws.xq @ WQ^T) * fl(ws.sx[b] * wscale[n]) + ws.xo[:, :n] @ bf16(WQ[:, ws.idx[:n]] * wscale)^T (+ residual), n = ws.meta[0]
    read on the device; the int8 sum is exact (v_mfma_i32_16x16x64_i8), the 16-bit outlier term accumulates in fp32, one rounding at the store.
    WQ: int8 [N, K] rows or a PackedI8; wscale fp32 [N] (`quant_int8_rows`); ws as left by `int8_decode_prepare`.  1 <= B <= 16, K % 64 == 0."""
    _req(wscale, torch.float32, "gemv_int8 wscale")
    _req(out, torch.float32 if out_f32 else torch.bfloat16, "gemv_int8 out")
    if isinstance(WQ, PackedI8):
        wp, ldw, N, pk = WQ.data.data_ptr(), 0, WQ.N, 1
        if WQ.K != K or WQ.data.numel() != (N + 15) // 16 * 16 * K:
            raise ValueError(f"gemv_int8: the tiled buffer does not belong to a weight of shape ({N}, {K})")
    else:
        _req(WQ, torch.int8, "gemv_int8 WQ")
        if WQ.dim() != 2 or WQ.shape[1] != K or WQ.stride(1) != 1:
            raise ValueError(f"gemv_int8: WQ {tuple(WQ.shape)} for K={K}; rows must be dense")
        wp, ldw, N, pk = WQ.data_ptr(), WQ.stride(0), WQ.shape[0], 0
    if out.dim() != 2:
        raise ValueError(f"gemv_int8: out {tuple(out.shape)}: expected [B, {N}]")
    B = out.shape[0]
    if out.shape[1] != N or out.stride(1) != 1 or B > ws.B or K > ws.kmax or wscale.numel() < N:
        raise ValueError(f"gemv_int8: out {tuple(out.shape)} / wscale {tuple(wscale.shape)} for a weight of shape ({N}, {K}) and a workspace "
                         f"of {ws.B} x {ws.kmax}; rows must be dense")
    if residual is not None:
        _req(residual, torch.bfloat16, "gemv_int8 residual")
        if tuple(residual.shape) != (B, N) or residual.stride(1) != 1:
            raise ValueError(f"gemv_int8: residual {tuple(residual.shape)}, expected ({B}, {N}) with dense rows")
    st = _L().lhrs_gemv_int8(wp, ldw, pk, wscale.data_ptr(), ws.xq.data_ptr(), ws.xq.stride(0), ws.sx.data_ptr(), ws.idx.data_ptr(),
                             ws.meta.data_ptr(), ws.xo.data_ptr(), ws.xo.stride(0), _p(residual), residual.stride(0) if residual is not None else 0,
                             out.data_ptr(), out.stride(0), B, N, K, int(out_f32), _stream())
    _lib.check(st, "gemv_int8")
    return out


# --------------------------------------------------------------------------------------------- decode with live adapters
LORA_DOWN_MAX_SLICES = 16
LORA_DOWN_MAX_LDS = 160 * 1024 - 16   # bytes of staged activations a lora_down workgroup can hold (the CU's LDS less the kernel's static words)


def lora_down_splits(K: int, R: int) -> int:
    """K-slices `lora_down` cuts a [R, K] stacked A into (1..16; a pure function of the shape)."""
    return int(_L().lhrs_lora_down_splits(int(K), int(R)))


def lora_down_lds_bytes(B: int, K: int, R: int) -> int:
    """bytes of LDS a `lora_down` workgroup stages: B rows of one K-slice in bf16 (the library rejects more than LORA_DOWN_MAX_LDS)"""
    nsl = lora_down_splits(K, R)
    return B * (-(-(K // 64) // nsl) * 64) * 2


def lora_down(x, A, tpart, K, R=None, *, prologue=PRO_NONE, norm_w=None, eps=1e-5) -> int:
    """tpart[i, b, j] = sum over K-slice i of pro(x)[b, k] * A[j, k] (fp32 [nsl, B, R], every element written) -> nsl.  A: bf16 [>= R, K] rows
    (the stacked A of a fused group; R = the rows in use, default all); prologue / norm_w / eps as `gemv_fused`.  tpart: a contiguous fp32
    buffer of at least nsl * B * R elements (a session sizes it for LORA_DOWN_MAX_SLICES)."""
    _req(x, torch.bfloat16, "lora_down x")
    _req(A, torch.bfloat16, "lora_down A")
    _req(tpart, torch.float32, "lora_down tpart")
    B = x.shape[0]
    R = A.shape[0] if R is None else int(R)
    if x.dim() != 2 or x.shape[1] != (2 * K if prologue == PRO_SWIGLU else K) or x.stride(1) != 1:
        raise ValueError(f"lora_down: x {tuple(x.shape)} for K={K}, prologue {prologue} (SwiGLU reads [B, 2K]); rows must be dense")
    if A.dim() != 2 or A.shape[0] < R or A.shape[1] != K or A.stride(1) != 1:
        raise ValueError(f"lora_down: A {tuple(A.shape)}, expected at least ({R}, {K}) with dense rows")
    if prologue == PRO_RMSNORM:
        if norm_w is None or norm_w.numel() != K or not norm_w.is_contiguous():
            raise ValueError(f"lora_down: the RMSNorm prologue needs a contiguous norm_w of {K} elements")
        _req(norm_w, torch.bfloat16, "lora_down norm_w")
    nsl = lora_down_splits(K, R)
    if not tpart.is_contiguous() or tpart.numel() < nsl * B * R:
        raise ValueError(f"lora_down: tpart holds {tpart.numel()} floats, {nsl} slices x {B} x {R} are written")
    st = _L().lhrs_lora_down(x.data_ptr(), x.stride(0), prologue, _p(norm_w), float(eps), A.data_ptr(), A.stride(0), tpart.data_ptr(), B, R, K, _stream())
    _lib.check(st, "lora_down")
    return nsl


def lora_up(acc, tpart, nsl, s, Bw, r, fout, out, *, residual=None, R=None):
    """out[b, n] = bf16(acc[b, n] + sum_{j in cols(n)} t[b, j] * Bw[n, j] (+ residual[b, n])), t = bf16(s * sum_i tpart[i, b, :]) and
    cols(n) = [(n // fout) * r, +r): only that block of the block-diagonal Bw = Bfull [N, >= R] is read (r == R and fout == N: dense).
    acc: fp32 [B, N], the base product of the same linear (`gemv_fused` / `gemv4` / `gemv_fp8_mfma*` with out_f32 and no residual)."""
    _req(acc, torch.float32, "lora_up acc")
    _req(tpart, torch.float32, "lora_up tpart")
    _req(Bw, torch.bfloat16, "lora_up Bw")
    _req(out, torch.bfloat16, "lora_up out")
    B, N = out.shape
    R = (N // fout) * r if R is None else int(R)
    if tuple(acc.shape) != (B, N) or acc.stride(1) != 1 or out.stride(1) != 1:
        raise ValueError(f"lora_up: acc {tuple(acc.shape)} / out {tuple(out.shape)} must both be [B, N] with dense rows")
    if Bw.dim() != 2 or Bw.shape[0] < N or Bw.shape[1] < (N // fout) * r or Bw.stride(1) != 1:
        raise ValueError(f"lora_up: Bw {tuple(Bw.shape)} for N={N}, {N // fout} blocks of r={r} columns")
    if not tpart.is_contiguous() or tpart.numel() < nsl * B * R:
        raise ValueError(f"lora_up: tpart holds {tpart.numel()} floats, {nsl} slices x {B} x {R} are read")
    if residual is not None:
        _req(residual, torch.bfloat16, "lora_up residual")
        if tuple(residual.shape) != (B, N) or residual.stride(1) != 1:
            raise ValueError(f"lora_up: residual {tuple(residual.shape)}, expected ({B}, {N}) with dense rows")
    st = _L().lhrs_lora_up(acc.data_ptr(), acc.stride(0), tpart.data_ptr(), int(nsl), float(s), Bw.data_ptr(), Bw.stride(0), int(r), int(fout),
                           _p(residual), residual.stride(0) if residual is not None else 0, out.data_ptr(), out.stride(0), B, N, R, _stream())
    _lib.check(st, "lora_up")
    return out


class Int8Workspace:
    """Device scratch of the LLM.int8 activation side: outlier flags per input feature, the compacted outlier column list, meta = [columns
    found by the last call, that count rounded up to 64] and the persistent [N, KP + K] buffers of the dequantised outlier weight columns."""

    def __init__(self, device, kmax: int = 32768, threshold: float = 6.0):
        self.threshold, self.kmax = float(threshold), (kmax + 63) // 64 * 64
        self.flags = torch.zeros(self.kmax, device=device, dtype=torch.int32)
        self.idx = torch.full((self.kmax,), -1, device=device, dtype=torch.int32)
        self.meta = torch.zeros(2, device=device, dtype=torch.int32)
        self._b2 = {}

    def b2(self, N: int, cols: int):
        key = (N, cols)
        if key not in self._b2:
            self._b2[key] = torch.empty((N, cols), device=self.flags.device, dtype=torch.bfloat16)
        return self._b2[key]

    def last_outlier_columns(self):
        """Host read (synchronises): the outlier feature columns of the most recent product, ascending."""
        n = int(self.meta[0].item())
        return self.idx[:n].tolist()


def int8_linear(x, WQ, wscale, ws: Int8Workspace, *, residual=None, a2=None, b2=None, alpha: float = 1.0, out=None):
    """bitsandbytes MatMul8bitLt forward: y = (int8(x') . WQ^T) * sx * wscale + x[:, O] . dequant(WQ)[:, O]^T (+ a2 . b2^T) (+ residual), O = the
    columns of x holding a value >= ws.threshold (however many there are), x' = x with those columns zeroed.  x bf16 [M, K]; WQ int8 [N, K] +
    wscale [N] from quant_int8_rows; (a2 [M, KP], b2 [N, KP]) an optional bf16 pair (LoRA update) riding on the same accumulators."""
    M, K = x.shape
    N = WQ.shape[0]
    KP = a2.shape[1] if a2 is not None else 0
    kpad = (K + 63) // 64 * 64
    assert kpad <= ws.kmax, (K, ws.kmax)
    xq = torch.empty((M, K), device=x.device, dtype=torch.int8)
    sx = torch.empty(M, device=x.device, dtype=torch.float32)
    A2 = torch.empty((M, KP + kpad), device=x.device, dtype=torch.bfloat16)
    B2 = ws.b2(N, KP + kpad)
    if KP:
        A2[:, :KP].copy_(a2)
        B2[:, :KP].copy_(b2)
    L = _L()
    _lib.check(L.lhrs_int8_prepare(x.data_ptr(), x.stride(0), M, K, ws.threshold, WQ.data_ptr(), WQ.stride(0), wscale.data_ptr(), N,
                                   xq.data_ptr(), xq.stride(0), sx.data_ptr(), ws.flags.data_ptr(), ws.idx.data_ptr(), ws.meta.data_ptr(),
                                   A2.data_ptr() + 2 * KP, A2.stride(0), B2.data_ptr() + 2 * KP, B2.stride(0), _stream()), "int8_prepare")
    out = torch.empty((M, N), device=x.device, dtype=torch.bfloat16) if out is None else out
    _lib.check(L.lhrs_gemm_int8_nt(xq.data_ptr(), xq.stride(0), sx.data_ptr(), WQ.data_ptr(), WQ.stride(0), wscale.data_ptr(), A2.data_ptr(),
                                   A2.stride(0), B2.data_ptr(), B2.stride(0), KP, ws.meta.data_ptr() + 4, out.data_ptr(), out.stride(0), M, N, K,
                                   _p(residual), residual.stride(0) if residual is not None else 0, float(alpha), _stream()), "gemm_int8_nt")
    return out
