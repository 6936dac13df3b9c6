"""The LLM.int8 base (csrc/int8.hip, gemm_fp8_256_kernel<true> of csrc/gemm.hip, hk.int8_linear) restated for tests/test_int8_cases_cpu.py,
tests/test_int8_paths_gpu.py and the int8 table of tests/test_gemm_paths_gpu.py.  Imports no GPU and shares no code with the HIP sources.

Three things live here:

  * ref_quant_rows / ref_prepare / ref_linear: the expected values.  Everything lhrs_quant_int8_rows and lhrs_int8_prepare write is a
    function of bf16 inputs through single correctly rounded fp32 operations (absmax, 127 / absmax, x * inv, rint, absmax / 127,
    code * scale rounded to bf16), so it has ONE right answer and is compared bit for bit.  numpy does the fp32 arithmetic (torch's
    vectorised CPU division is not correctly rounded, see oracle/int8_oracle.py::_codes).  The linear is the float64 value of
        alpha * (sx[m] sw[n] sum_k XQ WQ + A2 . B2^T + a2 . b2^T) + residual
    as a gemm_cases.Ref, judged by gemm_cases.check("bf16", ...).
  * emu_prepare / emu_product / emu_linear: a plain-torch model of the device pipeline (workspace state included) that takes a set of
    mutations.  tests/test_int8_cases_cpu.py shows that the unmutated model passes every comparison of the GPU tests and that every
    mutant fails a named case - the cases below were chosen so that each of them matters.
  * the case tables.  Each case names the edge it exists for.

Bounds (none of them measured on the kernel):
  prepare, weight side, k-mapping probe    exact equality
  linear, int8 GEMM                        gemm_cases.BOUNDS["bf16"] = (4.5, 4.5, 7.2e-3): the project's existing bound of bf16 GEMM results
  int8 GEMM without pair and residual      |got - want| <= (2^-8 + 2^-21) |want|: one bf16 round-to-nearest (2^-8 relative at the bottom
                                           of a binade) and four fp32 roundings (int32 -> f32, sa * alpha, the two factor products:
                                           (1 + 2^-24)^4 - 1 < 2^-21); the integer sum is exact, so there is no accumulation term
  int8 product without pair                additionally bit-equal to emu_product: with exact integer sums every operation behind them has
                                           one correctly rounded result (this is what tells "residual added before the bf16 store" apart)
Worst values of the int8 cases on an MI355X (element ratio at c_out = c_acc = 1 | cell rel-L2; bounds 4.5 | 7.2e-3), measured with these
tests on top of commit 6997d05 (the kernels are unchanged by them):
  lhrs_gemm_int8_nt   min_shape_no_pair 0.413 | 2.0e-3 (0.843 of the derived (2^-8 + 2^-21) |want|)   ragged_device_stage 0.481 | 1.8e-3
                      odd_stages_host_pair_device_zero_res_alpha 0.903 | 2.3e-3    odd_plus_odd_stages_res 0.831 | 2.6e-3
                      long_k_device_stage 0.362 | 1.7e-3                           device_count_equals_k 0.484 | 1.7e-3
  hk.int8_linear      m33_n264_k256_n0 0.493 | 1.7e-3    m70_n520_k384_n65_lora 0.859 | 2.4e-3    m5_n64_k24832_n3 0.289 | 1.5e-3
                      reuse 130 / 0 / 1 outlier columns: 0.455 | 1.7e-3, 0.490 | 1.7e-3, 0.421 | 1.7e-3
Every exact comparison (prepare, weight side, k-mapping probe, products without a bf16 stage against emu_product) held bit for bit.
"""
import math
from collections import namedtuple

import numpy as np
import torch

import gemm_cases as gc

THR = 6.0
BELOW_THR = 5.96875            # the largest bf16 below 6.0 (bf16 spacing in [4, 8) is 2^-5)
QCH_K = 24576                  # int8.hip keeps 12 x 256 16-byte chunks of a row in registers; columns from here on take the streaming loop
NAN = float("nan")

def ceil64(n):
    return (n + 63) // 64 * 64


def bits16(t):
    return t.contiguous().view(torch.int16)


def bits32(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------- references

def _np32(t):
    return t.detach().cpu().float().numpy().astype(np.float32)


def _codes_np(x32, absmax32):
    """rint(x * fl(127 / absmax)) clipped to +-127 in IEEE fp32; absmax == 0 -> inv = 0 (the kernel's rule: all codes 0)."""
    with np.errstate(divide="ignore"):
        inv = np.where(absmax32 > 0, np.float32(127.0) / absmax32, np.float32(0.0)).astype(np.float32)
    q = np.rint((x32 * inv[:, None]).astype(np.float32))
    return np.clip(q, -127, 127).astype(np.int8)


def ref_quant_rows(w):
    """bf16 [N, K] -> (codes int8 [N, K], scale fp32 [N] = absmax / 127 (0 for an all-zero row), dequantised bf16 [N, K])."""
    w32 = _np32(w)
    absmax = np.abs(w32).max(axis=1).astype(np.float32)
    q = _codes_np(w32, absmax)
    scale = (absmax / np.float32(127.0)).astype(np.float32)
    deq = (q.astype(np.float32) * scale[:, None]).astype(np.float32)
    return torch.from_numpy(q), torch.from_numpy(scale), torch.from_numpy(deq).to(torch.bfloat16)


Prepared = namedtuple("Prepared", "cols n n_pad idx sx XQ A2 B2 mask8")


def ref_prepare(x, wq, wscale, thr=THR):
    """What lhrs_int8_prepare must write for bf16 x [M, K], int8 wq [N, K], fp32 wscale [N]:
    cols (ascending list), n, n_pad = ceil64(n), idx int32 [n_pad] (-1 in [n, n_pad)), sx fp32 [M] = max{|x| : |x| < thr} / 127 (0.0 for a
    row without a counted non-zero entry - NOT the oracle's clamp_min(1e-30)), XQ int8 [M, K] with the outlier columns zeroed,
    A2 bf16 [M, n_pad] = x[:, idx], B2 bf16 [N, n_pad] = bf16(float(wq[:, idx]) * wscale), zeros under -1; mask8 uint8 [K / 8]: bit e of
    byte c = column 8 c + e."""
    x32 = _np32(x)
    M, K = x32.shape
    ax = np.abs(x32)
    out_col = (ax >= np.float32(thr)).any(axis=0)
    cols = np.nonzero(out_col)[0].astype(np.int32)
    n = int(cols.size)
    n_pad = ceil64(n)
    idx = np.full(n_pad, -1, dtype=np.int32)
    idx[:n] = cols
    absmax = np.where(ax < np.float32(thr), ax, np.float32(0.0)).max(axis=1).astype(np.float32)
    sx = (absmax / np.float32(127.0)).astype(np.float32)
    xq = _codes_np(x32, absmax)
    xq[:, out_col] = 0
    A2 = torch.zeros(M, n_pad, dtype=torch.bfloat16)
    B2 = torch.zeros(wq.shape[0], n_pad, dtype=torch.bfloat16)
    if n:
        ci = torch.from_numpy(cols).long()
        A2[:, :n] = x.cpu()[:, ci]
        b = (wq.cpu().numpy()[:, cols].astype(np.float32) * _np32(wscale)[:, None]).astype(np.float32)
        B2[:, :n] = torch.from_numpy(b).to(torch.bfloat16)
    mask8 = torch.from_numpy(np.packbits(out_col.reshape(K // 8, 8), axis=1, bitorder="little").reshape(-1).copy())
    return Prepared(cols.tolist(), n, n_pad, torch.from_numpy(idx), torch.from_numpy(sx), torch.from_numpy(xq), A2, B2, mask8)


def ref_int8(A8, sa, B8, sb, *, alpha=1.0, residual=None, A2=None, B2=None):
    """alpha * (sa[m] sb[n] (A8 . B8^T) + A2 . B2^T) + residual in float64 on int8 codes (lhrs_gemm_int8_nt)."""
    a = A8.double() * sa.double()[:, None]
    b = B8.double() * sb.double()[:, None]
    if A2 is not None and A2.shape[1] == 0:
        A2 = B2 = None
    return gc.ref_nt(a, b, alpha=alpha, residual=residual, A2=A2, B2=B2)


def ref_linear(x, wq, wscale, thr=THR, *, a2=None, b2=None, residual=None, alpha=1.0):
    """float64 value of hk.int8_linear as a gemm_cases.Ref; the bf16 pair is the LoRA columns followed by the n_pad outlier columns."""
    p = ref_prepare(x, wq, wscale, thr)
    A2, B2 = p.A2, p.B2
    if a2 is not None:
        A2, B2 = torch.cat([a2.cpu(), A2], 1), torch.cat([b2.cpu(), B2], 1)
    return ref_int8(p.XQ, p.sx, wq.cpu(), wscale.cpu(), alpha=alpha, residual=None if residual is None else residual.cpu(), A2=A2, B2=B2)


def tight_bound_ok(got, want):
    """|got - want| <= (2^-8 + 2^-21) |want| per element (int8 GEMM without pair and residual) -> (ok, worst error / bound)."""
    err = (got.double().cpu() - want.cpu()).abs()
    bound = (2.0 ** -8 + 2.0 ** -21) * want.cpu().abs()
    finite = bool(torch.isfinite(got).all())
    ratio = float((err / bound.clamp_min(1e-300)).max())
    return finite and bool((err <= bound).all()), ratio


# ---------------------------------------------------------------------------------------------------------------------- emulation

MUTANTS = ("absmax_counts_outlier_entries", "absmax_skips_outlier_columns", "outlier_columns_not_zeroed", "gt_instead_of_ge",
           "round_half_away_from_zero", "last_row_skipped_by_column_scan", "idx_pad_zero", "n_pad_is_n", "bf16_stage_dropped",
           "bf16_stage_doubled", "k_half_of_a_fragment_dropped", "stale_meta", "residual_before_bf16_store")


class EmuWorkspace:
    """Model of hk.Int8Workspace: idx, meta and the persistent B2 buffers survive a call; what torch.empty would return holds NaN."""

    def __init__(self, kmax):
        self.kmax = ceil64(kmax)
        self.idx = torch.full((self.kmax,), -1, dtype=torch.int32)
        self.meta = [0, 0]
        self.prev_meta = [0, 0]
        self._b2 = {}

    def b2(self, N, cols):
        if (N, cols) not in self._b2:
            self._b2[(N, cols)] = torch.full((N, cols), NAN, dtype=torch.bfloat16)
        return self._b2[(N, cols)]


def _f32_div(a, b):
    """fp32 quotient through float64 (a, b are bf16-valued or 127: the double rounding is harmless, the CPU tests compare with numpy)"""
    return (a.double() / b.double()).float()


def emu_prepare(x, wq, wscale, ws, A2, B2, thr=THR, mut=()):
    """The six steps of lhrs_int8_prepare in torch: column scan, compaction into ws.idx / ws.meta, row absmax + codes, the two gathers
    into the first meta[1] columns of A2 [M, >= kpad] / B2 [N, >= kpad].  -> (XQ int8 [M, K], sx fp32 [M], mask bool [K])."""
    xf = x.float()
    M, K = xf.shape
    ax = xf.abs()
    hit = ax > thr if "gt_instead_of_ge" in mut else ax >= thr
    mask = (hit[:-1] if "last_row_skipped_by_column_scan" in mut else hit).any(0)
    cols = mask.nonzero().flatten()
    n = int(cols.numel())
    n_pad = n if "n_pad_is_n" in mut else ceil64(n)
    ws.prev_meta = list(ws.meta)
    ws.idx[:n] = cols.int()
    ws.idx[n:n_pad] = 0 if "idx_pad_zero" in mut else -1
    ws.meta = [n, n_pad]
    counted = torch.ones_like(hit) if "absmax_counts_outlier_entries" in mut else ax < thr
    if "absmax_skips_outlier_columns" in mut:
        counted = counted & ~mask[None, :]
    absmax = torch.where(counted, ax, torch.zeros_like(ax)).amax(1)
    sx = _f32_div(absmax, torch.tensor(127.0))
    inv = torch.where(absmax > 0, _f32_div(torch.tensor(127.0), absmax.clamp_min(1e-38)), torch.zeros_like(absmax))
    p = xf * inv[:, None]
    q = torch.sign(p) * torch.floor(p.abs() + 0.5) if "round_half_away_from_zero" in mut else torch.round(p)
    q = q.clamp(-127, 127)
    if "outlier_columns_not_zeroed" not in mut:
        q = q.masked_fill(mask[None, :], 0.0)
    k = ws.idx[:n_pad].long()
    live = (k >= 0)[None, :]
    kc = k.clamp_min(0)
    A2[:, :n_pad] = torch.where(live, x[:, kc], torch.zeros((), dtype=torch.bfloat16))
    B2[:, :n_pad] = torch.where(live, (wq[:, kc].float() * wscale[:, None]).to(torch.bfloat16), torch.zeros((), dtype=torch.bfloat16))
    return q.to(torch.int8), sx, mask


def emu_product(XQ, sx, WQ, sw, A2, B2, K2, *, alpha=1.0, residual=None, mut=()):
    """gemm_fp8_256_kernel<true> in its order: exact integer sum -> one f32 conversion -> the two factors -> K2 / 64 bf16 stages accumulated
    in f32 -> alpha -> bf16 store -> residual added in bf16 after the store.  Without bf16 stages: acc * (sa * alpha) * sb."""
    acc = XQ.long() @ WQ.long().t()
    if "k_half_of_a_fragment_dropped" in mut:     # bytes [16, 32) of the first 32-byte fragment of every row
        acc = acc - XQ[:, 16:32].long() @ WQ[:, 16:32].long().t()
    f = acc.float()
    a32 = torch.tensor(alpha, dtype=torch.float32)
    stages = list(range(K2 // 64))
    if "bf16_stage_dropped" in mut and stages:
        stages = stages[:-1]
    if "bf16_stage_doubled" in mut and stages:
        stages = stages + stages[-1:]
    if K2 // 64 > 0:
        f = f * (sx[:, None] * sw[None, :])
        for s in stages:
            f = f + A2[:, 64 * s:64 * s + 64].float() @ B2[:, 64 * s:64 * s + 64].float().t()
        v = f * a32
    else:
        v = f * (sx * a32)[:, None] * sw[None, :]
    if residual is not None and "residual_before_bf16_store" in mut:
        return (v + residual.float()).to(torch.bfloat16)
    y = v.to(torch.bfloat16)
    if residual is not None:
        y = (y.float() + residual.float()).to(torch.bfloat16)
    return y


def emu_linear(x, wq, wscale, ws, *, a2=None, b2=None, residual=None, alpha=1.0, thr=THR, mut=()):
    """hk.int8_linear: fresh A2 (NaN where torch.empty leaves garbage), the workspace's persistent B2, prepare, product."""
    M, K = x.shape
    N = wq.shape[0]
    KP = a2.shape[1] if a2 is not None else 0
    kpad = ceil64(K)
    A2 = torch.full((M, KP + kpad), NAN, dtype=torch.bfloat16)
    B2 = ws.b2(N, KP + kpad)
    if KP:
        A2[:, :KP] = a2
        B2[:, :KP] = b2
    XQ, sx, _ = emu_prepare(x, wq, wscale, ws, A2[:, KP:], B2[:, KP:], thr, mut)
    k2_dev = ws.prev_meta[1] if "stale_meta" in mut else ws.meta[1]
    return emu_product(XQ, sx, wq, wscale, A2, B2, KP + k2_dev, alpha=alpha, residual=residual, mut=mut)


# ---------------------------------------------------------------------------------------------------------------------- inputs

VALS = (6.0, -6.0, 7.5, -9.0, 30.0, -6.03125)      # planted outliers; the first two sit exactly on the threshold


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def base_x(g, M, K):
    """bf16 [M, K], |x| <= 5.5: no accidental outlier"""
    return (torch.randn(M, K, generator=g) * 1.5).clamp(-5.5, 5.5).to(torch.bfloat16)


def outlier_columns(K, n, g):
    """n columns, ascending: K - 1 and 0 first, then 1 (same mask byte as 0), 31 and 32 (either side of a 32-bit mask word), then random"""
    if n >= K:
        return list(range(K))
    special = list(dict.fromkeys(c for c in (K - 1, 0, 1, 31, 32) if 0 <= c < K))[:n]
    rest = [c for c in torch.randperm(K, generator=g).tolist() if c not in special][:n - len(special)]
    return sorted(special + rest)


def make_x(seed, M, K, n, first=0):
    """base_x with n outlier columns; column j of them has its ONLY outlier in row 0 or row M - 1, alternating (first = 1: starts in M - 1)"""
    g = _gen(seed)
    x = base_x(g, M, K)
    for j, c in enumerate(outlier_columns(K, n, g)):
        x[(0, M - 1)[(j + first) % 2], c] = VALS[j % len(VALS)]
    return x


def make_w(seed, N, K):
    return (torch.randn(N, K, generator=_gen(seed)) * 0.02).to(torch.bfloat16)


def tie_values(absmax):
    """Positive bf16 values below absmax whose fp32 product with fl(127 / absmax) is exactly k + 0.5 with k even and < 127: half-to-even
    gives k, half-away-from-zero k + 1, and an inverse one ulp off gives either.  numpy float32 array."""
    inv = np.float32(127.0) / np.float32(absmax)
    cand = torch.arange(0x0100, 0x7F80, dtype=torch.int16).view(torch.bfloat16).float().numpy().astype(np.float32)
    cand = cand[cand < np.float32(absmax)]
    p = (cand * inv).astype(np.float32)
    fl = np.floor(p)
    return cand[(p - fl == np.float32(0.5)) & (fl % 2 == 0) & (p < 127)]


def count_ties(x, thr=THR, mask_outliers=True, even=True):
    """entries of bf16 x whose fp32 product with the row's inverse is exactly k + 0.5 (even = True: k even, where half-away-from-zero and
    half-to-even differ), in columns that are not zeroed"""
    x32 = _np32(x)
    ax = np.abs(x32)
    absmax = np.where(ax < np.float32(thr), ax, np.float32(0)).max(axis=1) if mask_outliers else ax.max(axis=1)
    with np.errstate(divide="ignore"):
        inv = np.where(absmax > 0, np.float32(127.0) / absmax.astype(np.float32), np.float32(0)).astype(np.float32)
    p = np.abs((x32 * inv[:, None]).astype(np.float32))
    fl = np.floor(p)
    tie = (p - fl == np.float32(0.5)) & ((fl % 2 == 0) | (not even)) & (p < 127)
    if mask_outliers:
        tie = tie & ~(ax >= np.float32(thr)).any(axis=0)[None, :]
    return int(tie.sum())


TIE_ABSMAX = (3.96875, 0.9921875)      # 127 / 32 and 127 / 128: the inverse is a power of two, x = (2 k + 1) / (2 inv) lands on k + 0.5
HALF_ABSMAX = 0.0810546875             # fl(127 / absmax) is inexact; x = absmax / 2 still gives exactly 63.5 under a correctly rounded inverse
                                       # (one ulp low, as a reciprocal approximation or torch's vectorised division give, makes it 63.49...)


def tie_row(K, absmax, g):
    """a row of K values with row maximum absmax made of tie values of both signs (zeros where there are too few)"""
    t = tie_values(absmax)
    assert t.size > 0, absmax
    pick = torch.from_numpy(t)[torch.randint(0, t.size, (K,), generator=g)]
    sign = torch.where(torch.rand(K, generator=g) < 0.5, -1.0, 1.0)
    row = (pick * sign).to(torch.bfloat16)
    row[K // 2] = absmax
    return row


def half_row(K, absmax, g):
    """random values with row maximum absmax; every eighth entry is +-absmax / 2, whose product is exactly 63.5"""
    row = (torch.randn(K, generator=g) * absmax / 3).clamp(-absmax, absmax).to(torch.bfloat16)
    row[::8] = torch.tensor([absmax / 2, -absmax / 2] * K, dtype=torch.bfloat16)[:row[::8].numel()]
    row[K // 2] = absmax
    return row


# ---------------------------------------------------------------------------------------------------------------------- prepare cases

PrepCase = namedtuple("PrepCase", "name edge M K N n build")


def _x_full_row(seed, M, K, row):
    """n = K: every column flagged by rows 0 / M - 1, and `row` holds nothing but entries >= 6 (no counted entry: sx == 0)"""
    x = make_x(seed, M, K, K)
    g = _gen(seed + 1)
    x[row] = (6.0 + 24.0 * torch.rand(K, generator=g)).to(torch.bfloat16) * torch.where(torch.rand(K, generator=g) < 0.5, -1.0, 1.0).to(torch.bfloat16)
    return x


def _x_thr_edges(seed, M, K):
    x = base_x(_gen(seed), M, K)
    x[0, 40] = 6.0                   # >= flags it
    x[M - 1, 41] = -6.0              # |x| >= thr
    x[M // 2, 42] = BELOW_THR        # does not; it is that row's absmax
    x[M // 2, 43] = -BELOW_THR
    return x


def _x_row_rules(seed, M, K):
    g = _gen(seed)
    x = base_x(g, M, K).float().clamp(-5.0, 5.0).to(torch.bfloat16)
    x[9, 100] = 7.5                  # column 100 is an outlier column because of row 9 alone ...
    x[4, 100] = 5.75                 # ... and holds the largest counted entry of row 4: it sets sx[4] and is stored as code 0
    x[3] = 0                         # all-zero row: sx == 0, codes 0
    for r, a in zip((5, 6), TIE_ABSMAX):
        x[r] = tie_row(K, a, g)
    x[7] = half_row(K, HALF_ABSMAX, g)
    x[5:8, 100] = 0
    return x


def _x_stream(seed, M, K, n_cols):
    """K > 24576: every row's absmax and the outlier columns in `n_cols` sit where only the streaming loop of quant_int8_rows_kernel looks"""
    g = _gen(seed)
    x = base_x(g, M, K).float().clamp(-5.0, 5.0).to(torch.bfloat16)
    for r in range(M):
        x[r, QCH_K + 8 * r + 3] = (5.25, -5.5, 5.75, -5.375, 5.625)[r % 5]
    for j, c in enumerate(n_cols):
        x[(0, M - 1)[j % 2], c] = VALS[(j + 2) % len(VALS)]
    return x


PREPARE = [
    PrepCase("m1_k8_n0", "M = 1, K = 8: one mask byte of a partial word, memset of 4 bytes, no outlier (n_pad = 0, nothing gathered)", 1, 8, 5, 0,
             lambda: make_x(11, 1, 8, 0)),
    PrepCase("m1_k8_nK", "M = 1, every entry >= 6: n = K = 8, n_pad = 64 rounds past K into the idx slack, sx == 0", 1, 8, 5, 8,
             lambda: _x_full_row(12, 1, 8, 0)),
    PrepCase("m31_k264_n1_last_row", "only outlier in row M - 1 of column K - 1; K / 8 = 33: partial mask word and partial column block", 31, 264, 5, 1,
             lambda: make_x(13, 31, 264, 1, first=1)),
    PrepCase("m33_k264_n63", "row 32 alone in the second strip of the scan; 63 columns incl. 0, 1 (one mask byte), 31 | 32 (word boundary), K - 1",
             33, 264, 5, 63, lambda: make_x(14, 33, 264, 63)),
    PrepCase("m70_k520_n64", "n = 64: n_pad == n, no -1 written; three strips, two column blocks", 70, 520, 5, 64, lambda: make_x(15, 70, 520, 64)),
    PrepCase("m70_k520_n65", "n = 65: one column into the second 64-column stage, 63 entries of -1", 70, 520, 5, 65, lambda: make_x(16, 70, 520, 65, first=1)),
    PrepCase("m33_k264_nK", "n = K = 264 (a row with every entry >= 6): n_pad = 320 > K, all codes 0", 33, 264, 5, 264, lambda: _x_full_row(17, 33, 264, 16)),
    PrepCase("thr_edges", "6.0 and -6.0 flag a column (>=), 5.96875 does not and becomes the absmax", 31, 264, 5, 2, lambda: _x_thr_edges(18, 31, 264)),
    PrepCase("row_rules", "absmax inside an outlier column flagged by another row; an all-zero row; rows of exact .5 ties", 33, 264, 5, 1,
             lambda: _x_row_rules(19, 33, 264)),
    PrepCase("m70_k4096_n5", "K = 4096: eight column blocks, four columns per compaction thread", 70, 4096, 5, 5, lambda: make_x(20, 70, 4096, 5)),
    PrepCase("m5_k24832_stream", "K = 24832 > 24576: absmax of every row and two of three outlier columns behind the register window", 5, 24832, 3, 3,
             lambda: _x_stream(21, 5, 24832, (7, QCH_K + 100, 24832 - 1))),
]

REUSE_N = (130, 0, 1)          # one workspace, three calls in a row: many outliers, none, one


def reuse_inputs(M, K):
    return [make_x(30 + i, M, K, n, first=i % 2) for i, n in enumerate(REUSE_N)]


# ---------------------------------------------------------------------------------------------------------------------- weight cases

WeightCase = namedtuple("WeightCase", "name edge N K build")


def _w_small():
    g = _gen(41)
    return tie_row(8, TIE_ABSMAX[0], g)[None, :].clone()


def _w_mid():
    g = _gen(42)
    w = make_w(43, 5, 264)
    w[1] = 0                                   # all-zero row: scale 0, codes 0, dequantised 0
    w[2] = 0
    w[2, 3] = -0.75                            # a row of one non-zero: code -127
    w[3] = tie_row(264, TIE_ABSMAX[1], g)
    w[4] = half_row(264, HALF_ABSMAX, g)
    return w


def _w_long():
    w = make_w(44, 3, 24832)
    w[0, QCH_K + 77] = 0.5                     # the row maximum behind the register window
    w[1] = 0
    w[2, 24832 - 1] = -0.375
    return w


WEIGHTS = [
    WeightCase("n1_k8_ties", "one row of one chunk, tie values", 1, 8, _w_small),
    WeightCase("n5_k264_rows", "K / 8 = 33; an all-zero row, a row of one non-zero, two rows of ties", 5, 264, _w_mid),
    WeightCase("n3_k24832_stream", "K > 24576: the streaming loop finds the absmax and converts the last chunks; an all-zero row", 3, 24832, _w_long),
]


# ---------------------------------------------------------------------------------------------------------------------- linear cases

LinCase = namedtuple("LinCase", "name edge M N K n KP res alpha build")


def _x_lin_stream():
    return _x_stream(53, 5, 24832, (7, QCH_K + 100, 24832 - 1))


LINEAR = [
    LinCase("m33_n264_k256_n0", "no outlier: k2_dev[0] == 0, two 8-bit stages (the minimum), no bf16 stage", 33, 264, 256, 0, 0, False, 1.0,
            lambda: make_x(51, 33, 256, 0)),
    LinCase("m70_n520_k384_n65_lora", "three 8-bit stages (odd), LoRA pair of 64 in front of 128 outlier columns, residual, alpha", 70, 520, 384, 65, 64,
            True, 0.5, lambda: make_x(52, 70, 384, 65)),
    LinCase("m5_n64_k24832_n3", "194 8-bit stages, the streaming prepare, one bf16 stage with 3 live columns", 5, 64, 24832, 3, 0, False, 1.0, _x_lin_stream),
]

REUSE_LINEAR = (33, 264, 256)


def lin_operands(case_or_shape, seed=60):
    """-> dict(w, wq, wscale, a2, b2, residual) for a LinCase or an (M, N, K, KP, res) tuple"""
    if isinstance(case_or_shape, LinCase):
        M, N, K, KP, res = case_or_shape.M, case_or_shape.N, case_or_shape.K, case_or_shape.KP, case_or_shape.res
    else:
        M, N, K, KP, res = case_or_shape
    g = _gen(seed + M + N + K)
    w = make_w(seed + N + K, N, K)
    wq, wscale, _ = ref_quant_rows(w)
    a2 = (torch.randn(M, KP, generator=g) * 0.5).to(torch.bfloat16) if KP else None
    b2 = (torch.randn(N, KP, generator=g) * 0.05).to(torch.bfloat16) if KP else None
    scale = float(math.sqrt(K) * 1.5 * 0.02)
    residual = (torch.randn(M, N, generator=g) * 0.5 * scale).to(torch.bfloat16) if res else None
    return dict(w=w, wq=wq, wscale=wscale, a2=a2, b2=b2, residual=residual)


# ---------------------------------------------------------------------------------------------------------------------- comparison

def prepare_mismatches(got, ref):
    """got: dict(meta=(n, n_pad), idx int32 [>= n_pad], sx, XQ, A2 [M, >= n_pad], B2 [N, >= n_pad], mask8 (optional)) -> the names of the
    products that are not bit-equal to ref (a Prepared)."""
    bad = []
    if tuple(int(v) for v in got["meta"]) != (ref.n, ref.n_pad):
        bad.append(f"meta {tuple(int(v) for v in got['meta'])} != {(ref.n, ref.n_pad)}")
    P = ref.n_pad
    if got["idx"].numel() < P or not torch.equal(got["idx"][:P].cpu().int(), ref.idx):
        bad.append("idx")
    if not torch.equal(bits32(got["sx"].cpu().float()), bits32(ref.sx)):
        bad.append("sx")
    if not torch.equal(got["XQ"].cpu(), ref.XQ):
        bad.append("XQ")
    for name, want in (("A2", ref.A2), ("B2", ref.B2)):
        g = got[name].cpu()
        if g.shape[1] < P or not torch.equal(bits16(g[:, :P]), bits16(want)):
            bad.append(name)
    if got.get("mask8") is not None and not torch.equal(got["mask8"].cpu(), ref.mask8):
        bad.append("mask8")
    return bad
