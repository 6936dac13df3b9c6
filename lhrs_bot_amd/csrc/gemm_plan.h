// Host-only planner of the GEMM dispatch: which kernels one call of an entry point of gemm.hip launches, on which rows, in which order.
// Plain C++, no HIP: gemm_plan() is a pure function of (GemmProblem, GemmKnobs) - no timing, no cache, no state, no device - so a run is
// bit-reproducible, every data-parallel rank runs the same kernels, and the dispatch is checkable without a GPU (lhrs_gemm_plan;
// tests/gemm_cases.py::path_of restates it).  gemm.hip runs the plan; gemm_u4.hip's launch wrappers decline by the same u4_*_ok predicates.
// Where the thresholds come from: DESIGN.md 3.1 / 4 and the profiles/ files named there.
#pragma once
#include <cstddef>

namespace gemm_plan_h {

// The A/B switches (lhrs_gemm_set_*; gemm.hip holds the one instance) and two device facts.
struct GemmKnobs {
  int u4_on = 1;             // the four-wave kernel for the long-k products (lhrs_gemm_set_u4 / LHRS_GEMM_U4)
  int allow_256 = 2;         // 0 = small tiles only (lhrs_gemm_set_policy)
  int bm144 = 1;             // 144-row tiles: 0 never, 1 by the cost model of pick_144, 2 whenever legal (lhrs_gemm_set_bm144)
  double bm144_cost = 0.8;   // time of a 144-row tile over a 256-row tile on a long k-loop
  int min256 = 128;          // fewest 256x256 tiles for the persistent kernels (lhrs_gemm_set_min_tiles)
  int small_thresh = 256;    // fewest 64x128 tiles for the 64x128 kernel over 64x64 (lhrs_gemm_set_small_thresh)
  int tail_split = 1;        // the tail-row rule (lhrs_gemm_set_tail_split)
  int persist = 1;           // executor only: at most one workgroup per CU walks the tiles (lhrs_gemm_set_persistent)
  int cus = 256;             // compute units of the device
  long ws_units = 0;         // registered GEMM workspace in 256x256 f32 slabs (lhrs_gemm_set_workspace); 0 = none
};
enum GemmEntry { GE_PLAIN, GE_SWIGLU_FWD, GE_SWIGLU_BWD, GE_ROPE, GE_FP8, GE_INT8, GE_SPLITK_F32 };

// One call of an entry point.  GE_PLAIN covers lhrs_gemm_bf16_nt, its LoRA pair (K2 > 0) and its dropout mask (drop_thresh != 0).  N is the
// width of the product (2 ff for SwiGLU forward, ff for backward).  Leading dimensions in elements (bytes for the 8-bit operands).  The
// planner reads the alignment of the pointers and the 32-bit-offset limits they imply, never what they point to.
struct GemmProblem {
  GemmEntry entry = GE_PLAIN;
  int M = 0, N = 0, K = 0, K2 = 0, act = 0, out_f32 = 0, accumulate = 0;
  float alpha = 1.f;
  const void* A = nullptr; const void* B = nullptr; void* C = nullptr;
  const void* bias = nullptr; const void* residual = nullptr; const void* A2 = nullptr; const void* B2 = nullptr;
  long lda = 0, ldb = 0;
  int ldc = 0, ldr = 0, lda2 = 0, ldb2 = 0;
  float drop_scale = 1.f; unsigned drop_seed = 0, drop_thresh = 0;     // dropout mask over alpha * A.B^T; thresh 0 = none
  int ff = 0, ld_gu = 0, ld_act = 0;                                   // SwiGLU: gu [M, 2 ff] (ld_gu), act [M, ff] (ld_act)
  const void* gu = nullptr; void* act_out = nullptr;
  const float* rope_cos = nullptr; const float* rope_sin = nullptr;    // RoPE: position of row m = m % rope_mod + rope_pos0
  int rope_mod = 1, rope_pos0 = 0, rope_cols = 0, head_dim = 0;
  const float* sa = nullptr; const float* sb = nullptr; const int* k2_dev = nullptr;   // 8-bit operands: per-row scales, device-known pair columns
  void* scratch = nullptr;   // SwiGLU backward: d_act [M, ff] of the unfused fallback; split-K f32: the caller's slabs
};
enum GemmKernel {
  GK_U4, GK_SPLITK_TAIL, GK_256, GK_144, GK_T128, GK_T64X128, GK_T64X64, GK_U4_SWIGLU_FWD, GK_U4_SWIGLU_BWD, GK_U4_ROPE,
  GK_SWIGLU_FWD_256, GK_SWIGLU_FWD_144, GK_SWIGLU_BWD_256, GK_SWIGLU_BWD_144, GK_ROPE_256, GK_ROPE_144, GK_FP8_256, GK_FP8_SMALL,
  GK_I8_256, GK_SPLITK_F32, GK_COUNT
};
// name (the one path_of uses), tile height and width, plain: a kernel of plan_rows - it computes a plain product, whatever the entry point
struct GemmKernelInfo { const char* name; int bm, bn; bool plain; };
inline const GemmKernelInfo& gemm_kernel_info(int k) {
  static const GemmKernelInfo info[GK_COUNT] = {
      {"u4", 256, 256, false}, {"splitk_tail", 128, 128, true}, {"256", 256, 256, true}, {"144", 144, 256, true}, {"t128", 128, 128, true},
      {"t64x128", 64, 128, true}, {"t64x64", 64, 64, true}, {"u4_swiglu_fwd", 256, 256, false}, {"u4_swiglu_bwd", 256, 256, false},
      {"u4_rope", 256, 256, false}, {"swiglu_fwd_256", 256, 256, false}, {"swiglu_fwd_144", 144, 256, false}, {"swiglu_bwd_256", 256, 256, false},
      {"swiglu_bwd_144", 144, 256, false}, {"rope_256", 256, 256, false}, {"rope_144", 144, 256, false}, {"fp8_256", 256, 256, false},
      {"fp8_small", 64, 128, false}, {"i8_256", 256, 256, false}, {"splitk_f32", 128, 128, false}};
  return info[k];
}
// Which product a segment computes: the small tiles have no second operand pair in their k-loop, so a LoRA product on them covers its
// rows twice - the base product, then the rank-K2 update as a product of its own accumulated on top of it.
enum GemmPart { GP_WHOLE, GP_BASE, GP_PAIR };
// One launch: rows [row0, row1).  prof_kind: the kind of lhrs_gemm_profile_read_kinds, -1 = counted but never timed.  splits: k-slabs of the
// split-K kernels.  pass_row0 >= 0: an unfused fallback runs the entry's elementwise pass on rows [pass_row0, row1) right behind this launch.
struct GemmSeg { int row0, row1, kernel, prof_kind, splits, part, pass_row0; };
// Room for a plan.  The longest the rules can produce is 6: a split SwiGLU forward whose main rows are an unfused two-launch LoRA fallback
// (2; only with lhrs_gemm_set_min_tiles raised) and whose tail rows are cut once more into two such fallbacks (2 + 2).  gemm_plan returns
// -1 rather than a truncated plan if a rule change ever outgrows it.
constexpr int GEMM_PLAN_CAP = 8;
inline long cdivl(long a, long b) { return (a + b - 1) / b; }
// ---- addressing predicates of the four-wave kernel: 16-B rows and pointers, 32-bit lane offsets of the operands and of a tile's output rows
inline bool u4_addressable(const void* A, long lda, const void* B, long ldb, const void* C, int ldc, int M, int N, int K) {
  return M > 0 && N > 0 && K >= 256 && K % 64 == 0 && N % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && ldc % 8 == 0 && lda >= K && ldb >= K && ldc >= N &&
         ((size_t)A | (size_t)B | (size_t)C) % 16 == 0 && (long)M * lda * 2 < (1L << 32) && (long)N * ldb * 2 < (1L << 32) &&
         (long)144 * ldc * 2 < (1L << 32);
}
// the optional second operand pair (fused LoRA update): rows of A2 / B2 as the rows of A / B; K2 a multiple of 64
inline bool u4_pair_ok(const void* A2, int lda2, const void* B2, int ldb2, int K2, int M, int rowsB) {
  return K2 == 0 || (K2 > 0 && K2 % 64 == 0 && A2 != nullptr && B2 != nullptr && lda2 % 8 == 0 && ldb2 % 8 == 0 && lda2 >= K2 && ldb2 >= K2 &&
                     ((size_t)A2 | (size_t)B2) % 16 == 0 && (long)M * lda2 * 2 < (1L << 32) && (long)rowsB * ldb2 * 2 < (1L << 32));
}
inline bool u4_nt_ok(const void* A, long lda, const void* B, long ldb, const void* C, int ldc, int M, int N, int K, const void* residual, int ldr,
                     const void* A2, int lda2, const void* B2, int ldb2, int K2) {
  return u4_addressable(A, lda, B, ldb, C, ldc, M, N, K) &&
         (residual == nullptr || (ldr % 8 == 0 && ldr >= N && (size_t)residual % 16 == 0 && (long)144 * ldr * 2 < (1L << 32))) &&
         u4_pair_ok(A2, lda2, B2, ldb2, K2, M, N);
}
inline bool u4_rope_ok(const void* X, long ldx, const void* W, long ldw, const void* C, int ldc, int M, int N, int K, const float* cos_t, const float* sin_t,
                       int pos_mod, int pos0, int rope_cols, const void* A2, int lda2, const void* B2, int ldb2, int K2) {
  return u4_addressable(X, ldx, W, ldw, C, ldc, M, N, K) && rope_cols % 256 == 0 && rope_cols <= N && pos_mod >= 16 && pos0 >= 0 && cos_t != nullptr &&
         sin_t != nullptr && ((size_t)cos_t | (size_t)sin_t) % 16 == 0 && (long)(pos_mod + pos0) * 64 * 4 < (1L << 31) &&
         u4_pair_ok(A2, lda2, B2, ldb2, K2, M, N);
}
inline bool u4_swiglu_fwd_ok(const void* X, long ldx, const void* Wgu, long ldw, const void* gu, int ld_gu, const void* act, int ld_act, int M, int ff, int K) {
  return ff > 0 && ff % 128 == 0 && u4_addressable(X, ldx, Wgu, ldw, gu, ld_gu, M, 2 * ff, K) && ld_act % 8 == 0 && ld_act >= ff && (size_t)act % 16 == 0 &&
         (long)144 * ld_act * 2 < (1L << 32) && (long)2 * ff * ldw * 2 < (1L << 32);
}
inline bool u4_swiglu_bwd_ok(const void* dY, long ldy, const void* WdT, long ldw, const void* gu, const void* dgu, int ld_gu, int M, int ff, int K) {
  return ff > 0 && ff % 8 == 0 && u4_addressable(dY, ldy, WdT, ldw, dgu, ld_gu, M, ff, K) && ld_gu >= 2 * ff && (size_t)gu % 16 == 0;
}
// ---- shape rules ------------------------------------------------------------------------------------------------------------------------
// A plain epilogue (no bias, no activation, bf16 out, alpha 1; optional residual) on a long k-loop runs the four-wave gemm_u4_kernel (5-18 %
// faster there) whenever its 256x256 tiles fill >= 80 % of one round of the CUs; it has one tile height, so a launch that cannot fill the
// chip stays on the 144-row / small-tile kernels (M = 2184, N = 4096: 144 tiles).
inline bool u4_takes(const GemmKnobs& k, int M, int N, int K, long lda, long ldb, int ldc, int ldr, bool has_bias, int act, bool out_f32, bool accumulate,
                     float alpha) {
  const long tiles = cdivl(M, 256) * cdivl(N, 256);
  return k.u4_on == 1 && k.allow_256 != 0 && !has_bias && act == 0 && !out_f32 && !accumulate && alpha == 1.f && K >= 4096 && K % 64 == 0 && M >= 1024 &&
         N >= 1024 && 5 * tiles >= 4L * k.cus && lda % 8 == 0 && ldb % 8 == 0 && ldc % 8 == 0 && ldr % 8 == 0;
}
// The fused-epilogue products on the four-wave kernel.  kind: 0 RoPE (tiles_n = N / 256; the only one with a LoRA pair in the k-loop),
// 1 SwiGLU forward (ff / 128), 2 SwiGLU backward (ff / 256).  K >= 4096 and a tile walk that leaves at most 15 % of all CU-rounds idle
// (R / T <= 1.15; SwiGLU backward 5 %: its write-out is VALU-bound on four waves and only wins where the walk fits) - one tile height, no
// tail-row split for the fused epilogues.
inline bool u4_fused_takes(const GemmKnobs& k, int kind, int M, long tiles_n, int K, int K2) {
  const long P = k.cus, T = cdivl(M, 256) * tiles_n, R = (T + P - 1) / P * P;
  const bool idle_ok = kind == 2 ? 100 * R <= 105 * T : 20 * R <= 23 * T;
  return k.u4_on == 1 && k.allow_256 != 0 && (kind == 0 ? K2 % 64 == 0 : K2 == 0) && K >= 4096 && K % 64 == 0 && M >= 1024 && 5 * T >= 4 * P && idle_ok;
}
// Rows of a plain product for gemm_u4_kernel (M itself: no cut).  When the last of its ceil(T / P) rounds would be mostly empty (M = 8736:
// 35 x 16 = 560 tiles = 2.19 rounds -> 3) the rows are cut behind the last tile row the whole rounds cover; the rest goes to plan_rows.
inline int u4_main_rows(const GemmKnobs& k, int M, long tiles_n) {
  const long P = k.cus, tm = cdivl(M, 256), T = tm * tiles_n, full = T / P;
  if (T % P == 0 || full < 1 || 20 * ((T + P - 1) / P * P) <= 23 * T) return M;        // whole rounds, or the idle share of the last round is <= 15 %
  const long tm_main = full * P / tiles_n;
  return tm_main >= 1 && tm_main < tm ? (int)(tm_main * 256) : M;
}
// Tile height of the persistent kernels: 256 rows (16 waves) or 144 rows (12 waves); both walk ceil(tiles / CUs) rounds.  A 144-row tile is
// 0.5625 of the MFMA work of a 256-row tile at ~0.8 of its time: take whichever finishes first.
inline bool pick_144(const GemmKnobs& k, int M, long tiles_n, int K, int K2, bool drop) {
  if (k.bm144 == 0 || K2 > 0 || drop || K < 192) return false;   // the second operand pair and the dropout mask live in the 256-row kernel only
  if (k.bm144 == 2) return true;
  const long P = k.cus, t256 = cdivl(M, 256) * tiles_n, t144 = cdivl(M, 144) * tiles_n;
  const int nk = K / 64;
  // short k-loops (ViT / projector, K = 1024 .. 2048): a tile's fixed part weighs as much as its stages and is smaller for the 144-row tile;
  // fitted on tools/gemm_vit_sweep.py, us per round: 256 rows 1.5 nk + 20, 144 rows 1.15 nk + 5
  if (nk <= 32) return (double)((t144 + P - 1) / P) * (1.15 * nk + 5.0) < (double)((t256 + P - 1) / P) * (1.5 * nk + 20.0);
  return (double)((t144 + P - 1) / P) * k.bm144_cost < (double)((t256 + P - 1) / P);
}
// the fused SwiGLU epilogues of the 16-wave kernels; tiles: ceil(M / 256) * (ff / 128) forward, * ceil(ff / 256) backward
inline bool swiglu_fusable(const GemmKnobs& k, long tiles, int ff, int K, int K2, long lda, long ldb) {
  return k.allow_256 == 2 && ff % 256 == 0 && K % 64 == 0 && K2 % 64 == 0 && K + K2 >= 128 && tiles >= k.min256 && lda % 8 == 0 && ldb % 8 == 0;
}
// the fused RoPE epilogue of the 16-wave kernels (heads of 128 in whole 256-column tiles)
inline bool rope_fusable(const GemmKnobs& k, int M, int N, int K, int K2, long lda, long ldb, int rope_cols, int head_dim) {
  return k.allow_256 == 2 && head_dim == 128 && rope_cols % 256 == 0 && N % 8 == 0 && K % 64 == 0 && K2 % 64 == 0 && K + K2 >= 128 &&
         cdivl(M, 256) * cdivl(N, 256) >= k.min256 && lda % 8 == 0 && ldb % 8 == 0;
}
// The tail-row rule -> main rows, 0: no cut.  T = tm * tiles_n 256x256 tiles run as rounds of the CUs and a nearly empty last round costs as
// much as a full one.  When the tile rows that spill over the last full round are cheaper as a small-tile launch (~2.5x the time per FLOP,
// but no idle CUs), the rows are cut there.  The cut and the split walk count rounds of 256 CUs.  unsplit_cus: what the UNSPLIT walk's
// rounds are counted in - plan_rows passes the device's CU count, SwiGLU forward and e4m3 pass 256.  On 256 CUs the two agree; elsewhere
// they do not, and each caller keeps the rule it was measured with.
inline int tail_main_rows(const GemmKnobs& k, int M, long tiles_n, long unsplit_cus) {
  if (!k.tail_split || tiles_n < 1) return 0;
  const long tm = cdivl(M, 256), T = tm * tiles_n, full = T / 256, tm_main = full * 256 / tiles_n;
  if (!(full >= 1 && T % 256 != 0 && tm_main >= 1 && tm_main < tm)) return 0;
  const long t_main = tm_main * tiles_n, t_tail = T - t_main;
  const double split_cost = (double)((t_main + 255) / 256) + 2.5 * (double)t_tail / 256.0 + 0.05;
  return split_cost < (double)((T + unsplit_cus - 1) / unsplit_cus) ? (int)(tm_main * 256) : 0;
}
// Slabs of the split-K tail, 0: does not apply.  Tail rows with a LONG k-loop (544 rows x 4096 columns walking K = 11008 .. 22016) are cut
// into k-slabs of ~4096 in the registered workspace, summed in a fixed order with the residual, so that every CU has work.
inline int splitk_tail_splits(const GemmKnobs& k, int M_tail, int N, int K) {
  const int splits = K >= 8192 ? (K + 2048) / 4096 : 1;
  return splits <= 1 || N % 128 != 0 || k.ws_units == 0 || (long)splits * M_tail * N * 4 > k.ws_units * 256 * 256 * 4 ? 0 : splits;
}
// slabs of lhrs_gemm_bf16_nt_splitk_f32 (long K, few tiles: the projector's weight gradients)
inline int splitk_f32_splits(int M, int N, int K) {
  const long tiles = cdivl(M, 128) * cdivl(N, 128);
  long s = (512 + tiles / 2) / tiles;
  s = s > K / 1024 ? K / 1024 : s;
  return s > 8 ? 8 : s < 1 ? 1 : (int)s;
}
// ---- the product a segment computes -------------------------------------------------------------------------------------------------------
// A plain kernel under a fused entry point is its unfused fallback (SwiGLU backward: d_act into the dense [M, ff] scratch); part selects the
// base product or the pair of a two-launch LoRA fallback.  The planner and the executor derive it here, from the same (problem, kernel, part).
inline GemmProblem gemm_seg_problem(const GemmProblem& p, int kernel, int part) {
  GemmProblem q = p;
  if (gemm_kernel_info(kernel).plain) {
    if (p.entry == GE_SWIGLU_BWD) { q.C = p.scratch; q.ldc = p.ff; }
    q.entry = GE_PLAIN;
  }
  if (part != GP_WHOLE) { q.A2 = q.B2 = nullptr; q.lda2 = q.ldb2 = q.K2 = 0; }
  if (part == GP_PAIR) {
    q.A = p.A2; q.lda = p.lda2; q.B = p.B2; q.ldb = p.ldb2; q.K = p.K2; q.bias = nullptr; q.act = 0;
    q.residual = p.out_f32 ? nullptr : q.C; q.ldr = q.ldc; q.accumulate = p.out_f32 ? 1 : 0;
  }
  return q;
}
// ---- the plan ---------------------------------------------------------------------------------------------------------------------------
struct GemmPlanOut {
  GemmSeg* segs; int n, cap;
  void add(int r0, int r1, int kernel, int prof_kind = -1, int splits = 0, int part = GP_WHOLE) {
    if (n < cap) segs[n] = GemmSeg{r0, r1, kernel, prof_kind, splits, part, -1};
    ++n;   // past cap: counted, not stored - gemm_plan reports it
  }
};

// rows [r0, r0 + M) of a plain product on the 16-wave family: the persistent 256- / 144-row kernels and the small tiles
inline void plan_rows(const GemmProblem& p, const GemmKnobs& k, int r0, int M, bool split_ok, int part, GemmPlanOut& out) {
  const int N = p.N, K = p.K, K2 = p.K2;
  const bool drop = p.drop_thresh != 0, out_f32 = p.out_f32 != 0;
  const long tn = cdivl(N, 256), t256 = cdivl(M, 256) * tn, t144 = cdivl(M, 144) * tn;
  const bool al16 = out_f32 || (N % 8 == 0 && p.ldc % 8 == 0 && (p.residual == nullptr || p.ldr % 8 == 0));  // 16-B epilogue rows
  bool use256 = k.allow_256 && t256 >= k.min256 && K >= 128 && al16;  // the persistent kernels' pipeline needs >= 2 stages
  // just under the big-tile threshold but nearly a full round of 144-row tiles (ViT o / fc2 at micro-batch 30: 124 tiles of 256 rows, 216 of
  // 144): the persistent 144-row kernel beats the small tiles
  if (!use256 && k.allow_256 == 2 && k.bm144 == 1 && al16 && !out_f32 && K % 64 == 0 && K >= 192 && K2 == 0 && !drop && t256 >= k.min256 / 2 &&
      t144 >= 200 && t144 <= k.cus)
    use256 = true;
  if (K2 > 0 && !use256) {  // the two-launch LoRA fallback
    plan_rows(gemm_seg_problem(p, GK_T128, GP_BASE), k, r0, M, split_ok, GP_BASE, out);
    plan_rows(gemm_seg_problem(p, GK_T128, GP_PAIR), k, r0, M, split_ok, GP_PAIR, out);
    return;
  }
  const bool bm144 = use256 && !out_f32 && pick_144(k, M, tn, K, K2, drop);
  if (use256 && !bm144 && split_ok && !drop) {
    if (const int Mm = tail_main_rows(k, M, tn, k.cus)) {
      plan_rows(p, k, r0, Mm, false, part, out);
      const int splits = !out_f32 && K2 == 0 && p.bias == nullptr && p.act == 0 ? splitk_tail_splits(k, M - Mm, N, K) : 0;
      if (splits) out.add(r0 + Mm, r0 + M, GK_SPLITK_TAIL, -1, splits, part);
      else plan_rows(p, k, r0 + Mm, M - Mm, false, part, out);
      return;
    }
  }
  if (use256) out.add(r0, r0 + M, bm144 ? GK_144 : GK_256, bm144 ? 4 : 0, 0, part);
  else if (cdivl(M, 128) * cdivl(N, 128) >= 384) out.add(r0, r0 + M, GK_T128, -1, 0, part);
  else if (cdivl(M, 64) * cdivl(N, 128) >= k.small_thresh) out.add(r0, r0 + M, GK_T64X128, -1, 0, part);
  else out.add(r0, r0 + M, GK_T64X64, -1, 0, part);
}
// the unfused fallback of a fused entry point: the plain product, and behind its last launch the entry's elementwise pass over the same rows
inline void plan_unfused(const GemmProblem& p, const GemmKnobs& k, int r0, int M, bool split_ok, bool pass, GemmPlanOut& out) {
  plan_rows(gemm_seg_problem(p, GK_T128, GP_WHOLE), k, r0, M, split_ok, GP_WHOLE, out);
  if (pass && out.n <= out.cap) out.segs[out.n - 1].pass_row0 = r0;
}
// a plain product: the four-wave kernel by its shape rule - if it can address the operands - on the rows its whole rounds cover, else plan_rows
inline void plan_plain(const GemmProblem& p, const GemmKnobs& k, GemmPlanOut& out) {
  const int M = p.M, N = p.N, K = p.K, Mu = u4_main_rows(k, M, cdivl(N, 256));
  if (!u4_takes(k, M, N, K, p.lda, p.ldb, p.ldc, p.residual ? p.ldr : 0, p.bias != nullptr, p.act, p.out_f32, p.accumulate, p.alpha) || p.drop_thresh != 0 ||
      !u4_nt_ok(p.A, p.lda, p.B, p.ldb, p.C, p.ldc, Mu, N, K, p.residual, p.ldr, p.A2, p.lda2, p.B2, p.ldb2, p.K2))
    return plan_rows(p, k, 0, M, true, GP_WHOLE, out);
  out.add(0, Mu, GK_U4, p.residual ? 5 : 6);
  if (Mu == M) return;
  // the split-K tail has no second operand pair: a product with one takes the small-tile kernels over its whole k-loop
  const int splits = p.K2 == 0 ? splitk_tail_splits(k, M - Mu, N, K) : 0;
  if (splits) out.add(Mu, M, GK_SPLITK_TAIL, -1, splits);
  else plan_rows(p, k, Mu, M - Mu, true, GP_WHOLE, out);     // the tail rows may be cut once more
}
// Tail rows as in plan_rows (M = 2184, ff = 11008: 9 x 86 = 774 tiles = 3 rounds + SIX tiles): the fused kernel takes the whole tile rows -
// planned again as a SwiGLU forward, so they may land on the four-wave kernel - and the remaining rows go through the unfused fallback.
inline void plan_swiglu_fwd(const GemmProblem& p, const GemmKnobs& k, int r0, int M, bool split_ok, GemmPlanOut& out) {
  const int ff = p.ff, K = p.K, K2 = p.K2;
  const long tn = ff / 128;
  if (ff % 128 == 0 && u4_fused_takes(k, 1, M, tn, K, K2) && u4_swiglu_fwd_ok(p.A, p.lda, p.B, p.ldb, p.C, p.ld_gu, p.act_out, p.ld_act, M, ff, K))
    return out.add(r0, r0 + M, GK_U4_SWIGLU_FWD, 7);
  if (!swiglu_fusable(k, cdivl(M, 256) * tn, ff, K, K2, p.lda, p.ldb)) return plan_unfused(p, k, r0, M, split_ok, true, out);
  const bool bm144 = pick_144(k, M, tn, K, K2, false);
  if (!bm144 && split_ok && p.ld_gu == 2 * ff && p.ld_act == ff) {
    if (const int Mm = tail_main_rows(k, M, tn, 256)) {
      plan_swiglu_fwd(p, k, r0, Mm, false, out);
      return plan_unfused(p, k, r0 + Mm, M - Mm, true, true, out);
    }
  }
  out.add(r0, r0 + M, bm144 ? GK_SWIGLU_FWD_144 : GK_SWIGLU_FWD_256, 1);
}
// -> number of segments written to segs[0 .. cap) in launch order; -1: more than cap (see GEMM_PLAN_CAP)
inline int gemm_plan(const GemmProblem& p, const GemmKnobs& k, GemmSeg* segs, int cap) {
  GemmPlanOut out{segs, 0, cap};
  const int M = p.M, N = p.N, K = p.K, K2 = p.K2;
  switch (p.entry) {
    case GE_PLAIN: plan_plain(p, k, out); break;
    case GE_SWIGLU_FWD: plan_swiglu_fwd(p, k, 0, M, true, out); break;
    case GE_SWIGLU_BWD: {
      const long tn = cdivl(p.ff, 256);
      if (u4_fused_takes(k, 2, M, tn, K, K2) && u4_swiglu_bwd_ok(p.A, p.lda, p.B, p.ldb, p.gu, p.C, p.ld_gu, M, p.ff, K)) out.add(0, M, GK_U4_SWIGLU_BWD, 8);
      else if (!swiglu_fusable(k, cdivl(M, 256) * tn, p.ff, K, K2, p.lda, p.ldb)) plan_unfused(p, k, 0, M, true, true, out);
      else out.add(0, M, pick_144(k, M, tn, K, K2, false) ? GK_SWIGLU_BWD_144 : GK_SWIGLU_BWD_256, 2);
      break;
    }
    case GE_ROPE: {
      const long tn = cdivl(N, 256);
      if (!rope_fusable(k, M, N, K, K2, p.lda, p.ldb, p.rope_cols, p.head_dim)) plan_unfused(p, k, 0, M, true, p.rope_cols != 0, out);
      else if (u4_fused_takes(k, 0, M, tn, K, K2) &&
               u4_rope_ok(p.A, p.lda, p.B, p.ldb, p.C, p.ldc, M, N, K, p.rope_cos, p.rope_sin, p.rope_mod, p.rope_pos0, p.rope_cols, p.A2, p.lda2, p.B2, p.ldb2, K2))
        out.add(0, M, GK_U4_ROPE, 9);
      else out.add(0, M, pick_144(k, M, tn, K, K2, false) ? GK_ROPE_144 : GK_ROPE_256, 3);
      break;
    }
    case GE_FP8: {   // the tail-row rule; the small-tile sibling exists for e4m3 only
      const int Mm = tail_main_rows(k, M, cdivl(N, 256), 256);
      out.add(0, Mm ? Mm : M, GK_FP8_256);
      if (Mm) out.add(Mm, M, GK_FP8_SMALL);
      break;
    }
    case GE_INT8: out.add(0, M, GK_I8_256); break;
    case GE_SPLITK_F32: {
      const int splits = splitk_f32_splits(M, N, K);
      if (splits == 1) plan_rows(p, k, 0, M, true, GP_WHOLE, out);
      else out.add(0, M, GK_SPLITK_F32, -1, splits);
      break;
    }
  }
  return out.n <= cap ? out.n : -1;
}

}  // namespace gemm_plan_h
