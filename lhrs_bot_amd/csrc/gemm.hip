// bf16 MFMA GEMM for gfx950:  C[M,N] = act(alpha * A[M,K] . B[N,K]^T + bias[N]) + residual[M,N]
//
// This is the kernel that bounds the whole stage-1 step (~96 % of the step's FLOPs are
// LLaMA linears).  Every linear of the reference (`nn.Linear` in HF CLIP / LLaMA and in
// lhrs/models/common_arch.py:276-295) is "NT": activations [M,K] row-major times a weight stored [N,K]
// row-major.  Backward dX through the *frozen* LLaMA uses a pre-transposed copy of each weight (resident in
// HBM; 288 GB makes the second copy free), so dX is NT as well; dW for the projector is NT over transposed
// activations.  One layout, one kernel family.
//
// Kernel family (CDNA4).  Which of them a call launches, on which rows, is decided by the host-only planner gemm_plan.h (the GemmKernel enum names
// them); the host code at the end of this file validates, plans and runs the plan (gemm_run):
//   * gemm_nt_256s_kernel<ACT, EPI, K2P> - THE dominant kernel (every LLaMA linear at training batch sizes): 256x256x64 tile, 16 waves (4x4 of
//     64x64 = 4x4 fragments of v_mfma_f32_16x16x32_bf16 - the dense bf16 shape that costs the least power per FLOP), two 64 KiB LDS stages
//     filled by direct-to-LDS DMA (global_load_lds_dwordx4, no VGPR round trip), one barrier per stage, PERSISTENT over tiles (one workgroup
//     per CU; the next tile's first stage is fetched under the epilogue), fused epilogues: bias / activation / residual / dropout mask
//     (EPI 0), SwiGLU forward / backward (EPI 1 / 2), RoPE (EPI 3).
//   * gemm_u4_kernel (gemm_u4.hip) - the four-wave 256x256x64 kernel for the plain long-k products.
//   * gemm_nt_kernel<WM, WN> - 128x128 / 64x128 / 64x64 tiles, 4 waves, for the small products of the ViT and the projector.
//   * e4m3 siblings (gemm_fp8_256_kernel, gemm_fp8_small_kernel) for the 8-bit frozen base of stages 2/3.
// Common to all:
//   * the LDS image of a DMA wave-instruction is lane-linear, so the bank-conflict swizzle (16-B chunk ^= f(row)) is applied to the
//     per-lane SOURCE address and to the ds_read_b128 address (both sides, same involution);
//   * operands are fed to the MFMA swapped (weight fragment as A, activation fragment as B) so that each lane ends up with consecutive n
//     of one m: row-contiguous stores, and bias / residual become vector loads;
//   * block id -> tile map is XCD-aware (block b runs on XCD b % 8; each XCD gets a contiguous run of tiles, rastered in groups of 8 tile
//     rows) so the 32 tiles an XCD works on at a time share 8 A panels and 4 B panels in its L2.
#include "common.h"
#include "gemm_plan.h"
#include "../../include/lhrs_hip.h"
#include <array>
#include <map>
#include <type_traits>

namespace {

struct GemmArgs {
  const bf16_t* A;
  const bf16_t* B;
  void* C;
  const bf16_t* bias;
  const bf16_t* res;
  int M, N, K;
  int lda, ldb, ldc, ldr;
  float alpha;
  int act;       // 0 none, 1 quick_gelu, 2 gelu(erf), 3 silu
  int out_f32;   // 0 -> bf16 C, 1 -> f32 C
  int accum;     // f32 only: C += result
  int tilesM, tilesN;
  // optional second operand pair, reduced in the same k-loop: C = alpha * (A.B^T + A2.B2^T) ...  (fused LoRA: A2 = s*X*A_lora^T,
  // B2 = B_lora).  K2 = 0 disables it.
  const bf16_t* A2;
  const bf16_t* B2;
  int lda2, ldb2, K2;
  // fused SwiGLU epilogues of the 16-wave 256x256 kernel (LLaMA MLP, HF LlamaMLP: down(silu(gate(x)) * up(x))):
  //   epi 1: B = [gate; up] weight [2*ff, K]; tile tn holds gate AND up of columns [tn*128, +128) (wave wn: 32 gate + 32 up);
  //          C = gate|up [M, 2*ff] in the usual layout, aux_out = silu(gate) * up [M, ff]
  //   epi 2: A.B^T = d_act [M, ff]; aux = gate|up [M, 2*ff]; C = d(gate|up) [M, 2*ff] (may alias aux)
  int epi, ff;
  const bf16_t* aux;
  bf16_t* aux_out;
  long ld_aux;
  // e4m3 operands (gemm_fp8_256_kernel): per-row dequantisation scales of A (length M) and B (length N)
  const float* sa;
  const float* sb;
  // dropout mask on alpha * A.B^T BEFORE bias / residual (LoRA dX path: dx = dy.W + mask * (U.A) / (1 - p)); drop_thresh = 0 -> off
  float drop_scale;
  unsigned drop_seed, drop_thresh;
  // EPI 3 (fused RoPE of the q / k heads of a qkv projection, head_dim 128): fp32 cos / sin tables [pos][64], position of row m =
  // m % rope_mod + rope_pos0, columns [0, rope_cols) are rotated (rope_cols % 256 == 0), the rest stored as computed
  const float* rope_cos;
  const float* rope_sin;
  int rope_mod, rope_pos0, rope_cols;
  // split-K of the small-tile kernel (skinny-N products): block (x, y) reduces K-slice y of length ksplit into f32 slab y of C
  int ksplit;
  // 8-bit kernels: bf16 columns of the second pair whose count is only known on the device (LLM.int8 outlier columns; a multiple of 64),
  // appended behind the K2 host-known ones (nullptr = none)
  const int* k2_dev;
};

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// tile `bid` of `nblk` (the order tiles are dispatched in) -> (tm, tn): consecutive bids alternate over the 8 XCDs (bid & 7), so each XCD
// gets a contiguous run of the m-fastest raster grouped by 8 tile rows - the 32 tiles an XCD works on at a time share 8 A and 4 B panels
// raster position `lin` -> (tm, tn): m-fastest inside groups of 8 tile rows
__device__ __forceinline__ void tile_coords_raster(const GemmArgs& g, int lin, int& tm, int& tn) {
  constexpr int GM = 8;
  const int per_group = GM * g.tilesN;
  const int group = lin / per_group;
  const int first_m = group * GM;
  const int gsize = min(g.tilesM - first_m, GM);
  const int in_g = lin - group * per_group;
  tm = first_m + in_g % gsize;
  tn = in_g / gsize;
}
__device__ __forceinline__ void tile_coords_lin(const GemmArgs& g, int bid, int nblk, int& tm, int& tn) {
  const int xcd = bid & 7, q = nblk >> 3, r = nblk & 7;
  const int lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  constexpr int GM = 8;
  const int per_group = GM * g.tilesN;
  const int group = lin / per_group;
  const int first_m = group * GM;
  const int gsize = min(g.tilesM - first_m, GM);
  const int in_g = lin - group * per_group;
  tm = first_m + in_g % gsize;
  tn = in_g / gsize;
}
__device__ __forceinline__ void tile_coords(const GemmArgs& g, int& tm, int& tn) { tile_coords_lin(g, blockIdx.x, gridDim.x, tm, tn); }

__device__ __forceinline__ float apply_act(float v, int act) {
  if (act == 1) return quick_gelu(v);
  if (act == 2) return gelu_erf(v);
  if (act == 3) return silu(v);
  return v;
}

// Epilogue for one lane's 4 consecutive n of row m.
template <int ACT>
__device__ __forceinline__ void store4(const GemmArgs& g, int m, int n, f32x4 acc) {
  float v[4] = {acc[0] * g.alpha, acc[1] * g.alpha, acc[2] * g.alpha, acc[3] * g.alpha};
  if (g.drop_thresh) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = drop_keep(g.drop_seed, (long)m * g.N + n + i, g.drop_thresh) ? v[i] * g.drop_scale : 0.f;
  }
  if (g.bias) {
    const uint2 b = *reinterpret_cast<const uint2*>(g.bias + n);
    v[0] += bflo(b.x); v[1] += bfhi(b.x); v[2] += bflo(b.y); v[3] += bfhi(b.y);
  }
  if (ACT) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = apply_act(v[i], ACT);
  }
  if (g.res) {
    const uint2 r = *reinterpret_cast<const uint2*>(g.res + (long)m * g.ldr + n);
    v[0] += bflo(r.x); v[1] += bfhi(r.x); v[2] += bflo(r.y); v[3] += bfhi(r.y);
  }
  if (g.out_f32) {
    float* c = reinterpret_cast<float*>(g.C) + (long)m * g.ldc + n;
    if (g.accum) {
      const float4 o = *reinterpret_cast<const float4*>(c);
      v[0] += o.x; v[1] += o.y; v[2] += o.z; v[3] += o.w;
    }
    *reinterpret_cast<float4*>(c) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    bf16_t* c = reinterpret_cast<bf16_t*>(g.C) + (long)m * g.ldc + n;
    *reinterpret_cast<uint2*>(c) = make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
  }
}

// ------------------------------------------------------------------------------------------------
// 128x128x64, 4 waves, 2-stage direct-to-LDS pipeline.
// ------------------------------------------------------------------------------------------------
template <int WM_FR, int WN_FR, int ACT>  // fragments per wave in m / n (4,4 -> 128x128 tile; 2,4 -> 64x128; 2,2 -> 64x64)
__global__ __launch_bounds__(256) void gemm_nt_kernel(GemmArgs g) {
  constexpr int BM = WM_FR * 32, BN = WN_FR * 32, BK = 64;
  constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE = A_BYTES + B_BYTES;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

  int tm, tn;
  tile_coords(g, tm, tn);
  if (g.ksplit > 0) {  // this block's K-slice and its private f32 output slab
    const int sp = blockIdx.y;
    g.A += (long)sp * g.ksplit; g.B += (long)sp * g.ksplit;
    g.C = reinterpret_cast<float*>(g.C) + (long)sp * g.M * g.ldc;
    g.K = min(g.ksplit, g.K - sp * g.ksplit);
  }

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // ---- DMA source addresses: one wave-instruction moves 8 rows x 128 B (1 KiB) ----
  constexpr int A_INSTR = BM / 32;  // per wave
  constexpr int B_INSTR = BN / 32;
  const int lrow = lane >> 3;
  const int lchunk = (lane & 7) ^ lrow;  // logical 16-B chunk this lane fetches (swizzle on the source side)
  const bf16_t* a_src[A_INSTR];
  const bf16_t* b_src[B_INSTR];
#pragma unroll
  for (int i = 0; i < A_INSTR; ++i) {
    int row = tm * BM + (wave * A_INSTR + i) * 8 + lrow;
    row = min(row, g.M - 1);
    a_src[i] = g.A + (long)row * g.lda + lchunk * 8;
  }
#pragma unroll
  for (int i = 0; i < B_INSTR; ++i) {
    int row = tn * BN + (wave * B_INSTR + i) * 8 + lrow;
    row = min(row, g.N - 1);
    b_src[i] = g.B + (long)row * g.ldb + lchunk * 8;
  }

  auto issue = [&](int stage, int kt) {
    char* sa = smem + stage * STAGE;
    char* sb = sa + A_BYTES;
#pragma unroll
    for (int i = 0; i < A_INSTR; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(a_src[i] + (long)kt * BK),
                                       (lptr_t)(sa + (wave * A_INSTR + i) * 1024), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < B_INSTR; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(b_src[i] + (long)kt * BK),
                                       (lptr_t)(sb + (wave * B_INSTR + i) * 1024), 16, 0, 0);
  };

  // ---- fragment addressing ----
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fg = lane >> 4;
  const int a_row0 = wm * (WM_FR * 16) + fr;  // + mi*16
  const int b_row0 = wn * (WN_FR * 16) + fr;
  int koff[2];
  koff[0] = ((0 * 4 + fg) ^ (fr & 7)) * 16;
  koff[1] = ((1 * 4 + fg) ^ (fr & 7)) * 16;

  f32x4 acc[WM_FR][WN_FR];
#pragma unroll
  for (int i = 0; i < WM_FR; ++i)
#pragma unroll
    for (int j = 0; j < WN_FR; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = g.K / BK;
  issue(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nk) issue((kt + 1) & 1, kt + 1);
    const char* sa = smem + (kt & 1) * STAGE;
    const char* sb = sa + A_BYTES;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[WM_FR], bfr[WN_FR];
#pragma unroll
      for (int mi = 0; mi < WM_FR; ++mi)
        af[mi] = *reinterpret_cast<const bf16x8*>(sa + (a_row0 + mi * 16) * 128 + koff[kk]);
#pragma unroll
      for (int ni = 0; ni < WN_FR; ++ni)
        bfr[ni] = *reinterpret_cast<const bf16x8*>(sb + (b_row0 + ni * 16) * 128 + koff[kk]);
#pragma unroll
      for (int mi = 0; mi < WM_FR; ++mi)
#pragma unroll
        for (int ni = 0; ni < WN_FR; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[ni], af[mi], acc[mi][ni], 0, 0, 0);
    }
  }

  // ---- epilogue: lane holds C[m = .. + fr][n = .. + fg*4 + 0..3] ----
#pragma unroll
  for (int mi = 0; mi < WM_FR; ++mi) {
    const int m = tm * BM + wm * (WM_FR * 16) + mi * 16 + fr;
    if (m >= g.M) continue;
#pragma unroll
    for (int ni = 0; ni < WN_FR; ++ni) {
      const int n = tn * BN + wn * (WN_FR * 16) + ni * 16 + fg * 4;
      if (n >= g.N) continue;
      store4<ACT>(g, m, n, acc[mi][ni]);
    }
  }
}


// ------------------------------------------------------------------------------------------------
// The 16-wave 256x256 kernel (4x4 waves of 64x64, 128 VGPRs -> 4 waves per SIMD: while one wave sits in a DMA issue or at the barrier three
// others feed the SIMD's MFMA pipe).  MFMA shape: v_mfma_f32_16x16x32_bf16, not the 32x32x16 this kernel used through round 2's first half
// (gemm_nt_256r_kernel, in the history).  Per FLOP the 16x16x32 instruction moves half the accumulator data (4 accumulator VGPRs per 16 KFLOP
// instead of 16 per 32 KFLOP) and under the 1400 W package cap a loop of nothing but MFMAs on random bf16 sustains 2.00 PFLOP/s with it
// against 1.78 (tools/mfma_peak.hip) - the GEMM is power-bound, so the cheaper instruction is the faster one: +3.4 .. +4.9 % on the LLaMA
// shapes, +3 % on the step, shader clock 1.87 -> 2.06 GHz under load, results bit-identical (profiles/r02_gemm_mfma_shape_ab.txt).
// A wave's 64x64 is 4x4 fragments of 16x16; one k-block = 32 k = 16 MFMAs, a stage = 2 k-blocks.  Fragment registers are single-buffered and
// ROLL - a fragment is re-read for the next block right behind the last MFMA that uses it (32 VGPRs; double-buffering 8 fragments of 4 VGPRs
// does not fit beside 64 accumulators) - and the MFMA order walks the 2x2 quadrants of the fragment grid (block 0: Q00 Q01 Q11 Q10, block 1:
// Q01 Q00 Q10 Q11) so that every fragment has >= 7 MFMA slots between its re-read and its next use; the waits are counted (LDS returns in
// order).  Order, re-reads, waits, barrier and DMA slots are generated: tools/gen_gemm16_sched.py -> gemm_256s_sched.inc.
// ------------------------------------------------------------------------------------------------
#include "gemm_256s_sched.inc"
__device__ __forceinline__ void lds_wait8(bf16x8 (&a)[4], bf16x8 (&b)[4]) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));
  __builtin_amdgcn_sched_barrier(0);
}

template <int ACT, int EPI, bool K2P>
__global__ __launch_bounds__(1024, 1) void gemm_nt_256s_kernel(GemmArgs g) {
  constexpr int BM = 256, BN = 256, BK = 64;
  constexpr int A_BYTES = BM * BK * 2, STAGE = A_BYTES + BN * BK * 2;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

  const int ntiles = g.tilesM * g.tilesN;
  int t = blockIdx.x;
  if (t >= ntiles) return;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // DMA: 64 pieces of 1 KiB per stage; wave w issues #4w..4w+3 (waves 0-7: A, 8-15: B)
  const bool isA = wave < 8;
  const char* base1 = reinterpret_cast<const char*>(isA ? g.A : g.B);
  const char* base2 = reinterpret_cast<const char*>(isA ? g.A2 : g.B2);
  const long ld1 = isA ? g.lda : g.ldb, ld2 = isA ? g.lda2 : g.ldb2;
  const int rmax = (isA ? g.M : g.N) - 1;
  const int nk1 = g.K / BK;
  const int nk = (g.K + (K2P ? g.K2 : 0)) / BK;  // >= 2 (host guarantees)
  // row of the operand that piece j of this lane reads for tile (tm_, tn_)
  auto dma_row = [&](int tm_, int tn_, int j) {
    const int row0 = isA ? tm_ * BM : tn_ * BN;
    const int ridx = (wave & 7) * 4 + j;
    int row = min(row0 + ridx * 8 + (lane >> 3), rmax);
    if (EPI == 1 && !isA) {  // B tile row r = 64*wn + 32*half + i  <-  weight row half*ff + tn*128 + wn*32 + i
      const int r = ridx * 8 + (lane >> 3);
      row = ((r >> 5) & 1) * g.ff + tn_ * 128 + (r >> 6) * 32 + (r & 31);
    }
    if (EPI == 3 && !isA && tn_ * BN < g.rope_cols) {  // B tile row r = 64*wn + 32*half + i  <-  head 2*tn + (wn >> 1), dim 64*half + 32*(wn & 1) + i
      const int r = ridx * 8 + (lane >> 3);
      row = tn_ * BN + ((r >> 7) << 7) + ((r >> 5) & 1) * 64 + ((r >> 6) & 1) * 32 + (r & 31);
    }
    return row;
  };
  // global byte offsets of this lane's four DMA rows for tile (tm_, tn_) in the FIRST operand pair.  The second pair (K2P: the fused LoRA
  // product, one or two stages at the end of the k-loop) gets its offsets where its pieces are issued: four more registers carried
  // through the main loop spilled there, and a scratch reload in the MFMA stream is followed by a full `vmcnt` wait - behind fresh DMA
  auto dma_rows = [&](int tm_, int tn_, unsigned (&o1)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int lchunk = (lane & 7) ^ ((((j & 1) << 2) + (lane >> 4)) & 7);
      o1[j] = (unsigned)(((long)dma_row(tm_, tn_, j) * ld1 + lchunk * 8) * 2);
    }
  };
  const int dst0 = (isA ? 0 : A_BYTES) + (wave & 7) * 4096;
  // wave-uniform 64-bit base (SGPR pair) + the lane's 32-bit row offset: the saddr form of global_load_lds.  The k offset goes through
  // readfirstlane so that the loop strength reduction cannot fold it into four loop-carried 64-bit VGPR pointers (8 registers).  The
  // instruction itself is inline asm: through the builtin the compiler forms a 64-bit VGPR address with two v_lshl_add_u64 and a v_mov per
  // piece - three VALU instructions in the MFMA stream for every DMA
  auto dma_piece = [&](const char* sp, unsigned vo, int buf, int j) {
    const unsigned lds_dst = (unsigned)(size_t)((__attribute__((address_space(3))) char*)smem) + buf * STAGE + dst0 + j * 1024;
    // the pointer goes through an SALU move: "VALU writes SGPR -> VMEM reads it" needs 5 wait states the compiler cannot pad inside asm (see gemm_u4.hip: U4_SPTR)
    asm volatile("s_mov_b64 s[100:101], %1\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, s[100:101]" ::"v"(vo), "s"(sp), "s"(lds_dst) : "memory", "m0", "s100", "s101");
  };
  auto issue1 = [&](const unsigned (&o1)[4], int kt, int buf, int j) {  // stage kt < nk1 of the first pair
    const int kb_ = __builtin_amdgcn_readfirstlane(kt * (BK * 2));
    dma_piece(base1 + kb_, o1[j], buf, j);
  };
  auto issue2 = [&](int tm_, int tn_, int kt2, int buf, int j) {        // stage kt2 of the second pair (K2P)
    const int kb_ = __builtin_amdgcn_readfirstlane(kt2 * (BK * 2));
    const int lchunk = (lane & 7) ^ ((((j & 1) << 2) + (lane >> 4)) & 7);
    dma_piece(base2 + kb_, (unsigned)(((long)dma_row(tm_, tn_, j) * ld2 + lchunk * 8) * 2), buf, j);
  };

  // fragment of 16 rows x 32 k: lane -> row (lane & 15), 16-byte chunk kb * 4 + (lane >> 4) of the 128-byte row (swizzled)
  const int wm = wave >> 2, wn = wave & 3;
  const int sw = ((lane & 15) >> 1) & 7;
  const unsigned lds0 = (unsigned)(size_t)((__attribute__((address_space(3))) char*)smem);
  // LDS address of this lane's fragment row in buffer 0, k-block 0 (the fragment index is the instruction's immediate offset).  smem is the
  // kernel's only LDS object (offset 0), so the other k-block is this address ^ 64 (chunk bit 2) and the other buffer ^ STAGE: every fragment
  // address of the main loop is ONE v_xor of these two registers with a loop-variant scalar (nothing for the compiler to hoist and keep)
  const unsigned a0 = lds0 + (wm * 64 + (lane & 15)) * 128 + (((lane >> 4)) ^ sw) * 16;
  const unsigned b0 = lds0 + A_BYTES + (wn * 64 + (lane & 15)) * 128 + (((lane >> 4)) ^ sw) * 16;

  const int nkl = nk;   // stages per tile
  int tm, tn;
  tile_coords_lin(g, t, ntiles, tm, tn);
  unsigned off1[4];
  dma_rows(tm, tn, off1);
  int pb = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) issue1(off1, 0, 0, j);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  bf16x8 A[4], B[4];
#define RDQ(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:" #off : "=v"(dst) : "v"(addr))
#define SB __builtin_amdgcn_sched_barrier(0);
#define MF(mi, ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(B[ni], A[mi], acc[mi][ni], 0, 0, 0); SB

  for (;;) {
    const int tnext = t + (int)gridDim.x;
    const bool has_next = tnext < ntiles;  // workgroup-uniform
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // stage 0 of this tile is in LDS buffer pb; the barrier publishes it and ends the previous tile's epilogue reads of the other buffer
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!K2P || 1 < nk1) issue1(off1, 1, pb ^ 1, j);
      else issue2(tm, tn, 1 - nk1, pb ^ 1, j);
    }
    {
      const unsigned aa = a0 ^ (unsigned)(pb * STAGE), ba = b0 ^ (unsigned)(pb * STAGE);
      RDQ(A[0], aa, 0); RDQ(A[1], aa, 2048); RDQ(A[2], aa, 4096); RDQ(A[3], aa, 6144);
      RDQ(B[0], ba, 0); RDQ(B[1], ba, 2048); RDQ(B[2], ba, 4096); RDQ(B[3], ba, 6144);
      lds_wait8(A, B);
    }
    // one stage = S_BLOCK0 (first 32 k; re-reads every fragment for the second 32 k of the same buffer) + S_BLOCK1 (the stage boundary -
    // full wait, vmcnt, barrier: stage s + 1 is published and the buffer of stage s is free - then the second 32 k, behind whose first
    // MFMAs the DMA of stage s + 2 goes into the freed buffer, and the re-reads from stage s + 1) - gemm_256s_sched.inc
#define STAGE_S(s_)                                                                                             \
    {                                                                                                           \
      const unsigned so = (((s_) + pb) & 1) * STAGE, sn = so ^ STAGE;                                           \
      { const unsigned aa = a0 ^ (so | 64u), ba = b0 ^ (so | 64u); S_BLOCK0(aa, ba) }                           \
      { const unsigned aa = a0 ^ sn, ba = b0 ^ sn; S_BLOCK1(aa, ba) }                                           \
    }
    // stage s fetches stage s + 2 of the tile: from the first pair while that is < nk1
    const int nA = K2P ? min(nkl - 2, nk1 - 2) : nkl - 2;
#define ISS(j) issue1(off1, s + 2, (s + pb) & 1, j);
    for (int s = 0; s < nA; ++s) STAGE_S(s)   // !K2P: every stage but the last two
#undef ISS
    if (K2P) {  // the stages whose DMA slot fetches the second pair
#define ISS(j) issue2(tm, tn, s + 2 - nk1, (s + pb) & 1, j);
      for (int s = max(nA, 0); s < nkl - 2; ++s) STAGE_S(s)
#undef ISS
    }
    int ntm = 0, ntn = 0;
    if (has_next) {  // this tile's DMA rows are not needed any more (its last stage is in flight): the offsets become the next tile's
      tile_coords_lin(g, tnext, ntiles, ntm, ntn);
      dma_rows(ntm, ntn, off1);
    }
    // stage nkl - 2: the buffer its barrier frees takes the first stage of the NEXT item (always a tile's stage 0)
#define ISS(j) if (has_next) issue1(off1, 0, (nkl + pb) & 1, j);
    STAGE_S(nkl - 2)
#undef ISS
#undef STAGE_S
    {  // last stage: nothing left to fetch behind it
      const unsigned so = ((nkl - 1 + pb) & 1) * STAGE;
      { const unsigned aa = a0 ^ (so | 64u), ba = b0 ^ (so | 64u); S_BLOCK0(aa, ba) }
      S_BLOCK1_FINAL(0, 0)
    }

    // accumulator element acc[mi][ni][i]: m = wm*64 + mi*16 + fr, n = wn*64 + ni*16 + fg*4 + i.
    // Everything the epilogue derives from the lane id is derived from an opaque copy made HERE, per tile: otherwise those values are
    // loop-invariant across tiles, get hoisted in front of the tile loop and sit in (or spill from) registers all through the main loop
    int le = lane;
    asm volatile("" : "+v"(le));
    const int fr = le & 15, fg = le >> 4;
    if (g.out_f32) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const int m = tm * BM + wm * 64 + mi * 16 + fr;
        if (m >= g.M) continue;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          const int n = tn * BN + wn * 64 + ni * 16 + fg * 4;
          if (n >= g.N) continue;
          store4<ACT>(g, m, n, acc[mi][ni]);
        }
      }
    } else {
      __builtin_amdgcn_s_barrier();  // every wave has read its last fragments: the last stage's buffer becomes the staging area
      char* reg = smem + ((nkl - 1 + pb) & 1) * STAGE + wave * 4096;  // [32 rows][64 cols] bf16, wave private, one pass per 32 rows
      const bool rope_tile = EPI == 3 && tn * BN < g.rope_cols;
      const int rsub = le >> 3, c = le & 7;
      const int n = EPI == 1   ? (c < 4 ? 0 : g.ff) + tn * 128 + wn * 32 + (c & 3) * 8
                    : rope_tile ? tn * BN + (wn >> 1) * 128 + (c < 4 ? 0 : 64) + (wn & 1) * 32 + (c & 3) * 8
                                : tn * BN + wn * 64 + c * 8;
      constexpr bool SWB = EPI == 2;   // SwiGLU-backward epilogue
      const int nlim = SWB ? g.ff : g.N;
      const bool col_ok = n < nlim;
#pragma unroll
      for (int ps = 0; ps < 2; ++ps) {
        uint4 pre_a[4], pre_b[4];
        if (SWB || (EPI == 0 && g.res)) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int m = tm * BM + wm * 64 + ps * 32 + i * 8 + rsub;
            pre_a[i] = make_uint4(0, 0, 0, 0); pre_b[i] = make_uint4(0, 0, 0, 0);
            if (m < g.M && col_ok) {
              if (SWB) {
                pre_a[i] = *reinterpret_cast<const uint4*>(g.aux + (long)m * g.ld_aux + n);
                pre_b[i] = *reinterpret_cast<const uint4*>(g.aux + (long)m * g.ld_aux + g.ff + n);
              } else {
                pre_a[i] = *reinterpret_cast<const uint4*>(g.res + (long)m * g.ldr + n);
              }
            }
          }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int mi = ps * 2 + h;
          const int row = h * 16 + fr;  // row inside this 32-row pass
          if (rope_tile) {
            // fragments ni = 0, 1 hold dims d = 32*(wn & 1) + 16*ni + 4*fg + i of the head, ni + 2 their rotate_half partners d + 64
            const int pos = (tm * BM + wm * 64 + mi * 16 + fr) % g.rope_mod + g.rope_pos0;
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
              const float4 c4 = *reinterpret_cast<const float4*>(g.rope_cos + (long)pos * 64 + (wn & 1) * 32 + ni * 16 + fg * 4);
              const float4 s4 = *reinterpret_cast<const float4*>(g.rope_sin + (long)pos * 64 + (wn & 1) * 32 + ni * 16 + fg * 4);
              const float cv[4] = {c4.x, c4.y, c4.z, c4.w}, sv[4] = {s4.x, s4.y, s4.z, s4.w};
              float o1[4], o2[4];
#pragma unroll
              for (int i = 0; i < 4; ++i)
                rope_pair(bf2f(f2bf(acc[mi][ni][i] * g.alpha)), bf2f(f2bf(acc[mi][ni + 2][i] * g.alpha)), cv[i], sv[i], o1[i], o2[i]);
              const int u = ni * 4 + fg;
              *reinterpret_cast<uint2*>(reg + row * 128 + ((u ^ ((row & 7) << 1)) << 3)) = make_uint2(pack2bf(o1[0], o1[1]), pack2bf(o1[2], o1[3]));
              *reinterpret_cast<uint2*>(reg + row * 128 + (((8 + u) ^ ((row & 7) << 1)) << 3)) = make_uint2(pack2bf(o2[0], o2[1]), pack2bf(o2[2], o2[3]));
            }
          } else {
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
              float v[4];
              uint2 bb = make_uint2(0, 0);
              if (EPI == 0 && g.bias) bb = *reinterpret_cast<const uint2*>(g.bias + min(tn * BN + wn * 64 + ni * 16 + fg * 4, g.N - 4));
              const float bias_v[4] = {bflo(bb.x), bfhi(bb.x), bflo(bb.y), bfhi(bb.y)};
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                v[i] = acc[mi][ni][i] * g.alpha;
                if (EPI == 0 && g.drop_thresh) {
                  const long e = (long)(tm * BM + wm * 64 + mi * 16 + fr) * g.N + tn * BN + wn * 64 + ni * 16 + fg * 4 + i;
                  v[i] = drop_keep(g.drop_seed, e, g.drop_thresh) ? v[i] * g.drop_scale : 0.f;
                }
                v[i] += bias_v[i];
                if (ACT) v[i] = apply_act(v[i], ACT);
              }
              const int u = ni * 4 + fg;
              *reinterpret_cast<uint2*>(reg + row * 128 + ((u ^ ((row & 7) << 1)) << 3)) = make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
            }
          }
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r32 = i * 8 + rsub;
          const int m = tm * BM + wm * 64 + ps * 32 + r32;
          uint4 val = *reinterpret_cast<const uint4*>(reg + r32 * 128 + ((c ^ (r32 & 7)) << 4));
          if (SWB && m < g.M && col_ok) {
            const uint4 gq = pre_a[i], uq = pre_b[i];
            float d[8], gg[8], uu[8], dg[8], du[8];
            unpack8(val, d); unpack8(gq, gg); unpack8(uq, uu);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float sg = sigmoid_f(gg[e]);
              du[e] = d[e] * gg[e] * sg;
              dg[e] = d[e] * uu[e] * sg * (1.f + gg[e] * (1.f - sg));
            }
            bf16_t* out = reinterpret_cast<bf16_t*>(g.C) + (long)m * g.ldc + n;
            *reinterpret_cast<uint4*>(out) = pack8(dg);
            *reinterpret_cast<uint4*>(out + g.ff) = pack8(du);
          }
          if (SWB) continue;
          if (m < g.M && col_ok) {
            if (EPI == 0 && g.res) {
              const uint4 r = pre_a[i];
              val.x = pack2bf(bflo(val.x) + bflo(r.x), bfhi(val.x) + bfhi(r.x));
              val.y = pack2bf(bflo(val.y) + bflo(r.y), bfhi(val.y) + bfhi(r.y));
              val.z = pack2bf(bflo(val.z) + bflo(r.z), bfhi(val.z) + bfhi(r.z));
              val.w = pack2bf(bflo(val.w) + bflo(r.w), bfhi(val.w) + bfhi(r.w));
            }
            *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(g.C) + (long)m * g.ldc + n) = val;
          }
        }
      }
      if (EPI == 1) {
        // second output: act = silu(gate) * up on the bf16-rounded gate / up (fragments ni = 0, 1 / ni + 2), staged [64][32]
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
          const int row = mi * 16 + fr;
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) {
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float gv = bf2f(f2bf(acc[mi][ni][i] * g.alpha)), uv = bf2f(f2bf(acc[mi][ni + 2][i] * g.alpha));
              v[i] = silu(gv) * uv;
            }
            const int u = ni * 4 + fg;  // 8-byte unit 0..7 of the 64-byte row
            *reinterpret_cast<uint2*>(reg + row * 64 + ((u ^ ((row & 3) << 1)) << 3)) = make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
          }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const int rsub4 = le >> 2, c4 = le & 3;
        const int n2 = tn * 128 + wn * 32 + c4 * 8;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = i * 16 + rsub4;
          const int m = tm * BM + wm * 64 + row;
          const uint4 val = *reinterpret_cast<const uint4*>(reg + row * 64 + ((c4 ^ (row & 3)) << 4));
          if (m < g.M) *reinterpret_cast<uint4*>(g.aux_out + (long)m * g.ld_aux + n2) = val;
        }
      }
    }
    if (!has_next) break;
    if (g.out_f32) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    t = tnext; tm = ntm; tn = ntn;
    pb = (pb + nkl) & 1;
  }
#undef MF
#undef SB
#undef RDQ
}



#include "gemm_144s_kernel.inc"

// ------------------------------------------------------------------------------------------------
// e4m3 x e4m3 -> bf16 GEMM for FROZEN base weights in 8-bit (the reference trains stages 2/3 with `bits: 8` base weights,
// lhrs/models/text_modal.py:91-131 -> bitsandbytes LLM.int8): C[m][n] = sa[m] * sb[n] * sum_k A8[m][k] * B8[n][k]
// (+ residual).  Same skeleton as the bf16 256x256 kernels - 256x256 tile, 8 waves, two 64 KiB LDS buffers filled by global_load_lds,
// one barrier per stage - but a stage row is 128 BYTES = 128 k and the product runs on v_mfma_scale_f32_32x32x64_f8f6f4 with unit
// block scales (the only 2x-rate fp8 MFMA of gfx950): a stage is two blocks of 8 MFMAs (64 k each, 16 passes), every lane feeds
// 32 consecutive k-bytes of its row (two ds_read_b128) to both operands.  Twice the FLOPs of the bf16 kernel per byte moved.
// ------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(8))) int i32x8;

// I8 = true: the same kernel on LLM.int8 operands (int8.hip; the reference's `bits: 8` base, text_modal.py:91-131 -> bitsandbytes MatMul8bitLt):
// a lane's 32 k-bytes feed TWO v_mfma_i32_32x32x32_i8 (bytes [0,16) and [16,32): both operands are read with the same addressing, so which k
// a byte slot holds does not matter) into int32 accumulators - exact -, converted to f32 once the 8-bit stages are done; the per-row factors
// sa[m] = absmax / 127 and sb[n] = absmax / 127 then turn them into real units, and the optional bf16 stages behind them carry the 16-bit
// outlier-column product (and the LoRA update) on the same accumulators.
template <bool I8>
__global__ __launch_bounds__(512, 2) void gemm_fp8_256_kernel(GemmArgs g) {
  constexpr int BM = 256, BN = 256, BKB = 128;  // bytes (= k) per stage row
  constexpr int A_BYTES = BM * BKB, STAGE = A_BYTES + BN * BKB;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

  int tm, tn;
  tile_coords(g, tm, tn);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  const bool isA = wave < 4;
  const char* base1 = reinterpret_cast<const char*>(isA ? g.A : g.B);
  const long ld1 = isA ? g.lda : g.ldb;  // bytes
  const int row0 = isA ? tm * BM : tn * BN, rmax = (isA ? g.M : g.N) - 1;
  // optional bf16 pair (fused LoRA update, K2 % 64 == 0): its 64-k stages have the same 128-byte row image and follow the e4m3 stages
  const char* base2 = reinterpret_cast<const char*>(isA ? g.A2 : g.B2);
  const long ld2 = (isA ? g.lda2 : g.ldb2) * 2L;  // bytes
  const int nk1 = g.K / BKB;
  const int K2 = g.K2 + (g.k2_dev ? __builtin_amdgcn_readfirstlane(g.k2_dev[0]) : 0);   // host-known + device-known bf16 columns
  unsigned off1[8], off2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ridx = (wave & 3) * 8 + j;
    const int lchunk = (lane & 7) ^ ((((j & 1) << 2) + (lane >> 4)) & 7);
    const int row = min(row0 + ridx * 8 + (lane >> 3), rmax);
    off1[j] = (unsigned)((long)row * ld1 + lchunk * 16);
    off2[j] = K2 > 0 ? (unsigned)((long)row * ld2 + lchunk * 16) : 0u;
  }
  const int dst0 = (isA ? 0 : A_BYTES) + (wave & 3) * 8192;
  const int nk_all = nk1 + K2 / 64;    // e4m3 stages + bf16 stages of the fused pair
  auto issue1 = [&](int kt, int j) {
    if (kt >= nk_all) return;            // (wave-uniform) nothing left to fetch
    const char* p = kt < nk1 ? base1 + (long)kt * BKB + off1[j] : base2 + (long)(kt - nk1) * BKB + off2[j];
    __builtin_amdgcn_global_load_lds((gptr_t)p, (lptr_t)(smem + (kt & 1) * STAGE + dst0 + j * 1024), 16, 0, 0);
  };

  const int wm = wave >> 2, wn = wave & 3;
  const int fr = lane & 31, fh = lane >> 5;
  const int sw = (fr >> 1) & 7;
  const unsigned lds0 = (unsigned)(size_t)((__attribute__((address_space(3))) char*)smem);
  const unsigned a_base = lds0 + (wm * 128 + fr) * 128;
  const unsigned b_base = lds0 + A_BYTES + (wn * 64 + fr) * 128;
  unsigned kofs[2][2];  // [k-step][16-B half]
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) kofs[ks][hh] = ((ks * 4 + fh * 2 + hh) ^ sw) * 16;

  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  i32x8 a0[4], b0[2], a1[4], b1[2];
  // one fragment = two ds_read_b128 (k-bytes [0,16) and [16,32) of the lane's 32) forming one 8-VGPR operand.  Plain LDS loads, not
  // inline asm as in the bf16 kernels: the halves of an 8-register tuple cannot be named as asm outputs, and letting the compiler see
  // the loads keeps its register reuse and s_waitcnt placement correct around the 16-pass MFMAs (sched_barriers pin the interleave)
  typedef const __attribute__((address_space(3))) i32x4* lds4_t;
#define RD8(dst, addr0, addr1, off)                                                                                  \
  do {                                                                                                               \
    const i32x4 lo_ = *reinterpret_cast<lds4_t>((size_t)((addr0) + (off)));                                          \
    const i32x4 hi_ = *reinterpret_cast<lds4_t>((size_t)((addr1) + (off)));                                          \
    dst = i32x8{lo_[0], lo_[1], lo_[2], lo_[3], hi_[0], hi_[1], hi_[2], hi_[3]};                                     \
  } while (0)
  typedef __attribute__((ext_vector_type(16))) int i32x16_t;
#define MF8(A_, B_, mi, ni)                                                                                          \
  if constexpr (I8) {                                                                                                \
    i32x16_t c_ = __builtin_bit_cast(i32x16_t, acc[mi][ni]);                                                         \
    c_ = __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_shufflevector(B_[ni], B_[ni], 0, 1, 2, 3),                  \
                                               __builtin_shufflevector(A_[mi], A_[mi], 0, 1, 2, 3), c_, 0, 0, 0);   \
    c_ = __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_shufflevector(B_[ni], B_[ni], 4, 5, 6, 7),                  \
                                               __builtin_shufflevector(A_[mi], A_[mi], 4, 5, 6, 7), c_, 0, 0, 0);   \
    acc[mi][ni] = __builtin_bit_cast(f32x16, c_);                                                                    \
  } else {                                                                                                           \
    acc[mi][ni] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(B_[ni], A_[mi], acc[mi][ni], 0, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F); \
  }                                                                                                                  \
  __builtin_amdgcn_sched_barrier(0);
#define SB8 __builtin_amdgcn_sched_barrier(0);
  // one block: 8 MFMAs (64 k); fillers: the 6 fragments (12 reads) of the next block and up to 8 DMA pieces of stage kd
#define BLOCK8(Ac, Bc, An, Bn, aa0, aa1, ba0, ba1, RD, kd, d0, NDMA)                                       \
  MF8(Ac, Bc, 0, 0) if (RD) RD8(Bn[0], ba0, ba1, 0);     if (NDMA > 0) issue1(kd, d0);     SB8             \
  MF8(Ac, Bc, 0, 1) if (RD) RD8(Bn[1], ba0, ba1, 4096);  if (NDMA > 1) issue1(kd, d0 + 1); SB8             \
  MF8(Ac, Bc, 1, 0) if (RD) RD8(An[0], aa0, aa1, 0);     if (NDMA > 2) issue1(kd, d0 + 2); SB8             \
  MF8(Ac, Bc, 1, 1) if (RD) RD8(An[1], aa0, aa1, 4096);  if (NDMA > 3) issue1(kd, d0 + 3); SB8             \
  MF8(Ac, Bc, 2, 0) if (RD) RD8(An[2], aa0, aa1, 8192);  if (NDMA > 4) issue1(kd, d0 + 4); SB8             \
  MF8(Ac, Bc, 2, 1) if (RD) RD8(An[3], aa0, aa1, 12288); if (NDMA > 5) issue1(kd, d0 + 5); SB8             \
  MF8(Ac, Bc, 3, 0)                                      if (NDMA > 6) issue1(kd, d0 + 6); SB8             \
  MF8(Ac, Bc, 3, 1)                                      if (NDMA > 7) issue1(kd, d0 + 7); SB8

  const int nk = nk1;                    // e4m3 stages, >= 2 (host guarantees)
#pragma unroll
  for (int j = 0; j < 8; ++j) issue1(0, j);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int j = 0; j < 8; ++j) issue1(1, j);
  {
    const unsigned aa0 = a_base + kofs[0][0], aa1 = a_base + kofs[0][1], ba0 = b_base + kofs[0][0], ba1 = b_base + kofs[0][1];
    RD8(b0[0], ba0, ba1, 0); RD8(b0[1], ba0, ba1, 4096);
    RD8(a0[0], aa0, aa1, 0); RD8(a0[1], aa0, aa1, 4096); RD8(a0[2], aa0, aa1, 8192); RD8(a0[3], aa0, aa1, 12288);
  }
  {  // block ks0 of stage 0; loads ks1 of stage 0
    const unsigned aa0 = a_base + kofs[1][0], aa1 = a_base + kofs[1][1], ba0 = b_base + kofs[1][0], ba1 = b_base + kofs[1][1];
    BLOCK8(a0, b0, a1, b1, aa0, aa1, ba0, ba1, true, 0, 0, 0)
  }
  auto stage = [&](int kt) {
    constexpr bool DMA = true;  // issue1 is a no-op past the last stage
    const unsigned so = (kt & 1) * STAGE;
    // block ks1(kt-1): retire its fragment reads, then the barrier that publishes stage kt and frees the other buffer
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    {
      const unsigned aa0 = a_base + so + kofs[0][0], aa1 = a_base + so + kofs[0][1], ba0 = b_base + so + kofs[0][0], ba1 = b_base + so + kofs[0][1];
      BLOCK8(a1, b1, a0, b0, aa0, aa1, ba0, ba1, true, kt + 1, 0, (DMA ? 8 : 0))
    }
      {
      const unsigned aa0 = a_base + so + kofs[1][0], aa1 = a_base + so + kofs[1][1], ba0 = b_base + so + kofs[1][0], ba1 = b_base + so + kofs[1][1];
      BLOCK8(a0, b0, a1, b1, aa0, aa1, ba0, ba1, true, 0, 0, 0)
    }
  };
  for (int kt = 1; kt < nk; ++kt) stage(kt);  // the last e4m3 stage already fetches the first bf16 stage of a fused pair
  { BLOCK8(a1, b1, a0, b0, a_base, a_base, b_base, b_base, false, 0, 0, 0) }
#undef BLOCK8
#undef SB8
#undef MF8
#undef RD8

  if constexpr (I8) {  // int32 sums -> f32 (exact below 2^24; |sum| <= 127 * 127 * K stays far inside f32's range, the rounding is 2^-24 relative)
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const i32x16_t c_ = __builtin_bit_cast(i32x16_t, acc[mi][ni]);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][ni][r] = (float)c_[r];
      }
  }
  bool scaled = false;
  if (nk_all > nk) {
    // ---- fused LoRA pair: bring the e4m3 sums to real units, then keep accumulating bf16 products (C layout is dtype-independent)
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const float sa = g.sa[min(tm * BM + wm * 128 + mi * 32 + fr, g.M - 1)];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 s4 = *reinterpret_cast<const float4*>(g.sb + min(tn * BN + wn * 64 + ni * 32 + q * 8 + fh * 4, g.N - 4));
          acc[mi][ni][4 * q] *= sa * s4.x; acc[mi][ni][4 * q + 1] *= sa * s4.y;
          acc[mi][ni][4 * q + 2] *= sa * s4.z; acc[mi][ni][4 * q + 3] *= sa * s4.w;
        }
    }
    scaled = true;
    typedef const __attribute__((address_space(3))) bf16x8* ldsb_t;
    for (int kt = nk; kt < nk_all; ++kt) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // stage kt has landed everywhere; every wave is done with the other buffer
      if (kt + 1 < nk_all) {
#pragma unroll
        for (int j = 0; j < 8; ++j) issue1(kt + 1, j);
      }
      const unsigned so = (kt & 1) * STAGE;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const unsigned ko = (((kk * 2 + fh) ^ sw) * 16);
        bf16x8 af[4], bfr[2];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) af[mi] = *reinterpret_cast<ldsb_t>((size_t)(a_base + so + ko + mi * 4096));
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) bfr[ni] = *reinterpret_cast<ldsb_t>((size_t)(b_base + so + ko + ni * 4096));
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bfr[ni], af[mi], acc[mi][ni], 0, 0, 0);
      }
    }
  }

  __builtin_amdgcn_s_barrier();
  char* reg = smem + wave * 16384;
  {
    float sbv[2][4][4];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = min(tn * BN + wn * 64 + ni * 32 + q * 8 + fh * 4, g.N - 4);
        float4 s4 = *reinterpret_cast<const float4*>(g.sb + n);
        if (scaled) s4 = make_float4(1.f, 1.f, 1.f, 1.f);
        sbv[ni][q][0] = s4.x; sbv[ni][q][1] = s4.y; sbv[ni][q][2] = s4.z; sbv[ni][q][3] = s4.w;
      }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int row = mi * 32 + fr;
      const float sa = (scaled ? 1.f : g.sa[min(tm * BM + wm * 128 + row, g.M - 1)]) * g.alpha;
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float v[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = acc[mi][ni][4 * q + i] * sa * sbv[ni][q][i];
          const int u = ni * 8 + q * 2 + fh;
          *reinterpret_cast<uint2*>(reg + row * 128 + ((u ^ ((row & 7) << 1)) << 3)) = make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
        }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  {
    const int rsub = lane >> 3, c = lane & 7;
    const int n = tn * BN + wn * 64 + c * 8;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = i * 8 + rsub;
      const int m = tm * BM + wm * 128 + row;
      uint4 val = *reinterpret_cast<const uint4*>(reg + row * 128 + ((c ^ (row & 7)) << 4));
      if (m < g.M && n < g.N) {
        if (g.res) {
          const uint4 r = *reinterpret_cast<const uint4*>(g.res + (long)m * g.ldr + n);
          val.x = pack2bf(bflo(val.x) + bflo(r.x), bfhi(val.x) + bfhi(r.x));
          val.y = pack2bf(bflo(val.y) + bflo(r.y), bfhi(val.y) + bfhi(r.y));
          val.z = pack2bf(bflo(val.z) + bflo(r.z), bfhi(val.z) + bfhi(r.z));
          val.w = pack2bf(bflo(val.w) + bflo(r.w), bfhi(val.w) + bfhi(r.w));
        }
        *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(g.C) + (long)m * g.ldc + n) = val;
      }
    }
  }
}

// sum of `splits` f32 slabs [M, ldc] -> bf16 C[M, N] * alpha
// (+ residual[M, ldr] added in fp32 before the one rounding, as the GEMM epilogues do; res may alias C)
__global__ void splitk_reduce_kernel(const float* __restrict__ part, bf16_t* C, long ldc, int M, int N, int splits, float alpha,
                                     const bf16_t* res = nullptr, long ldr = 0) {
  const long total = (long)M * (N / 4);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long m = i / (N / 4);
    const int n = (int)(i % (N / 4)) * 4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < splits; ++k) {
      const float4 v = *reinterpret_cast<const float4*>(part + ((long)k * M + m) * N + n);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    s.x *= alpha; s.y *= alpha; s.z *= alpha; s.w *= alpha;
    if (res) {
      const uint2 r = *reinterpret_cast<const uint2*>(res + m * ldr + n);
      s.x += bflo(r.x); s.y += bfhi(r.x); s.z += bflo(r.y); s.w += bfhi(r.y);
    }
    *reinterpret_cast<uint2*>(C + m * ldc + n) = make_uint2(pack2bf(s.x, s.y), pack2bf(s.z, s.w));
  }
}

// sum of `splits` f32 slabs [M, N] -> f32 C[M, ldc]
__global__ void splitk_reduce_f32_kernel(const float* __restrict__ part, float* __restrict__ C, long ldc, int M, int N, int splits) {
  const long total = (long)M * (N / 4);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long m = i / (N / 4);
    const int n = (int)(i % (N / 4)) * 4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < splits; ++k) {
      const float4 v = *reinterpret_cast<const float4*>(part + ((long)k * M + m) * N + n);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *reinterpret_cast<float4*>(C + m * ldc + n) = s;
  }
}

}  // namespace

// ---- optional live timing of the GEMM launches (bench.py roofline leg) -----------------------------------
// When enabled, every launch of the 128x128 kernel is bracketed by HIP events ON THE LAUNCH STREAM until the
// event pool is used up; lhrs_gemm_profile_read synchronises those events and returns summed time and flops.
namespace {
struct GemmProf {
  bool on = false;
  int cap = 0, used = 0;
  hipEvent_t* ev = nullptr;   // 2 * cap
  double* flops = nullptr;    // cap
  int* kind = nullptr;        // cap: epilogue variant of the sampled launch (0 plain <ACT,0>, 1 SwiGLU fwd, 2 SwiGLU bwd, 3 RoPE)
  double total_flops_all = 0; // every GEMM launch while enabled (sampled or not)
  long launches_all = 0;
  int stride = 1;             // every stride-th launch of each epilogue variant is bracketed (lhrs_gemm_profile_stride)
  long seen[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // kinds: see lhrs_gemm_profile_read_kinds
  bool take(int kind) { return (seen[kind]++ % stride) == 0; }
} g_prof;
}  // namespace

// Sampling stride of the live timing: the two event records around a launch cost the stream ~3 us of idle time each (measured: timing
// EVERY dominant launch slows the step by 1.0 % at micro-batch 30 and 2.2 % at micro-batch 8), so bench.py brackets every 7th launch of
// each variant - 7 is coprime to the period of the launch sequence (2 plain launches per layer forward, 3 backward), so the sample keeps
// the shape mix.  Default 1 (every launch).
extern "C" int lhrs_gemm_profile_stride(int n) { g_prof.stride = n > 0 ? n : 1; return 0; }

extern "C" int lhrs_gemm_profile_enable(int max_samples) {
  if (g_prof.ev) {
    for (int i = 0; i < 2 * g_prof.cap; ++i) (void)hipEventDestroy(g_prof.ev[i]);
    delete[] g_prof.ev; delete[] g_prof.flops; delete[] g_prof.kind;
    g_prof.ev = nullptr; g_prof.flops = nullptr; g_prof.kind = nullptr;
  }
  g_prof.on = max_samples > 0; g_prof.cap = max_samples > 0 ? max_samples : 0; g_prof.used = 0;
  g_prof.total_flops_all = 0; g_prof.launches_all = 0;
  for (int k = 0; k < 10; ++k) g_prof.seen[k] = 0;
  if (g_prof.on) {
    g_prof.ev = new hipEvent_t[2 * g_prof.cap];
    g_prof.flops = new double[g_prof.cap];
    g_prof.kind = new int[g_prof.cap];
    for (int i = 0; i < 2 * g_prof.cap; ++i)
      if (hipEventCreate(&g_prof.ev[i]) != hipSuccess) LHRS_FAIL("gemm_profile_enable: hipEventCreate failed");
  }
  return 0;
}

// out[0] = sampled launches, out[1] = their summed duration (ms), out[2] = their summed flops,
// out[3] = all GEMM launches while enabled, out[4] = flops of all of them
extern "C" int lhrs_gemm_profile_read(double* out) {
  double ms = 0, fl = 0, n = 0;
  for (int i = 0; i < g_prof.used; ++i) {
    if (g_prof.kind[i] != 0 && g_prof.kind[i] != 4) continue;  // the plain-epilogue persistent kernels (256-row + 144-row tiles); per kernel / variant: lhrs_gemm_profile_read_kinds
    float t = 0;
    if (hipEventSynchronize(g_prof.ev[2 * i + 1]) != hipSuccess) LHRS_FAIL("gemm_profile_read: event sync failed");
    if (hipEventElapsedTime(&t, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]) != hipSuccess) LHRS_FAIL("gemm_profile_read: elapsed failed");
    ms += t; fl += g_prof.flops[i]; n += 1;
  }
  out[0] = n; out[1] = ms; out[2] = fl; out[3] = (double)g_prof.launches_all; out[4] = g_prof.total_flops_all;
  return 0;
}

// out[10][3] = {sampled launches, their summed duration (ms), their summed flops} per kind - one kind per kernel instantiation a rocprofv3 kernel trace lists:
//   0 gemm_nt_256s_kernel<ACT, 0, ..> plain (16 waves)   1 <0, 1> SwiGLU fwd   2 <0, 2> SwiGLU bwd   3 <0, 3> RoPE   4 gemm_nt_144s_kernel<ACT, 0> plain 144-row tiles
//   5 gemm_u4_kernel<0, true> plain + residual (four waves)   6 gemm_u4_kernel<0, false> plain   7 gemm_u4_kernel<1, false> SwiGLU fwd   8 <2, false> SwiGLU bwd   9 <3, false> RoPE
extern "C" int lhrs_gemm_profile_read_kinds(double* out) {
  for (int i = 0; i < 30; ++i) out[i] = 0;
  for (int i = 0; i < g_prof.used; ++i) {
    float t = 0;
    if (hipEventSynchronize(g_prof.ev[2 * i + 1]) != hipSuccess) LHRS_FAIL("gemm_profile_read_kinds: event sync failed");
    if (hipEventElapsedTime(&t, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]) != hipSuccess) LHRS_FAIL("gemm_profile_read_kinds: elapsed failed");
    const int k = g_prof.kind[i];
    out[3 * k] += 1; out[3 * k + 1] += t; out[3 * k + 2] += g_prof.flops[i];
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Small-tile sibling of gemm_fp8_256_kernel (64x128 tile, 4 waves, the 2-stage DMA skeleton of gemm_nt_kernel; a stage row is 128 e4m3
// bytes = one v_mfma_scale_f32_16x16x128_f8f6f4 step per fragment pair).  Takes the tail rows that the 256x256 kernel would run as a
// nearly empty last round (the tail-row rule: tail_main_rows, gemm_plan.h).  Same arithmetic and roundings as the big kernel: scale the e4m3 sum by
// sa[m] * sb[n], add the optional bf16 pair (LoRA) on the same accumulators, * alpha, round to bf16, then add the bf16 residual.
// ------------------------------------------------------------------------------------------------
template <int WM_FR, int WN_FR>
__global__ __launch_bounds__(256) void gemm_fp8_small_kernel(GemmArgs g) {
  constexpr int BM = WM_FR * 32, BN = WN_FR * 32, ROWB = 128;
  constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB, STAGE = A_BYTES + B_BYTES;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  int tm, tn;
  tile_coords(g, tm, tn);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr int A_INSTR = BM / 32, B_INSTR = BN / 32;  // 1-KiB pieces (8 rows x 128 B) per wave
  const int lrow = lane >> 3;
  const int lchunk = (lane & 7) ^ lrow;
  const char *a_src[A_INSTR], *b_src[B_INSTR], *a2_src[A_INSTR], *b2_src[B_INSTR];
#pragma unroll
  for (int i = 0; i < A_INSTR; ++i) {
    const int row = min(tm * BM + (wave * A_INSTR + i) * 8 + lrow, g.M - 1);
    a_src[i] = reinterpret_cast<const char*>(g.A) + (long)row * g.lda + lchunk * 16;
    a2_src[i] = reinterpret_cast<const char*>(g.A2) + ((long)row * g.lda2 + lchunk * 8) * 2;
  }
#pragma unroll
  for (int i = 0; i < B_INSTR; ++i) {
    const int row = min(tn * BN + (wave * B_INSTR + i) * 8 + lrow, g.N - 1);
    b_src[i] = reinterpret_cast<const char*>(g.B) + (long)row * g.ldb + lchunk * 16;
    b2_src[i] = reinterpret_cast<const char*>(g.B2) + ((long)row * g.ldb2 + lchunk * 8) * 2;
  }
  const int nk1 = g.K / 128, nk = nk1 + g.K2 / 64;
  auto issue = [&](int kt) {
    char* sa = smem + (kt & 1) * STAGE;
    char* sb = sa + A_BYTES;
    const bool e4 = kt < nk1;  // wave-uniform
    const long ko = (long)(e4 ? kt : kt - nk1) * ROWB;
#pragma unroll
    for (int i = 0; i < A_INSTR; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)((e4 ? a_src[i] : a2_src[i]) + ko), (lptr_t)(sa + (wave * A_INSTR + i) * 1024), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < B_INSTR; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)((e4 ? b_src[i] : b2_src[i]) + ko), (lptr_t)(sb + (wave * B_INSTR + i) * 1024), 16, 0, 0);
  };
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fg = lane >> 4;
  const int a_row0 = wm * (WM_FR * 16) + fr, b_row0 = wn * (WN_FR * 16) + fr;
  f32x4 acc[WM_FR][WN_FR];
#pragma unroll
  for (int i = 0; i < WM_FR; ++i)
#pragma unroll
    for (int j = 0; j < WN_FR; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  issue(0);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nk) issue(kt + 1);
    const char* sa = smem + (kt & 1) * STAGE;
    const char* sb = sa + A_BYTES;
    if (kt < nk1) {  // 128 e4m3 k per row: lane (r, g) feeds bytes [32g, 32g + 32) = chunks 2g, 2g + 1
      const int c0 = ((2 * fg) ^ (fr & 7)) * 16, c1 = ((2 * fg + 1) ^ (fr & 7)) * 16;
      i32x8 af[WM_FR], bfr[WN_FR];
#pragma unroll
      for (int mi = 0; mi < WM_FR; ++mi) {
        const i32x4 lo = *reinterpret_cast<const i32x4*>(sa + (a_row0 + mi * 16) * ROWB + c0), hi = *reinterpret_cast<const i32x4*>(sa + (a_row0 + mi * 16) * ROWB + c1);
        af[mi] = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
#pragma unroll
      for (int ni = 0; ni < WN_FR; ++ni) {
        const i32x4 lo = *reinterpret_cast<const i32x4*>(sb + (b_row0 + ni * 16) * ROWB + c0), hi = *reinterpret_cast<const i32x4*>(sb + (b_row0 + ni * 16) * ROWB + c1);
        bfr[ni] = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
#pragma unroll
      for (int mi = 0; mi < WM_FR; ++mi)
#pragma unroll
        for (int ni = 0; ni < WN_FR; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bfr[ni], af[mi], acc[mi][ni], 0, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
      if (kt + 1 == nk1 && g.K2 > 0) {  // the bf16 pair rides on the SCALED sums
#pragma unroll
        for (int mi = 0; mi < WM_FR; ++mi) {
          const float sam = g.sa[min(tm * BM + wm * (WM_FR * 16) + mi * 16 + fr, g.M - 1)];
#pragma unroll
          for (int ni = 0; ni < WN_FR; ++ni) {
            const float4 s4 = *reinterpret_cast<const float4*>(g.sb + min(tn * BN + wn * (WN_FR * 16) + ni * 16 + fg * 4, g.N - 4));
            acc[mi][ni][0] *= sam * s4.x; acc[mi][ni][1] *= sam * s4.y; acc[mi][ni][2] *= sam * s4.z; acc[mi][ni][3] *= sam * s4.w;
          }
        }
      }
    } else {  // 64 bf16 k per row, exactly gemm_nt_kernel's stage
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int ko = ((kk * 4 + fg) ^ (fr & 7)) * 16;
        bf16x8 af[WM_FR], bfr[WN_FR];
#pragma unroll
        for (int mi = 0; mi < WM_FR; ++mi) af[mi] = *reinterpret_cast<const bf16x8*>(sa + (a_row0 + mi * 16) * ROWB + ko);
#pragma unroll
        for (int ni = 0; ni < WN_FR; ++ni) bfr[ni] = *reinterpret_cast<const bf16x8*>(sb + (b_row0 + ni * 16) * ROWB + ko);
#pragma unroll
        for (int mi = 0; mi < WM_FR; ++mi)
#pragma unroll
          for (int ni = 0; ni < WN_FR; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[ni], af[mi], acc[mi][ni], 0, 0, 0);
      }
    }
  }
  const bool scaled = g.K2 > 0;
#pragma unroll
  for (int mi = 0; mi < WM_FR; ++mi) {
    const int m = tm * BM + wm * (WM_FR * 16) + mi * 16 + fr;
    if (m >= g.M) continue;
    const float sam = (scaled ? 1.f : g.sa[m]) * g.alpha;
#pragma unroll
    for (int ni = 0; ni < WN_FR; ++ni) {
      const int n = tn * BN + wn * (WN_FR * 16) + ni * 16 + fg * 4;
      if (n >= g.N) continue;
      float4 s4 = scaled ? make_float4(1.f, 1.f, 1.f, 1.f) : *reinterpret_cast<const float4*>(g.sb + n);
      uint2 o = make_uint2(pack2bf(acc[mi][ni][0] * sam * s4.x, acc[mi][ni][1] * sam * s4.y), pack2bf(acc[mi][ni][2] * sam * s4.z, acc[mi][ni][3] * sam * s4.w));
      if (g.res) {
        const uint2 r = *reinterpret_cast<const uint2*>(g.res + (long)m * g.ldr + n);
        o.x = pack2bf(bflo(o.x) + bflo(r.x), bfhi(o.x) + bfhi(r.x));
        o.y = pack2bf(bflo(o.y) + bflo(r.y), bfhi(o.y) + bfhi(r.y));
      }
      *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(g.C) + (long)m * g.ldc + n) = o;
    }
  }
}

// ==== Host dispatch: an entry point validates its arguments, fills a GemmProblem, and gemm_plan() (gemm_plan.h: every shape rule, no device)
// lists the launches - rows, kernel, profile kind - that gemm_run() below executes in order =====================================================
using namespace gemm_plan_h;

// ---- knobs, device facts, workspace -------------------------------------------------------------------------------------------------------
// the one instance the lhrs_gemm_set_* entry points write; LHRS_GEMM_U4=0: the 16-wave kernels everywhere (kernel A/B tests)
static GemmKnobs g_knobs = [] { GemmKnobs k; const char* e = getenv("LHRS_GEMM_U4"); k.u4_on = (e == nullptr || e[0] != '0') ? 1 : 0; return k; }();
// Caller-owned device memory, registered per device (lhrs_gemm_set_workspace; 64 MiB + 4 KiB for 256 CUs).  One user: the tail rows of a
// row-split product with a long k-loop (GK_SPLITK_TAIL).  Launches that use it must be ordered on ONE stream per device.
static struct { float* slabs; long units; } g_sk[16];

static int num_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    n = hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess || prop.multiProcessorCount <= 0 ? 256 : prop.multiProcessorCount;
  }
  return n;
}
// a copy of g_knobs with the facts of the calling thread's device filled in (*dev_out: that device, -1 = none)
static GemmKnobs knobs(int* dev_out = nullptr) {
  GemmKnobs k = g_knobs;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = -1;
  k.cus = num_cus();
  k.ws_units = dev >= 0 && g_sk[dev].slabs != nullptr ? g_sk[dev].units : 0;
  if (dev_out) *dev_out = dev;
  return k;
}
extern "C" int lhrs_gemm_set_u4(int on) { g_knobs.u4_on = on ? 1 : 0; return 0; }
extern "C" int lhrs_gemm_set_policy(int allow_256) { g_knobs.allow_256 = allow_256 ? 2 : 0; return 0; }
extern "C" int lhrs_gemm_set_bm144(int mode) { g_knobs.bm144 = mode; return 0; }
extern "C" int lhrs_gemm_set_min_tiles(int n) { g_knobs.min256 = n; return 0; }
extern "C" int lhrs_gemm_set_small_thresh(int n) { g_knobs.small_thresh = n; return 0; }
extern "C" int lhrs_gemm_set_tail_split(int on) { g_knobs.tail_split = on; return 0; }
extern "C" int lhrs_gemm_set_persistent(int on) { g_knobs.persist = on; return 0; }
extern "C" long lhrs_gemm_workspace_bytes() { return 4096 + (long)num_cus() * 256 * 256 * 4; }
// ws == nullptr: forget the workspace of the current device
extern "C" int lhrs_gemm_set_workspace(void* ws, long bytes) {
  int dev = 0;
  LHRS_REQUIRE(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 16, "gemm_set_workspace: device %d", dev);
  if (ws == nullptr) { g_sk[dev].slabs = nullptr; g_sk[dev].units = 0; return 0; }
  LHRS_REQUIRE(bytes >= lhrs_gemm_workspace_bytes() && ((size_t)ws & 255) == 0, "gemm_set_workspace: %ld bytes (need %ld, 256-B aligned)", bytes,
               lhrs_gemm_workspace_bytes());
  g_sk[dev].slabs = (float*)((char*)ws + 4096); g_sk[dev].units = num_cus();
  return 0;
}
// ---- the exported rules: pure functions of their arguments and of the knobs ----------------------------------------------------------------
extern "C" int lhrs_gemm_u4_takes(int M, int N, int K, int lda, int ldb, int ldc, int ldr, int has_bias, int act, int out_f32, int accumulate, float alpha) {
  return u4_takes(knobs(), M, N, K, lda, ldb, ldc, ldr, has_bias, act, out_f32, accumulate, alpha);
}
extern "C" int lhrs_gemm_u4_fused_takes(int kind, int M, int tiles_n, int K, int K2) { return u4_fused_takes(knobs(), kind, M, tiles_n, K, K2); }
extern "C" int lhrs_gemm_u4_main_rows(int M, int N) { return u4_main_rows(knobs(), M, cdiv(N, 256)); }
// 1 when lhrs_gemm_swiglu_fwd / _bwd will take the fused kernel for this problem (dense operands), else 0 (they fall back)
extern "C" int lhrs_gemm_swiglu_fusable(int M, int ff, int K_fwd, int K_bwd, int K2) {
  const GemmKnobs k = knobs();
  return swiglu_fusable(k, (long)cdiv(M, 256) * (ff / 128), ff, K_fwd, K2, 8, 8) && swiglu_fusable(k, (long)cdiv(M, 256) * cdiv(ff, 256), ff, K_bwd, K2, 8, 8);
}
extern "C" int lhrs_gemm_splitk_splits(int M, int N, int K) { return splitk_f32_splits(M, N, K); }
extern "C" const char* lhrs_gemm_kernel_name(int kernel) { return kernel >= 0 && kernel < GK_COUNT ? gemm_kernel_info(kernel).name : nullptr; }

static GemmProblem problem(GemmEntry entry, const void* A, long lda, const void* B, long ldb, void* C, int ldc, int M, int N, int K, const void* A2 = nullptr,
                           int lda2 = 0, const void* B2 = nullptr, int ldb2 = 0, int K2 = 0) {
  GemmProblem p;
  p.entry = entry; p.A = A; p.lda = lda; p.B = B; p.ldb = ldb; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K;
  p.A2 = A2; p.lda2 = lda2; p.B2 = B2; p.ldb2 = ldb2; p.K2 = K2;
  return p;
}
// the plan of one call without running it (include/lhrs_hip.h); with cus > 0 no device is asked anything
extern "C" int lhrs_gemm_plan(int entry, int M, int N, int K, int K2, int flags, int act, float alpha, int lda, int ldb, int ldc, int ldr, int ff, int ld_gu,
                              int ld_act, int rope_cols, int head_dim, int ptr_align, int cus, int has_workspace, int* out, int cap) {
  LHRS_REQUIRE(entry >= GE_PLAIN && entry <= GE_SPLITK_F32 && M > 0 && K > 0 && (N > 0 || ff > 0) && out != nullptr, "gemm_plan: entry=%d M=%d N=%d K=%d", entry, M, N, K);
  GemmKnobs k = cus > 0 ? g_knobs : knobs();
  if (cus > 0) k.cus = cus;
  k.ws_units = has_workspace ? k.cus : 0;
  void* const ptr = (void*)(size_t)(0x10000 + ptr_align);   // never dereferenced: the rules read its alignment only
  const bool swiglu = entry == GE_SWIGLU_FWD || entry == GE_SWIGLU_BWD;
  GemmProblem p = problem((GemmEntry)entry, ptr, lda, ptr, ldb, ptr, swiglu ? ld_gu : ldc, M, entry == GE_SWIGLU_FWD ? 2 * ff : swiglu ? ff : N, K,
                          K2 > 0 ? ptr : nullptr, K2, K2 > 0 ? ptr : nullptr, K2, K2);
  p.act = act; p.alpha = alpha; p.ldr = ldr; p.bias = flags & 1 ? ptr : nullptr; p.residual = flags & 2 ? ptr : nullptr;
  p.out_f32 = (flags & 4) != 0 || entry == GE_SPLITK_F32; p.accumulate = (flags & 8) != 0; p.drop_thresh = flags & 16 ? 1 : 0;
  p.ff = ff; p.gu = p.act_out = p.scratch = ptr; p.ld_gu = ld_gu; p.ld_act = ld_act;
  p.rope_cos = p.rope_sin = (const float*)ptr; p.rope_mod = 4096; p.rope_cols = rope_cols; p.head_dim = head_dim;
  GemmSeg segs[GEMM_PLAN_CAP];
  const int n = gemm_plan(p, k, segs, GEMM_PLAN_CAP);
  LHRS_REQUIRE(n > 0 && n <= cap, "gemm_plan: %d segments, room for %d", n, cap);
  for (int i = 0; i < n; ++i) { out[4 * i] = segs[i].row0; out[4 * i + 1] = segs[i].row1; out[4 * i + 2] = segs[i].kernel; out[4 * i + 3] = segs[i].prof_kind; }
  return n;
}
// ---- the executor -------------------------------------------------------------------------------------------------------------------------
// the persistent kernels: at most one workgroup per CU, workgroup b takes tiles b, b + grid, ...; lhrs_gemm_set_persistent(0): one per tile
static dim3 grid_256s(const GemmArgs& g) {
  const long tiles = (long)g.tilesM * g.tilesN;
  return dim3((unsigned)(g_knobs.persist ? (tiles < num_cus() ? tiles : num_cus()) : tiles));
}
// a second operand pair (K2 > 0: the fused LoRA product) is a template parameter of the 256-row kernel
template <int ACT, int EPI>
static void launch_256s(GemmArgs& g, hipStream_t s) {
  if (g.K2 > 0) hipLaunchKernelGGL((gemm_nt_256s_kernel<ACT, EPI, true>), grid_256s(g), dim3(1024), 0, s, g);
  else hipLaunchKernelGGL((gemm_nt_256s_kernel<ACT, EPI, false>), grid_256s(g), dim3(1024), 0, s, g);
}
template <int ACT, int EPI>
static void launch_144s(GemmArgs& g, hipStream_t s) { hipLaunchKernelGGL((gemm_nt_144s_kernel<ACT, EPI>), grid_256s(g), dim3(768), 0, s, g); }
template <int WM, int WN, int ACT>
static void launch_tile(GemmArgs& g, hipStream_t s) { hipLaunchKernelGGL((gemm_nt_kernel<WM, WN, ACT>), dim3(g.tilesM * g.tilesN), dim3(256), 0, s, g); }
// f(std::integral_constant<int, act>): the activation is a template parameter of the plain-epilogue kernels
template <class F>
static void by_act(int act, F f) {
  switch (act) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, 3>{}); break;
  }
}
static int check_plain(const GemmProblem& q) {
  LHRS_REQUIRE(q.K % 64 == 0, "gemm: K=%d must be a multiple of 64 (zero-pad the reduction dim)", q.K);
  LHRS_REQUIRE(q.N % 4 == 0, "gemm: N=%d must be a multiple of 4", q.N);
  LHRS_REQUIRE(q.lda % 8 == 0 && q.ldb % 8 == 0, "gemm: lda=%d ldb=%d must be multiples of 8 (16-B rows)", (int)q.lda, (int)q.ldb);
  LHRS_REQUIRE(q.ldc % 4 == 0 && (q.residual == nullptr || q.ldr % 4 == 0), "gemm: ldc/ldr must be multiples of 4");
  LHRS_REQUIRE(q.lda >= q.K && q.ldb >= q.K && q.ldc >= q.N, "gemm: leading dims too small");
  LHRS_REQUIRE(!q.accumulate || q.out_f32, "gemm: accumulate needs f32 output");
  LHRS_REQUIRE(q.act >= 0 && q.act <= 3, "gemm: unknown activation %d", q.act);
  return 0;
}
// the kernel arguments of one segment: the problem's, with every row-indexed operand moved to row0 and the tile counts of the segment's kernel
static GemmArgs seg_args(const GemmProblem& q, const GemmSeg& sg) {
  GemmArgs g; memset(&g, 0, sizeof(g));
  const long r = sg.row0, esz = q.out_f32 ? 4 : 2, asz = q.entry == GE_FP8 || q.entry == GE_INT8 ? 1 : 2;
  auto at_row = [r](const void* ptr, long ld, long size) { return ptr ? (char*)ptr + r * ld * size : nullptr; };
  g.A = (const bf16_t*)at_row(q.A, q.lda, asz); g.B = (const bf16_t*)q.B; g.C = at_row(q.C, q.ldc, esz);
  g.bias = (const bf16_t*)q.bias; g.res = (const bf16_t*)at_row(q.residual, q.ldr, 2);
  g.M = sg.row1 - sg.row0; g.N = q.N; g.K = q.K; g.lda = (int)q.lda; g.ldb = (int)q.ldb; g.ldc = q.ldc; g.ldr = q.ldr;
  g.alpha = q.alpha; g.act = q.act; g.out_f32 = q.out_f32; g.accum = q.accumulate;
  g.A2 = (const bf16_t*)at_row(q.A2, q.lda2, 2); g.B2 = (const bf16_t*)q.B2; g.lda2 = q.lda2; g.ldb2 = q.ldb2; g.K2 = q.K2;
  g.sa = q.sa ? q.sa + r : nullptr; g.sb = q.sb; g.k2_dev = q.k2_dev;
  g.drop_scale = q.drop_scale; g.drop_seed = q.drop_seed; g.drop_thresh = q.drop_thresh;
  const GemmKernelInfo& ki = gemm_kernel_info(sg.kernel);
  g.tilesM = cdiv(g.M, ki.bm); g.tilesN = cdiv(g.N, ki.bn);
  switch (q.entry) {   // the fused epilogues of the 16-wave kernels
    case GE_SWIGLU_FWD: g.epi = 1; g.ff = q.ff; g.aux_out = (bf16_t*)at_row(q.act_out, q.ld_act, 2); g.ld_aux = q.ld_act; break;
    case GE_SWIGLU_BWD: g.epi = 2; g.ff = q.ff; g.aux = (const bf16_t*)at_row(q.gu, q.ld_gu, 2); g.ld_aux = q.ld_gu; break;
    case GE_ROPE: g.epi = 3; g.rope_cos = q.rope_cos; g.rope_sin = q.rope_sin; g.rope_mod = q.rope_mod; g.rope_pos0 = q.rope_pos0; g.rope_cols = q.rope_cols; break;
    default: break;
  }
  return g;
}
// split-K of the 128x128 kernel: `splits` k-slabs across blockIdx.y, each an f32 [rows, N] image in `slabs`, summed in a fixed order by one small
// launch - into bf16 C with alpha and the residual (the tail rows), or into f32 C (lhrs_gemm_bf16_nt_splitk_f32)
static void launch_splitk(const GemmProblem& q, const GemmSeg& sg, GemmArgs g, float* slabs, hipStream_t s) {
  void* const C = g.C; const bf16_t* const res = g.res;
  const int ks = cdiv(q.K / 64, sg.splits) * 64, used = cdiv(q.K, ks);
  g.C = slabs; g.ldc = q.N; g.res = nullptr; g.ldr = 0; g.alpha = 1.f; g.out_f32 = 1; g.accum = 0; g.ksplit = ks;
  const dim3 grid(g.tilesM * g.tilesN, used);
  if (sg.kernel == GK_T64X128) hipLaunchKernelGGL((gemm_nt_kernel<2, 4, 0>), grid, dim3(256), 0, s, g);       // the skinny-N product
  else if (sg.kernel == GK_T64X64) hipLaunchKernelGGL((gemm_nt_kernel<2, 2, 0>), grid, dim3(256), 0, s, g);
  else hipLaunchKernelGGL((gemm_nt_kernel<4, 4, 0>), grid, dim3(256), 0, s, g);
  const long work = (long)g.M * (q.N / 4);
  int rg = (int)((work + 255) / 256); if (rg > 8192) rg = 8192;
  if (!q.out_f32) hipLaunchKernelGGL(splitk_reduce_kernel, dim3(rg), dim3(256), 0, s, (const float*)slabs, (bf16_t*)C, (long)q.ldc, g.M, q.N, used, q.alpha, res, (long)q.ldr);
  else hipLaunchKernelGGL(splitk_reduce_f32_kernel, dim3(rg), dim3(256), 0, s, (const float*)slabs, (float*)C, (long)q.ldc, g.M, q.N, used);
}
// The four-wave kernels keep their own argument block (gemm_u4.hip); their wrappers cannot decline: the planner asked their predicates.
static int seg_launch(const GemmProblem& q, const GemmSeg& sg, int dev, hipStream_t s) {
  GemmArgs g = seg_args(q, sg);
  const dim3 tiles(g.tilesM * g.tilesN);
  int u4 = 0;
  switch (sg.kernel) {
    case GK_256: by_act(g.act, [&](auto a) { launch_256s<decltype(a)::value, 0>(g, s); }); break;
    case GK_144: by_act(g.act, [&](auto a) { launch_144s<decltype(a)::value, 0>(g, s); }); break;
    case GK_T128: by_act(g.act, [&](auto a) { launch_tile<4, 4, decltype(a)::value>(g, s); }); break;
    case GK_T64X128: by_act(g.act, [&](auto a) { launch_tile<2, 4, decltype(a)::value>(g, s); }); break;
    case GK_T64X64: by_act(g.act, [&](auto a) { launch_tile<2, 2, decltype(a)::value>(g, s); }); break;
    case GK_SWIGLU_FWD_256: launch_256s<0, 1>(g, s); break;
    case GK_SWIGLU_FWD_144: launch_144s<0, 1>(g, s); break;
    case GK_SWIGLU_BWD_256: launch_256s<0, 2>(g, s); break;
    case GK_SWIGLU_BWD_144: launch_144s<0, 2>(g, s); break;
    case GK_ROPE_256: launch_256s<0, 3>(g, s); break;
    case GK_ROPE_144: launch_144s<0, 3>(g, s); break;
    case GK_FP8_256: hipLaunchKernelGGL(gemm_fp8_256_kernel<false>, tiles, dim3(512), 0, s, g); break;
    case GK_I8_256: hipLaunchKernelGGL(gemm_fp8_256_kernel<true>, tiles, dim3(512), 0, s, g); break;
    case GK_FP8_SMALL: hipLaunchKernelGGL((gemm_fp8_small_kernel<2, 4>), tiles, dim3(256), 0, s, g); break;
    case GK_SPLITK_TAIL:
      LHRS_REQUIRE(dev >= 0 && g_sk[dev].slabs != nullptr, "gemm: the split-K tail rows need the registered workspace");
      launch_splitk(q, sg, g, g_sk[dev].slabs, s);
      break;
    case GK_SPLITK_F32: launch_splitk(q, sg, g, (float*)q.scratch, s); break;
    case GK_U4:
      u4 = lhrs_gemm_u4_nt_lora(g.A, g.lda, g.B, g.ldb, g.A2, g.lda2, g.B2, g.ldb2, g.K2, g.C, g.ldc, g.M, g.N, g.K, g.res, g.ldr, s);   // K2 = 0: no pair
      break;
    case GK_U4_SWIGLU_FWD: u4 = lhrs_gemm_u4_swiglu_fwd(g.A, g.lda, g.B, g.ldb, g.C, g.ldc, g.aux_out, (int)g.ld_aux, g.M, g.ff, g.K, s); break;
    case GK_U4_SWIGLU_BWD: u4 = lhrs_gemm_u4_swiglu_bwd(g.A, g.lda, g.B, g.ldb, g.aux, g.C, g.ldc, g.M, g.ff, g.K, s); break;
    case GK_U4_ROPE:
      u4 = lhrs_gemm_u4_rope_lora(g.A, g.lda, g.B, g.ldb, g.A2, g.lda2, g.B2, g.ldb2, g.K2, g.C, g.ldc, g.M, g.N, g.K, g.rope_cos, g.rope_sin, g.rope_mod,
                                  g.rope_pos0, g.rope_cols, s);
      break;
    default: LHRS_FAIL("gemm: no launch for kernel %d", sg.kernel);
  }
  LHRS_REQUIRE(u4 <= 0, "gemm: the four-wave kernel declined a planned launch (%s)", gemm_kernel_info(sg.kernel).name);
  return u4;
}
// The elementwise pass of an unfused fallback (elementwise.hip) on what the segments wrote.  Only SwiGLU forward is ever planned in row
// ranges; the passes of SwiGLU backward and RoPE always cover the whole result (the plain product in front of them may be row-split).
static int seg_pass(const GemmProblem& p, const GemmSeg& sg, hipStream_t s) {
  const long r0 = sg.pass_row0, rows = sg.row1 - r0;
  switch (p.entry) {
    case GE_SWIGLU_FWD:
      LHRS_REQUIRE(p.ld_gu == 2 * p.ff && p.ld_act == p.ff, "gemm_swiglu_fwd: the unfused fallback needs dense gu / act");
      return lhrs_swiglu_fwd((bf16_t*)p.C + r0 * p.ld_gu, (bf16_t*)p.act_out + r0 * p.ld_act, rows, p.ff, s);
    case GE_SWIGLU_BWD: return lhrs_swiglu_bwd(p.scratch, p.gu, p.C, p.M, p.ff, s);
    case GE_ROPE: return lhrs_rope(p.C, p.ldc, p.M, p.rope_cols / p.head_dim, p.head_dim, p.rope_cos, p.rope_sin, nullptr, p.rope_mod, p.rope_pos0, 0, s);
    default: LHRS_FAIL("gemm: no elementwise pass for entry %d", (int)p.entry);
  }
}
// Runs a plan.  Every segment is counted in the live profile; one with a prof_kind is bracketed by HIP events when its kind's sampling
// stride takes it (the fused-epilogue kinds count towards the GEMM FLOPs but are not "the dominant kernel" of lhrs_gemm_profile_read).
static int gemm_run(const GemmProblem& p, void* stream, const char* what) {
  LHRS_REQUIRE(p.M > 0 && p.N > 0 && p.K > 0, "gemm: empty problem M=%d N=%d K=%d", p.M, p.N, p.K);
  int dev = -1;
  const GemmKnobs k = knobs(&dev);
  GemmSeg segs[GEMM_PLAN_CAP];
  const int n = gemm_plan(p, k, segs, GEMM_PLAN_CAP);
  LHRS_REQUIRE(n > 0, "gemm: the plan outgrew GEMM_PLAN_CAP");
  hipStream_t s = (hipStream_t)stream;
  LHRS_REQUIRE(p.entry != GE_SWIGLU_BWD || segs[n - 1].pass_row0 < 0 || (p.scratch != nullptr && p.ld_gu == 2 * p.ff),
               "gemm_swiglu_bwd: the unfused fallback needs a [M, ff] scratch and dense gu");
  for (int i = 0; i < n; ++i) {
    const GemmSeg& sg = segs[i];
    const GemmProblem q = gemm_seg_problem(p, sg.kernel, sg.part);
    if (gemm_kernel_info(sg.kernel).plain && check_plain(q)) return -1;
    int slot = -1;
    if (g_prof.on) {
      // (the four-wave RoPE launch has always been counted without its LoRA pair)
      const double flops = 2.0 * (sg.row1 - sg.row0) * q.N * (q.K + (sg.kernel == GK_U4_ROPE ? 0 : q.K2));
      g_prof.launches_all++; g_prof.total_flops_all += flops;
      if (sg.prof_kind >= 0 && g_prof.used < g_prof.cap && g_prof.take(sg.prof_kind)) {
        slot = g_prof.used++;
        g_prof.flops[slot] = flops; g_prof.kind[slot] = sg.prof_kind;
        (void)hipEventRecord(g_prof.ev[2 * slot], s);
      }
    }
    if (seg_launch(q, sg, dev, s)) return -1;
    if (slot >= 0) (void)hipEventRecord(g_prof.ev[2 * slot + 1], s);
    LHRS_CHECK_LAUNCH(what);
    if (sg.pass_row0 >= 0 && seg_pass(p, sg, s)) return -1;
  }
  return 0;
}
// ---- C ABI ----------------------------------------------------------------------------------------------------------------------------------
extern "C" int lhrs_gemm_bf16_nt(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K, const void* bias, const void* residual,
                                 int ldr, int act, int out_f32, int accumulate, float alpha, void* stream) {
  GemmProblem p = problem(GE_PLAIN, A, lda, B, ldb, C, ldc, M, N, K);
  p.bias = bias; p.residual = residual; p.ldr = ldr; p.act = act; p.out_f32 = out_f32; p.accumulate = accumulate; p.alpha = alpha;
  return gemm_run(p, stream, "gemm_bf16_nt");
}

// ... + A2.B2^T: the rank-K2 LoRA update rides in the k-loop of the base GEMM (K2 / 64 more stages of either kernel family; bit-identical)
extern "C" int lhrs_gemm_bf16_nt_lora(const void* A, int lda, const void* B, int ldb, const void* A2, int lda2, const void* B2, int ldb2, int K2, void* C, int ldc,
                                      int M, int N, int K, const void* bias, const void* residual, int ldr, int out_f32, int accumulate, float alpha, void* stream) {
  LHRS_REQUIRE(A2 && B2 && K2 > 0 && K2 % 64 == 0 && lda2 % 8 == 0 && ldb2 % 8 == 0 && lda2 >= K2 && ldb2 >= K2,
               "gemm_lora: bad second operand pair (K2=%d lda2=%d ldb2=%d)", K2, lda2, ldb2);
  GemmProblem p = problem(GE_PLAIN, A, lda, B, ldb, C, ldc, M, N, K, A2, lda2, B2, ldb2, K2);
  p.bias = bias; p.residual = residual; p.ldr = ldr; p.out_f32 = out_f32; p.accumulate = accumulate; p.alpha = alpha;
  return gemm_run(p, stream, "gemm_bf16_nt");
}

// C = mask * (alpha * A.B^T) / (1 - p) + residual, mask = the counter-based LoRA dropout mask over the [M, N] result (see common.h)
extern "C" int lhrs_gemm_bf16_nt_dropmask(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K, const void* residual, int ldr,
                                          float alpha, float p_drop, unsigned seed, void* stream) {
  LHRS_REQUIRE(p_drop > 0.f && p_drop < 1.f, "gemm_dropmask: p=%f", p_drop);
  GemmProblem p = problem(GE_PLAIN, A, lda, B, ldb, C, ldc, M, N, K);
  p.residual = residual; p.ldr = ldr; p.alpha = alpha;
  p.drop_scale = 1.f / (1.f - p_drop); p.drop_seed = seed; p.drop_thresh = (unsigned)((double)p_drop * 4294967296.0);
  return gemm_run(p, stream, "gemm_bf16_nt");
}

// LLaMA MLP with the SwiGLU / SwiGLU' fused into the GEMM epilogue (include/lhrs_hip.h): one launch, bit-identical to GEMM + lhrs_swiglu_fwd /
// _bwd, which is also the fallback for shapes the fused kernels do not take (swiglu_fusable)
extern "C" int lhrs_gemm_swiglu_fwd(const void* X, int ldx, const void* Wgu, int ldw, const void* A2, int lda2, const void* B2, int ldb2, int K2, void* gu, int ld_gu,
                                    void* act, int ld_act, int M, int ff, int K, void* stream) {
  LHRS_REQUIRE(M > 0 && ff > 0 && K > 0 && ff % 8 == 0 && ld_gu >= 2 * ff && ld_act >= ff && ld_gu % 8 == 0 && ld_act % 8 == 0,
               "gemm_swiglu_fwd: M=%d ff=%d K=%d ld_gu=%d ld_act=%d", M, ff, K, ld_gu, ld_act);
  GemmProblem p = problem(GE_SWIGLU_FWD, X, ldx, Wgu, ldw, gu, ld_gu, M, 2 * ff, K, A2, lda2, B2, ldb2, K2);
  p.ff = ff; p.ld_gu = ld_gu; p.act_out = act; p.ld_act = ld_act;
  return gemm_run(p, stream, "gemm_swiglu_fwd");
}

extern "C" int lhrs_gemm_swiglu_bwd(const void* dY, int ldy, const void* WdT, int ldw, const void* A2, int lda2, const void* B2, int ldb2, int K2, const void* gu,
                                    void* dgu, int ld_gu, void* dact_scratch, int M, int ff, int K, void* stream) {
  LHRS_REQUIRE(M > 0 && ff > 0 && K > 0 && ff % 8 == 0 && ld_gu >= 2 * ff && ld_gu % 8 == 0, "gemm_swiglu_bwd: M=%d ff=%d K=%d ld_gu=%d", M, ff, K, ld_gu);
  GemmProblem p = problem(GE_SWIGLU_BWD, dY, ldy, WdT, ldw, dgu, ld_gu, M, ff, K, A2, lda2, B2, ldb2, K2);
  p.ff = ff; p.gu = gu; p.ld_gu = ld_gu; p.scratch = dact_scratch;
  return gemm_run(p, stream, "gemm_swiglu_bwd");
}

// qkv projection with the RoPE of its q / k heads in the GEMM epilogue; bit-identical to lhrs_gemm_bf16_nt(_lora) + lhrs_rope, which is also
// the fallback when the fused kernels do not apply (rope_fusable)
extern "C" int lhrs_gemm_rope_fwd(const void* X, int ldx, const void* W, int ldw, const void* A2, int lda2, const void* B2, int ldb2, int K2, void* C, int ldc, int M,
                                  int N, int K, const float* cos_t, const float* sin_t, int pos_mod, int pos0, int rope_cols, int head_dim, void* stream) {
  LHRS_REQUIRE(M > 0 && N > 0 && K > 0 && head_dim % 16 == 0 && rope_cols >= 0 && rope_cols <= N && rope_cols % head_dim == 0 && pos_mod > 0 &&
                   cos_t && sin_t && ldc % 8 == 0,
               "gemm_rope_fwd: M=%d N=%d K=%d rope_cols=%d head_dim=%d pos_mod=%d", M, N, K, rope_cols, head_dim, pos_mod);
  GemmProblem p = problem(GE_ROPE, X, ldx, W, ldw, C, ldc, M, N, K, A2, lda2, B2, ldb2, K2);
  p.rope_cos = cos_t; p.rope_sin = sin_t; p.rope_mod = pos_mod; p.rope_pos0 = pos0; p.rope_cols = rope_cols; p.head_dim = head_dim;
  return gemm_run(p, stream, "gemm_rope_fwd");
}

// C[M, N] (bf16) = alpha * sa[m] * sb[n] * (A8[M, K] . B8[N, K]^T) (+ residual): e4m3 operands with per-row fp32 scales
// (lhrs_quant_fp8_rows).  K % 128 == 0, N % 8 == 0; lda / ldb in BYTES (>= K, multiples of 16).  The tile rows that spill over the last full
// round of the CUs go to the small-tile sibling (the tail-row rule); int8 has no such sibling and takes no split.
static int gemm_8bit(GemmEntry entry, const void* A8, long lda, const float* sa, const void* B8, long ldb, const float* sb, const void* A2, int lda2, const void* B2,
                     int ldb2, int K2, const int* k2_dev, void* C, int ldc, int M, int N, int K, const void* residual, int ldr, float alpha, void* stream) {
  LHRS_REQUIRE(M > 0 && N > 0 && K >= 256 && K % 128 == 0, "gemm_fp8: M=%d N=%d K=%d (K %% 128 == 0, K >= 256)", M, N, K);
  LHRS_REQUIRE(lda % 16 == 0 && ldb % 16 == 0 && lda >= K && ldb >= K && sa && sb, "gemm_fp8: lda=%ld ldb=%ld", lda, ldb);
  LHRS_REQUIRE(N % 8 == 0 && ldc % 8 == 0 && ldc >= N && (residual == nullptr || ldr % 8 == 0), "gemm_fp8: N=%d ldc=%d ldr=%d", N, ldc, ldr);
  LHRS_REQUIRE((K2 == 0 && !k2_dev) || (A2 && B2 && K2 % 64 == 0 && lda2 % 8 == 0 && ldb2 % 8 == 0 && lda2 >= K2 && ldb2 >= K2),
               "gemm_fp8: bad bf16 pair (K2=%d lda2=%d ldb2=%d)", K2, lda2, ldb2);
  GemmProblem p = problem(entry, A8, lda, B8, ldb, C, ldc, M, N, K, A2, lda2, B2, ldb2, K2);
  p.k2_dev = k2_dev;   // (int8: the pair may have device-known columns only)
  p.residual = residual; p.ldr = ldr; p.alpha = alpha; p.sa = sa; p.sb = sb;
  return gemm_run(p, stream, "gemm_fp8_nt");
}
extern "C" int lhrs_gemm_fp8_nt(const void* A8, long lda, const float* sa, const void* B8, long ldb, const float* sb, void* C, int ldc, int M, int N, int K,
                                const void* residual, int ldr, float alpha, void* stream) {
  return gemm_8bit(GE_FP8, A8, lda, sa, B8, ldb, sb, nullptr, 0, nullptr, 0, 0, nullptr, C, ldc, M, N, K, residual, ldr, alpha, stream);
}
// ... + alpha * A2[M, K2] . B2[N, K2]^T in bf16 on the same accumulators (the LoRA update of an 8-bit base linear), K2 % 64 == 0
extern "C" int lhrs_gemm_fp8_nt_lora(const void* A8, long lda, const float* sa, const void* B8, long ldb, const float* sb, const void* A2, int lda2, const void* B2,
                                     int ldb2, int K2, void* C, int ldc, int M, int N, int K, const void* residual, int ldr, float alpha, void* stream) {
  LHRS_REQUIRE(K2 > 0, "gemm_fp8_lora: K2=%d", K2);
  return gemm_8bit(GE_FP8, A8, lda, sa, B8, ldb, sb, A2, lda2, B2, ldb2, K2, nullptr, C, ldc, M, N, K, residual, ldr, alpha, stream);
}
// LLM.int8 product: int8 operands, int32 accumulation; the bf16 pair holds K2 host-known columns and k2_dev[0] device-known outlier columns
extern "C" int lhrs_gemm_int8_nt(const void* A8, long lda, const float* sa, const void* B8, long ldb, const float* sb, const void* A2, int lda2, const void* B2,
                                 int ldb2, int K2, const int* k2_dev, void* C, int ldc, int M, int N, int K, const void* residual, int ldr, float alpha, void* stream) {
  return gemm_8bit(GE_INT8, A8, lda, sa, B8, ldb, sb, A2, lda2, B2, ldb2, K2, k2_dev, C, ldc, M, N, K, residual, ldr, alpha, stream);
}

// long-K, few-tile product with f32 output (the projector's weight gradients): split-K through f32 slabs of `workspace`; 1 split: a plain launch
extern "C" int lhrs_gemm_bf16_nt_splitk_f32(const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int K, float* workspace, void* stream) {
  LHRS_REQUIRE(M > 0 && N > 0 && K > 0 && K % 64 == 0 && N % 4 == 0 && ldc % 4 == 0 && ldc >= N && lda % 8 == 0 && ldb % 8 == 0 && lda >= K && ldb >= K,
               "gemm_splitk_f32: M=%d N=%d K=%d lda=%d ldb=%d ldc=%d", M, N, K, lda, ldb, ldc);
  const int splits = splitk_f32_splits(M, N, K);
  LHRS_REQUIRE(splits == 1 || workspace != nullptr, "gemm_splitk_f32: %d splits need a workspace of splits * M * N floats", splits);
  GemmProblem p = problem(GE_SPLITK_F32, A, lda, B, ldb, C, ldc, M, N, K);
  p.out_f32 = 1; p.scratch = workspace;
  return gemm_run(p, stream, "gemm_splitk_f32");
}

// Skinny-N product (N <= 384: the LoRA down-projections): HBM-bound on A, latency-bound as one 64-row block per tile walking all of K, so K is
// split lhrs_gemm_skinny_splits(K, N) ways into f32 slabs of the workspace, then summed.  No rule beyond its split count: no plan.
extern "C" int lhrs_gemm_skinny_splits(int K, int N) {
  int s = K / 512;
  const int cap = N <= 128 ? 16 : 4;  // wide adapters: the f32 slabs (splits * M * N * 4 B) soon cost more than the latency they hide
  return s < 1 ? 1 : (s > cap ? cap : s);
}
extern "C" int lhrs_gemm_bf16_nt_skinny(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K, float alpha,
                                        float* workspace, void* stream) {
  LHRS_REQUIRE(M > 0 && N > 0 && N <= 384 && N % 64 == 0 && K % 64 == 0 && workspace != nullptr, "gemm_skinny: M=%d N=%d K=%d", M, N, K);
  LHRS_REQUIRE(lda % 8 == 0 && ldb % 8 == 0 && lda >= K && ldb >= K && ldc >= N && ldc % 4 == 0, "gemm_skinny: lda=%d ldb=%d ldc=%d", lda, ldb, ldc);
  GemmProblem p = problem(GE_PLAIN, A, lda, B, ldb, C, ldc, M, N, K);
  p.alpha = alpha;
  // 64x128 tiles when N allows: the rows of A are read once per 128 columns, not per 64 (M = 8190: 5-11 % faster)
  const GemmSeg sg{0, M, N % 128 == 0 ? GK_T64X128 : GK_T64X64, -1, lhrs_gemm_skinny_splits(K, N), GP_WHOLE, -1};
  if (g_prof.on) { g_prof.launches_all++; g_prof.total_flops_all += 2.0 * M * N * K; }
  launch_splitk(p, sg, seg_args(p, sg), workspace, (hipStream_t)stream);
  LHRS_CHECK_LAUNCH("gemm_skinny");
  return 0;
}
