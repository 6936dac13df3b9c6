// Decode from the 4-bit base: the single-token weight stream reads the bitsandbytes codes and block statistics that quantize_base(4) keeps
// beside every decoder linear (quant4.hip) instead of the bf16 weight dequantised from them - 0.5 B of codes + 1/16 B of fp32 absmax per
// weight element instead of 2 B.
//
// bitsandbytes' Linear4bit computes every product on bf16(table[code] * absmax) (quant4.hip header).  Both kernels here form EXACTLY that
// value in registers - one fp32 multiply, one round-to-nearest-even to bf16, the bits dequant4_blocks_kernel stores - and then run the
// arithmetic of the bf16 GEMVs of decode.hip: the result is the bf16 GEMV's up to the order of the fp32 sums.  The absmax is NOT factored
// out of the block sum (absmax * sum level * x would skip the rounding of the weight and compute something Linear4bit does not).
//
//   layout        codes [N][ldc bytes]: byte j of a row holds elements 2j (HIGH nibble) and 2j + 1 (low nibble); absmax [N][lda floats],
//                 one per 64 consecutive k.  K % 64 == 0, so a block never straddles a row.  A 16-B lane load is 32 codes = half a block.
//   gemv4_kernel       batch 1, and batches 2..8 where K % 128 != 0: one wave per RPW rows, fp32 FMAs, the structure of gemv_kernel.
//   gemv4_mfma_kernel  batch 2..16, K % 128 == 0: v_mfma_f32_16x16x32_bf16 with the batch as N, the structure of gemv_mfma_kernel; the A
//                      fragments are dequantised in registers.
//   Both take the activation prologue (stage_x) and the write-out (store_y, mfma_tile_store) of the bf16 GEMVs from decode_linear.h.
//   level lookup  a 16-entry fp32 table in LDS: 16 words on 16 banks and equal addresses broadcast, so the divergent lookup is conflict-free
//                 (a divergently indexed __constant__ array would serialise).
// Cost per weight element: ~5.5 VALU instructions in the VALU kernel (shift and mask for the table offset, multiply, half a packed convert,
// unpack, FMA) and ~3.5 in the MFMA kernel, plus one LDS lookup in both.  Both reach 1.1-1.55 TB/s of codes (measured per launch: DESIGN.md
// "Decode from the 4-bit base"): not HBM-bound; which part of the dequantisation limits them has not been separated by counters.
#include "decode_linear.h"

namespace {

// the level tables of quant4.hip (NF4_LEVEL, FP4_LEVEL), repeated: [0] nf4, [1] fp4.  tests/test_gemv4_gpu.py compares single products
// with lhrs_dequant4_blocks bit for bit, so the two copies cannot drift apart unnoticed.
__constant__ float LEVEL4[2][16] = {
    {-1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f, -0.28444138169288635f, -0.18477343022823334f,
     -0.09105003625154495f, 0.0f, 0.07958029955625534f, 0.16093020141124725f, 0.24611230194568634f, 0.33791524171829224f,
     0.44070982933044434f, 0.5626170039176941f, 0.7229568362236023f, 1.0f},
    {0.0f, 5.208333333e-03f, 0.66666667f, 1.0f, 0.33333333f, 0.5f, 0.16666667f, 0.25f,
     -0.0f, -5.208333333e-03f, -0.66666667f, -1.0f, -0.33333333f, -0.5f, -0.16666667f, -0.25f}};

// four code bytes (memory order) -> the eight bf16 weights as four packed pairs: element 2t from the high nibble of byte t, 2t + 1 from the low
__device__ __forceinline__ void dequant8(uint32_t v, float a, const float* tab, uint32_t (&p)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) p[t] = pack2bf(tab[(v >> (8 * t + 4)) & 15u] * a, tab[(v >> (8 * t)) & 15u] * a);
}

// ------------------------------------------------------------------------------------------------------------------
// gemv4_kernel: 4 waves x RPW rows per block.  Lane l of a row's wave takes the 16-B chunks (32 codes, one absmax) l, l + 64, ... of the
// row in order; a chunk adds four times the sum of 8 products (one expression, left to right) to the lane's fp32 accumulator; then the
// wave butterfly.  RPW * UNR chunk loads (codes + absmax) per lane are prefetched one iteration ahead; the first ones are issued before
// the prologue, clamped to the row's last chunk.  The per-row summation order does not depend on RPW / UNR.
// ------------------------------------------------------------------------------------------------------------------
template <int NB, int PRO, int RPW, int UNR>
__global__ __launch_bounds__(256) void gemv4_kernel(const uint8_t* __restrict__ codes, long ldc, const float* __restrict__ absmax, long lda, int fp4,
                                                    const bf16_t* __restrict__ x, long ldx, const bf16_t* __restrict__ norm_w, float eps,
                                                    const bf16_t* res, long ldr, void* y, long ldy, int N, int K, int out_f32) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float red[4];
  __shared__ float tab[16];
  bf16_t* xs = reinterpret_cast<bf16_t*>(smem);  // [NB][K]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nch = K / 32;
  const int row0 = (blockIdx.x * 4 + wave) * RPW;
  i32x4 wcur[UNR][RPW];
  float acur[UNR][RPW];
#pragma unroll
  for (int u = 0; u < UNR; ++u) {
    const int c = min(lane + 64 * u, nch - 1);
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const long row = min(row0 + r, N - 1);  // guards the address only: rows past N are never stored
      wcur[u][r] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(codes + row * ldc + c * 16));
      acur[u][r] = absmax[row * lda + (c >> 1)];
    }
  }
  if (tid < 16) tab[tid] = LEVEL4[fp4][tid];
  stage_x<PRO, 256>(x, ldx, norm_w, eps, xs, red, NB, K);
  __syncthreads();
  float acc[RPW][NB];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[r][b] = 0.f;
  for (int c = lane; c < nch; c += 64 * UNR) {
    i32x4 wnext[UNR][RPW];
    float anext[UNR][RPW];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int cn = min(c + 64 * (UNR + u), nch - 1);
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        const long row = min(row0 + r, N - 1);
        wnext[u][r] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(codes + row * ldc + cn * 16));
        anext[u][r] = absmax[row * lda + (cn >> 1)];
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int cc = c + 64 * u;
      if (cc < nch) {
        uint4 xv[4];
        if (NB == 1) {
#pragma unroll
          for (int j = 0; j < 4; ++j) xv[j] = *reinterpret_cast<const uint4*>(xs + cc * 32 + j * 8);
        }
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
          uint32_t w[4][4];
#pragma unroll
          for (int j = 0; j < 4; ++j) dequant8((uint32_t)wcur[u][r][j], acur[u][r], tab, w[j]);
#pragma unroll
          for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const uint4 v = NB == 1 ? xv[j] : *reinterpret_cast<const uint4*>(xs + b * K + cc * 32 + j * 8);
              acc[r][b] += bflo(w[j][0]) * bflo(v.x) + bfhi(w[j][0]) * bfhi(v.x) + bflo(w[j][1]) * bflo(v.y) + bfhi(w[j][1]) * bfhi(v.y) +
                           bflo(w[j][2]) * bflo(v.z) + bfhi(w[j][2]) * bfhi(v.z) + bflo(w[j][3]) * bflo(v.w) + bfhi(w[j][3]) * bfhi(v.w);
            }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        wcur[u][r] = wnext[u][r];
        acur[u][r] = anext[u][r];
      }
  }
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const float s = wave_sum(acc[r][b]);
      const int row = row0 + r;
      if (lane == 0 && row < N) store_y(y, out_f32, b, ldy, row, s, res, ldr);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// gemv4_mfma_kernel: 16 output rows per block, the batch is the N dimension of v_mfma_f32_16x16x32_bf16.  K is walked in steps of 128:
// lane (r, g) loads the 16 B that hold k = 128 s + 32 g .. + 32 of row r (plus that half block's absmax) and dequantises them into FOUR A
// fragments - MFMA m of the step takes elements 8 m .. 8 m + 8 of every lane, i.e. the k set {128 s + 32 g + 8 m + j}.  That is a
// permutation of k inside the step, applied to both operands alike: the B fragment of MFMA m is x[b][128 s + 32 g + 8 m .. + 8] (what
// gemv_fp8_mfma_kernel does with its two halves).  The 8 waves take ceil(steps / 8) consecutive steps each (the last ones fewer or
// none); two steps per wave are in flight; the partial 16x16 tiles are summed through LDS in wave order.
// PRO 0 reads x straight from L2 (nothing staged, no LDS limit on the batch); batch columns >= NB read zeros.
// ------------------------------------------------------------------------------------------------------------------
template <int PRO>
__global__ __launch_bounds__(512) void gemv4_mfma_kernel(const uint8_t* __restrict__ codes, long ldc, const float* __restrict__ absmax, long lda,
                                                         int fp4, const bf16_t* __restrict__ x, long ldx, const bf16_t* __restrict__ norm_w,
                                                         float eps, const bf16_t* res, long ldr, void* y, long ldy, int NB, int N, int K,
                                                         int out_f32) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float red[8];
  __shared__ float part[8][16][17];
  __shared__ float tab[16];
  bf16_t* xs = reinterpret_cast<bf16_t*>(smem);  // [NB][K]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
  const int row0 = blockIdx.x * 16;
  const int ns = K / 128, per = (ns + 7) / 8;
  const int sb = min(wave * per, ns), nst = min(sb + per, ns) - sb;  // this wave's steps [sb, sb + nst); nst may be 0
  const long wrow = min(row0 + fr, N - 1);                           // guards the address only
  const uint8_t* wp = codes + wrow * ldc + fg * 16;                  // + 64 s
  const float* ap = absmax + wrow * lda + (fg >> 1);                 // + 2 s
  constexpr int U = 2;
  i32x4 wreg[U];
  float areg[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {  // before the prologue, clamped into the wave's own steps (an idle wave re-reads the row's last step)
    const int s = min(sb + min(u, max(nst - 1, 0)), ns - 1);
    wreg[u] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp + (long)s * 64));
    areg[u] = ap[s * 2];
  }
  if (tid < 16) tab[tid] = LEVEL4[fp4][tid];
  if (PRO != 0) stage_x<PRO, 512>(x, ldx, norm_w, eps, xs, red, NB, K);
  __syncthreads();
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const bf16_t* xq = (PRO == 0 ? x + (long)min(fr, NB - 1) * ldx : xs + (long)min(fr, NB - 1) * K) + fg * 32;
  const bool live = fr < NB;
  for (int s0 = 0; s0 < nst; s0 += U) {
    i32x4 wnext[U];
    float anext[U];
    bf16x8 xfrag[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int sn = sb + min(s0 + U + u, nst - 1);
      wnext[u] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp + (long)sn * 64));
      anext[u] = ap[sn * 2];
      const int sx = sb + min(s0 + u, nst - 1);
#pragma unroll
      for (int m = 0; m < 4; ++m) xfrag[u][m] = *reinterpret_cast<const bf16x8*>(xq + (long)sx * 128 + m * 8);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (s0 + u < nst) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          uint32_t p[4];
          dequant8((uint32_t)wreg[u][m], areg[u], tab, p);
          const i32x4 afrag = {(int)p[0], (int)p[1], (int)p[2], (int)p[3]};
          bf16x8 bfrag = xfrag[u][m];
          if (!live) bfrag = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, afrag), bfrag, acc, 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      wreg[u] = wnext[u];
      areg[u] = anext[u];
    }
  }
  mfma_tile_store<8, 0>(part, acc, wave, fr, fg, row0, NB, N, nullptr, nullptr, res, ldr, y, ldy, out_f32);
}

constexpr long MFMA_STATIC_LDS = (8 + 8 * 16 * 17 + 16) * 4;  // red + part + tab of gemv4_mfma_kernel
constexpr long VALU_STATIC_LDS = (4 + 16) * 4;                // red + tab of gemv4_kernel

template <int PRO>
int gemv4_valu(const uint8_t* codes, long ldc, const float* absmax, long lda, int fp4, const bf16_t* x, long ldx, const bf16_t* norm_w, float eps,
               const bf16_t* residual, long ldr, void* y, long ldy, int B, int N, int K, int out_f32, hipStream_t s) {
  const size_t sm = (size_t)B * K * 2;
#define GEMV4_LAUNCH(NB, RPW, UNR)                                                                                                  \
  do {                                                                                                                              \
    if (sm > 65536) (void)hipFuncSetAttribute((const void*)gemv4_kernel<NB, PRO, RPW, UNR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm); \
    hipLaunchKernelGGL((gemv4_kernel<NB, PRO, RPW, UNR>), dim3(cdiv(N, 4 * RPW)), dim3(256), sm, s, codes, ldc, absmax, lda, fp4, x, ldx, norm_w, \
                       eps, residual, ldr, y, ldy, N, K, out_f32);                                                                  \
  } while (0)
  // batch 1: a row is a quarter of the bf16 row's bytes, so the loads in flight come from rows, not from chunks of one row: two rows x two
  // chunks per lane-iteration for the 4096-row projections (512 blocks), four rows x two chunks for the tall ones
  switch (B) {
    case 1: if (N <= 4096) GEMV4_LAUNCH(1, 2, 2); else GEMV4_LAUNCH(1, 4, 2); break;
    case 2: GEMV4_LAUNCH(2, 4, 1); break;
    case 3: GEMV4_LAUNCH(3, 4, 1); break;
    case 4: GEMV4_LAUNCH(4, 4, 1); break;
    case 5: GEMV4_LAUNCH(5, 4, 1); break;
    case 6: GEMV4_LAUNCH(6, 4, 1); break;
    case 7: GEMV4_LAUNCH(7, 4, 1); break;
    default: GEMV4_LAUNCH(8, 4, 1); break;
  }
#undef GEMV4_LAUNCH
  LHRS_CHECK_LAUNCH("gemv4");
  return 0;
}

template <int PRO>
int gemv4_mfma(const uint8_t* codes, long ldc, const float* absmax, long lda, int fp4, const bf16_t* x, long ldx, const bf16_t* norm_w, float eps,
               const bf16_t* residual, long ldr, void* y, long ldy, int B, int N, int K, int out_f32, hipStream_t s) {
  const size_t sm = PRO == 0 ? 0 : (size_t)B * K * 2;
  if (sm > 65536) (void)hipFuncSetAttribute((const void*)gemv4_mfma_kernel<PRO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm);
  hipLaunchKernelGGL((gemv4_mfma_kernel<PRO>), dim3(cdiv(N, 16)), dim3(512), sm, s, codes, ldc, absmax, lda, fp4, x, ldx, norm_w, eps, residual, ldr,
                     y, ldy, B, N, K, out_f32);
  LHRS_CHECK_LAUNCH("gemv4_mfma");
  return 0;
}

}  // namespace

// y[B, N] = pro(x)[B, K] . w[N, K]^T (+ residual[B, N]) with w[n, k] = bf16(LEVEL[code[n, k]] * absmax[n][k / 64]); see include/lhrs_hip.h
extern "C" int lhrs_gemv4(const void* codes, long ldc, const float* absmax, long lda, int fp4, const void* x, long ldx, int prologue,
                          const void* norm_w, float eps, const void* residual, long ldr, void* y, long ldy, int B, int N, int K, int out_f32,
                          void* stream) {
  LHRS_REQUIRE(B >= 1 && B <= 16 && N > 0 && K >= 64 && K % 64 == 0, "gemv4: B=%d (1..16) N=%d K=%d (blocks of 64 must not straddle a row)", B, N, K);
  LHRS_REQUIRE(B <= 8 || K % 128 == 0, "gemv4: batches above 8 need K %% 128 == 0 (B=%d K=%d)", B, K);
  LHRS_REQUIRE(codes != nullptr && absmax != nullptr && x != nullptr && y != nullptr, "gemv4: null codes / absmax / x / y");
  LHRS_REQUIRE(ldc % 16 == 0 && ldc >= K / 2 && (uintptr_t)codes % 16 == 0 && lda >= K / 64 && ldx % 8 == 0 && (uintptr_t)x % 16 == 0,
               "gemv4: strides / alignment (16-B lane loads): ldc=%ld lda=%ld ldx=%ld", ldc, lda, ldx);
  LHRS_REQUIRE(prologue >= 0 && prologue <= 2 && (prologue != 1 || norm_w != nullptr), "gemv4: prologue %d", prologue);
  // batches past the LDS are split as lhrs_gemv splits them; a chunk of one row goes to the VALU kernel
  const bool mfma = B >= 2 && K % 128 == 0;
  int bmax = staged_rows_max(K, mfma ? MFMA_STATIC_LDS : VALU_STATIC_LDS);
  if (mfma && prologue == 0) bmax = 16;  // the MFMA kernel reads x from L2
  LHRS_REQUIRE(bmax >= 1, "gemv4: one activation vector does not fit LDS (K=%d)", K);
  const long esz = out_f32 ? 4 : 2;
  hipStream_t s = (hipStream_t)stream;
  for (int b0 = 0; b0 < B; b0 += bmax) {
    const int nb = B - b0 < bmax ? B - b0 : bmax;
    const bf16_t* xb = (const bf16_t*)x + b0 * ldx;
    const bf16_t* rb = residual ? (const bf16_t*)residual + b0 * ldr : nullptr;
    void* yb = (char*)y + b0 * ldy * esz;
    int rc;
#define GO(F, P) rc = F<P>((const uint8_t*)codes, ldc, absmax, lda, fp4 ? 1 : 0, xb, ldx, (const bf16_t*)norm_w, eps, rb, ldr, yb, ldy, nb, N, K, out_f32, s)
    if (nb >= 2 && K % 128 == 0) { if (prologue == 0) GO(gemv4_mfma, 0); else if (prologue == 1) GO(gemv4_mfma, 1); else GO(gemv4_mfma, 2); }
    else { if (prologue == 0) GO(gemv4_valu, 0); else if (prologue == 1) GO(gemv4_valu, 1); else GO(gemv4_valu, 2); }
#undef GO
    if (rc) return -1;
  }
  return 0;
}
