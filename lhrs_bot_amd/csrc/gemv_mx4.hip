// OCP MXFP4 decode weights for gfx950: e2m1 codes with one e8m0 scale per 32 consecutive k, multiplied by the block-scaled MFMA
// itself (v_mfma_scale_f32_16x16x128_f8f6f4, A = FP4 with its block scales, B = the e4m3 activations of the fp8 decode mode with unit
// scales).  A lane's 32 weights are 16 B of codes + 1 scale byte and cost no VALU work: ~0.53 B per weight element per token.
//   quant_mx4_rows   : bf16 [N, K] -> codes uint8 [N, K/2] (element k in byte k/2, even k in the low nibble) + scales uint8 [N, K/32]
//                      (OCP MX v1.0: byte = clamp(floor(log2 max|v|) - 2 + 127, 0, 254), elements RNE-to-even-code, saturating at 6)
//   dequant_mx4_rows : the inverse, exact in bf16 (level * 2^(byte - 127))
//   repack_mx4_mfma  : row-major codes / scales -> the operand order gemv_mx4_kernel streams
//   gemv_mx4_kernel  : y[b][n] = xscale[b] * sum_k x8[b][k] * w[n][k] (+ residual), 1..16 sequences
#include "decode_linear.h"

namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8_t;

// ---- storage format ----------------------------------------------------------------------------------------------
// one thread per block of 32: 64 B of bf16 in, 16 B of codes + 1 scale byte out
__global__ __launch_bounds__(256) void quant_mx4_rows_kernel(const bf16_t* __restrict__ W, long ldw, uint8_t* __restrict__ codes, long ldc,
                                                             uint8_t* __restrict__ scales, long lds, int N, int K) {
  const int nb = K / 32;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)N * nb) return;
  const long n = t / nb;
  const int blk = (int)(t % nb);
  const bf16_t* src = W + n * ldw + (long)blk * 32;
  float v[32];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float f[8];
    unpack8(*reinterpret_cast<const uint4*>(src + i * 8), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[i * 8 + e] = f[e];
  }
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < 32; ++i) m = fmaxf(m, fabsf(v[i]));
  int byte = 127;
  if (m > 0.f) {
    const uint32_t mb = __float_as_uint(m);
    const int ex = (int)(mb >> 23);                                         // bf16 subnormals are fp32 subnormals: exponent field 0
    const int lg = ex ? ex - 127 : (31 - __clz((int)mb)) - 149;              // floor(log2 m)
    byte = min(max(lg - 2 + 127, 0), 254);
  }
  uint32_t out[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t word = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float x = v[i * 8 + e];
      const float a = ldexpf(fabsf(x), 127 - byte);                         // exact: a power-of-two scaling of a bf16 value
      // nearest of {0, .5, 1, 1.5, 2, 3, 4, 6}; a tie goes to the even code (>= at the midpoints below an even index)
      const uint32_t idx = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.f);
      const uint32_t sign = m > 0.f ? (__float_as_uint(x) >> 31) << 3 : 0u;  // a zero block is all +0
      word |= (sign | idx) << (4 * e);
    }
    out[i] = word;
  }
  *reinterpret_cast<uint4*>(codes + n * ldc + (long)blk * 16) = make_uint4(out[0], out[1], out[2], out[3]);
  scales[n * lds + blk] = (uint8_t)byte;
}

__device__ __forceinline__ float e2m1_level(uint32_t c) {
  const uint32_t i = c & 7u;
  const float mag = i < 4 ? 0.5f * (float)i : (i == 4 ? 2.f : (i == 5 ? 3.f : (i == 6 ? 4.f : 6.f)));
  return (c & 8u) ? -mag : mag;
}

__global__ __launch_bounds__(256) void dequant_mx4_rows_kernel(const uint8_t* __restrict__ codes, long ldc, const uint8_t* __restrict__ scales,
                                                               long lds, bf16_t* __restrict__ W, long ldw, int N, int K) {
  const int nb = K / 32;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)N * nb) return;
  const long n = t / nb;
  const int blk = (int)(t % nb);
  const uint4 c = *reinterpret_cast<const uint4*>(codes + n * ldc + (long)blk * 16);
  const int ex = (int)scales[n * lds + blk] - 127;
  const uint32_t w[4] = {c.x, c.y, c.z, c.w};
  bf16_t* dst = W + n * ldw + (long)blk * 32;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = ldexpf(e2m1_level(w[i] >> (4 * e)), ex);
    *reinterpret_cast<uint4*>(dst + i * 8) = pack8(f);
  }
}

// codes_t  [ceil(N/16)][K/128][64 lanes][16 B]: lane (r = lane & 15, g = lane >> 4) of step s holds block 4 s + g of row 16 rg + r
// scales_t [ceil(N/16)][ceil(K/512)][64 lanes][4 B]: byte j of the lane's dword t is the scale of that lane's block in step 4 t + j
// rows past N: zero codes, byte 127; steps past K/128: byte 127
__global__ __launch_bounds__(256) void repack_mx4_mfma_kernel(const uint8_t* __restrict__ codes, long ldc, const uint8_t* __restrict__ scales,
                                                              long lds, uint8_t* __restrict__ codes_t, uint32_t* __restrict__ scales_t, int N,
                                                              int K) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  const int nsteps = K / 128, nd = (nsteps + 3) / 4;
  const long ngroups = (N + 15) / 16;
  if (p < ngroups * nsteps * 64) {
    const int lane = (int)(p & 63);
    const long t = p >> 6;
    const int step = (int)(t % nsteps);
    const long row = (t / nsteps) * 16 + (lane & 15);
    i32x4 v = {0, 0, 0, 0};
    if (row < N) v = *reinterpret_cast<const i32x4*>(codes + row * ldc + ((long)step * 4 + (lane >> 4)) * 16);
    *reinterpret_cast<i32x4*>(codes_t + p * 16) = v;
  }
  if (p < ngroups * nd * 64) {
    const int lane = (int)(p & 63);
    const long t = p >> 6;
    const int dw = (int)(t % nd);
    const long row = (t / nd) * 16 + (lane & 15);
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int step = dw * 4 + j;
      uint32_t b = 127;
      if (row < N && step < nsteps) b = scales[row * lds + step * 4 + (lane >> 4)];
      v |= b << (8 * j);
    }
    scales_t[p] = v;
  }
}

// ---- the GEMV ----------------------------------------------------------------------------------------------------
// 16 output rows per block; the eight waves split the 128-k steps in runs that start on a multiple of 4 (the scale byte of a step is
// picked by an immediate), four steps - 4 KiB of codes and one scale dword per wave - in flight, issued before the prologue.  Lane (r, g)
// of a step holds the 32 CONSECUTIVE k of block 4 step + g of row r: one 16-B load in the low four registers of the FP4 A operand
// (cbsz 4; the instruction's k = 32 g + element), its e8m0 scale in scale_a.  The 8-register e4m3 B operand (blgp 0, unit scale) is laid out
// differently by the hardware - registers 0-3 of lane (c, g) are k = 16 g .. +16 and registers 4-7 are k = 64 + 16 g .. +16 of the step, found
// with one-hot operands through lhrs_gemv_mx4 and pinned by tests/test_mx4_gpu.py - so a lane reads bytes [16 g, +16) and [64 + 16 g, +16) of
// its activation row, as gemv_fp8_mfma_kernel does (there on both operands, where any common order would do).
// The partial tiles of the waves are folded by mfma_tile_store of decode_linear.h.
// PRO < 0: x8 / xscale come from global memory (any batch <= 16).  PRO 0 / 1 / 2 (batch <= 2): bf16 x; copy / RMSNorm (HF roundings) /
// SwiGLU over [B, 2K] and the per-row e4m3 quantisation run in the block, in the steps of stage_x_e4m3 of decode_linear.h (what the fused
// e4m3 GEMV of decode.hip runs; this kernel has its block of QX_WAVES waves) and from the same pieces.
template <int PRO>
__global__ __launch_bounds__(QX_THREADS) void gemv_mx4_kernel(const uint8_t* __restrict__ Wc, const uint32_t* __restrict__ Ws,
                                                              const void* __restrict__ xin, long ldx, const float* __restrict__ xscale,
                                                              const bf16_t* __restrict__ norm_w, float eps, const bf16_t* res, long ldr, void* y,
                                                              long ldy, int NB, int N, int K, int out_f32) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // PRO >= 0: [NB][K] e4m3 bytes
  __shared__ float part[QX_WAVES][16][17];
  __shared__ float red[QX_WAVES];
  __shared__ float s_scale[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
  const int row0 = blockIdx.x * 16;
  const int nsteps = K / 128, nd = (nsteps + 3) / 4;
  const int per = ((nsteps + QX_WAVES - 1) / QX_WAVES + 3) / 4 * 4;  // K 11008: 86 steps = 7 x 12 + 2
  const int s_begin = min(wave * per, nsteps), s_end = min(nsteps, s_begin + per);
  const uint8_t* wp = Wc + (long)blockIdx.x * nsteps * 1024 + lane * 16;
  const uint32_t* sp = Ws + (long)blockIdx.x * nd * 64 + lane;
  constexpr int U = 4;  // 128-k steps in flight per wave = one scale dword
  i32x4 wq[U];
#pragma unroll
  for (int u = 0; u < U; ++u)  // first weight lines before the prologue
    wq[u] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp + (long)min(s_begin + u, max(s_end - 1, 0)) * 1024));
  int wsc = (int)__builtin_nontemporal_load(sp + (long)min(s_begin / 4, nd - 1) * 64);
  const uint8_t* xp;
  if (PRO >= 0) {
    uint8_t* x8s = reinterpret_cast<uint8_t*>(smem);
    // stage_x_e4m3 of decode_linear.h, step for step, on this kernel's own text: inlined from the header, the same arithmetic is allocated
    // 2 VGPRs more (PRO 0) / fewer (PRO 1) and 2 SGPRs more (PRO 2) here, and this kernel's register table is kept as it was
    const bf16_t* x = reinterpret_cast<const bf16_t*>(xin);
    const int nch = K / 8;
    for (int b = 0; b < NB; ++b) {
      float v[QX_MAXC][8], g[QX_MAXC][8];
      float q = 0.f;
#pragma unroll
      for (int i = 0; i < QX_MAXC; ++i) {
        const int c = tid + i * QX_THREADS;
        if (c < nch) {
          uint4 t = *reinterpret_cast<const uint4*>(x + b * ldx + c * 8);
          if (PRO == 2) t = swiglu8(t, *reinterpret_cast<const uint4*>(x + b * ldx + K + c * 8));
          unpack8(t, v[i]);
          if (PRO == 1) {
            unpack8(*reinterpret_cast<const uint4*>(norm_w + c * 8), g[i]);
            q = sumsq8_serial(q, v[i]);
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[i][e] = 0.f;
        }
      }
      if (PRO == 1) {
        const float rstd = rsqrtf(block_sum<QX_WAVES>(q, red) / (float)K + eps);
#pragma unroll
        for (int i = 0; i < QX_MAXC; ++i)
          if (tid + i * QX_THREADS < nch) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[i][e] = rms_hf(v[i][e], g[i][e], rstd);
          }
      }
      float m = 0.f;
#pragma unroll
      for (int i = 0; i < QX_MAXC; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf(v[i][e]));
      m = block_max<QX_WAVES>(m, red);
      const float sc = m > 0.f ? m / 448.f : 1.f;
      if (tid == 0) s_scale[b] = sc;
      const float inv = 1.f / sc;
#pragma unroll
      for (int i = 0; i < QX_MAXC; ++i) {
        const int c = tid + i * QX_THREADS;
        if (c < nch) *reinterpret_cast<int2*>(x8s + (size_t)b * K + c * 8) = cvt8_e4m3(v[i], inv);
      }
    }
    __syncthreads();
    xp = x8s + (size_t)min(fr, NB - 1) * K + fg * 16;
  } else {
    xp = reinterpret_cast<const uint8_t*>(xin) + (long)min(fr, NB - 1) * ldx + fg * 16;
  }
  const bool live = fr < NB;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s0 = s_begin; s0 < s_end; s0 += U) {  // s0 % 4 == 0: step s0 + u reads byte u of the scale dword
    const bool more = s0 + U < s_end;            // wave-uniform
    i32x4 wn[U], xlo[U], xhi[U];
    int wscn = 0;
    if (more) {
#pragma unroll
      for (int u = 0; u < U; ++u) wn[u] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp + (long)min(s0 + U + u, s_end - 1) * 1024));
      wscn = (int)__builtin_nontemporal_load(sp + (long)(s0 / 4 + 1) * 64);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long o = (long)min(s0 + u, s_end - 1) * 128;
      xlo[u] = *reinterpret_cast<const i32x4*>(xp + o);
      xhi[u] = *reinterpret_cast<const i32x4*>(xp + o + 64);
    }
#define MX4_STEP(u)                                                                                                         \
  if (s0 + u < s_end) {                                                                                                     \
    const i32x8_t a = {wq[u][0], wq[u][1], wq[u][2], wq[u][3], 0, 0, 0, 0};                                                 \
    i32x8_t b = {xlo[u][0], xlo[u][1], xlo[u][2], xlo[u][3], xhi[u][0], xhi[u][1], xhi[u][2], xhi[u][3]};                   \
    if (!live) b = i32x8_t{0, 0, 0, 0, 0, 0, 0, 0};                                                                         \
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, 4, 0, u, wsc, 0, 0x7F7F7F7F);                         \
  }
    MX4_STEP(0) MX4_STEP(1) MX4_STEP(2) MX4_STEP(3)
#undef MX4_STEP
    if (more) {
#pragma unroll
      for (int u = 0; u < U; ++u) wq[u] = wn[u];
      wsc = wscn;
    }
  }
  mfma_tile_store<QX_WAVES, 1>(part, acc, wave, fr, fg, row0, NB, N, nullptr, PRO >= 0 ? s_scale : xscale, res, ldr, y, ldy, out_f32);
}

}  // namespace

// bf16 W [N, ldw] -> codes [N, ldc] (K/2 bytes per row) + scales [N, lds] (K/32 bytes per row); K % 32 == 0
extern "C" int lhrs_quant_mx4_rows(const void* W, long ldw, void* codes, long ldc, void* scales, long lds, int N, int K, void* stream) {
  LHRS_REQUIRE(N > 0 && K >= 32 && K % 32 == 0, "quant_mx4_rows: N=%d K=%d (K %% 32 == 0)", N, K);
  LHRS_REQUIRE(W && codes && scales && al16(W) && al16(codes) && ldw % 8 == 0 && ldc % 16 == 0 && ldw >= K && ldc >= K / 2 && lds >= K / 32,
               "quant_mx4_rows: pointers / strides (ldw=%ld ldc=%ld lds=%ld)", ldw, ldc, lds);
  const long nthreads = (long)N * (K / 32);
  hipLaunchKernelGGL(quant_mx4_rows_kernel, dim3(cdiv(nthreads, 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)W, ldw, (uint8_t*)codes,
                     ldc, (uint8_t*)scales, lds, N, K);
  LHRS_CHECK_LAUNCH("quant_mx4_rows");
  return 0;
}

extern "C" int lhrs_dequant_mx4_rows(const void* codes, long ldc, const void* scales, long lds, void* W, long ldw, int N, int K, void* stream) {
  LHRS_REQUIRE(N > 0 && K >= 32 && K % 32 == 0, "dequant_mx4_rows: N=%d K=%d (K %% 32 == 0)", N, K);
  LHRS_REQUIRE(W && codes && scales && al16(W) && al16(codes) && ldw % 8 == 0 && ldc % 16 == 0 && ldw >= K && ldc >= K / 2 && lds >= K / 32,
               "dequant_mx4_rows: pointers / strides (ldw=%ld ldc=%ld lds=%ld)", ldw, ldc, lds);
  const long nthreads = (long)N * (K / 32);
  hipLaunchKernelGGL(dequant_mx4_rows_kernel, dim3(cdiv(nthreads, 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)codes, ldc,
                     (const uint8_t*)scales, lds, (bf16_t*)W, ldw, N, K);
  LHRS_CHECK_LAUNCH("dequant_mx4_rows");
  return 0;
}

// codes_t: ceil(N/16) * K/128 * 1024 bytes; scales_t: ceil(N/16) * ceil(K/512) * 256 bytes (see repack_mx4_mfma_kernel)
extern "C" int lhrs_repack_mx4_mfma(const void* codes, long ldc, const void* scales, long lds, void* codes_t, void* scales_t, int N, int K,
                                    void* stream) {
  LHRS_REQUIRE(N > 0 && K >= 128 && K % 128 == 0, "repack_mx4_mfma: N=%d K=%d (K %% 128 == 0)", N, K);
  LHRS_REQUIRE(codes && scales && codes_t && scales_t && al16(codes) && al16(codes_t) && al16(scales_t) && ldc % 16 == 0 && ldc >= K / 2 &&
                   lds >= K / 32, "repack_mx4_mfma: pointers / strides (ldc=%ld lds=%ld)", ldc, lds);
  const long nthreads = (long)cdiv(N, 16) * (K / 128) * 64;  // >= the scale dwords
  hipLaunchKernelGGL(repack_mx4_mfma_kernel, dim3(cdiv(nthreads, 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)codes, ldc,
                     (const uint8_t*)scales, lds, (uint8_t*)codes_t, (uint32_t*)scales_t, N, K);
  LHRS_CHECK_LAUNCH("repack_mx4_mfma");
  return 0;
}

// y[B, N] = xscale[b] * (x8[B, K] . w[N, K]^T) (+ residual[B, N]); w = the MXFP4 weight behind codes_t / scales_t; 1 <= B <= 16
extern "C" int lhrs_gemv_mx4(const void* codes_t, const void* scales_t, const void* x8, long ldx, const float* xscale, const void* residual,
                             long ldr, void* y, long ldy, int B, int N, int K, int out_f32, void* stream) {
  LHRS_REQUIRE(B >= 1 && B <= 16 && N > 0 && K >= 128 && K % 128 == 0, "gemv_mx4: B=%d (1..16) N=%d K=%d (K %% 128 == 0)", B, N, K);
  LHRS_REQUIRE(codes_t && scales_t && x8 && xscale && y && al16(codes_t) && al16(scales_t) && al16(x8) && ldx % 16 == 0 && ldx >= K,
               "gemv_mx4: pointers / strides (ldx=%ld)", ldx);
  hipLaunchKernelGGL((gemv_mx4_kernel<-1>), dim3(cdiv(N, 16)), dim3(QX_THREADS), 0, (hipStream_t)stream, (const uint8_t*)codes_t,
                     (const uint32_t*)scales_t, x8, ldx, xscale, (const bf16_t*)nullptr, 0.f, (const bf16_t*)residual, ldr, y, ldy, B, N, K,
                     out_f32);
  LHRS_CHECK_LAUNCH("gemv_mx4");
  return 0;
}

// the same with bf16 activations: prologue (0 none, 1 RMSNorm(norm_w, eps), 2 SwiGLU with x = [B, 2K]) + per-row e4m3 quantisation of x
// inside the kernel; B <= 2 (five launches per layer for a batch-1 token)
extern "C" int lhrs_gemv_mx4_fused(const void* codes_t, const void* scales_t, const void* x, long ldx, int prologue, const void* norm_w,
                                   float eps, const void* residual, long ldr, void* y, long ldy, int B, int N, int K, int out_f32,
                                   void* stream) {
  LHRS_REQUIRE(B >= 1 && B <= 2 && N > 0 && K >= 128 && K % 128 == 0, "gemv_mx4_fused: B=%d (1..2) N=%d K=%d (K %% 128 == 0)", B, N, K);
  LHRS_REQUIRE(codes_t && scales_t && x && y && al16(codes_t) && al16(scales_t) && al16(x) && ldx % 8 == 0 && prologue >= 0 && prologue <= 2 &&
                   (prologue != 1 || (norm_w && al16(norm_w))) && ldx >= (prologue == 2 ? 2L * K : (long)K),
               "gemv_mx4_fused: args (ldx=%ld prologue=%d)", ldx, prologue);
  LHRS_REQUIRE(K <= QX_MAX_K, "gemv_mx4_fused: K=%d exceeds the %d values the prologue keeps in registers", K, QX_MAX_K);
  const size_t sm = (size_t)B * K;
  const dim3 grid(cdiv(N, 16)), blk(QX_THREADS);
#define GOX(P)                                                                                                                      \
  hipLaunchKernelGGL((gemv_mx4_kernel<P>), grid, blk, sm, (hipStream_t)stream, (const uint8_t*)codes_t, (const uint32_t*)scales_t, x, ldx, \
                     (const float*)nullptr, (const bf16_t*)norm_w, eps, (const bf16_t*)residual, ldr, y, ldy, B, N, K, out_f32)
  if (prologue == 0) GOX(0); else if (prologue == 1) GOX(1); else GOX(2);
#undef GOX
  LHRS_CHECK_LAUNCH("gemv_mx4_fused");
  return 0;
}
