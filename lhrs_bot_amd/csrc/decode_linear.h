// The activation side and the write-out that every single-token linear shares, whatever its weight format: decode.hip (bf16, e4m3),
// gemv4.hip (NF4 / FP4), gemv_mx4.hip (MXFP4), gemv_int8.hip (LLM.int8) and lora_decode.hip (live adapters).  The formats must agree in
// rounding and in summation order (the adapter sees the activation the base product sees; fused == stand-alone quantisation bit for bit),
// so each of these steps is written once, here.  The main loops - weight prefetch, dequantisation, MFMA steps - stay with their kernels.
#pragma once
#include "common.h"

// ---- activation prologues ------------------------------------------------------------------------------------------
// PRO: 0 plain copy    1 RMSNorm (HF LlamaRMSNorm: bf16(w * bf16(x * rsqrt(mean x^2 + eps))))    2 SwiGLU: bf16(silu(x[k]) * x[K + k]), x = [B, 2K]

// eight gate | up pairs -> eight bf16 of silu(g) * u
__device__ __forceinline__ uint4 swiglu8(const uint4& g, const uint4& u) {
  uint4 o;
  o.x = pack2bf(silu(bflo(g.x)) * bflo(u.x), silu(bfhi(g.x)) * bfhi(u.x));
  o.y = pack2bf(silu(bflo(g.y)) * bflo(u.y), silu(bfhi(g.y)) * bfhi(u.y));
  o.z = pack2bf(silu(bflo(g.z)) * bflo(u.z), silu(bfhi(g.z)) * bfhi(u.z));
  o.w = pack2bf(silu(bflo(g.w)) * bflo(u.w), silu(bfhi(g.w)) * bfhi(u.w));
  return o;
}

// the HF LlamaRMSNorm roundings of one element: xhat is rounded to bf16 before the weight, the product again
__device__ __forceinline__ float rms_hf(float v, float g, float rstd) { return bf2f(f2bf(g * bf2f(f2bf(v * rstd)))); }

// The sum of squares of a row comes in TWO forms that round differently; both are pinned by tests (and restated by the emulators of
// tests/gemv_cases.py), so they stay apart:
//   sumsq8_chunk  one eight-term expression per 16-B chunk, left to right, added to the thread's sum as a whole:
//                 the LDS stagers (stage_x: gemv_kernel, gemv_mfma_kernel, gemv4_kernel, gemv4_mfma_kernel) and lora_down_kernel
//   sumsq8_serial element by element into the thread's sum: the register-resident prologues (stage_x_e4m3: gemv_fp8_mfma_kernel,
//                 gemv_mx4_kernel; int8_decode_prepare_kernel), which equal the stand-alone rmsnorm_fwd_q bit for bit
__device__ __forceinline__ float sumsq8_chunk(const uint4& v) {
  return bflo(v.x) * bflo(v.x) + bfhi(v.x) * bfhi(v.x) + bflo(v.y) * bflo(v.y) + bfhi(v.y) * bfhi(v.y) + bflo(v.z) * bflo(v.z) +
         bfhi(v.z) * bfhi(v.z) + bflo(v.w) * bflo(v.w) + bfhi(v.w) * bfhi(v.w);
}
__device__ __forceinline__ float sumsq8_serial(float q, const float (&v)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) q += v[e] * v[e];
  return q;
}

// rows 0 .. NB-1 of x -> xs [NB][K] bf16 in LDS, by a block of T threads (every block redoes it: 8-22 KB from L2); red: T / 64 floats.
// The caller syncs before it reads xs.
template <int PRO, int T>
__device__ __forceinline__ void stage_x(const bf16_t* __restrict__ x, long ldx, const bf16_t* __restrict__ norm_w, float eps, bf16_t* xs, float* red,
                                        int NB, int K) {
  const int tid = threadIdx.x, nx = K / 8;
  for (int b = 0; b < NB; ++b) {
    if (PRO == 2) {
      for (int c = tid; c < nx; c += T) {
        const uint4 g = *reinterpret_cast<const uint4*>(x + b * ldx + c * 8);
        const uint4 u = *reinterpret_cast<const uint4*>(x + b * ldx + K + c * 8);
        *reinterpret_cast<uint4*>(xs + b * K + c * 8) = swiglu8(g, u);
      }
    } else {
      float q = 0.f;
      for (int c = tid; c < nx; c += T) {
        const uint4 v = *reinterpret_cast<const uint4*>(x + b * ldx + c * 8);
        *reinterpret_cast<uint4*>(xs + b * K + c * 8) = v;
        if (PRO == 1) q += sumsq8_chunk(v);
      }
      if (PRO == 1) {
        const float rstd = rsqrtf(block_sum<T / 64>(q, red) / (float)K + eps);
        __syncthreads();
        for (int c = tid; c < K; c += T) xs[b * K + c] = f2bf(bf2f(norm_w[c]) * bf2f(f2bf(bf2f(xs[b * K + c]) * rstd)));
      }
    }
  }
}

// The same prologue followed by the per-row e4m3 quantisation (scale = max|v| / 448, as lhrs_quant_fp8_rows) for the kernels that multiply
// e4m3 activations: rows 0 .. NB-1 of x -> x8s [NB][K] e4m3 bytes in LDS and s_scale[NB].  The row stays in registers between the
// reductions - QX_MAXC chunks of 8 per thread of a QX_THREADS block, hence K <= QX_MAX_K (the host checks it) - and only the bytes go to
// LDS.  red: QX_WAVES floats.  The caller syncs before it reads x8s / s_scale.
constexpr int QX_WAVES = 8, QX_THREADS = QX_WAVES * 64, QX_MAXC = 3, QX_MAX_K = QX_THREADS * QX_MAXC * 8;  // 12288
template <int PRO>
__device__ __forceinline__ void stage_x_e4m3(const bf16_t* x, long ldx, const bf16_t* norm_w, float eps, uint8_t* x8s, float* red, float* s_scale,
                                             int NB, int K) {
  const int tid = threadIdx.x, nch = K / 8;
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
}

// host: the most rows of K bf16 activations one launch stages (larger batches are split): at most 152 KiB, and with the static LDS of
// the kernel the chunk goes to no more than the 160 KiB of a CU
static inline int staged_rows_max(int K, long static_lds) {
  const long lds_x = 152L * 1024 < 160L * 1024 - static_lds ? 152L * 1024 : 160L * 1024 - static_lds;
  return (int)(lds_x / ((long)K * 2));
}

// ---- write-out -----------------------------------------------------------------------------------------------------
// y[b][row] = v (+ residual), bf16 or fp32
__device__ __forceinline__ void store_y(void* y, int out_f32, int b, long ldy, int row, float v, const bf16_t* res, long ldr) {
  if (res) v += bf2f(res[b * ldr + row]);
  if (out_f32) reinterpret_cast<float*>(y)[b * ldy + row] = v;
  else reinterpret_cast<bf16_t*>(y)[b * ldy + row] = f2bf(v);
}

// The epilogue of the 16-row MFMA kernels whose NW waves split K: acc[r] of lane (fr = lane & 15, fg = lane >> 4) of wave `wave` is that
// wave's partial y[batch = fr][row0 + 4 fg + r].  The caller passes the three indices it addressed its operands with: recomputed here from
// the thread id, the same values take another form and the register allocation of the kernels moves.  The partial tiles go through
// part[NW][16][17]; the first 256 threads (16 rows x 16 batch columns) fold them in wave order - no atomics, bit-reproducible -, apply
// the scales of the quantised formats and store.
// SCALES 0: v (bf16, 4-bit; the pointers are not read)   1: v * xscale[b] (MXFP4)   2: v * (wscale[row] * xscale[b]) (e4m3)
template <int NW, int SCALES>
__device__ __forceinline__ void mfma_tile_store(float (&part)[NW][16][17], f32x4 acc, int wave, int fr, int fg, int row0, int NB, int N,
                                                const float* wscale, const float* xscale, const bf16_t* res, long ldr, void* y, long ldy,
                                                int out_f32) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int r = 0; r < 4; ++r) part[wave][fg * 4 + r][fr] = acc[r];
  __syncthreads();
  const int i = tid >> 4, b = tid & 15;
  const int row = row0 + i;
  if (tid < 256 && b < NB && row < N) {
    const float xs_b = SCALES ? xscale[b] : 1.f;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) v += part[w][i][b];
    if (SCALES == 2) v *= wscale[row] * xs_b;
    if (SCALES == 1) v *= xs_b;
    store_y(y, out_f32, b, ldy, row, v, res, ldr);
  }
}
