// Decode with live LoRA adapters on gfx950: the adapter half of a decoder linear at S_q = 1, next to the weight-streaming GEMVs of decode.hip /
// gemv4.hip (which stay untouched and know nothing about adapters).
//
// peft lora.Linear.forward (reached from the reference's lhrs/models/text_modal.py:133-151):
//     y = W x + s * B (A x),  s = lora_alpha / r
// on ONE fp32 accumulator per output, the arithmetic the training forward runs (gemm_nt_skinny(alpha = s) stores T = bf16(s x A^T), then
// lhrs_gemm_bf16_nt_lora adds T B^T to the base product before the single rounding).  A decode step does the same in three launches:
//     lora_down : tpart[i][b][j] = sum over K-slice i of pro(x)[b, k] A[j, k]                       (fp32, one slice per workgroup row)
//     (GEMV)    : acc[b][n]      = pro(x)[b, :] . W[n, :]                                           (any weight format, out_f32, no residual)
//     lora_up   : y[b][n]        = bf16(acc[b][n] + sum_{j in cols(n)} t[b][j] Bw[n][j] + residual) with t = bf16(s * sum_i tpart[i])
// No atomics, no tickets: every output has one writer and a fixed summation order, so a replayed graph and eager launches agree bit for bit.
//
// lora_down streams 0.5-3 MB of stacked A rows: 8 rows per workgroup would put a [24, 4096] A on 3 CUs, so K is cut into up to 16 slices of
// whole 64-element chunks (grid = R / 8 x slices) and the slice sums meet in lora_up, in ascending slice order.  The activation prologues are
// those of gemv_kernel, built from the same pieces of decode_linear.h (RMSNorm: bf16(w * bf16(x * rstd)) with rstd from the whole row, which
// every workgroup forms itself from L2; SwiGLU: bf16(silu(g) * u)), so the adapter sees the activation the base product sees.
// lora_up reads of Bfull [N, ldb] only the one non-zero block of each block-diagonal row: columns [(n / fout) r, +r).
#include "decode_linear.h"

namespace {

constexpr int DOWN_ROWS = 8;     // rows of A per workgroup: 4 waves x 2
constexpr int MAX_R = 768, MAX_SLICES = 16, MAX_B = 16;
constexpr size_t DOWN_STATIC_LDS = 16, MAX_LDS = 160 * 1024;  // red[4] of lora_down_kernel; LDS of a CU

__device__ __forceinline__ float dot8(const float (&w)[8], const float (&x)[8]) {
  return w[0] * x[0] + w[1] * x[1] + w[2] * x[2] + w[3] * x[3] + w[4] * x[4] + w[5] * x[5] + w[6] * x[6] + w[7] * x[7];
}

// NB: compile-time bound of the batch loop (accumulators stay in registers); rows b >= B are skipped
template <int NB>
__global__ __launch_bounds__(256) void lora_down_kernel(const bf16_t* __restrict__ x, long ldx, int pro, const bf16_t* __restrict__ norm_w, float eps,
                                                        const bf16_t* __restrict__ A, long lda, float* __restrict__ tpart, int B, int R, int K,
                                                        int ks) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float red[4];
  bf16_t* xs = reinterpret_cast<bf16_t*>(smem);  // [B][ks]: this slice of the activations after the prologue
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k0 = blockIdx.y * ks;
  const int kl = max(0, min(ks, K - k0));        // elements of this slice (a multiple of 64; 0: an empty trailing slice still writes its zeros)
  const int nch = kl / 8;
  const int row0 = blockIdx.x * DOWN_ROWS + wave * 2;
  float rstd[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    rstd[b] = 1.f;
    if (pro == 1 && b < B) {  // the whole row, as the GEMV blocks do: thread t takes the 16-B chunks t, t + 256, ...
      float q = 0.f;
      for (int c = tid; c < K / 8; c += 256) q += sumsq8_chunk(*reinterpret_cast<const uint4*>(x + b * ldx + c * 8));
      rstd[b] = rsqrtf(block_sum<4>(q, red) / (float)K + eps);
    }
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    if (b < B) {
      for (int c = tid; c < nch; c += 256) {
        const bf16_t* xp = x + b * ldx + k0 + c * 8;
        uint4 o = *reinterpret_cast<const uint4*>(xp);
        if (pro == 2) {
          o = swiglu8(o, *reinterpret_cast<const uint4*>(xp + K));
        } else if (pro == 1) {
          float v[8], w[8];
          unpack8(o, v);
          unpack8(*reinterpret_cast<const uint4*>(norm_w + k0 + c * 8), w);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = w[e] * bf2f(f2bf(v[e] * rstd[b]));
          o = pack8(v);  // rms_hf: its last rounding is the one pack8 does (through the helper the compiler converts twice)
        }
        *reinterpret_cast<uint4*>(xs + b * ks + c * 8) = o;
      }
    }
  }
  __syncthreads();
  float acc[2][NB];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[r][b] = 0.f;
  const bf16_t* a0 = A + (long)row0 * lda + k0;
  for (int c = lane; c < nch; c += 64) {  // lane l takes the chunks l, l + 64, ... of the slice, in order
    float w0[8], w1[8];
    unpack8(*reinterpret_cast<const uint4*>(a0 + c * 8), w0);
    unpack8(*reinterpret_cast<const uint4*>(a0 + lda + c * 8), w1);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (b < B) {
        float xv[8];
        unpack8(*reinterpret_cast<const uint4*>(xs + b * ks + c * 8), xv);
        acc[0][b] += dot8(w0, xv);
        acc[1][b] += dot8(w1, xv);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (b < B) {
        const float s = wave_sum(acc[r][b]);
        if (lane == 0) tpart[((long)blockIdx.y * B + b) * R + row0 + r] = s;
      }
    }
}

// lpr lanes share an output row (a power of two, >= r / 8 chunks up to a whole wave): lane g of the group takes the 16-B chunks g, g + lpr, ...
// of the row's block and the group folds with the xor butterfly below lpr.  A workgroup takes `rows` consecutive output rows, 256 / lpr per pass,
// and first forms the bf16 t of the columns those rows touch.
template <int NB>
__global__ __launch_bounds__(256) void lora_up_kernel(const float* __restrict__ acc, long ldacc, const float* __restrict__ tpart, int nsl, float s,
                                                      const bf16_t* __restrict__ Bw, long ldb, int r, int fout, const bf16_t* __restrict__ res,
                                                      long ldr, bf16_t* __restrict__ y, long ldy, int B, int N, int R, int lpr, int rows) {
  __shared__ __attribute__((aligned(16))) bf16_t ts[MAX_B * MAX_R];  // [B][ncols]
  const int tid = threadIdx.x;
  const int n0 = blockIdx.x * rows, n1 = min(N, n0 + rows);
  const int p0 = n0 / fout, p1 = (n1 - 1) / fout;
  const int c0 = p0 * r, ncols = (p1 - p0 + 1) * r;  // <= R: the host checked (N / fout) r <= R
  for (int idx = tid; idx < B * ncols; idx += 256) {
    const int b = idx / ncols, j = idx - b * ncols;
    float sum = 0.f;
    for (int i = 0; i < nsl; ++i) sum += tpart[((long)i * B + b) * R + c0 + j];  // ascending slice order
    ts[idx] = f2bf(s * sum);                                                     // the T that gemm_nt_skinny(alpha = s) stores
  }
  __syncthreads();
  const int g = tid / lpr, gl = tid & (lpr - 1), rpp = 256 / lpr, nch = r / 8;
  for (int nb = n0; nb < n1; nb += rpp) {
    const int n = nb + g;
    const bool live = n < n1;
    const int nn = live ? n : n1 - 1;  // address clamp: an idle group recomputes the last row and stores nothing
    const int p = nn / fout;
    const bf16_t* bw = Bw + (long)nn * ldb + (long)p * r;
    const bf16_t* tp = ts + (p - p0) * r;
    float a[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) a[b] = 0.f;
    for (int c = gl; c < nch; c += lpr) {
      float w[8];
      unpack8(*reinterpret_cast<const uint4*>(bw + c * 8), w);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (b < B) {
          float tv[8];
          unpack8(*reinterpret_cast<const uint4*>(tp + b * ncols + c * 8), tv);
          a[b] += dot8(w, tv);
        }
      }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (b < B) {
        float v = a[b];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
          if (o < lpr) v += __shfl_xor(v, o, 64);
        if (live && gl == 0) {
          v = acc[b * ldacc + n] + v;
          if (res) v += bf2f(res[b * ldr + n]);
          y[b * ldy + n] = f2bf(v);
        }
      }
    }
  }
}

}  // namespace

// K-slices of lhrs_lora_down: enough that R / 8 row blocks x slices reach the chip's 256 CUs, whole 64-element chunks, none empty
extern "C" int lhrs_lora_down_splits(int K, int R) {
  if (K < 64 || R < 8) return 1;
  const int nch = K / 64, rb = R / DOWN_ROWS;
  int want = (256 + rb - 1) / rb;
  if (want > MAX_SLICES) want = MAX_SLICES;
  if (want > nch) want = nch;
  const int per = (nch + want - 1) / want;
  return (nch + per - 1) / per;
}

extern "C" int lhrs_lora_down(const void* x, long ldx, int prologue, const void* norm_w, float eps, const void* A, long lda, float* tpart, int B, int R,
                              int K, void* stream) {
  LHRS_REQUIRE(B >= 1 && B <= MAX_B, "lora_down: B=%d (1..16)", B);
  LHRS_REQUIRE(K >= 64 && K % 64 == 0, "lora_down: K=%d (K %% 64 == 0)", K);
  LHRS_REQUIRE(R >= 8 && R % 8 == 0 && R <= MAX_R, "lora_down: R=%d (a multiple of 8, at most 768)", R);
  LHRS_REQUIRE(x != nullptr && A != nullptr && tpart != nullptr, "lora_down: null x / A / tpart");
  LHRS_REQUIRE(prologue >= 0 && prologue <= 2 && (prologue != 1 || norm_w != nullptr), "lora_down: prologue %d", prologue);
  LHRS_REQUIRE(ldx % 8 == 0 && ldx >= (prologue == 2 ? 2L * K : (long)K) && lda % 8 == 0 && lda >= K && (uintptr_t)x % 16 == 0 && (uintptr_t)A % 16 == 0 &&
                   (uintptr_t)norm_w % 16 == 0,
               "lora_down: strides / alignment (16-B lane loads): ldx=%ld lda=%ld", ldx, lda);
  const int nsl = lhrs_lora_down_splits(K, R);
  const int ks = ((K / 64 + nsl - 1) / nsl) * 64;
  const size_t sm = (size_t)B * ks * 2;
  LHRS_REQUIRE(sm + DOWN_STATIC_LDS <= MAX_LDS, "lora_down: a K-slice of %d activations x %d rows does not fit the 160 KiB of LDS", ks, B);
  const dim3 grid(R / DOWN_ROWS, nsl), blk(256);
  hipStream_t st = (hipStream_t)stream;
#define DOWN_LAUNCH(NB)                                                                                                                          \
  if (sm + DOWN_STATIC_LDS > 65536)                                                                                                              \
    (void)hipFuncSetAttribute((const void*)lora_down_kernel<NB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm);                           \
  hipLaunchKernelGGL((lora_down_kernel<NB>), grid, blk, sm, st, (const bf16_t*)x, ldx, prologue, (const bf16_t*)norm_w, eps, (const bf16_t*)A, lda, \
                     tpart, B, R, K, ks)
  if (B == 1) { DOWN_LAUNCH(1); }
  else if (B == 2) { DOWN_LAUNCH(2); }
  else if (B <= 4) { DOWN_LAUNCH(4); }
  else if (B <= 8) { DOWN_LAUNCH(8); }
  else { DOWN_LAUNCH(16); }
#undef DOWN_LAUNCH
  LHRS_CHECK_LAUNCH("lora_down");
  return 0;
}

extern "C" int lhrs_lora_up(const float* acc, long ldacc, const float* tpart, int nsl, float s, const void* Bw, long ldb, int r, int fout,
                            const void* residual, long ldr, void* y, long ldy, int B, int N, int R, void* stream) {
  LHRS_REQUIRE(B >= 1 && B <= MAX_B, "lora_up: B=%d (1..16)", B);
  LHRS_REQUIRE(R >= 8 && R % 8 == 0 && R <= MAX_R, "lora_up: R=%d (a multiple of 8, at most 768)", R);
  LHRS_REQUIRE(nsl >= 1 && nsl <= MAX_SLICES, "lora_up: nsl=%d (1..16)", nsl);
  LHRS_REQUIRE(acc != nullptr && tpart != nullptr && Bw != nullptr && y != nullptr, "lora_up: null acc / tpart / Bw / y");
  LHRS_REQUIRE(N > 0 && fout > 0 && N % fout == 0, "lora_up: N=%d is not a whole number of blocks of fout=%d rows", N, fout);
  LHRS_REQUIRE(r >= 8 && r % 8 == 0 && (long)(N / fout) * r <= R, "lora_up: r=%d (a multiple of 8) x %d blocks must fit R=%d", r, N / fout, R);
  LHRS_REQUIRE(ldb % 8 == 0 && ldb >= (long)(N / fout) * r && (uintptr_t)Bw % 16 == 0 && ldacc >= N && ldy >= N && (residual == nullptr || ldr >= N),
               "lora_up: strides / alignment (16-B lane loads): ldb=%ld ldacc=%ld ldy=%ld ldr=%ld", ldb, ldacc, ldy, ldr);
  int lpr = 1;
  while (lpr < r / 8 && lpr < 64) lpr <<= 1;
  const int rows = 256 / lpr > 32 ? 256 / lpr : 32;
  const dim3 grid(cdiv(N, rows)), blk(256);
  hipStream_t st = (hipStream_t)stream;
#define UP_LAUNCH(NB)                                                                                                                          \
  hipLaunchKernelGGL((lora_up_kernel<NB>), grid, blk, 0, st, acc, ldacc, tpart, nsl, s, (const bf16_t*)Bw, ldb, r, fout, (const bf16_t*)residual, \
                     ldr, (bf16_t*)y, ldy, B, N, R, lpr, rows)
  if (B == 1) UP_LAUNCH(1);
  else if (B == 2) UP_LAUNCH(2);
  else if (B <= 4) UP_LAUNCH(4);
  else if (B <= 8) UP_LAUNCH(8);
  else UP_LAUNCH(16);
#undef UP_LAUNCH
  LHRS_CHECK_LAUNCH("lora_up");
  return 0;
}
