// Decode from the LLM.int8 base (generate(weights="int8")): the single-token linears read the int8 rows and their row factors directly -
// 1 B per weight per token, the e4m3 stream's size, with the base's exact codes - in the arithmetic of bitsandbytes' MatMul8bitLt that
// int8.hip / gemm_fp8_256_kernel<true> reproduce for the multi-row products.
//   int8_decode_prepare : ONE launch for the activation side of a decode linear (1..16 rows): prologue (copy / RMSNorm / SwiGLU, with the
//                         roundings every decode linear shares: swiglu8 / rms_hf of decode_linear.h), outlier columns (any row with |h| >= thr), per-row absmax of the
//                         entries below thr, int8 codes with the outlier columns zeroed, the ascending column list and the gathered 16-bit
//                         activations.  The values of lhrs_int8_prepare(h) with M = B, bit for bit; nothing returns to the host.
//   repack_int8_mfma    : int8 [N, ldw] rows -> the operand order the GEMV streams
//   gemv_int8_kernel    : y[b][n] = f32(sum_k xq[b][k] WQ[n][k]) * fl(sx[b] * wscale[n])
//                                   + sum_{j < meta[0]} xo[b][j] * bf16(WQ[n][idx[j]] * wscale[n])   (+ residual), one rounding at the store
#include "decode_linear.h"

namespace {

// ---- the activation side -------------------------------------------------------------------------------------------
constexpr int DP_WAVES = 16, DP_THREADS = DP_WAVES * 64, DP_MAXC = 2;  // a thread owns chunks tid and tid + 1024 of 8 columns: K <= 16384

__device__ __forceinline__ int dq8(float v, float inv) {
  const int q = __float2int_rn(v * inv);  // ties to even
  return max(-127, min(127, q));
}
__device__ __forceinline__ int dpack4(int a, int b, int c, int d) { return (a & 0xff) | ((b & 0xff) << 8) | ((c & 0xff) << 16) | ((d & 0xff) << 24); }

// h = pro(x) of chunk c of one row, as exact bf16 values in fp32
template <int PRO>
__device__ __forceinline__ void dp_chunk(const bf16_t* __restrict__ xrow, const bf16_t* __restrict__ norm_w, float rstd, int K, int c, float (&h)[8]) {
  uint4 t = *reinterpret_cast<const uint4*>(xrow + c * 8);
  if (PRO == 2) t = swiglu8(t, *reinterpret_cast<const uint4*>(xrow + K + c * 8));
  unpack8(t, h);
  if (PRO == 1) {
    float g[8];
    unpack8(*reinterpret_cast<const uint4*>(norm_w + c * 8), g);
#pragma unroll
    for (int e = 0; e < 8; ++e) h[e] = rms_hf(h[e], g[e], rstd);
  }
}

// exclusive prefix sum of one int per thread over the block, in thread order; *total = the block's sum
__device__ __forceinline__ int dp_scan(int v, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();  // wsum may still be read from an earlier call
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < DP_WAVES; ++i) {
    const int s = wsum[i];
    if (i < w) base += s;
    tot += s;
  }
  *total = tot;
  return base + inc - v;
}

// grid = B blocks, block b finishes row b.  Every block scans all B rows for the column flags (a thread sees the same chunks of every row,
// so the flags of its columns never leave its registers) and runs the same column scan, which gives every block the same positions
// without a pass between blocks; the rows are a few KB each and come from L2.  Block 0 writes idx and meta.
template <int PRO>
__global__ __launch_bounds__(DP_THREADS) void int8_decode_prepare_kernel(const bf16_t* __restrict__ x, long ldx, const bf16_t* __restrict__ norm_w,
                                                                         float eps, float thr, bf16_t* __restrict__ h_out, long ldh,
                                                                         int8_t* __restrict__ xq, long ldq, float* __restrict__ sx,
                                                                         int* __restrict__ idx, int* __restrict__ meta, bf16_t* __restrict__ xo,
                                                                         long ldo, int B, int K) {
  __shared__ float red[DP_WAVES];
  __shared__ int wsum[DP_WAVES];
  const int tid = threadIdx.x, own = blockIdx.x;
  const int nch = K / 8;
  float keep[DP_MAXC][8];
  unsigned hit[DP_MAXC] = {0u, 0u};
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < DP_MAXC; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) keep[i][e] = 0.f;
  for (int r = 0; r < B; ++r) {  // block-uniform
    const bf16_t* xrow = x + (long)r * ldx;
    float rstd = 0.f;
    if (PRO == 1) {
      float q = 0.f;
#pragma unroll
      for (int i = 0; i < DP_MAXC; ++i) {
        const int c = tid + i * DP_THREADS;
        if (c < nch) {
          float v[8];
          unpack8(*reinterpret_cast<const uint4*>(xrow + c * 8), v);
          q = sumsq8_serial(q, v);
        }
      }
      rstd = rsqrtf(block_sum<DP_WAVES>(q, red) / (float)K + eps);
    }
#pragma unroll
    for (int i = 0; i < DP_MAXC; ++i) {
      const int c = tid + i * DP_THREADS;
      if (c < nch) {
        float h[8];
        dp_chunk<PRO>(xrow, norm_w, rstd, K, c, h);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float a = fabsf(h[e]);
          hit[i] |= (a >= thr ? 1u : 0u) << e;
          if (r == own) {
            keep[i][e] = h[e];
            if (a < thr) m = fmaxf(m, a);
          }
        }
      }
    }
  }
  m = block_max<DP_WAVES>(m, red);
  // positions of this thread's flagged columns in the ascending list: chunks tid (all threads) come before chunks tid + 1024
  int pos[DP_MAXC], n = 0;
#pragma unroll
  for (int i = 0; i < DP_MAXC; ++i) {
    int tot;
    pos[i] = n + dp_scan(__popc(hit[i]), wsum, &tot);
    n += tot;
  }
  const float inv = m > 0.f ? 127.f / m : 0.f;
  if (tid == 0) {
    sx[own] = m / 127.f;
    if (own == 0) meta[0] = n;
  }
#pragma unroll
  for (int i = 0; i < DP_MAXC; ++i) {
    const int c = tid + i * DP_THREADS;
    if (c < nch) {
      int q[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) q[e] = ((hit[i] >> e) & 1u) ? 0 : dq8(keep[i][e], inv);
      *reinterpret_cast<int2*>(xq + (long)own * ldq + c * 8) = make_int2(dpack4(q[0], q[1], q[2], q[3]), dpack4(q[4], q[5], q[6], q[7]));
      if (h_out) *reinterpret_cast<uint4*>(h_out + (long)own * ldh + c * 8) = pack8(keep[i]);
      int p = pos[i];
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if ((hit[i] >> e) & 1u) {  // p < n <= K <= ldo
          xo[(long)own * ldo + p] = f2bf(keep[i][e]);
          if (own == 0) idx[p] = c * 8 + e;
          ++p;
        }
    }
  }
}

// ---- the weight stream ---------------------------------------------------------------------------------------------
constexpr int GI_WAVES = 8, GI_THREADS = GI_WAVES * 64;

// int8 [N, ldw] rows -> piece p = (rg * K/64 + step) * 64 + lane holds WQ[16 rg + (lane & 15)][64 step + 16 (lane >> 4) .. +16]; rows past N
// are zero.  WQ[n][k] is byte ((n / 16 * K/64 + k / 64) * 64 + 16 ((k / 16) & 3) + n % 16) * 16 + k % 16 of the copy.
__global__ __launch_bounds__(256) void repack_int8_mfma_kernel(const int8_t* __restrict__ W, long ldw, int8_t* __restrict__ out, int N, int K) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  const int nsteps = K / 64;
  const long total = (long)((N + 15) / 16) * nsteps * 64;
  if (p >= total) return;
  const int lane = (int)(p & 63);
  const long t = p >> 6;
  const int step = (int)(t % nsteps);
  const long row = (t / nsteps) * 16 + (lane & 15);
  i32x4 v = {0, 0, 0, 0};
  if (row < N) v = *reinterpret_cast<const i32x4*>(W + row * ldw + (long)step * 64 + (lane >> 4) * 16);
  *reinterpret_cast<i32x4*>(out + p * 16) = v;
}

// 16 output rows per block; the eight waves split the 64-k steps, eight steps (8 KiB of weights per wave) in flight.  Lane (r, g) of a step
// holds bytes [16 g, +16) of the step of weight row r (A operand) and of activation row r (B operand): the A and B lane maps of an MFMA
// are the same function of k, so the product only needs both operands in a common order.  The accumulator has the batch on lane & 15
// and weight rows 4 g .. 4 g + 3 in its registers (the map of every 16x16 MFMA here); the one-hot probe of tests/test_gemv_int8_gpu.py
// pins both.  The activation codes are read from global memory (16 rows x 11008 do not fit the LDS, and all blocks share them in L2).
// The int32 partials of the waves are summed as integers: exact, no atomics, any order gives the same bits.
// The 16-bit outlier term is a gather pass over idx after the k-loop (nothing when meta[0] = 0): a wave takes two weight rows, lane l the
// columns j = l, l + 64, ... of all batch rows (one chain per batch row), then the 64-lane butterfly; the sum joins the scaled int term.
template <bool PK>
__global__ __launch_bounds__(GI_THREADS) void gemv_int8_kernel(const int8_t* __restrict__ W, long ldw, const float* __restrict__ wscale,
                                                               const int8_t* __restrict__ xq, long ldq, const float* __restrict__ sx,
                                                               const int* __restrict__ idx, const int* __restrict__ meta,
                                                               const bf16_t* __restrict__ xo, long ldo, const bf16_t* res, long ldr, void* y,
                                                               long ldy, int NB, int N, int K, int out_f32) {
  __shared__ int part[GI_WAVES][16][17];
  __shared__ float opart[16][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fg = lane >> 4;
  const int row0 = blockIdx.x * 16;
  const int nsteps = K / 64, per = (nsteps + GI_WAVES - 1) / GI_WAVES;
  const int s_begin = min(wave * per, nsteps), s_end = min(nsteps, s_begin + per);
  const int8_t* wp = PK ? W + (long)blockIdx.x * nsteps * 1024 + lane * 16 : W + (long)min(row0 + fr, N - 1) * ldw + fg * 16;
  constexpr long WSTEP = PK ? 1024 : 64;
  constexpr int U = 8;  // 64-k steps in flight per wave: 8 KiB, what gemv_fp8_mfma_kernel keeps with four 128-k steps
  i32x4 wq[U];
#pragma unroll
  for (int u = 0; u < U; ++u)
    wq[u] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp + (long)min(s_begin + u, max(s_end - 1, 0)) * WSTEP));
  const int8_t* xp = xq + (long)min(fr, NB - 1) * ldq + fg * 16;
  const bool live = fr < NB;
  i32x4 acc = {0, 0, 0, 0};
  for (int s0 = s_begin; s0 < s_end; s0 += U) {
    const bool more = s0 + U < s_end;  // wave-uniform
    i32x4 wn[U], xv[U];
    if (more) {
#pragma unroll
      for (int u = 0; u < U; ++u) wn[u] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp + (long)min(s0 + U + u, s_end - 1) * WSTEP));
    }
#pragma unroll
    for (int u = 0; u < U; ++u) xv[u] = *reinterpret_cast<const i32x4*>(xp + (long)min(s0 + u, s_end - 1) * 64);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (s0 + u < s_end) {
        i32x4 b = xv[u];
        if (!live) b = i32x4{0, 0, 0, 0};
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(wq[u], b, acc, 0, 0, 0);
      }
    }
    if (more) {
#pragma unroll
      for (int u = 0; u < U; ++u) wq[u] = wn[u];
    }
  }
  // acc[r] = partial sum of y[batch = fr][row0 + 4 fg + r] over this wave's steps
#pragma unroll
  for (int r = 0; r < 4; ++r) part[wave][fg * 4 + r][fr] = acc[r];
  const int n = min(max(meta[0], 0), (int)min((long)K, ldo));  // block-uniform; never past a row of xo
  if (n > 0) {
#pragma unroll
    for (int ii = 0; ii < 16 / GI_WAVES; ++ii) {  // a wave takes two weight rows, its lanes every 64th outlier column of all batch rows
      const int wi = wave * (16 / GI_WAVES) + ii;
      float o[16];
#pragma unroll
      for (int bb = 0; bb < 16; ++bb) o[bb] = 0.f;
      if (row0 + wi < N) {  // wave-uniform
        const float sw = wscale[row0 + wi];
        const int8_t* wrow = PK ? W + ((long)blockIdx.x * nsteps * 64 + wi) * 16 : W + (long)(row0 + wi) * ldw;
        for (int j = lane; j < n; j += 64) {
          const int k = idx[j];
          if ((unsigned)k < (unsigned)K) {
            const long off = PK ? (long)(k >> 6) * 1024 + ((k >> 4) & 3) * 256 + (k & 15) : (long)k;
            const float wd = bf2f(f2bf((float)wrow[off] * sw));
#pragma unroll
            for (int bb = 0; bb < 16; ++bb)
              if (bb < NB) o[bb] = fmaf(bf2f(xo[(long)bb * ldo + j]), wd, o[bb]);  // the product of two bf16 values is exact in fp32
          }
        }
      }
#pragma unroll
      for (int bb = 0; bb < 16; ++bb) {
        if (bb < NB) {  // block-uniform
          float v = o[bb];
#pragma unroll
          for (int sh = 32; sh > 0; sh >>= 1) v += __shfl_xor(v, sh, 64);
          if (lane == 0) opart[wi][bb] = v;
        }
      }
    }
  }
  __syncthreads();
  const int i = tid >> 4, b = tid & 15;
  const int row = row0 + i;
  const bool mine = b < NB && row < N;
  if (tid < 256 && mine) {
    int sum = 0;
#pragma unroll
    for (int w = 0; w < GI_WAVES; ++w) sum += part[w][i][b];
    float v = __fmul_rn((float)sum, __fmul_rn(sx[b], wscale[row]));
    if (n > 0) v = __fadd_rn(v, opart[i][b]);
    store_y(y, out_f32, b, ldy, row, v, res, ldr);
  }
}

}  // namespace

// The activation side of one decode linear on the LLM.int8 base, one launch, 1 <= B <= 16, K % 64 == 0, K <= 16384.
//   x bf16 [B, ldx] (K columns; 2K for prologue 2); prologue / norm_w / eps as lhrs_gemv; thr > 0 the outlier threshold
//   h_out bf16 [B, ldh] or NULL; xq int8 [B, ldq]; sx fp32 [B]; idx int [K]; xo bf16 [B, ldo], ldo >= K; meta int [1]
// Padding convention: there is none.  idx[0 .. n) and xo[:, 0 .. n) are written, n = meta[0]; entries past n keep what they held and
// lhrs_gemv_int8 reads none of them.
extern "C" int lhrs_int8_decode_prepare(const void* x, long ldx, int prologue, const void* norm_w, float eps, float thr, void* h_out, long ldh,
                                        void* xq, long ldq, float* sx, int* idx, int* meta, void* xo, long ldo, int B, int K, void* stream) {
  LHRS_REQUIRE(B >= 1 && B <= 16 && K >= 64 && K % 64 == 0 && K <= DP_THREADS * DP_MAXC * 8,
               "int8_decode_prepare: B=%d (1..16) K=%d (K %% 64 == 0, K <= %d)", B, K, DP_THREADS * DP_MAXC * 8);
  LHRS_REQUIRE(prologue >= 0 && prologue <= 2 && (prologue != 1 || (norm_w && al16(norm_w))) && thr > 0.f,
               "int8_decode_prepare: prologue=%d (0..2; 1 needs norm_w) thr=%g (> 0)", prologue, (double)thr);
  LHRS_REQUIRE(x && xq && sx && idx && meta && xo && al16(x) && al16(xq) && (!h_out || al16(h_out)) && ldx % 8 == 0 &&
                   ldx >= (prologue == 2 ? 2L * K : (long)K) && ldq % 16 == 0 && ldq >= K && ldo >= K && (!h_out || (ldh % 8 == 0 && ldh >= K)),
               "int8_decode_prepare: pointers / strides (ldx=%ld ldh=%ld ldq=%ld ldo=%ld)", ldx, ldh, ldq, ldo);
#define GOP(P)                                                                                                                          \
  hipLaunchKernelGGL((int8_decode_prepare_kernel<P>), dim3(B), dim3(DP_THREADS), 0, (hipStream_t)stream, (const bf16_t*)x, ldx,          \
                     (const bf16_t*)norm_w, eps, thr, (bf16_t*)h_out, ldh, (int8_t*)xq, ldq, sx, idx, meta, (bf16_t*)xo, ldo, B, K)
  if (prologue == 0) GOP(0); else if (prologue == 1) GOP(1); else GOP(2);
#undef GOP
  LHRS_CHECK_LAUNCH("int8_decode_prepare");
  return 0;
}

// out: ceil(N/16) * K bytes (see repack_int8_mfma_kernel)
extern "C" int lhrs_repack_int8_mfma(const void* WQ, long ldw, void* out, int N, int K, void* stream) {
  LHRS_REQUIRE(N > 0 && K >= 64 && K % 64 == 0, "repack_int8_mfma: N=%d K=%d (K %% 64 == 0)", N, K);
  LHRS_REQUIRE(WQ && out && al16(WQ) && al16(out) && ldw % 16 == 0 && ldw >= K, "repack_int8_mfma: pointers / strides (ldw=%ld)", ldw);
  const long nthreads = (long)cdiv(N, 16) * (K / 64) * 64;
  hipLaunchKernelGGL(repack_int8_mfma_kernel, dim3(cdiv(nthreads, 256)), dim3(256), 0, (hipStream_t)stream, (const int8_t*)WQ, ldw, (int8_t*)out, N, K);
  LHRS_CHECK_LAUNCH("repack_int8_mfma");
  return 0;
}

// y[B, N] = f32(xq . WQ^T) * fl(sx[b] * wscale[n]) + xo[:, :n] . bf16(WQ[:, idx[:n]] * wscale)^T (+ residual), n = meta[0] read on the device.
// WQ: int8 [N, ldw] rows (w_packed 0) or the copy of lhrs_repack_int8_mfma (w_packed 1, ldw ignored); xq / sx / idx / meta / xo as written by
// lhrs_int8_decode_prepare.  1 <= B <= 16, K % 64 == 0; y is bf16, or fp32 with out_f32.
extern "C" int lhrs_gemv_int8(const void* WQ, long ldw, int w_packed, const float* wscale, const void* xq, long ldq, const float* sx,
                              const int* idx, const int* meta, const void* xo, long ldo, const void* residual, long ldr, void* y, long ldy, int B,
                              int N, int K, int out_f32, void* stream) {
  LHRS_REQUIRE(B >= 1 && B <= 16 && N > 0 && K >= 64 && K % 64 == 0, "gemv_int8: B=%d (1..16) N=%d K=%d (K %% 64 == 0)", B, N, K);
  LHRS_REQUIRE(WQ && wscale && xq && sx && idx && meta && xo && y && al16(WQ) && al16(xq) && (w_packed || (ldw % 16 == 0 && ldw >= K)) &&
                   ldq % 16 == 0 && ldq >= K && ldo >= 1 && ldy >= N && (!residual || ldr >= N),
               "gemv_int8: pointers / strides (ldw=%ld ldq=%ld ldo=%ld ldr=%ld ldy=%ld)", ldw, ldq, ldo, ldr, ldy);
#define GOI(P)                                                                                                                         \
  hipLaunchKernelGGL((gemv_int8_kernel<P>), dim3(cdiv(N, 16)), dim3(GI_THREADS), 0, (hipStream_t)stream, (const int8_t*)WQ, ldw, wscale, \
                     (const int8_t*)xq, ldq, sx, idx, meta, (const bf16_t*)xo, ldo, (const bf16_t*)residual, ldr, y, ldy, B, N, K, out_f32)
  if (w_packed) GOI(true); else GOI(false);
#undef GOI
  LHRS_CHECK_LAUNCH("gemv_int8");
  return 0;
}
