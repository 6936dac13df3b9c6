// Single-token decode from an 8-bit KV cache ("kv8") for gfx950: generate(kv_cache="fp8").
//
// Format.  One cache position of one head - 128 values, keys after RoPE and already rounded to bf16 - is 128 OCP e4m3fn codes and one
// e8m0 scale byte.  With m = max|v| of the group: m == 0 gives byte 127 and +0 codes; else e = floor(log2 m) - 8, raised by one if
// m > 448 * 2^e (the smallest power of two with every |v| / 2^e <= 448), byte = clamp(e + 127, 0, 254), code = RNE_e4m3(v / 2^e).
// Nothing saturates, no code is a NaN, and v / 2^e is exact in fp32: the bytes have one answer (tests/kv8_cases.py restates them).
// Storage per layer, position-major like the bf16 caches: codes uint8 [rows * max_ctx][H * 128], scales uint8 [rows * max_ctx][H].
//
//   kv8_quant_rows   : strided bf16 rows [n][H * 128] -> codes and scale bytes of n consecutive cache positions (the prefill's append).
//   decode_attn_kv8  : lhrs_decode_attn_split on that cache - RoPE of the new q / k row, quantisation of the new K and V head rows, their
//                      append at pos[b] and attention over keys 0..pos[b] in ONE launch.  A 128-byte head row is 8 lanes x 16 B, so an
//                      8-lane group owns a key: eight keys per wave load, a three-step dot reduction, RoPE partner lane ^ 4.  The new token
//                      attends to the DEQUANTISED row it has just written: the output is a function of the cache bytes alone.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(2))) float f32x2_t;

constexpr int K8_D = 128;

// exact 2^e, e in [-127, 128] (2^-127 is the fp32 subnormal 0x00400000; 128 gives +inf, the decode of the byte 255 no writer produces)
__device__ __forceinline__ float k8_pow2(int e) { return __uint_as_float(e >= -126 ? (unsigned)(e + 127) << 23 : 0x00400000u); }

__device__ __forceinline__ float group8_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 1, 64)); v = fmaxf(v, __shfl_xor(v, 2, 64)); v = fmaxf(v, __shfl_xor(v, 4, 64));
  return v;
}
__device__ __forceinline__ float group8_sum(float v) {
  v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
  return v;
}

// scale byte of a group whose largest magnitude is m (finite, >= 0): with ex the biased exponent of m, floor(log2 m) = ex - 127 and
// m > 448 * 2^e = 1.75 * 2^(ex - 127) iff the fraction exceeds .75; a subnormal m (ex = 0) clamps to byte 0 either way
__device__ __forceinline__ int k8_scale_byte(float m) {
  const unsigned bits = __float_as_uint(m);
  if (bits == 0) return 127;
  const int ex = (int)(bits >> 23);
  const int byte = ex - 8 + ((bits & 0x7fffffu) > 0x600000u ? 1 : 0);
  return min(max(byte, 0), 254);
}

// 16 values of one lane (an 8-lane group holds the 128 of a head row) -> 16 e4m3 codes; byte = the group's scale byte
__device__ __forceinline__ uint4 k8_quant16(const float (&v)[16], int& byte) {
  float m = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) m = fmaxf(m, fabsf(v[e]));
  m = group8_max(m);
  byte = k8_scale_byte(m);
  if (m == 0.f) return make_uint4(0, 0, 0, 0);   // a zero row is all +0, whatever the signs of its zeros
  const float inv = k8_pow2(127 - byte);         // v * 2^-e: exact
  unsigned w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int t = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * j] * inv, v[4 * j + 1] * inv, 0, false);
    t = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * j + 2] * inv, v[4 * j + 3] * inv, t, true);
    w[j] = (unsigned)t;
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ void k8_dequant16(const uint4& c, float (&v)[16]) {
  const unsigned w[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], true);
    v[4 * j] = lo[0]; v[4 * j + 1] = lo[1]; v[4 * j + 2] = hi[0]; v[4 * j + 3] = hi[1];
  }
}

__device__ __forceinline__ void k8_unpack16(const uint4& a, const uint4& b, float (&v)[16]) {
  float lo[8], hi[8];
  unpack8(a, lo); unpack8(b, hi);
#pragma unroll
  for (int e = 0; e < 8; ++e) { v[e] = lo[e]; v[8 + e] = hi[e]; }
}

// one 8-lane group per (row, head): two 16-B loads and one 16-B store per lane, the row maximum by __shfl_xor
__global__ __launch_bounds__(256) void kv8_quant_rows_kernel(const bf16_t* __restrict__ src, long ld, unsigned char* __restrict__ codes,
                                                             unsigned char* __restrict__ scales, long row0, int n, int H) {
  const long g = (long)blockIdx.x * 32 + (threadIdx.x >> 3);   // (row, head) pair; the 8 lanes of a group leave together
  if (g >= (long)n * H) return;
  const int l8 = threadIdx.x & 7;
  const long r = g / H;
  const int h = (int)(g - r * H);
  const bf16_t* p = src + r * ld + h * K8_D + l8 * 16;
  float v[16];
  k8_unpack16(*reinterpret_cast<const uint4*>(p), *reinterpret_cast<const uint4*>(p + 8), v);
  int byte;
  const uint4 c = k8_quant16(v, byte);
  *reinterpret_cast<uint4*>(codes + (row0 + r) * ((long)H * K8_D) + h * K8_D + l8 * 16) = c;
  if (l8 == 0) scales[(row0 + r) * H + h] = (unsigned char)byte;
}

// ------------------------------------------------------------------------------------------------------------------
// decode_attn_kv8_kernel: decode_attn_split_kernel (csrc/decode.hip) on the kv8 cache.  Workgroup (head, sp) owns the 128-key slices
// sp, sp + NS, ... and issues ALL loads of its first slice - codes and scale bytes - before it knows the context length (any cache row
// < max_ctx is readable; what it holds past the context never reaches a sum).  Wave w of a slice: keys 32 w + grp + 8 i, grp = lane / 8,
// i < 4.  Online-softmax partials, the sc1 / ticket exchange and the ticket reset are those of the bf16 kernel, unchanged.
// ------------------------------------------------------------------------------------------------------------------
constexpr int K8_WAVES = 4, K8_KPG = 4, K8_SLICE = K8_WAVES * 8 * K8_KPG;   // 4 waves x 8 lane groups x 4 keys = 128 keys per slice
constexpr int K8_PART = 132;                                                 // floats per partial: m, l, -, -, o[128]

__global__ __launch_bounds__(K8_WAVES * 64) void decode_attn_kv8_kernel(const bf16_t* __restrict__ qkv, long ld, unsigned char* kc8,
                                                                       unsigned char* vc8, unsigned char* ks, unsigned char* vs,
                                                                       const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                                       const int* __restrict__ pos, const unsigned char* __restrict__ kmask,
                                                                       long ld_kmask, bf16_t* __restrict__ out, long ldo, int H, int max_ctx,
                                                                       float scale, int NS, float* part_g, int* tickets,
                                                                       const float* __restrict__ cs) {
  constexpr int D = K8_D, HALF = 64;
  __shared__ float part[K8_WAVES][K8_PART];
  __shared__ int s_ticket;
  const int h = blockIdx.x / NS, sp = blockIdx.x - h * NS, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l8 = lane & 7, grp = lane >> 3;
  const int d_model = H * D;
  const long cache_row0 = (long)b * max_ctx;
  const unsigned char* kbase = kc8 + cache_row0 * d_model + h * D + l8 * 16;
  const unsigned char* vbase = vc8 + cache_row0 * d_model + h * D + l8 * 16;
  const unsigned char* ksbase = ks + cache_row0 * H + h;
  const unsigned char* vsbase = vs + cache_row0 * H + h;
  int key0 = sp * K8_SLICE + wave * (8 * K8_KPG) + grp;   // this 8-lane group: keys key0, key0 + 8, ... (K8_KPG of them) of the current slice
  uint4 kr[K8_KPG], vr[K8_KPG];
  int kb[K8_KPG], vb[K8_KPG];
#pragma unroll
  for (int i = 0; i < K8_KPG; ++i) {
    const long key = min(key0 + i * 8, max_ctx - 1);
    kr[i] = *reinterpret_cast<const uint4*>(kbase + key * d_model);
    vr[i] = *reinterpret_cast<const uint4*>(vbase + key * d_model);
    kb[i] = ksbase[key * H];
    vb[i] = vsbase[key * H];
  }
  const bf16_t* row = qkv + (long)b * ld + h * D + l8 * 16;
  const uint4 q_raw0 = *reinterpret_cast<const uint4*>(row), q_raw1 = *reinterpret_cast<const uint4*>(row + 8);
  const uint4 k_raw0 = *reinterpret_cast<const uint4*>(row + d_model), k_raw1 = *reinterpret_cast<const uint4*>(row + d_model + 8);
  const uint4 v_raw0 = *reinterpret_cast<const uint4*>(row + 2 * d_model), v_raw1 = *reinterpret_cast<const uint4*>(row + 2 * d_model + 8);
  // cos | sin of the new position for the lane's 16 frequencies: from the row lhrs_decode_advance_cs left (no dependence on `pos`), else the tables
  const int f0 = (l8 & 3) * 16;
  float4 cw[4], sw[4];
  if (cs != nullptr) {
    const float* r = cs + (long)b * 128 + f0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { cw[j] = *reinterpret_cast<const float4*>(r + 4 * j); sw[j] = *reinterpret_cast<const float4*>(r + 64 + 4 * j); }
  }
  const int p = pos[b];  // position of the new token; keys 0..p are visible
  if (p < 0 || p >= max_ctx) return;                     // no cache row to append to (workgroup-uniform; the ticket is not touched)
  if (sp * K8_SLICE > p) return;                         // no visible key in any slice of this workgroup (workgroup-uniform)
  const int nact = min(NS, p / K8_SLICE + 1);            // workgroups of this head that own a visible key
  if (cs == nullptr) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      cw[j] = *reinterpret_cast<const float4*>(cos_t + (long)p * HALF + f0 + 4 * j);
      sw[j] = *reinterpret_cast<const float4*>(sin_t + (long)p * HALF + f0 + 4 * j);
    }
  }
  // ---- rotated q (pre-scaled), and the codes + scale byte of the rotated new k and of the new v for dims [16 l8, +16); RoPE partner: lane ^ 4
  float q[16];
  uint4 kn_c, vn_c;
  int kn_b, vn_b;
  {
    float qa[16], ka[16], vn[16], kn[16];
    k8_unpack16(q_raw0, q_raw1, qa); k8_unpack16(k_raw0, k_raw1, ka); k8_unpack16(v_raw0, v_raw1, vn);
    const bool hi = l8 >= 4;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float4 c4 = cw[i >> 2], s4 = sw[i >> 2];
      const float co = (i & 3) == 0 ? c4.x : (i & 3) == 1 ? c4.y : (i & 3) == 2 ? c4.z : c4.w;
      const float si = (i & 3) == 0 ? s4.x : (i & 3) == 1 ? s4.y : (i & 3) == 2 ? s4.z : s4.w;
      const float qb = __shfl_xor(qa[i], 4, 64), kp = __shfl_xor(ka[i], 4, 64);
      // rotate_half: x[d] * cos - x[d+64] * sin (d < 64);  x[d] * cos + x[d-64] * sin (d >= 64); rounded to bf16 like the stored rows
      q[i] = bf2f(f2bf(hi ? qa[i] * co + qb * si : qa[i] * co - qb * si)) * scale;
      kn[i] = bf2f(f2bf(hi ? ka[i] * co + kp * si : ka[i] * co - kp * si));
    }
    kn_c = k8_quant16(kn, kn_b);
    vn_c = k8_quant16(vn, vn_b);
  }
  float m = -INFINITY, l = 0.f, o[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) o[e] = 0.f;
  for (int base = sp * K8_SLICE; base <= p; base += NS * K8_SLICE) {
    if (base > sp * K8_SLICE) {  // further slices of this workgroup (context > 128 NS)
      key0 = base + wave * (8 * K8_KPG) + grp;
#pragma unroll
      for (int i = 0; i < K8_KPG; ++i) {
        const long key = min(key0 + i * 8, max_ctx - 1);
        kr[i] = *reinterpret_cast<const uint4*>(kbase + key * d_model);
        vr[i] = *reinterpret_cast<const uint4*>(vbase + key * d_model);
        kb[i] = ksbase[key * H];
        vb[i] = vsbase[key * H];
      }
    }
    float sc[K8_KPG];
    float mp = -INFINITY;
#pragma unroll
    for (int i = 0; i < K8_KPG; ++i) {
      const int key = key0 + i * 8;
      if (key == p) {   // append: this group owns the new key, and attends to what it stores
        kr[i] = kn_c; vr[i] = vn_c; kb[i] = kn_b; vb[i] = vn_b;
        *reinterpret_cast<uint4*>(kc8 + (cache_row0 + p) * d_model + h * D + l8 * 16) = kn_c;
        *reinterpret_cast<uint4*>(vc8 + (cache_row0 + p) * d_model + h * D + l8 * 16) = vn_c;
        if (l8 == 0) {
          ks[(cache_row0 + p) * H + h] = (unsigned char)kn_b;
          vs[(cache_row0 + p) * H + h] = (unsigned char)vn_b;
        }
      }
      float kv[16];
      k8_dequant16(kr[i], kv);
      float dot = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) dot += q[e] * kv[e];
      dot = group8_sum(dot) * k8_pow2(kb[i] - 127);   // one exact multiply per key
      bool ok = key <= p;
      if (ok && kmask != nullptr) ok = kmask[(long)b * ld_kmask + key] != 0;
      sc[i] = ok ? dot : -INFINITY;   // rows past the context and masked keys: whatever their bytes decode to stays out
      mp = fmaxf(mp, sc[i]);
    }
    mp = fmaxf(mp, __shfl_xor(mp, 8, 64));
    mp = fmaxf(mp, __shfl_xor(mp, 16, 64));
    mp = fmaxf(mp, __shfl_xor(mp, 32, 64));
    const float m_new = fmaxf(m, mp);
    const float m_use = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = __expf(m - m_use);
    l *= alpha;
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e] *= alpha;
    m = m_new;
#pragma unroll
    for (int i = 0; i < K8_KPG; ++i) {
      if (sc[i] == -INFINITY) continue;
      const float pr = __expf(sc[i] - m_use);
      const float vsc = k8_pow2(vb[i] - 127);
      float vv[16];
      k8_dequant16(vr[i], vv);
      l += pr;
#pragma unroll
      for (int e = 0; e < 16; ++e) o[e] += pr * (vv[e] * vsc);   // vv * vsc: exact
    }
  }
  // ---- fold the 8 key groups of the wave (each accumulated with the wave-wide max, so plain sums), then the waves
  l += __shfl_xor(l, 8, 64); l += __shfl_xor(l, 16, 64); l += __shfl_xor(l, 32, 64);
#pragma unroll
  for (int e = 0; e < 16; ++e) { o[e] += __shfl_xor(o[e], 8, 64); o[e] += __shfl_xor(o[e], 16, 64); o[e] += __shfl_xor(o[e], 32, 64); }
  if (lane < 8) {
#pragma unroll
    for (int e = 0; e < 16; ++e) part[wave][4 + l8 * 16 + e] = o[e];
    if (lane == 0) { part[wave][0] = m; part[wave][1] = l; }
  }
  __syncthreads();
  // ---- this workgroup's partial: thread d < 128 holds o[d] relative to the workgroup maximum M
  float M = -INFINITY, L = 0.f, acc = 0.f;
  if (tid < D) {
#pragma unroll
    for (int i = 0; i < K8_WAVES; ++i) M = fmaxf(M, part[i][0]);
#pragma unroll
    for (int i = 0; i < K8_WAVES; ++i) {
      const float mi = part[i][0];
      const float w = mi == -INFINITY ? 0.f : __expf(mi - M);
      L += w * part[i][1];
      acc += w * part[i][4 + tid];
    }
  }
  if (nact == 1) {   // short context: nothing to exchange
    if (tid < D) out[(long)b * ldo + h * D + tid] = f2bf(L > 0.f ? acc / L : 0.f);
    return;
  }
  unsigned* mine = reinterpret_cast<unsigned*>(part_g + ((long)(b * H + h) * NS + sp) * K8_PART);
  if (tid < D) {
    __hip_atomic_store(mine + 4 + tid, __float_as_uint(acc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // sc1: write-through
    if (tid == 0) {
      __hip_atomic_store(mine + 0, __float_as_uint(M), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(mine + 1, __float_as_uint(L), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // every storing wave drains its write-through stores ...
  __syncthreads();
  if (tid == 0) s_ticket = __hip_atomic_fetch_add(tickets + b * H + h, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ... before ONE lane takes the ticket
  __syncthreads();
  if (s_ticket != nact - 1) return;
  // ---- last arriver: every other partial of this head is complete in memory (sc1 stores drained before each ticket)
  if (tid == 0) __hip_atomic_store(tickets + b * H + h, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid < D) {
    const unsigned* base_p = reinterpret_cast<const unsigned*>(part_g + (long)(b * H + h) * NS * K8_PART);
    float Mx = -INFINITY;
    for (int s2 = 0; s2 < nact; ++s2)
      Mx = fmaxf(Mx, __uint_as_float(__hip_atomic_load(base_p + (long)s2 * K8_PART, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
    float Ls = 0.f, As = 0.f;
    for (int s2 = 0; s2 < nact; ++s2) {
      const unsigned* ps = base_p + (long)s2 * K8_PART;
      const float ms = __uint_as_float(__hip_atomic_load(ps + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      const float ls = __uint_as_float(__hip_atomic_load(ps + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      const float os = __uint_as_float(__hip_atomic_load(ps + 4 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      const float w = ms == -INFINITY ? 0.f : __expf(ms - Mx);
      Ls += w * ls;
      As += w * os;
    }
    out[(long)b * ldo + h * D + tid] = f2bf(Ls > 0.f ? As / Ls : 0.f);
  }
}

}  // namespace

// src: bf16 rows [n][H * 128] with a row stride of ld elements (ld % 8 == 0, 16-byte aligned: the K or V column block of a qkv buffer read
// in place) -> codes [.., H * 128] and scales [.., H] of the cache rows row0 .. row0 + n - 1
extern "C" int lhrs_kv8_quant_rows(const void* src, long ld, void* codes, void* scales, long row0, int n, int H, void* stream) {
  LHRS_REQUIRE(n >= 1 && H >= 1 && row0 >= 0 && ld >= (long)H * K8_D && ld % 8 == 0, "kv8_quant_rows: n=%d H=%d row0=%ld ld=%ld (ld %% 8 == 0, >= H * 128)",
               n, H, row0, ld);
  LHRS_REQUIRE(src != nullptr && codes != nullptr && scales != nullptr && (uintptr_t)src % 16 == 0 && (uintptr_t)codes % 16 == 0,
               "kv8_quant_rows: src=%p codes=%p scales=%p (16-byte aligned)", src, codes, scales);
  hipLaunchKernelGGL(kv8_quant_rows_kernel, dim3(cdiv((long)n * H, 32)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, ld,
                     (unsigned char*)codes, (unsigned char*)scales, row0, n, H);
  LHRS_CHECK_LAUNCH("kv8_quant_rows");
  return 0;
}

extern "C" int lhrs_decode_attn_kv8(const void* qkv, long ld, void* kcodes, void* vcodes, void* kscales, void* vscales, const float* cos_t,
                                    const float* sin_t, const int* pos, const unsigned char* key_mask, long ld_mask, void* out, long ldo,
                                    int B, int H, int D, int max_ctx, float scale, int nsplit, float* part, int* tickets, const float* cs,
                                    void* stream) {
  LHRS_REQUIRE(D == K8_D, "decode_attn_kv8: head_dim %d (only 128)", D);
  LHRS_REQUIRE(B >= 1 && H >= 1 && max_ctx >= 1 && ld % 8 == 0 && ld >= 3L * H * D && ldo >= (long)H * D && nsplit >= 1 && nsplit <= 16,
               "decode_attn_kv8: B=%d H=%d max_ctx=%d nsplit=%d ld=%ld ldo=%ld", B, H, max_ctx, nsplit, ld, ldo);
  LHRS_REQUIRE(nsplit == 1 || (part != nullptr && tickets != nullptr), "decode_attn_kv8: nsplit=%d needs part and tickets", nsplit);
  LHRS_REQUIRE(qkv != nullptr && kcodes != nullptr && vcodes != nullptr && kscales != nullptr && vscales != nullptr && pos != nullptr && out != nullptr &&
                   (cs != nullptr || (cos_t != nullptr && sin_t != nullptr)),
               "decode_attn_kv8: a required pointer is NULL");
  LHRS_REQUIRE((uintptr_t)qkv % 16 == 0 && (uintptr_t)kcodes % 16 == 0 && (uintptr_t)vcodes % 16 == 0, "decode_attn_kv8: qkv / code caches must be 16-byte aligned");
  hipLaunchKernelGGL(decode_attn_kv8_kernel, dim3(H * nsplit, B), dim3(K8_WAVES * 64), 0, (hipStream_t)stream, (const bf16_t*)qkv, ld,
                     (unsigned char*)kcodes, (unsigned char*)vcodes, (unsigned char*)kscales, (unsigned char*)vscales, cos_t, sin_t, pos, key_mask,
                     ld_mask, (bf16_t*)out, ldo, H, max_ctx, scale, nsplit, part, tickets, cs);
  LHRS_CHECK_LAUNCH("decode_attn_kv8");
  return 0;
}
