// Single-token decode attention for gfx950 (head_dim 128): RoPE of the new q / k row (HF rotate_half), append of (rotated k, v) to the
// cache at pos[b] and attention over keys 0..pos[b] in ONE launch per layer and token.  One kernel template, decode_attn_kernel, serves
//   lhrs_decode_attn       : bf16 cache, one workgroup per (sequence, head)            <CacheBf16, 8, 16, false>
//   lhrs_decode_attn_split : bf16 cache, the context split over nsplit workgroups      <CacheBf16, 4, 8, true>
//   lhrs_decode_attn_kv8   : the same split on the 8-bit cache, generate(kv_cache="fp8") <CacheE4m3, 4, 4, true>
// and kv8_quant_rows writes the prefill's rows of that cache; kv8_dequant_rows reads rows back as bf16 for a prefill behind cached positions.
//
// The 8-bit cache ("kv8").  One cache position of one head - 128 values, keys after RoPE and already rounded to bf16 - is 128 OCP e4m3fn
// codes and one e8m0 scale byte.  With m = max|v| of the group: m == 0 gives byte 127 and +0 codes; else e = floor(log2 m) - 8, raised by
// one if m > 448 * 2^e (the smallest power of two with every |v| / 2^e <= 448), byte = clamp(e + 127, 0, 254), code = RNE_e4m3(v / 2^e).
// Nothing saturates, no code is a NaN, and v / 2^e is exact in fp32: the bytes have one answer (tests/kv8_cases.py restates them).
// Storage per layer, position-major like the bf16 caches: codes uint8 [rows * max_ctx][H * 128], scales uint8 [rows * max_ctx][H].
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

// N (8 or 16) consecutive bf16 values as 16-byte words, and those words as floats
template <int N>
__device__ __forceinline__ void load_bf16(const bf16_t* p, uint4 (&raw)[N / 8]) {
#pragma unroll
  for (int j = 0; j < N / 8; ++j) raw[j] = *reinterpret_cast<const uint4*>(p + 8 * j);
}
template <int N>
__device__ __forceinline__ void unpack_bf16(const uint4 (&raw)[N / 8], float (&v)[N]) {
#pragma unroll
  for (int j = 0; j < N / 8; ++j) {
    float t[8];
    unpack8(raw[j], t);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[8 * j + e] = t[e];
  }
}

// one 8-lane group per (row, head): two 16-B loads and one 16-B store per lane, the row maximum by __shfl_xor
__global__ __launch_bounds__(256) void kv8_quant_rows_kernel(const bf16_t* __restrict__ src, long ld, unsigned char* __restrict__ codes,
                                                             unsigned char* __restrict__ scales, long row0, int n, int H) {
  const long g = (long)blockIdx.x * 32 + (threadIdx.x >> 3);   // (row, head) pair; the 8 lanes of a group leave together
  if (g >= (long)n * H) return;
  const int l8 = threadIdx.x & 7;
  const long r = g / H;
  const int h = (int)(g - r * H);
  uint4 raw[2];
  load_bf16<16>(src + r * ld + h * K8_D + l8 * 16, raw);
  float v[16];
  unpack_bf16<16>(raw, v);
  int byte;
  const uint4 c = k8_quant16(v, byte);
  *reinterpret_cast<uint4*>(codes + (row0 + r) * ((long)H * K8_D) + h * K8_D + l8 * 16) = c;
  if (l8 == 0) scales[(row0 + r) * H + h] = (unsigned char)byte;
}

// The inverse, for a multi-row prefill behind cached positions (generate(prefix_cache=...)): cache rows row0 .. row0 + n - 1 -> bf16 rows
// of dst (row pitch ld elements).  value = e4m3(code) * 2^(byte - 127) in fp32, rounded to bf16 RNE.  An e4m3 value has at most 4
// significant bits and the scale is a power of two, so the product is exact in fp32 and the bf16 is exact too wherever the product is a
// normal fp32 number that bf16 can hold (below 2^-126 the bf16 subnormals keep fewer bits: the RNE then rounds).  One 8-lane group per
// (row, head): one 16-B code load and the scale byte per lane, two 16-B stores per lane.
__global__ __launch_bounds__(256) void kv8_dequant_rows_kernel(const unsigned char* __restrict__ codes, const unsigned char* __restrict__ scales,
                                                               long row0, int n, int H, bf16_t* __restrict__ dst, long ld) {
  const long g = (long)blockIdx.x * 32 + (threadIdx.x >> 3);   // (row, head) pair
  if (g >= (long)n * H) return;
  const int l8 = threadIdx.x & 7;
  const long r = g / H;
  const int h = (int)(g - r * H);
  const uint4 c = *reinterpret_cast<const uint4*>(codes + (row0 + r) * ((long)H * K8_D) + h * K8_D + l8 * 16);
  const float sc = k8_pow2((int)scales[(row0 + r) * H + h] - 127);
  float v[16];
  k8_dequant16(c, v);
  bf16_t* out = dst + r * ld + h * K8_D + l8 * 16;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    float t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = v[8 * j + e] * sc;
    *reinterpret_cast<uint4*>(out + 8 * j) = pack8(t);
  }
}

// ---- the two cache formats.  A lane owns 16 bytes of a cached head row: LPG lanes hold the row, EPL = 128 / LPG values each.  `at` is the
// element offset of those bytes in the K and V arrays, `sat` the row's place in the scale arrays.  from(at, sat, lane) is the same cache with
// its arrays starting at + lane: the kernel moves to its lane's bytes of the sequence's first row once (at, sat: workgroup-uniform).  load / store move the K and the V row of one
// key together, codes before scale bytes: in this order the e4m3 instance issues what the kernel it replaced issued (K row and V row as two
// calls measured 0.1-0.25 us per launch slower at batch 8).
struct CacheBf16 {
  static constexpr int LPG = 16, EPL = 8;
  static constexpr bool CHECKS_POS = false;    // pos[b] is trusted, as it always was here
  static constexpr bool ATTENDS_STORED = false;
  bf16_t *k, *v;
  struct Row { uint4 x; };
  __device__ __forceinline__ CacheBf16 from(long at, long, int lane) const { return {k + (at + lane), v + (at + lane)}; }   // one sum: two steps cost the split kernel 0.5 us at batch 8
  __device__ __forceinline__ void load(long at, long, Row& kr, Row& vr) const {
    kr.x = *reinterpret_cast<const uint4*>(k + at);
    vr.x = *reinterpret_cast<const uint4*>(v + at);
  }
  __device__ __forceinline__ void store(long at, long, bool, const Row& kr, const Row& vr) const {
    *reinterpret_cast<uint4*>(k + at) = kr.x;
    *reinterpret_cast<uint4*>(v + at) = vr.x;
  }
  __device__ static __forceinline__ void values(const Row& r, float (&f)[EPL]) { unpack8(r.x, f); }
  __device__ static __forceinline__ float scale(const Row&) { return 1.f; }
  __device__ static __forceinline__ Row make(const float (&f)[EPL]) { return {pack8(f)}; }
};

struct CacheE4m3 {
  static constexpr int LPG = 8, EPL = 16;
  static constexpr bool CHECKS_POS = true;     // a pos[b] outside the cache leaves the workgroup before anything is appended
  static constexpr bool ATTENDS_STORED = true;
  unsigned char *k, *v, *ks, *vs;
  struct Row { uint4 x; int byte; };
  __device__ __forceinline__ CacheE4m3 from(long at, long sat, int lane) const {   // the uniform step first: scalar arithmetic, and every kernel-argument load ahead of the first wait
    return {k + at + lane, v + at + lane, ks + sat, vs + sat};
  }
  __device__ __forceinline__ void load(long at, long sat, Row& kr, Row& vr) const {
    kr.x = *reinterpret_cast<const uint4*>(k + at);
    vr.x = *reinterpret_cast<const uint4*>(v + at);
    kr.byte = ks[sat];
    vr.byte = vs[sat];
  }
  __device__ __forceinline__ void store(long at, long sat, bool lead, const Row& kr, const Row& vr) const {   // lead: the group's lane 0 writes the scale bytes
    *reinterpret_cast<uint4*>(k + at) = kr.x;
    *reinterpret_cast<uint4*>(v + at) = vr.x;
    if (lead) { ks[sat] = (unsigned char)kr.byte; vs[sat] = (unsigned char)vr.byte; }
  }
  __device__ static __forceinline__ void values(const Row& r, float (&f)[EPL]) { k8_dequant16(r.x, f); }
  __device__ static __forceinline__ float scale(const Row& r) { return k8_pow2(r.byte - 127); }   // exact
  __device__ static __forceinline__ Row make(const float (&f)[EPL]) {
    Row r;
    r.x = k8_quant16(f, r.byte);
    return r;
  }
};

// ------------------------------------------------------------------------------------------------------------------
// decode_attn_kernel: latency-bound (ctx * 512 B per head of bf16), so the design minimises dependent memory round trips.  A pass covers
// WAVES * (64 / LPG) * KPG keys: an LPG-lane group owns a key row (whole rows per wave-instruction), group grp of wave w the keys
// w * (64 / LPG) * KPG + grp + i * (64 / LPG), i < KPG, and ALL K and V row loads of the first pass are issued before anything else - before
// the context length is known (any cache row < max_ctx is readable; rows past the context never reach a sum).  Waves keep online-softmax
// partials (m, l, o[128]) across passes and merge them through LDS.
//   SPLIT = false: one workgroup per (sequence, head) walks the passes in turn.  8 waves x 16 keys, not 16 x 8: 256 VGPRs per lane hold the
//     32 row loads without scratch.  Reads cos / sin from the tables; NS, part_g, tickets and cs are ignored.
//   SPLIT = true: one workgroup streams at most ~27 GB/s from HBM (the per-CU miss path), so workgroup (head, sp) of NS owns the 128-key
//     slices sp, sp + NS, ...; the only dependent round trips are pos -> cos / sin (none with the `cs` row lhrs_decode_advance_cs left) and
//     the exchange.  Exchange: every workgroup that owns a visible key publishes (m, l, o[128]) with write-through (sc1) stores, drains
//     them and takes a ticket; the LAST arriver reads all partials with sc1 loads (both sides sc1: no fence needed), merges and writes the
//     bf16 row; it resets the ticket (tickets are zero between launches: hipGraph replays need no memset node).
// ------------------------------------------------------------------------------------------------------------------
constexpr int DA_PART = 132;   // floats per partial, in LDS and in part_g: m, l, -, -, o[128]

template <int LPG>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int d = 1; d < LPG; d <<= 1) v += __shfl_xor(v, d, 64);
  return v;
}

template <class Cache, int WAVES, int KPG, bool SPLIT>
__global__ __launch_bounds__(WAVES * 64) void decode_attn_kernel(const bf16_t* __restrict__ qkv, long ld, Cache cache,
                                                                  const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                                  const int* __restrict__ pos, const unsigned char* __restrict__ kmask,
                                                                  long ld_kmask, bf16_t* __restrict__ out, long ldo, int H, int max_ctx,
                                                                  float scale, int NS, float* part_g, int* tickets, const float* __restrict__ cs) {
  using Row = typename Cache::Row;
  constexpr int D = 128, HALF = 64, LPG = Cache::LPG, EPL = Cache::EPL, GPW = 64 / LPG, SLICE = WAVES * GPW * KPG;
  __shared__ float part[WAVES][DA_PART];
  __shared__ int s_ticket;
  const int ns = SPLIT ? NS : 1;
  const int h = SPLIT ? blockIdx.x / ns : blockIdx.x, sp = SPLIT ? blockIdx.x - h * ns : 0, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lg = lane & (LPG - 1), grp = lane / LPG;
  const int d_model = H * D;
  const long cache_row0 = (long)b * max_ctx;
  const Cache mine = cache.from(cache_row0 * d_model + h * D, cache_row0 * H + h, lg * EPL);   // this lane's bytes / this head's scale byte, from row 0 of the sequence
  int key0 = sp * SLICE + wave * (GPW * KPG) + grp;   // this lane group: keys key0, key0 + GPW, ... (KPG of them) of the current pass
  Row kr[KPG], vr[KPG];
  auto load_rows = [&]() {   // every load of a pass, issued together: none depends on another
#pragma unroll
    for (int i = 0; i < KPG; ++i) {
      const long key = min(key0 + i * GPW, max_ctx - 1);
      mine.load(key * d_model, key * H, kr[i], vr[i]);
    }
  };
  load_rows();
  const bf16_t* row = qkv + (long)b * ld + h * D + lg * EPL;
  uint4 q_raw[EPL / 8], k_raw[EPL / 8], v_raw[EPL / 8];
  load_bf16<EPL>(row, q_raw); load_bf16<EPL>(row + d_model, k_raw); load_bf16<EPL>(row + 2 * d_model, v_raw);
  // cos | sin of the new position for the lane's EPL frequencies: from the row lhrs_decode_advance_cs left (no dependence on `pos`), else the tables
  const int f0 = (lg & (LPG / 2 - 1)) * EPL;
  float4 cw[EPL / 4], sw[EPL / 4];
  auto load_cs = [&](const float* c, const float* s) {
#pragma unroll
    for (int j = 0; j < EPL / 4; ++j) { cw[j] = *reinterpret_cast<const float4*>(c + 4 * j); sw[j] = *reinterpret_cast<const float4*>(s + 4 * j); }
  };
  if constexpr (SPLIT) {
    if (cs != nullptr) load_cs(cs + (long)b * 128 + f0, cs + (long)b * 128 + 64 + f0);
  }
  const int p = pos[b];  // position of the new token; keys 0..p are visible
  if constexpr (Cache::CHECKS_POS) {
    if (p < 0 || p >= max_ctx) return;                 // no cache row to append to (workgroup-uniform; the ticket is not touched)
  }
  if constexpr (SPLIT) {
    if (sp * SLICE > p) return;                        // no visible key in any slice of this workgroup (workgroup-uniform)
  }
  const int nact = SPLIT ? min(ns, p / SLICE + 1) : 1;   // workgroups of this head that own a visible key
  if (!SPLIT || cs == nullptr) load_cs(cos_t + (long)p * HALF + f0, sin_t + (long)p * HALF + f0);
  // ---- rotated q (pre-scaled), rotated new k and new v for dims [lg * EPL, +EPL), and their cache rows; RoPE partner: lane ^ (LPG / 2)
  float q[EPL], kn[EPL], vn[EPL];
  {
    float qa[EPL], ka[EPL];
    unpack_bf16<EPL>(q_raw, qa); unpack_bf16<EPL>(k_raw, ka); unpack_bf16<EPL>(v_raw, vn);
    const bool hi = lg >= LPG / 2;
#pragma unroll
    for (int i = 0; i < EPL; ++i) {
      const float4 c4 = cw[i >> 2], s4 = sw[i >> 2];
      const float co = (i & 3) == 0 ? c4.x : (i & 3) == 1 ? c4.y : (i & 3) == 2 ? c4.z : c4.w;
      const float si = (i & 3) == 0 ? s4.x : (i & 3) == 1 ? s4.y : (i & 3) == 2 ? s4.z : s4.w;
      const float qb = __shfl_xor(qa[i], LPG / 2, 64), kb = __shfl_xor(ka[i], LPG / 2, 64);
      // rotate_half: x[d] * cos - x[d+64] * sin (d < 64);  x[d] * cos + x[d-64] * sin (d >= 64); rounded to bf16 like the stored rows
      q[i] = bf2f(f2bf(hi ? qa[i] * co + qb * si : qa[i] * co - qb * si)) * scale;
      kn[i] = bf2f(f2bf(hi ? ka[i] * co + kb * si : ka[i] * co - kb * si));
    }
  }
  const Row kn_row = Cache::make(kn), vn_row = Cache::make(vn);   // bf16: pack8 of the unpacked v is v again
  auto append = [&]() { mine.store((long)p * d_model, (long)p * H, lg == 0, kn_row, vn_row); };   // by the group that owns key p
  float m = -INFINITY, l = 0.f, o[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) o[e] = 0.f;
  for (int base = sp * SLICE; base <= p; base += ns * SLICE) {
    if (base > sp * SLICE) {  // later passes: same load pattern, issued together at the top of the pass
      key0 = base + wave * (GPW * KPG) + grp;
      load_rows();
    }
    float sc[KPG];
    float mp = -INFINITY;
#pragma unroll
    for (int i = 0; i < KPG; ++i) {
      const int key = key0 + i * GPW;
      float kv[EPL];
      if constexpr (Cache::ATTENDS_STORED) {   // e4m3: the new token attends to the dequantised row it has just written
        if (key == p) { append(); kr[i] = kn_row; vr[i] = vn_row; }
        Cache::values(kr[i], kv);
      } else {   // bf16: the floats ARE the stored row; swapped in the append branch (outside it: 8 selects per key and 0.2-0.5 us per launch)
        Cache::values(kr[i], kv);
        if (key == p) {
#pragma unroll
          for (int e = 0; e < EPL; ++e) kv[e] = kn[e];
          append();
        }
      }
      float dot = 0.f;
#pragma unroll
      for (int e = 0; e < EPL; ++e) dot += q[e] * kv[e];
      dot = group_sum<LPG>(dot) * Cache::scale(kr[i]);   // one exact multiply per key
      bool ok = key <= p;
      if (ok && kmask != nullptr) ok = kmask[(long)b * ld_kmask + key] != 0;
      sc[i] = ok ? dot : -INFINITY;   // rows past the context and masked keys: whatever their bytes decode to stays out
      mp = fmaxf(mp, sc[i]);
    }
#pragma unroll
    for (int d = LPG; d < 64; d <<= 1) mp = fmaxf(mp, __shfl_xor(mp, d, 64));
    const float m_new = fmaxf(m, mp);
    const float m_use = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = __expf(m - m_use);  // 0 on the first contribution (m = -inf)
    l *= alpha;
#pragma unroll
    for (int e = 0; e < EPL; ++e) o[e] *= alpha;
    m = m_new;
#pragma unroll
    for (int i = 0; i < KPG; ++i) {
      if (sc[i] == -INFINITY) continue;  // masked / absent key: its (possibly uninitialised) cache row must not touch the sum
      const float pr = __expf(sc[i] - m_use);
      const float vsc = Cache::scale(vr[i]);
      float vv[EPL];
      Cache::values(vr[i], vv);
      if constexpr (!Cache::ATTENDS_STORED) {
        if (key0 + i * GPW == p) {
#pragma unroll
          for (int e = 0; e < EPL; ++e) vv[e] = vn[e];
        }
      }
      l += pr;
#pragma unroll
      for (int e = 0; e < EPL; ++e) o[e] += pr * (vv[e] * vsc);   // vv * vsc: exact
    }
  }
  // ---- fold the key groups of the wave (each lane group accumulated with the wave-wide max, so plain sums), then the waves
#pragma unroll
  for (int d = LPG; d < 64; d <<= 1) l += __shfl_xor(l, d, 64);
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
#pragma unroll
    for (int d = LPG; d < 64; d <<= 1) o[e] += __shfl_xor(o[e], d, 64);
  }
  if (lane < LPG) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) part[wave][4 + lg * EPL + e] = o[e];
    if (lane == 0) { part[wave][0] = m; part[wave][1] = l; }
  }
  __syncthreads();
  // ---- this workgroup's partial: thread d < 128 holds o[d] relative to the workgroup maximum M
  float M = -INFINITY, L = 0.f, acc = 0.f;
  if (tid < D) {
#pragma unroll
    for (int i = 0; i < WAVES; ++i) M = fmaxf(M, part[i][0]);
#pragma unroll
    for (int i = 0; i < WAVES; ++i) {
      const float mi = part[i][0];
      const float w = mi == -INFINITY ? 0.f : __expf(mi - M);
      L += w * part[i][1];
      acc += w * part[i][4 + tid];
    }
  }
  if (nact == 1) {   // one workgroup, or a short context: nothing to exchange
    if (tid < D) out[(long)b * ldo + h * D + tid] = f2bf(L > 0.f ? acc / L : 0.f);
    return;
  }
  if constexpr (SPLIT) {
    unsigned* own = reinterpret_cast<unsigned*>(part_g + ((long)(b * H + h) * NS + sp) * DA_PART);
    if (tid < D) {
      __hip_atomic_store(own + 4 + tid, __float_as_uint(acc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // sc1: write-through
      if (tid == 0) {
        __hip_atomic_store(own + 0, __float_as_uint(M), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(own + 1, __float_as_uint(L), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
      const unsigned* base_p = reinterpret_cast<const unsigned*>(part_g + (long)(b * H + h) * NS * DA_PART);
      float Mx = -INFINITY;
      for (int s2 = 0; s2 < nact; ++s2)
        Mx = fmaxf(Mx, __uint_as_float(__hip_atomic_load(base_p + (long)s2 * DA_PART, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
      float Ls = 0.f, As = 0.f;
      for (int s2 = 0; s2 < nact; ++s2) {
        const unsigned* ps = base_p + (long)s2 * DA_PART;
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
}

// what the three launchers require alike; each reports a violation in its own words
bool attn_shape_ok(int B, int H, int max_ctx, long ld, int nsplit) {
  return B >= 1 && H >= 1 && max_ctx >= 1 && ld % 8 == 0 && nsplit >= 1 && nsplit <= 16;
}

}  // namespace

// One launch per layer and token: RoPE(q, k_new) + KV append + attention over the cache (+ HF attention_mask bytes) -> o [B, H*128].
extern "C" int lhrs_decode_attn(const void* qkv, long ld, void* kcache, void* vcache, const float* cos_t, const float* sin_t,
                                const int* pos, const unsigned char* key_mask, long ld_mask, void* out, long ldo, int B, int H, int D,
                                int max_ctx, float scale, void* stream) {
  LHRS_REQUIRE(D == 128, "decode_attn: head_dim %d (only 128)", D);
  LHRS_REQUIRE(attn_shape_ok(B, H, max_ctx, ld, 1), "decode_attn: B=%d H=%d max_ctx=%d", B, H, max_ctx);
  hipLaunchKernelGGL((decode_attn_kernel<CacheBf16, 8, 16, false>), dim3(H, B), dim3(8 * 64), 0, (hipStream_t)stream, (const bf16_t*)qkv, ld,
                     CacheBf16{(bf16_t*)kcache, (bf16_t*)vcache}, cos_t, sin_t, pos, key_mask, ld_mask, (bf16_t*)out, ldo, H, max_ctx, scale, 1,
                     (float*)nullptr, (int*)nullptr, (const float*)nullptr);
  LHRS_CHECK_LAUNCH("decode_attn");
  return 0;
}

// The same with the context split over nsplit workgroups per head (nsplit slices of 128 keys in flight per head, 1 <= nsplit <= 16).
// part: fp32 [B][H][nsplit][132] partials, tickets: int32 [B][H], ZERO before the first call (the kernel leaves them zero); both
// caller-owned and private to the stream the calls are ordered on.  cs (may be NULL): float [B][128], the cos | sin rows of pos[b]
// written by lhrs_decode_advance_cs - the kernel then takes the rotation from there instead of waiting for pos[b] to index the tables.
extern "C" int lhrs_decode_attn_split(const void* qkv, long ld, void* kcache, void* vcache, const float* cos_t, const float* sin_t,
                                      const int* pos, const unsigned char* key_mask, long ld_mask, void* out, long ldo, int B, int H, int D,
                                      int max_ctx, float scale, int nsplit, float* part, int* tickets, const float* cs, void* stream) {
  LHRS_REQUIRE(D == 128, "decode_attn_split: head_dim %d (only 128)", D);
  LHRS_REQUIRE(attn_shape_ok(B, H, max_ctx, ld, nsplit) && part && tickets, "decode_attn_split: B=%d H=%d max_ctx=%d nsplit=%d", B, H, max_ctx, nsplit);
  hipLaunchKernelGGL((decode_attn_kernel<CacheBf16, 4, 8, true>), dim3(H * nsplit, B), dim3(4 * 64), 0, (hipStream_t)stream, (const bf16_t*)qkv, ld,
                     CacheBf16{(bf16_t*)kcache, (bf16_t*)vcache}, cos_t, sin_t, pos, key_mask, ld_mask, (bf16_t*)out, ldo, H, max_ctx, scale, nsplit,
                     part, tickets, cs);
  LHRS_CHECK_LAUNCH("decode_attn_split");
  return 0;
}

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

// codes [.., H * 128] and scales [.., H] of the cache rows row0 .. row0 + n - 1 -> dst: bf16 rows [n][H * 128] with a row pitch of ld
// elements (ld % 8 == 0, 16-byte aligned)
extern "C" int lhrs_kv8_dequant_rows(const void* codes, const void* scales, long row0, int n, int H, void* dst, long ld, void* stream) {
  LHRS_REQUIRE(n >= 1 && H >= 1 && row0 >= 0 && ld >= (long)H * K8_D && ld % 8 == 0, "kv8_dequant_rows: n=%d H=%d row0=%ld ld=%ld (ld %% 8 == 0, >= H * 128)",
               n, H, row0, ld);
  LHRS_REQUIRE(dst != nullptr && codes != nullptr && scales != nullptr && (uintptr_t)dst % 16 == 0 && (uintptr_t)codes % 16 == 0,
               "kv8_dequant_rows: codes=%p scales=%p dst=%p (16-byte aligned)", codes, scales, dst);
  hipLaunchKernelGGL(kv8_dequant_rows_kernel, dim3(cdiv((long)n * H, 32)), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)codes,
                     (const unsigned char*)scales, row0, n, H, (bf16_t*)dst, ld);
  LHRS_CHECK_LAUNCH("kv8_dequant_rows");
  return 0;
}

// lhrs_decode_attn_split on the kv8 caches, nsplit >= 1 in one entry point (1: no exchange, part / tickets may be NULL).  A 128-byte head
// row is 8 lanes x 16 B, so an 8-lane group owns a key: eight keys per wave load, a three-step dot reduction, RoPE partner lane ^ 4.
extern "C" int lhrs_decode_attn_kv8(const void* qkv, long ld, void* kcodes, void* vcodes, void* kscales, void* vscales, const float* cos_t,
                                    const float* sin_t, const int* pos, const unsigned char* key_mask, long ld_mask, void* out, long ldo,
                                    int B, int H, int D, int max_ctx, float scale, int nsplit, float* part, int* tickets, const float* cs,
                                    void* stream) {
  LHRS_REQUIRE(D == K8_D, "decode_attn_kv8: head_dim %d (only 128)", D);
  LHRS_REQUIRE(attn_shape_ok(B, H, max_ctx, ld, nsplit) && ld >= 3L * H * D && ldo >= (long)H * D,
               "decode_attn_kv8: B=%d H=%d max_ctx=%d nsplit=%d ld=%ld ldo=%ld", B, H, max_ctx, nsplit, ld, ldo);
  LHRS_REQUIRE(nsplit == 1 || (part != nullptr && tickets != nullptr), "decode_attn_kv8: nsplit=%d needs part and tickets", nsplit);
  LHRS_REQUIRE(qkv != nullptr && kcodes != nullptr && vcodes != nullptr && kscales != nullptr && vscales != nullptr && pos != nullptr && out != nullptr &&
                   (cs != nullptr || (cos_t != nullptr && sin_t != nullptr)),
               "decode_attn_kv8: a required pointer is NULL");
  LHRS_REQUIRE((uintptr_t)qkv % 16 == 0 && (uintptr_t)kcodes % 16 == 0 && (uintptr_t)vcodes % 16 == 0, "decode_attn_kv8: qkv / code caches must be 16-byte aligned");
  hipLaunchKernelGGL((decode_attn_kernel<CacheE4m3, 4, 4, true>), dim3(H * nsplit, B), dim3(4 * 64), 0, (hipStream_t)stream, (const bf16_t*)qkv, ld,
                     CacheE4m3{(unsigned char*)kcodes, (unsigned char*)vcodes, (unsigned char*)kscales, (unsigned char*)vscales}, cos_t, sin_t, pos,
                     key_mask, ld_mask, (bf16_t*)out, ldo, H, max_ctx, scale, nsplit, part, tickets, cs);
  LHRS_CHECK_LAUNCH("decode_attn_kv8");
  return 0;
}
