// Sampled decoding pick (gfx950): HF's RepetitionPenaltyLogitsProcessor -> TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper and
// one multinomial draw, for each fp32 logits row, in ONE launch with one 16-wave workgroup per row (generation/logits_process.py; the
// reference's callers: text_modal.py generate do_sample=True, cli_qa.py temperature 0.4, the web UI's top_p / repetition_penalty).
//
// Phases:
//   A  load the row (all 16-byte pieces of a batch requested before any is used, as argmax_rows_kernel), penalty, z = x / temperature by IEEE
//      division, store the ORDER-PRESERVING integer image of z in LDS (the whole row: 32768 x 4 B) and reduce the maximum
//   B  top-k: radix select of the k-th largest key, four 8-bit passes over LDS integer histograms - exact, ties at the cut kept
//   C  integer weights q = rint(exp(z - zmax) * 2^40); from here on everything is integer arithmetic, accumulated with integer adds only, so the
//      result does not depend on the order in which lanes and waves arrive
//   D  top-p: a second radix select, on histograms of q: the lowest key whose strictly-larger keys hold less than top_p of the mass
//   E  draw: Philox4x32-10 -> R = (rand64 * W) >> 64; first index, in index order, whose inclusive prefix sum of surviving q exceeds R
// Mode 1 (greedy on the penalised logits) stops after the penalty and returns the first maximum, exactly as argmax_rows_kernel does.
// NaN / +inf logits are outside the contract: every loop is bounded by V and every index written is < V, but the token may be wrong.
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int SM_THREADS = 1024, SM_WAVES = SM_THREADS / 64, SM_UNROLL = 8;
constexpr int SM_MAXV = 32768;   // the row lives in LDS: 128 KB of keys + 22 KB of histograms and scratch < 160 KB
constexpr int SM_COPIES = 8;     // histogram copies (lane & 7): logits share their leading exponent bits, one copy would serialise the adds
constexpr int SM_SEGS = SM_MAXV / 64;
constexpr int SM_PIECES = SM_MAXV / 4 / SM_THREADS;   // 16-byte pieces of the key row per thread

struct SmShared {
  unsigned keys[SM_MAXV];
  u64 hist[256 * SM_COPIES];
  u64 bins[256];
  u64 seg[SM_SEGS];
  u64 red[SM_WAVES];
  float redv[SM_WAVES];
  int redi[SM_WAVES];
  unsigned redk[SM_WAVES];
  u64 sel_excl, sel_at, sel_target, sel_total;
  int sel_digit, token;
};

__device__ __forceinline__ unsigned sm_key(float f) {  // a > b  <=>  key(a) > key(b)   (no NaN; -0 was folded into +0)
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sm_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
// q = rint(exp(z - zmax) * 2^40); the maximum gets exactly 2^40.  Below exp(-29) * 2^40 = 0.28 the weight is 0 without the exp.
__device__ __forceinline__ u64 sm_weight(unsigned key, float zmax) {
  const float d = sm_unkey(key) - zmax;
  if (!(d >= -29.f)) return 0;
  const float e = expf(d) * 0x1p40f;
  return e >= 0.5f ? (u64)rintf(e) : 0;
}
__device__ __forceinline__ u64 sm_shfl(u64 v, int src) {
  return ((u64)__shfl((unsigned)(v >> 32), src, 64) << 32) | (u64)__shfl((unsigned)v, src, 64);
}
__device__ __forceinline__ u64 sm_shfl_up(u64 v, int o) {
  return ((u64)__shfl_up((unsigned)(v >> 32), o, 64) << 32) | (u64)__shfl_up((unsigned)v, o, 64);
}
__device__ __forceinline__ u64 sm_wave_sum(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    v += ((u64)__shfl_xor((unsigned)(v >> 32), o, 64) << 32) | (u64)__shfl_xor((unsigned)v, o, 64);
  return v;
}
__device__ __forceinline__ u64 sm_wave_scan(u64 v, int lane) {  // inclusive, lane 0 first
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 t = sm_shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}
__device__ __forceinline__ void sm_take(float v, int i, float& best, int& bi) {
  if (v > best || (v == best && i < bi)) { best = v; bi = i; }
}

// Philox4x32-10 (Salmon et al., SC'11)
__device__ __forceinline__ void sm_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&o)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// Radix select over the keys >= lo, highest byte first.  Every key carries a mass (1, or its integer weight q); returns the key K with
// mass(keys > K) < target <= mass(keys >= K).  use_mass: target = ceil(top_p * total mass), known once the first histogram is complete.
// Leaves mass(keys > K) in `above`, mass(keys == K) in `at` and the total in `total`.  Called by all threads.
__device__ unsigned sm_select(SmShared& S, int V, bool use_mass, unsigned lo, float zmax, u64 target, float top_p, u64& above, u64& at, u64& total) {
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned prefix = 0;
  above = 0; at = 0; total = 0;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned himask = pass ? (0xffffffffu << (shift + 8)) : 0u;
    for (int i = tid; i < 256 * SM_COPIES; i += SM_THREADS) S.hist[i] = 0;
    __syncthreads();
    if (tid == 0) { S.sel_digit = 0; S.sel_excl = 0; S.sel_at = 0; S.sel_target = 1; }  // what a pass without a crossing (bad input) leaves
    // the order of the adds does not matter: 16-byte LDS reads, all of a thread's requested before the first is used; the pieces past V
    // hold whatever the LDS held and are masked by i < V
#pragma unroll
    for (int j = 0; j < SM_PIECES; ++j) {
      const int c = j * SM_THREADS + tid;
      const uint4 k4 = c * 4 < V ? reinterpret_cast<const uint4*>(S.keys)[c] : make_uint4(0u, 0u, 0u, 0u);
      const unsigned kk[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned k = kk[e];
        if (c * 4 + e < V && k >= lo && (k & himask) == prefix) {
          const u64 w = use_mass ? sm_weight(k, zmax) : 1;
          if (w) atomicAdd(&S.hist[((k >> shift) & 255u) * SM_COPIES + (tid & (SM_COPIES - 1))], w);
        }
      }
    }
    __syncthreads();
    if (tid < 256) {
      u64 s = 0;
#pragma unroll
      for (int c = 0; c < SM_COPIES; ++c) s += S.hist[tid * SM_COPIES + c];
      S.bins[tid] = s;
    }
    __syncthreads();
    if (tid < 64) {  // lane l owns digits 255 - 4l .. 252 - 4l; scan from the top digit down
      u64 b[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = S.bins[255 - 4 * lane - j];
      const u64 s = b[0] + b[1] + b[2] + b[3];
      const u64 incl = sm_wave_scan(s, lane);
      const u64 tot = sm_shfl(incl, 63);
      u64 tgt = target;
      if (pass == 0) {
        if (use_mass) {
          const double t = ceil((double)top_p * (double)tot);
          tgt = t >= 1.0 ? (u64)t : 1;
          if (tgt > tot) tgt = tot;
        }
        if (lane == 0) S.sel_total = tot;
      }
      u64 c = incl - s;
      if (c < tgt && tgt <= incl) {  // one lane at most
        int j = 0;
        while (j < 3 && c + b[j] < tgt) { c += b[j]; ++j; }
        S.sel_digit = 255 - 4 * lane - j;
        S.sel_excl = c;
        S.sel_at = b[j];
        S.sel_target = tgt - c;
      }
    }
    __syncthreads();
    prefix |= (unsigned)S.sel_digit << shift;
    above += S.sel_excl;
    at = S.sel_at;
    target = S.sel_target;
    if (pass == 0) total = S.sel_total;
  }
  __syncthreads();
  return prefix;
}

__global__ __launch_bounds__(SM_THREADS) void sample_rows_kernel(const float* __restrict__ x, long ld, long* __restrict__ out, int V, int vec,
                                                                 int mode, float temperature, int top_k, float top_p, float pen,
                                                                 unsigned* seen, int words, unsigned seed_lo, unsigned seed_hi,
                                                                 const int* __restrict__ step_dev, long step_host, long long* wout) {
  extern __shared__ __align__(16) unsigned char sm_raw[];
  SmShared& S = *reinterpret_cast<SmShared*>(sm_raw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = blockIdx.x;
  const float* row = x + (long)r * ld;
  unsigned* seen_row = seen ? seen + (long)r * words : nullptr;
  const bool pen_on = pen != 1.f && seen_row != nullptr;

  // ---- A: load, penalty, temperature -> keys in LDS (mode 0) or the running first maximum (mode 1)
  float best = -__builtin_huge_valf();
  int bi = 0x7fffffff;
  unsigned kmax = 0;
  auto take = [&](float v, unsigned sw, int i) -> unsigned {
    if (pen_on && ((sw >> (i & 31)) & 1u)) v = v < 0.f ? v * pen : __fdiv_rn(v, pen);
    if (mode == 1) { sm_take(v, i, best, bi); return 0u; }
    float z = __fdiv_rn(v, temperature);
    if (z == 0.f) z = 0.f;  // -0 and +0 are one value to every comparison that follows
    const unsigned k = sm_key(z);
    kmax = max(kmax, k);
    return k;
  };
  if (vec) {
    const int nv = V / 4;
    for (int c0 = tid; c0 < nv; c0 += SM_THREADS * SM_UNROLL) {
      float4 t[SM_UNROLL];
      unsigned sw[SM_UNROLL];
#pragma unroll
      for (int u = 0; u < SM_UNROLL; ++u) {
        const int c = c0 + u * SM_THREADS;
        t[u] = c < nv ? *reinterpret_cast<const float4*>(row + (long)c * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        sw[u] = (pen_on && c < nv) ? seen_row[c >> 3] : 0u;  // the four tokens of a piece share one bitmap word
      }
#pragma unroll
      for (int u = 0; u < SM_UNROLL; ++u) {
        const int c = c0 + u * SM_THREADS, i = c * 4;
        if (c < nv) {
          uint4 k;
          k.x = take(t[u].x, sw[u], i); k.y = take(t[u].y, sw[u], i + 1); k.z = take(t[u].z, sw[u], i + 2); k.w = take(t[u].w, sw[u], i + 3);
          if (mode == 0) *reinterpret_cast<uint4*>(&S.keys[i]) = k;
        }
      }
    }
    for (int i = nv * 4 + tid; i < V; i += SM_THREADS) {
      const unsigned k = take(row[i], pen_on ? seen_row[i >> 5] : 0u, i);
      if (mode == 0) S.keys[i] = k;
    }
  } else {
    for (int i0 = tid; i0 < V; i0 += SM_THREADS * SM_UNROLL) {
      float t[SM_UNROLL];
      unsigned sw[SM_UNROLL];
#pragma unroll
      for (int u = 0; u < SM_UNROLL; ++u) {
        const int i = i0 + u * SM_THREADS;
        t[u] = i < V ? row[i] : 0.f;
        sw[u] = (pen_on && i < V) ? seen_row[i >> 5] : 0u;
      }
#pragma unroll
      for (int u = 0; u < SM_UNROLL; ++u) {
        const int i = i0 + u * SM_THREADS;
        if (i < V) {
          const unsigned k = take(t[u], sw[u], i);
          if (mode == 0) S.keys[i] = k;
        }
      }
    }
  }

  if (mode == 1) {  // the reduction of argmax_rows_kernel
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      sm_take(ov, oi, best, bi);
    }
    if (lane == 0) { S.redv[wave] = best; S.redi[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < SM_WAVES; ++w) sm_take(S.redv[w], S.redi[w], best, bi);
      if (bi < 0 || bi >= V) bi = 0;  // a row of NaN: no element ever compared greater
      out[r] = bi;
      if (seen_row) seen_row[bi >> 5] |= 1u << (bi & 31);
    }
    return;
  }

#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, (unsigned)__shfl_xor(kmax, o, 64));
  if (lane == 0) S.redk[wave] = kmax;
  if (tid == 0) S.token = 0;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < SM_WAVES; ++w) kmax = max(kmax, S.redk[w]);
  const float zmax = sm_unkey(kmax);

  // ---- B: top-k
  unsigned thresh = 0;  // survivors: key >= thresh
  u64 above, at, total;
  if (top_k > 0 && top_k < V) thresh = sm_select(S, V, false, 0u, zmax, (u64)top_k, 1.f, above, at, total);

  // ---- C + D: integer weights, top-p
  u64 W;
  if (top_p < 1.f) {
    thresh = sm_select(S, V, true, thresh, zmax, 0, top_p, above, at, total);
    W = above + at;
  } else {
    u64 s = 0;
#pragma unroll
    for (int j = 0; j < SM_PIECES; ++j) {
      const int c = j * SM_THREADS + tid;
      const uint4 k4 = c * 4 < V ? reinterpret_cast<const uint4*>(S.keys)[c] : make_uint4(0u, 0u, 0u, 0u);
      const unsigned kk[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c * 4 + e < V && kk[e] >= thresh) s += sm_weight(kk[e], zmax);
    }
    s = sm_wave_sum(s);
    if (lane == 0) S.red[wave] = s;
    __syncthreads();
    W = 0;
#pragma unroll
    for (int w = 0; w < SM_WAVES; ++w) W += S.red[w];
  }

  // ---- E: draw.  Index order = segment order: segment j * 16 + wave holds indices j * 1024 + wave * 64 + lane
  for (int j = 0; j < SM_MAXV / SM_THREADS; ++j) {
    const int i = j * SM_THREADS + tid;
    const unsigned k = i < V ? S.keys[i] : 0u;
    const bool sv = i < V && k >= thresh;
    u64 q = 0;
    if (__ballot(sv)) q = sm_wave_sum(sv ? sm_weight(k, zmax) : 0);
    if (lane == 0) S.seg[j * SM_WAVES + wave] = q;
  }
  __syncthreads();
  if (wave == 0) {
    unsigned rnd[4];
    const unsigned step = (unsigned)(unsigned long)(step_host + (step_dev ? (long)*step_dev : 0L));
    sm_philox(step, (unsigned)r, 0u, 0u, seed_lo, seed_hi, rnd);
    const u64 R = __umul64hi(((u64)rnd[1] << 32) | (u64)rnd[0], W);
    constexpr int PER = SM_SEGS / 64;  // 8 consecutive segments per lane
    u64 b[PER], s = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) { b[j] = S.seg[lane * PER + j]; s += b[j]; }
    const u64 incl = sm_wave_scan(s, lane);
    u64 c = incl - s;
    const bool mine = c <= R && R < incl;  // one lane at most; none only if W == 0 (bad input)
    int j = 0;
    if (mine)
      while (j < PER - 1 && c + b[j] <= R) { c += b[j]; ++j; }
    const u64 found = __ballot(mine);
    if (found) {
      const int src = __ffsll((unsigned long long)found) - 1;
      const int sg = __shfl(lane * PER + j, src, 64);
      const u64 base = sm_shfl(c, src);
      const int i = (sg / SM_WAVES) * SM_THREADS + (sg % SM_WAVES) * 64 + lane;
      const unsigned k = i < V ? S.keys[i] : 0u;
      const u64 q = (i < V && k >= thresh) ? sm_weight(k, zmax) : 0;
      const u64 pre = sm_wave_scan(q, lane);
      const u64 hit = __ballot(q != 0 && base + pre > R);
      if (hit && lane == 0) S.token = i + (__ffsll((unsigned long long)hit) - 1);
    }
  }
  __syncthreads();
  if (tid == 0) {
    int t = S.token;
    if (t < 0 || t >= V) t = 0;
    out[r] = t;
    if (seen_row) seen_row[t >> 5] |= 1u << (t & 31);
  }
  if (wout) {
    long long* wr = wout + (long)r * V;
    for (int i = tid; i < V; i += SM_THREADS) {
      const unsigned k = S.keys[i];
      wr[i] = k >= thresh ? (long long)sm_weight(k, zmax) : -1;
    }
  }
}

}  // namespace

extern "C" int lhrs_sample_rows(const float* logits, long ld, long* out, int n, int V, int mode, float temperature, int top_k, float top_p,
                                float repetition_penalty, unsigned* seen, unsigned long long seed, const int* step_dev, long step_host,
                                long long* weights_out, void* stream) {
  LHRS_REQUIRE(n >= 1, "sample_rows: n=%d", n);
  LHRS_REQUIRE(V > 0 && V <= SM_MAXV, "sample_rows: V=%d (the row is held in LDS: 1..%d)", V, SM_MAXV);
  LHRS_REQUIRE(mode == 0 || mode == 1, "sample_rows: mode=%d (0 = draw, 1 = first maximum)", mode);
  LHRS_REQUIRE(mode == 1 || temperature > 0.f, "sample_rows: temperature=%g must be > 0", (double)temperature);
  LHRS_REQUIRE(top_p > 0.f, "sample_rows: top_p=%g must be > 0", (double)top_p);
  LHRS_REQUIRE(repetition_penalty > 0.f, "sample_rows: repetition_penalty=%g must be > 0", (double)repetition_penalty);
  LHRS_REQUIRE(repetition_penalty == 1.f || seen != nullptr, "sample_rows: repetition_penalty=%g needs the seen bitmap",
               (double)repetition_penalty);
  LHRS_REQUIRE(logits != nullptr && out != nullptr && ld >= V, "sample_rows: logits=%p out=%p ld=%ld V=%d", (const void*)logits, (void*)out, ld, V);
  // per process, not per device, and unsynchronised - the pattern of lhrs_debug_poison_lds: one GPU per process (the data-parallel ranks are
  // processes) and calls from one host thread; two racing first calls would both set the same value
  static bool attr_set = false;
  if (!attr_set) {  // more than 64 KB of LDS per workgroup
    hipError_t e = hipFuncSetAttribute((const void*)sample_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(SmShared));
    if (e != hipSuccess) LHRS_FAIL("sample_rows: %s", hipGetErrorString(e));
    attr_set = true;
  }
  const int vec = ld % 4 == 0 && ((uintptr_t)logits & 15) == 0;  // 16-B aligned rows
  hipLaunchKernelGGL(sample_rows_kernel, dim3(n), dim3(SM_THREADS), sizeof(SmShared), (hipStream_t)stream, logits, ld, out, V, vec, mode,
                     temperature, top_k, top_p, repetition_penalty, seen, (V + 31) / 32, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32),
                     step_dev, step_host, weights_out);
  LHRS_CHECK_LAUNCH("sample_rows");
  return 0;
}
