// Deterministic beam search on the device (gfx950): the per-token bookkeeping of HF generate(num_beams > 1, do_sample=False)
// (generation/utils.py _beam_search) in three launches that sit between the model step and decode_emit of the captured decode graph
// (DESIGN 3.4):
//   beam_topk_rows   one 16-wave workgroup per running beam: log_softmax of the fp32 logits row, HF's repetition penalty over the beam's own
//                    generated tokens, + the beam's running score, and the row's own top K = 2 * num_beams (score, token), sorted.  The
//                    group's top K of num_beams * V totals is contained in the union of its rows' lists.
//   beam_step        one wave per batch row (one workgroup for the batch): merge of the num_beams * K candidates, next running beams, parents,
//                    next tokens, token history, finished set, the sticky early-stop heuristic and the batch-wide `done` word.
//   kv_beam_reorder  cache row [b * nb + j] takes the positions [t0, t1) of row [b * nb + parent[j]], in place, all layers in one launch.
// Every reduction has a fixed order (no atomics at all): graph replay and eager launches give the same bits.  NaN / +inf logits are outside the
// contract: every loop is bounded and every index written is in range, but the tokens may be wrong.
#include <utility>

#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int BM_THREADS = 1024, BM_WAVES = BM_THREADS / 64, BM_UNROLL = 8;
constexpr int BM_MAXV = 32768;   // the row lives in LDS: 128 KB
constexpr int BM_MAXNB = 8, BM_MAXK = 2 * BM_MAXNB, BM_MAXB = 8;
constexpr int BM_PER = BM_MAXV / BM_THREADS;   // elements a thread owns: i = j * 1024 + tid
constexpr float BM_NEG = -1.0e9f;              // HF's "minus infinity" of beam scores

struct BmShared {
  unsigned keys[BM_MAXV];   // the row as floats first, then the order-preserving image of the totals
  float redf[BM_WAVES];
  u64 redk[BM_WAVES];
};

__device__ __forceinline__ unsigned bm_key(float f) {  // a > b  <=>  key(a) > key(b)   (no NaN; -0 folded into +0 by the caller)
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float bm_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ u64 bm_wave_max(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 t = ((u64)__shfl_xor((unsigned)(v >> 32), o, 64) << 32) | (u64)__shfl_xor((unsigned)v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}
// larger key first, lower index first among equal keys
__device__ __forceinline__ u64 bm_pack(unsigned key, int i) { return ((u64)key << 32) | (u64)(0xffffffffu - (unsigned)i); }

__global__ __launch_bounds__(BM_THREADS) void beam_topk_rows_kernel(const float* __restrict__ x, long ld, int V, int vec, int K,
                                                                    const float* __restrict__ run_score, float pen,
                                                                    const int* __restrict__ hist, int max_new, const int* __restrict__ bstate,
                                                                    float* __restrict__ cand_score, int* __restrict__ cand_tok) {
  extern __shared__ __align__(16) unsigned char bm_raw[];
  BmShared& S = *reinterpret_cast<BmShared*>(bm_raw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = blockIdx.x;
  int t = 0;
  if (bstate) {
    if (bstate[1]) return;   // the search is over: leave the candidate lists as they are
    t = min(max(bstate[0], 0), max_new);
  }
  const float* row = x + (long)r * ld;
  float* xs = reinterpret_cast<float*>(S.keys);

  // ---- A: the row -> LDS, its maximum
  float m = -__builtin_huge_valf();
  if (vec) {
    const int nv = V / 4;
    for (int c0 = tid; c0 < nv; c0 += BM_THREADS * BM_UNROLL) {
      float4 v[BM_UNROLL];
#pragma unroll
      for (int u = 0; u < BM_UNROLL; ++u) {   // all 16-byte pieces of a batch requested before any is used
        const int c = c0 + u * BM_THREADS;
        v[u] = c < nv ? *reinterpret_cast<const float4*>(row + (long)c * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < BM_UNROLL; ++u) {
        const int c = c0 + u * BM_THREADS;
        if (c < nv) {
          *reinterpret_cast<float4*>(&xs[c * 4]) = v[u];
          m = fmaxf(m, fmaxf(fmaxf(v[u].x, v[u].y), fmaxf(v[u].z, v[u].w)));
        }
      }
    }
    for (int i = nv * 4 + tid; i < V; i += BM_THREADS) {
      const float v = row[i];
      xs[i] = v;
      m = fmaxf(m, v);
    }
  } else {
    for (int i0 = tid; i0 < V; i0 += BM_THREADS * BM_UNROLL) {
      float v[BM_UNROLL];
#pragma unroll
      for (int u = 0; u < BM_UNROLL; ++u) {
        const int i = i0 + u * BM_THREADS;
        v[u] = i < V ? row[i] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < BM_UNROLL; ++u) {
        const int i = i0 + u * BM_THREADS;
        if (i < V) {
          xs[i] = v[u];
          m = fmaxf(m, v[u]);
        }
      }
    }
  }
  m = block_max<BM_WAVES>(m, S.redf);   // its barriers also publish the row

  // ---- B: log-sum-exp, fixed order: thread, wave butterfly, waves 0..15
  float se = 0.f;
#pragma unroll 8
  for (int j = 0; j < BM_PER; ++j) {
    const int i = j * BM_THREADS + tid;
    if (i < V) se += expf(xs[i] - m);
  }
  se = block_sum<BM_WAVES>(se, S.redf);
  const float lg = logf(se);
  const float run = run_score[r];

  // ---- C: total = log_softmax + running score, as keys, in place (a thread rewrites only the elements it owns)
  auto total_key = [&](float v, bool seen) -> unsigned {
    float lp = (v - m) - lg;
    if (seen) lp = lp < 0.f ? lp * pen : __fdiv_rn(lp, pen);   // HF RepetitionPenaltyLogitsProcessor on the log-probabilities
    float tot = lp + run;
    if (tot == 0.f) tot = 0.f;
    return bm_key(tot);
  };
#pragma unroll 8
  for (int j = 0; j < BM_PER; ++j) {
    const int i = j * BM_THREADS + tid;
    if (i < V) S.keys[i] = total_key(xs[i], false);
  }
  __syncthreads();
  if (pen != 1.f && hist != nullptr) {   // the beam's own tokens: the same value from every duplicate
    const int* h = hist + ((long)(t & 1) * gridDim.x + r) * max_new;
    for (int j = tid; j < t; j += BM_THREADS) {
      const int tok = h[j];
      if (tok >= 0 && tok < V) S.keys[tok] = total_key(row[tok], true);
    }
    __syncthreads();
  }

  // ---- D: K rounds of "largest key, lowest index"; only the winner's owner looks at its elements again
  auto scan = [&]() -> u64 {
    u64 best = 0;
#pragma unroll 8
    for (int j = 0; j < BM_PER; ++j) {
      const int i = j * BM_THREADS + tid;
      if (i < V) {
        const u64 c = bm_pack(S.keys[i], i);
        best = c > best ? c : best;
      }
    }
    return best;
  };
  u64 mine = scan();
  for (int k = 0; k < K; ++k) {
    const u64 w = bm_wave_max(mine);
    if (lane == 0) S.redk[wave] = w;
    __syncthreads();
    u64 win = S.redk[0];
#pragma unroll
    for (int i = 1; i < BM_WAVES; ++i) win = S.redk[i] > win ? S.redk[i] : win;
    __syncthreads();
    int idx = (int)(0xffffffffu - (unsigned)win);
    if (idx < 0 || idx >= V) idx = 0;   // nothing left (V < K is rejected on the host)
    if (tid == 0) {
      cand_score[(long)r * K + k] = bm_unkey((unsigned)(win >> 32));
      cand_tok[(long)r * K + k] = idx;
    }
    if ((idx & (BM_THREADS - 1)) == tid) {
      S.keys[idx] = 0u;   // below the key of every float
      mine = scan();
    }
  }
}

struct BmStepShared {
  float sc[BM_MAXB][BM_MAXNB * BM_MAXK];
  int fl[BM_MAXB][BM_MAXNB * BM_MAXK];
  float top_sc[BM_MAXB][BM_MAXK];
  int top_beam[BM_MAXB][BM_MAXK], top_tok[BM_MAXB][BM_MAXK];
  int new_parent[BM_MAXB][BM_MAXNB], new_tok[BM_MAXB][BM_MAXNB];
  int ins_slot[BM_MAXB][BM_MAXNB], ins_beam[BM_MAXB][BM_MAXNB], ins_tok[BM_MAXB][BM_MAXNB], n_ins[BM_MAXB];
  float f_sc[BM_MAXB][BM_MAXNB];
  int f_len[BM_MAXB][BM_MAXNB], f_slot[BM_MAXB][BM_MAXNB];
  int row_heur[BM_MAXB], row_full[BM_MAXB], row_allhit[BM_MAXB];
};

// bstate: int32 [4] = {t = tokens generated before this step, done, -, -}.  hist: int32 [2][B * nb][max_new], buffer t & 1 is current.
// The finished set of a row is kept sorted by score; fin_slot[rank] names the row of fin_seq that holds the hypothesis, so that an
// insertion moves three small arrays and writes ONE sequence (into the storage of the evicted worst).
__global__ __launch_bounds__(BM_MAXB * 64) void beam_step_kernel(const float* __restrict__ cand_score, const int* __restrict__ cand_tok, int B,
                                                                 int nb, int V, int max_new, int eos, int early,
                                                                 const float* __restrict__ len_pow, float* run_score, int* parent, long* next_ids,
                                                                 int* hist, float* fin_score, int* fin_len, int* fin_slot, int* fin_seq,
                                                                 int* heur, int* bstate) {
  __shared__ BmStepShared S;
  const int g = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int t = bstate[0];
  if (bstate[1] || t < 0 || t >= max_new) return;   // done: a further launch changes nothing (uniform over the workgroup)
  const int K = 2 * nb, N = nb * K, R = B * nb;
  const int* h_old = hist + (long)(t & 1) * R * max_new;
  int* h_new = hist + (long)((t + 1) & 1) * R * max_new;

  // ---- merge: rank of every candidate among the group's nb * K by (total descending, flat index beam * V + token ascending)
  for (int c = lane; c < N; c += 64) {
    const int tok = min(max(cand_tok[(long)g * N + c], 0), V - 1);
    S.sc[g][c] = cand_score[(long)g * N + c];
    S.fl[g][c] = (c / K) * V + tok;
  }
  if (lane < K) { S.top_sc[g][lane] = -__builtin_huge_valf(); S.top_beam[g][lane] = 0; S.top_tok[g][lane] = 0; }
  __syncthreads();
  for (int c = lane; c < N; c += 64) {
    const float s = S.sc[g][c];
    const int f = S.fl[g][c];
    int rank = 0;
    for (int o = 0; o < N; ++o) {
      const float so = S.sc[g][o];
      rank += (so > s || (so == s && S.fl[g][o] < f)) ? 1 : 0;
    }
    if (rank < K) { S.top_sc[g][rank] = s; S.top_beam[g][rank] = f / V; S.top_tok[g][rank] = f % V; }
  }
  __syncthreads();

  // ---- the bookkeeping of one row, serial (K <= 16 candidates)
  if (lane == 0) {
    const int n = t + 1;
    const float lenp = len_pow[n];
    unsigned hit = 0;
    for (int k = 0; k < K; ++k)
      if (S.top_tok[g][k] == eos || n == max_new) hit |= 1u << k;
    // next running beams: the best nb candidates that did not hit; if fewer exist, hit ones follow with -1e9 added (HF's topk of the sum)
    int cnt = 0;
    for (int pass = 0; pass < 2; ++pass)
      for (int k = 0; k < K && cnt < nb; ++k)
        if (((hit >> k) & 1u) == (unsigned)pass) {
          S.new_parent[g][cnt] = S.top_beam[g][k];
          S.new_tok[g][cnt] = S.top_tok[g][k];
          run_score[g * nb + cnt] = pass ? S.top_sc[g][k] + BM_NEG : S.top_sc[g][k];
          parent[g * nb + cnt] = S.top_beam[g][k];
          next_ids[g * nb + cnt] = S.top_tok[g][k];
          ++cnt;
        }
    // finished set
    for (int j = 0; j < nb; ++j) { S.f_sc[g][j] = fin_score[g * nb + j]; S.f_len[g][j] = fin_len[g * nb + j]; S.f_slot[g][j] = fin_slot[g * nb + j]; }
    const int heur_old = heur[g];
    const bool full_old = S.f_len[g][nb - 1] > 0;
    int n_ins = 0;
    if (heur_old && !(full_old && early)) {
      for (int k = 0; k < nb; ++k) {   // a hit of rank >= nb is dropped
        if (!((hit >> k) & 1u)) continue;
        const float s = __fdiv_rn(S.top_sc[g][k], lenp);
        if (!(s > S.f_sc[g][nb - 1])) continue;
        const int slot = min(max(S.f_slot[g][nb - 1], 0), nb - 1);
        int p = nb - 1;
        while (p > 0 && S.f_sc[g][p - 1] < s) {   // entries that are already there win ties
          S.f_sc[g][p] = S.f_sc[g][p - 1]; S.f_len[g][p] = S.f_len[g][p - 1]; S.f_slot[g][p] = S.f_slot[g][p - 1];
          --p;
        }
        S.f_sc[g][p] = s; S.f_len[g][p] = n; S.f_slot[g][p] = slot;
        S.ins_slot[g][n_ins] = slot; S.ins_beam[g][n_ins] = S.top_beam[g][k]; S.ins_tok[g][n_ins] = S.top_tok[g][k];
        ++n_ins;
      }
      for (int j = 0; j < nb; ++j) { fin_score[g * nb + j] = S.f_sc[g][j]; fin_len[g * nb + j] = S.f_len[g][j]; fin_slot[g * nb + j] = S.f_slot[g][j]; }
    }
    S.n_ins[g] = n_ins;
    // can a running beam still beat the worst finished hypothesis?  (sticky once false)
    const bool full_new = S.f_len[g][nb - 1] > 0;
    const float worst = full_new ? S.f_sc[g][nb - 1] : BM_NEG;
    const int heur_new = (heur_old && __fdiv_rn(run_score[g * nb], lenp) > worst) ? 1 : 0;
    heur[g] = heur_new;
    S.row_heur[g] = heur_new;
    S.row_full[g] = full_new ? 1 : 0;
    S.row_allhit[g] = hit == (K >= 32 ? 0xffffffffu : (1u << K) - 1u) ? 1 : 0;
  }
  __syncthreads();

  // ---- sequences: finished hypotheses first (they read the old history), then the permuted history into the other buffer
  for (int e = 0; e < S.n_ins[g]; ++e) {
    int* dst = fin_seq + (long)(g * nb + S.ins_slot[g][e]) * max_new;
    const int* src = h_old + (long)(g * nb + S.ins_beam[g][e]) * max_new;
    for (int i = lane; i < t; i += 64) dst[i] = src[i];
    if (lane == 0) dst[t] = S.ins_tok[g][e];
  }
  for (int j = 0; j < nb; ++j) {
    int* dst = h_new + (long)(g * nb + j) * max_new;
    const int* src = h_old + (long)(g * nb + S.new_parent[g][j]) * max_new;
    for (int i = lane; i < t; i += 64) dst[i] = src[i];
    if (lane == 0) dst[t] = S.new_tok[g][j];
  }
  __syncthreads();
  if (threadIdx.x == 0) {   // the batch-wide stop of HF's _beam_search_has_unfinished_sequences
    int any_heur = 0, all_full = 1, all_hit = 1;
    for (int b = 0; b < B; ++b) { any_heur |= S.row_heur[b]; all_full &= S.row_full[b]; all_hit &= S.row_allhit[b]; }
    const int go = any_heur && !(all_full && early) && !all_hit;
    bstate[0] = t + 1;
    bstate[1] = go ? 0 : 1;
  }
}

// One thread owns one 16-byte chunk of one position of one cache for all NB beams of its group: it loads the NB rows, then stores the
// permuted ones.  Nobody else touches these addresses, so the permutation is in place without a second cache or a barrier.
// The beams are a parameter pack, not a loop: every value then has a name of its own and stays in registers.
template <int... J>
__device__ __forceinline__ void kv_beam_reorder_body(bf16_t* base, long row_stride, const int* __restrict__ parent_g, std::integer_sequence<int, J...>) {
  constexpr int NB = sizeof...(J);
  const int p[NB] = {min(max(parent_g[J], 0), NB - 1)...};
  if (((p[J] == J) && ...)) return;   // identity: nothing to load
  const i32x4 v[NB] = {*reinterpret_cast<const i32x4*>(base + p[J] * row_stride)...};
  ((p[J] != J ? (void)(*reinterpret_cast<i32x4*>(base + J * row_stride) = v[J]) : (void)0), ...);
}

template <int NB>
__global__ __launch_bounds__(256) void kv_beam_reorder_kernel(const long* __restrict__ table, int max_ctx, int d, const int* __restrict__ parent,
                                                              int t0, const int* __restrict__ t1_dev, int t1_host, int max_pos,
                                                              const int* __restrict__ done) {
  if (done && *done) return;
  const int cpr = d / 8;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)max_pos * cpr) return;
  const int pos = t0 + (int)(idx / cpr), c = (int)(idx % cpr);
  const int t1 = min(t1_dev ? *t1_dev : t1_host, max_ctx);
  if (pos >= t1) return;
  const int g = blockIdx.z;
  bf16_t* base = reinterpret_cast<bf16_t*>(table[blockIdx.y]) + ((long)g * NB * max_ctx + pos) * d + c * 8;   // beam 0 of the group
  kv_beam_reorder_body(base, (long)max_ctx * d, parent + g * NB, std::make_integer_sequence<int, NB>{});
}

}  // namespace

extern "C" int lhrs_beam_topk_rows(const float* logits, long ld, int n_rows, int V, int K, const float* run_score, float repetition_penalty,
                                   const int* hist, int max_new, const int* bstate, float* cand_score, int* cand_tok, void* stream) {
  LHRS_REQUIRE(n_rows >= 1 && n_rows <= 16, "beam_topk_rows: n_rows=%d (batch * num_beams, 1..16)", n_rows);
  LHRS_REQUIRE(K >= 2 && K <= BM_MAXK, "beam_topk_rows: K=%d (2 * num_beams, 2..%d)", K, BM_MAXK);
  LHRS_REQUIRE(V >= K && V <= BM_MAXV, "beam_topk_rows: V=%d (the row is held in LDS: K..%d)", V, BM_MAXV);
  LHRS_REQUIRE(repetition_penalty > 0.f, "beam_topk_rows: repetition_penalty=%g must be > 0", (double)repetition_penalty);
  LHRS_REQUIRE(repetition_penalty == 1.f || (hist != nullptr && bstate != nullptr && max_new >= 1),
               "beam_topk_rows: repetition_penalty=%g needs the token history and the step state", (double)repetition_penalty);
  LHRS_REQUIRE(logits != nullptr && run_score != nullptr && cand_score != nullptr && cand_tok != nullptr && ld >= V,
               "beam_topk_rows: logits=%p run_score=%p cand_score=%p cand_tok=%p ld=%ld V=%d", (const void*)logits, (const void*)run_score,
               (void*)cand_score, (void*)cand_tok, ld, V);
  static bool attr_set = false;   // per process, as lhrs_sample_rows
  if (!attr_set) {  // more than 64 KB of LDS per workgroup
    hipError_t e = hipFuncSetAttribute((const void*)beam_topk_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(BmShared));
    if (e != hipSuccess) LHRS_FAIL("beam_topk_rows: %s", hipGetErrorString(e));
    attr_set = true;
  }
  const int vec = ld % 4 == 0 && ((uintptr_t)logits & 15) == 0;
  hipLaunchKernelGGL(beam_topk_rows_kernel, dim3(n_rows), dim3(BM_THREADS), sizeof(BmShared), (hipStream_t)stream, logits, ld, V, vec, K, run_score,
                     repetition_penalty, hist, max_new, bstate, cand_score, cand_tok);
  LHRS_CHECK_LAUNCH("beam_topk_rows");
  return 0;
}

extern "C" int lhrs_beam_step(const float* cand_score, const int* cand_tok, int B, int num_beams, int V, int max_new, int eos_token_id,
                              int early_stopping, const float* len_pow, float* run_score, int* parent, long* next_ids, int* hist,
                              float* fin_score, int* fin_len, int* fin_slot, int* fin_seq, int* heur, int* bstate, void* stream) {
  LHRS_REQUIRE(num_beams >= 2 && num_beams * 2 <= BM_MAXK, "beam_step: num_beams=%d (2..%d)", num_beams, BM_MAXNB);
  LHRS_REQUIRE(B >= 1 && B <= BM_MAXB && B * num_beams <= 16, "beam_step: B=%d num_beams=%d (B * num_beams <= 16)", B, num_beams);
  LHRS_REQUIRE(V >= 2 * num_beams && V <= BM_MAXV, "beam_step: V=%d", V);
  LHRS_REQUIRE(max_new >= 1, "beam_step: max_new=%d", max_new);
  LHRS_REQUIRE(cand_score && cand_tok && len_pow && run_score && parent && next_ids && hist && fin_score && fin_len && fin_slot && fin_seq &&
                   heur && bstate, "beam_step: a NULL buffer");
  hipLaunchKernelGGL(beam_step_kernel, dim3(1), dim3(B * 64), 0, (hipStream_t)stream, cand_score, cand_tok, B, num_beams, V, max_new,
                     eos_token_id, early_stopping ? 1 : 0, len_pow, run_score, parent, next_ids, hist, fin_score, fin_len, fin_slot, fin_seq, heur,
                     bstate);
  LHRS_CHECK_LAUNCH("beam_step");
  return 0;
}

extern "C" int lhrs_kv_beam_reorder(const long* table, int n_caches, int B, int num_beams, int max_ctx, int d, const int* parent, int t0,
                                    const int* t1_dev, int t1_host, int max_pos, const int* done, void* stream) {
  LHRS_REQUIRE(num_beams >= 2 && num_beams <= BM_MAXNB, "kv_beam_reorder: num_beams=%d (2..%d)", num_beams, BM_MAXNB);
  LHRS_REQUIRE(B >= 1 && B * num_beams <= 16, "kv_beam_reorder: B=%d num_beams=%d (B * num_beams <= 16)", B, num_beams);
  LHRS_REQUIRE(n_caches >= 1 && n_caches <= 65535, "kv_beam_reorder: n_caches=%d", n_caches);
  LHRS_REQUIRE(d >= 8 && d % 8 == 0, "kv_beam_reorder: d=%d (16-byte chunks)", d);
  LHRS_REQUIRE(t0 >= 0 && max_pos >= 0 && max_ctx >= 1 && t0 + max_pos <= max_ctx, "kv_beam_reorder: t0=%d max_pos=%d max_ctx=%d", t0, max_pos,
               max_ctx);
  LHRS_REQUIRE(t1_dev != nullptr || (t1_host >= t0 && t1_host <= t0 + max_pos), "kv_beam_reorder: t1=%d outside [t0=%d, t0 + max_pos=%d]", t1_host,
               t0, t0 + max_pos);
  LHRS_REQUIRE(table != nullptr && parent != nullptr, "kv_beam_reorder: table=%p parent=%p", (const void*)table, (const void*)parent);
  if (max_pos == 0) return 0;
  const long total = (long)max_pos * (d / 8);
  const dim3 grid((unsigned)cdiv(total, 256), (unsigned)n_caches, (unsigned)B);
#define LHRS_BEAM_REORDER(NB)                                                                                                                \
  case NB:                                                                                                                                   \
    hipLaunchKernelGGL(kv_beam_reorder_kernel<NB>, grid, dim3(256), 0, (hipStream_t)stream, table, max_ctx, d, parent, t0, t1_dev, t1_host, \
                       max_pos, done);                                                                                                       \
    break;
  switch (num_beams) {
    LHRS_BEAM_REORDER(2) LHRS_BEAM_REORDER(3) LHRS_BEAM_REORDER(4) LHRS_BEAM_REORDER(5) LHRS_BEAM_REORDER(6) LHRS_BEAM_REORDER(7)
    LHRS_BEAM_REORDER(8)
  }
#undef LHRS_BEAM_REORDER
  LHRS_CHECK_LAUNCH("kv_beam_reorder");
  return 0;
}
