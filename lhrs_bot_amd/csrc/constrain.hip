// Constrained decoding pick (gfx950): the greedy pick of each fp32 logits row restricted to the out-edges of the row's state in a token
// automaton, and the walk along the picked edge, in ONE launch with one 16-wave workgroup per row (HF: prefix_allowed_tokens_fn ->
// PrefixConstrainedLogitsProcessor -> argmax; DESIGN 3.4 "Constrained decoding").
//
// The automaton is CSR over int32: off[n_states + 1], tok[E] (ascending and unique inside a state), nxt[E], label[n_states].  A state
// without out-edges is final.  Row r in state s:
//   s outside [0, n_states) or final   out[r] = pad_token_id, nothing else of the row changes (an invalid s reads no automaton memory)
//   otherwise                          e* = the edge of s with the largest logits[r][tok[e]] - first maximum, i.e. the lowest token among
//                                      equals, as argmax_rows_kernel; NaN compares as -inf, so an allowed set of -inf / NaN picks the first edge;
//                                      out[r] = tok[e*], len[r] += 1, state[r] = nxt[e*], and if that state is final fin[r] = 1,
//                                      choice[r] = label[nxt[e*]]
// score != NULL: score[r] += logits[r][tok[e*]] - lse(r), lse = max + log(sum exp(x - max)) over the WHOLE row in fp32 (HF normalises with
// log_softmax BEFORE the processor masks).  The row is read once, into registers (V <= 32768: 32 values per thread).  score == NULL: the row
// of V is not read at all, only the allowed logits are gathered.
// The edges are gathered thread-strided (1 edge and V edges run the same loop), then (value, token, edge) is reduced over the block.  Every
// row writes its own slots only, with plain vector stores: no atomics, no tickets.
#include "common.h"

namespace {

constexpr int CN_THREADS = 1024, CN_WAVES = CN_THREADS / 64, CN_UNROLL = 4;
constexpr int CN_MAXV = 32768;
constexpr int CN_PIECES = CN_MAXV / 4 / CN_THREADS;   // 16-byte pieces of a row per thread
constexpr int CN_VALUES = CN_MAXV / CN_THREADS;       // values of a row per thread on the scalar path

__device__ __forceinline__ void cn_take(float v, int t, int e, float& best, int& bt, int& be) {
  if (v > best || (v == best && t < bt)) { best = v; bt = t; be = e; }
}

__global__ __launch_bounds__(CN_THREADS) void constrain_rows_kernel(const float* __restrict__ x, long ld, long* __restrict__ out, int V, int vec,
                                                                    const int* __restrict__ off, const int* __restrict__ tok,
                                                                    const int* __restrict__ nxt, const int* __restrict__ label, int n_states,
                                                                    int n_edges, int pad, int* state, int* __restrict__ fin,
                                                                    int* __restrict__ len, int* __restrict__ choice, float* __restrict__ score) {
  __shared__ float sv[CN_WAVES];
  __shared__ int st[CN_WAVES], se[CN_WAVES];
  __shared__ float red[CN_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = blockIdx.x;
  const float* row = x + (long)r * ld;
  const float ninf = -__builtin_huge_valf();

  const int s = state[r];   // uniform; thread 0 rewrites it behind the block reduction below
  int e0 = 0, e1 = 0;
  if (s >= 0 && s < n_states) {
    e0 = max(off[s], 0);
    e1 = min(off[s + 1], n_edges);
  }
  if (e1 <= e0) {  // invalid or final: the pad token, and the walk stays where it is
    if (tid == 0) out[r] = pad;
    return;
  }

  // ---- the pick: gather tok and logits[tok] thread-strided, all loads of a batch requested before the first is compared
  float best = ninf;
  int bt = 0x7fffffff, be = e0;
  for (int b0 = e0 + tid; b0 < e1; b0 += CN_THREADS * CN_UNROLL) {
    int t[CN_UNROLL];
    float v[CN_UNROLL];
#pragma unroll
    for (int u = 0; u < CN_UNROLL; ++u) {
      const int e = b0 + u * CN_THREADS;
      t[u] = e < e1 ? tok[e] : -1;
    }
#pragma unroll
    for (int u = 0; u < CN_UNROLL; ++u) v[u] = (unsigned)t[u] < (unsigned)V ? row[t[u]] : ninf;
#pragma unroll
    for (int u = 0; u < CN_UNROLL; ++u) {
      const int e = b0 + u * CN_THREADS;
      if (e < e1) cn_take(v[u] == v[u] ? v[u] : ninf, t[u], e, best, bt, be);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int ot = __shfl_xor(bt, o, 64);
    const int oe = __shfl_xor(be, o, 64);
    cn_take(ov, ot, oe, best, bt, be);
  }
  if (lane == 0) { sv[wave] = best; st[wave] = bt; se[wave] = be; }

  // ---- the score: log-sum-exp of the whole row, read once into registers
  float lse = 0.f;
  if (score) {
    float m = ninf, sum = 0.f;
    if (vec) {
      const int nv = V / 4;
      float4 p[CN_PIECES];
#pragma unroll
      for (int u = 0; u < CN_PIECES; ++u) {
        const int c = u * CN_THREADS + tid;
        p[u] = c < nv ? *reinterpret_cast<const float4*>(row + (long)c * 4) : make_float4(ninf, ninf, ninf, ninf);
      }
      const int it = nv * 4 + tid;   // V % 4 values behind the last piece
      const float tail = it < V ? row[it] : ninf;
#pragma unroll
      for (int u = 0; u < CN_PIECES; ++u) m = fmaxf(m, fmaxf(fmaxf(p[u].x, p[u].y), fmaxf(p[u].z, p[u].w)));
      m = block_max<CN_WAVES>(fmaxf(m, tail), red);
#pragma unroll
      for (int u = 0; u < CN_PIECES; ++u) {
        if (u * CN_THREADS + tid < nv) sum += (expf(p[u].x - m) + expf(p[u].y - m)) + (expf(p[u].z - m) + expf(p[u].w - m));
      }
      if (it < V) sum += expf(tail - m);
    } else {
      float p[CN_VALUES];
#pragma unroll
      for (int u = 0; u < CN_VALUES; ++u) {
        const int i = u * CN_THREADS + tid;
        p[u] = i < V ? row[i] : ninf;
      }
#pragma unroll
      for (int u = 0; u < CN_VALUES; ++u) m = fmaxf(m, p[u]);
      m = block_max<CN_WAVES>(m, red);
#pragma unroll
      for (int u = 0; u < CN_VALUES; ++u) {
        if (u * CN_THREADS + tid < V) sum += expf(p[u] - m);
      }
    }
    sum = block_sum<CN_WAVES>(sum, red);
    lse = m + logf(sum);
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < CN_WAVES; ++w) cn_take(sv[w], st[w], se[w], best, bt, be);
    out[r] = bt;
    len[r] += 1;
    const int ns = nxt[be];
    state[r] = ns;
    if (ns >= 0 && ns < n_states && off[ns + 1] <= off[ns]) {
      fin[r] = 1;
      choice[r] = label[ns];
    }
    if (score) score[r] += best - lse;
  }
}

}  // namespace

extern "C" int lhrs_constrain_rows(const float* logits, long ld, long* out, int n, int V, const int* off, const int* tok, const int* nxt,
                                   const int* label, int n_states, int n_edges, int pad_token_id, int* state, int* fin, int* len, int* choice,
                                   float* score, void* stream) {
  LHRS_REQUIRE(n >= 1, "constrain_rows: n=%d", n);
  LHRS_REQUIRE(V > 0 && V <= CN_MAXV, "constrain_rows: V=%d (a row is held in registers for the score: 1..%d)", V, CN_MAXV);
  LHRS_REQUIRE(logits != nullptr && ld >= V, "constrain_rows: logits=%p ld=%ld V=%d", (const void*)logits, ld, V);
  LHRS_REQUIRE(out != nullptr && state != nullptr && fin != nullptr && len != nullptr && choice != nullptr,
               "constrain_rows: out=%p state=%p fin=%p len=%p choice=%p (score alone may be NULL)", (void*)out, (void*)state, (void*)fin, (void*)len,
               (void*)choice);
  LHRS_REQUIRE(off != nullptr && tok != nullptr && nxt != nullptr && label != nullptr && n_states >= 1 && n_edges >= 1,
               "constrain_rows: automaton off=%p tok=%p nxt=%p label=%p n_states=%d n_edges=%d", (const void*)off, (const void*)tok, (const void*)nxt,
               (const void*)label, n_states, n_edges);
  const int vec = ld % 4 == 0 && ((uintptr_t)logits & 15) == 0;  // 16-B aligned rows
  hipLaunchKernelGGL(constrain_rows_kernel, dim3(n), dim3(CN_THREADS), 0, (hipStream_t)stream, logits, ld, out, V, vec, off, tok, nxt, label, n_states,
                     n_edges, pad_token_id, state, fin, len, choice, score);
  LHRS_CHECK_LAUNCH("constrain_rows");
  return 0;
}
