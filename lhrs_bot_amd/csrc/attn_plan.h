// Host-only planner of the attention dispatch: which kernels one call of an entry point of attention.hip launches, in which order, and the three
// facts the kernels are told.  Plain C++, no HIP: attn_plan() is a pure function of AttnProblem - no device, no state, no pointer dereferenced -
// so the dispatch is checkable without a GPU (lhrs_attn_plan; tests/attention_cases.py::path_of restates it).  attention.hip runs the plan.
#pragma once

namespace attn_plan_h {

// rows of ONE operand matrix the resident kernels keep in the LDS: 160 KiB hold two [rows, D] bf16 matrices (320 at D = 128, 640 at D = 64)
constexpr int attn_res_rows(int D) { return 163840 / (2 * D * 2); }

enum AttnEntry { AE_FWD, AE_FWD_KMASK, AE_BWD, AE_BWD_ROPE, AE_BWD_O, AE_COUNT };
// One call.  max_q / max_kv: the longest q_len / kv_rows of the descriptors; LTq: row length of lse / delta.  has_rope: cos / sin tables were
// given (lhrs_attn_bwd_rope always, lhrs_attn_bwd_o when cos_t != nullptr; the other entries take none).  out_wide: every output row of the
// call can leave as 16-byte stores (row strides % 8 == 0 elements, pointers % 16 == 0 bytes).
struct AttnProblem { int entry, D, max_q, max_kv, LTq; bool has_rope, out_wide; };
enum AttnKernel { AK_DELTA, AK_FWD_RES, AK_FWD_TILED, AK_DQ_RES, AK_DQ_TILED, AK_DKV_RES, AK_DKV_TILED, AK_ROPE_DQ, AK_ROPE_DK, AK_COUNT };
inline const char* attn_kernel_name(int k) {
  static const char* const name[AK_COUNT] = {"delta", "fwd_res", "fwd_tiled", "dq_res", "dq_tiled", "dkv_res", "dkv_tiled", "rope_dq", "rope_dk"};
  return k >= 0 && k < AK_COUNT ? name[k] : "?";
}
// The longest plan: delta kernel, dQ, dK/dV, lhrs_rope over dq, lhrs_rope over dk.
constexpr int ATTN_PLAN_CAP = 5;
// kernels[0 .. n) in launch order (n = -1: the problem was rejected).  wide: the resident kernels store 16-byte rows.  rope_fused: the inverse
// RoPE rides in the resident kernels' stores.  delta_by_dq: the resident dQ kernel computes delta = rowsum(dO * O) and writes it for the dK/dV
// kernel behind it.
struct AttnPlan {
  int n = 0, kernels[ATTN_PLAN_CAP] = {};
  bool wide = false, rope_fused = false, delta_by_dq = false;
  void add(int k) {
    if (n < ATTN_PLAN_CAP) kernels[n] = k;
    ++n;  // past the cap: counted, not stored - attn_plan rejects the plan
  }
};

// n = -1: rejected (head_dim, entry, lhrs_attn_bwd_rope without tables; or a plan longer than ATTN_PLAN_CAP, which no rule produces today)
inline AttnPlan attn_plan(const AttnProblem& p) {
  AttnPlan out;
  if ((p.D != 64 && p.D != 128) || p.entry < 0 || p.entry >= AE_COUNT || (p.entry == AE_BWD_ROPE && !p.has_rope)) { out.n = -1; return out; }
  const long R = attn_res_rows(p.D);
  out.wide = p.out_wide;
  if (p.entry == AE_FWD || p.entry == AE_FWD_KMASK) {
    // both operands fit one CU's LDS; the key mask lives in the tiled kernel only
    out.add(p.entry == AE_FWD && p.max_kv > 0 && p.max_kv <= R ? AK_FWD_RES : AK_FWD_TILED);
    return out;
  }
  const bool rope = p.has_rope && p.entry != AE_BWD;
  const bool dq_res = p.max_kv <= R;
  // the resident dK/dV kernel keeps lse | delta of the sequence (2 x LTq floats) behind its Q image (rows rounded up to 32): head_dim 128 up
  // to 288 queries
  const bool dkv_res = p.max_q <= R && (long)((p.max_q + 31) / 32 * 32) * p.D * 2 + 2L * p.LTq * 4 <= R * p.D * 2;
  out.rope_fused = rope && dq_res && dkv_res;             // both resident kernels run; otherwise two lhrs_rope passes behind the tiled launches
  out.delta_by_dq = p.entry == AE_BWD_O && dq_res;        // lhrs_attn_bwd_o: delta is an output - of the resident dQ kernel, else of a launch of its own
  if (p.entry == AE_BWD_O && !dq_res) out.add(AK_DELTA);
  // The resident dQ kernel stays in front of any dK/dV kernel (which reads the delta it writes); the resident launches go out first.
  if (dq_res) out.add(AK_DQ_RES);
  if (dkv_res) out.add(AK_DKV_RES);
  if (!dq_res) out.add(AK_DQ_TILED);
  if (!dkv_res) out.add(AK_DKV_TILED);
  if (rope && !out.rope_fused) { out.add(AK_ROPE_DQ); out.add(AK_ROPE_DK); }
  if (out.n > ATTN_PLAN_CAP) out.n = -1;  // a rule change outgrew the cap
  return out;
}

}  // namespace attn_plan_h
