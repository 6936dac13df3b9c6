// Sweep of csrc/attn_plan.h on the CPU: every entry, head_dim 64 / 128, every max_q and max_kv in 0..704, every LTq from pad64(max_q) to 2048, rope on / off
// where the entry takes it, both store widths.  Each plan must have between 1 and ATTN_PLAN_CAP launches, list no kernel twice, keep the
// resident dQ kernel in front of any dK/dV kernel, and match the rules restated below.  Prints the number of plans and the longest one.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/attn_plan_sweep.cpp -o /tmp/attn_plan_sweep && /tmp/attn_plan_sweep
#include <cstdio>
#include <cstdlib>

#include "../lhrs_bot_amd/csrc/attn_plan.h"

using namespace attn_plan_h;

#define CHECK(cond)                                                                                                                        \
  do {                                                                                                                                     \
    if (!(cond)) {                                                                                                                         \
      std::printf("FAILED %s: entry %d D %d max_q %d max_kv %d LTq %d rope %d wide %d\n", #cond, p.entry, p.D, p.max_q, p.max_kv, p.LTq,     \
                  (int)p.has_rope, (int)p.out_wide);                                                                                       \
      return 1;                                                                                                                            \
    }                                                                                                                                      \
  } while (0)

int main() {
  long plans = 0;
  int longest = 0;
  AttnProblem longest_p{};
  for (int entry = 0; entry < AE_COUNT; ++entry)
    for (int D = 64; D <= 128; D += 64)
      for (int max_q = 0; max_q <= 704; ++max_q)
        for (int max_kv = 0; max_kv <= 704; ++max_kv)
          for (int LTq = (max_q + 63) / 64 * 64; LTq <= 2048; LTq += 64)
            for (int rope = entry == AE_BWD_ROPE; rope <= (entry == AE_BWD_ROPE || entry == AE_BWD_O); ++rope)
              for (int wide = 0; wide <= 1; ++wide) {
                const AttnProblem p{entry, D, max_q, max_kv, LTq, rope != 0, wide != 0};
                const AttnPlan plan = attn_plan(p);
                const int n = plan.n;
                ++plans;
                CHECK(n >= 1 && n <= ATTN_PLAN_CAP);
                int seen = 0, pos[AK_COUNT];
                for (int k = 0; k < AK_COUNT; ++k) pos[k] = -1;
                for (int i = 0; i < n; ++i) {
                  const int k = plan.kernels[i];
                  CHECK(k >= 0 && k < AK_COUNT && !(seen >> k & 1));
                  seen |= 1 << k;
                  pos[k] = i;
                }
                const bool fwd = entry == AE_FWD || entry == AE_FWD_KMASK;
                const int R = attn_res_rows(D);
                CHECK(plan.wide == p.out_wide);
                if (fwd) {
                  CHECK(n == 1 && !plan.rope_fused && !plan.delta_by_dq);
                  CHECK(plan.kernels[0] == (entry == AE_FWD && max_kv > 0 && max_kv <= R ? AK_FWD_RES : AK_FWD_TILED));
                } else {
                  CHECK((pos[AK_DQ_RES] >= 0) != (pos[AK_DQ_TILED] >= 0) && (pos[AK_DKV_RES] >= 0) != (pos[AK_DKV_TILED] >= 0));
                  CHECK((pos[AK_DQ_RES] >= 0) == (max_kv <= R));
                  if (pos[AK_DQ_RES] >= 0) CHECK(pos[AK_DQ_RES] < (pos[AK_DKV_RES] >= 0 ? pos[AK_DKV_RES] : pos[AK_DKV_TILED]));
                  CHECK(plan.delta_by_dq == (entry == AE_BWD_O && pos[AK_DQ_RES] >= 0));
                  CHECK((pos[AK_DELTA] == 0) == (entry == AE_BWD_O && !plan.delta_by_dq) && pos[AK_DELTA] <= 0);
                  CHECK(plan.rope_fused == (rope && pos[AK_DQ_RES] >= 0 && pos[AK_DKV_RES] >= 0));
                  const bool passes = rope && !plan.rope_fused;
                  CHECK((pos[AK_ROPE_DQ] == n - 2) == passes && (pos[AK_ROPE_DK] == n - 1) == passes);
                  CHECK(passes || (pos[AK_ROPE_DQ] < 0 && pos[AK_ROPE_DK] < 0));
                  CHECK(pos[AK_FWD_RES] < 0 && pos[AK_FWD_TILED] < 0);
                }
                if (n > longest) { longest = n; longest_p = p; }
              }
  const AttnProblem bad[] = {{AE_FWD, 96, 64, 64, 64, false, true}, {AE_COUNT, 128, 64, 64, 64, false, true}, {-1, 128, 64, 64, 64, false, true},
                             {AE_BWD_ROPE, 128, 64, 64, 64, false, true}};
  for (const AttnProblem& p : bad) CHECK(attn_plan(p).n == -1);
  std::printf("attn_plan sweep ok: %ld plans, longest %d launches (entry %d D %d max_q %d max_kv %d LTq %d rope %d)\n", plans, longest, longest_p.entry,
              longest_p.D, longest_p.max_q, longest_p.max_kv, longest_p.LTq, (int)longest_p.has_rope);
  return 0;
}
