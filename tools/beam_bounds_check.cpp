// Host-side bounds of the beam-search entry points (csrc/beam.hip): every out-of-contract call must return -1 with a message BEFORE any HIP call,
// so this program needs no GPU.  Build it with the host sanitizers and run it:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I include \
//         tools/beam_bounds_check.cpp lhrs_bot_amd/csrc/beam.hip lhrs_bot_amd/csrc/lib.cpp -o beam_bounds_check && ./beam_bounds_check
#include <stdio.h>
#include <string.h>

#include "lhrs_hip.h"

static int failures = 0;

static void expect_rejected(int status, const char* needle, const char* what) {
  const char* msg = lhrs_last_error();
  if (status != -1 || msg == nullptr || strstr(msg, needle) == nullptr) {
    printf("FAIL %s: status %d, message '%s' (expected -1 and '%s')\n", what, status, msg ? msg : "(null)", needle);
    ++failures;
  } else {
    printf("ok   %s: %s\n", what, msg);
  }
}

int main() {
  // storage that a call COULD touch if a check were missing: the sanitizer then sees the access
  static float f[64];
  static int i[64];
  static long l[16];
  // beam_topk_rows
  expect_rejected(lhrs_beam_topk_rows(f, 40000, 4, 40000, 8, f, 1.f, nullptr, 8, nullptr, f, i, nullptr), "V=40000", "topk: V too large");
  expect_rejected(lhrs_beam_topk_rows(f, 32000, 4, 32000, 18, f, 1.f, nullptr, 8, nullptr, f, i, nullptr), "K=18", "topk: 2 * nb > 16");
  expect_rejected(lhrs_beam_topk_rows(f, 32000, 0, 32000, 8, f, 1.f, nullptr, 8, nullptr, f, i, nullptr), "n_rows=0", "topk: no rows");
  expect_rejected(lhrs_beam_topk_rows(f, 32000, 17, 32000, 8, f, 1.f, nullptr, 8, nullptr, f, i, nullptr), "n_rows=17", "topk: too many rows");
  expect_rejected(lhrs_beam_topk_rows(f, 6, 4, 6, 8, f, 1.f, nullptr, 8, nullptr, f, i, nullptr), "V=6", "topk: V < K");
  expect_rejected(lhrs_beam_topk_rows(f, 31999, 4, 32000, 8, f, 1.f, nullptr, 8, nullptr, f, i, nullptr), "ld=31999", "topk: ld < V");
  expect_rejected(lhrs_beam_topk_rows(nullptr, 32000, 4, 32000, 8, f, 1.f, nullptr, 8, nullptr, f, i, nullptr), "logits=", "topk: NULL logits");
  expect_rejected(lhrs_beam_topk_rows(f, 32000, 4, 32000, 8, f, 1.f, nullptr, 8, nullptr, nullptr, i, nullptr), "cand_score=", "topk: NULL output");
  expect_rejected(lhrs_beam_topk_rows(f, 32000, 4, 32000, 8, f, 1.3f, nullptr, 8, i, f, i, nullptr), "history", "topk: penalty without history");
  expect_rejected(lhrs_beam_topk_rows(f, 32000, 4, 32000, 8, f, 0.f, i, 8, i, f, i, nullptr), "repetition_penalty", "topk: penalty 0");
  // beam_step
  expect_rejected(lhrs_beam_step(f, i, 1, 9, 32000, 8, -1, 0, f, f, i, l, i, f, i, i, i, i, i, nullptr), "num_beams=9", "step: 2 * nb > 16");
  expect_rejected(lhrs_beam_step(f, i, 1, 1, 32000, 8, -1, 0, f, f, i, l, i, f, i, i, i, i, i, nullptr), "num_beams=1", "step: nb < 2");
  expect_rejected(lhrs_beam_step(f, i, 5, 4, 32000, 8, -1, 0, f, f, i, l, i, f, i, i, i, i, i, nullptr), "B=5", "step: B * nb > 16");
  expect_rejected(lhrs_beam_step(f, i, 1, 4, 40000, 8, -1, 0, f, f, i, l, i, f, i, i, i, i, i, nullptr), "V=40000", "step: V too large");
  expect_rejected(lhrs_beam_step(f, i, 1, 4, 32000, 0, -1, 0, f, f, i, l, i, f, i, i, i, i, i, nullptr), "max_new=0", "step: max_new 0");
  expect_rejected(lhrs_beam_step(f, i, 1, 4, 32000, 8, -1, 0, f, f, i, l, nullptr, f, i, i, i, i, i, nullptr), "NULL", "step: NULL history");
  expect_rejected(lhrs_beam_step(nullptr, i, 1, 4, 32000, 8, -1, 0, f, f, i, l, i, f, i, i, i, i, i, nullptr), "NULL", "step: NULL candidates");
  expect_rejected(lhrs_beam_step(f, i, 1, 4, 32000, 8, -1, 0, f, f, i, l, i, f, i, i, i, i, nullptr, nullptr), "NULL", "step: NULL state");
  // kv_beam_reorder
  expect_rejected(lhrs_kv_beam_reorder(l, 4, 1, 9, 16, 256, i, 3, nullptr, 5, 4, nullptr, nullptr), "num_beams=9", "reorder: nb > 8");
  expect_rejected(lhrs_kv_beam_reorder(l, 4, 9, 2, 16, 256, i, 3, nullptr, 5, 4, nullptr, nullptr), "B=9", "reorder: B * nb > 16");
  expect_rejected(lhrs_kv_beam_reorder(l, 0, 1, 4, 16, 256, i, 3, nullptr, 5, 4, nullptr, nullptr), "n_caches=0", "reorder: no caches");
  expect_rejected(lhrs_kv_beam_reorder(l, 4, 1, 4, 16, 12, i, 3, nullptr, 5, 4, nullptr, nullptr), "d=12", "reorder: d not a multiple of 8");
  expect_rejected(lhrs_kv_beam_reorder(l, 4, 1, 4, 16, 256, i, 10, nullptr, 12, 8, nullptr, nullptr), "max_pos=8", "reorder: grid past max_ctx");
  expect_rejected(lhrs_kv_beam_reorder(l, 4, 1, 4, 16, 256, i, 3, nullptr, 9, 4, nullptr, nullptr), "t1=9", "reorder: t1 past the grid");
  expect_rejected(lhrs_kv_beam_reorder(l, 4, 1, 4, 16, 256, i, 3, nullptr, 2, 4, nullptr, nullptr), "t1=2", "reorder: t1 < t0");
  expect_rejected(lhrs_kv_beam_reorder(nullptr, 4, 1, 4, 16, 256, i, 3, nullptr, 5, 4, nullptr, nullptr), "table=", "reorder: NULL table");
  expect_rejected(lhrs_kv_beam_reorder(l, 4, 1, 4, 16, 256, nullptr, 3, nullptr, 5, 4, nullptr, nullptr), "parent=", "reorder: NULL parents");
  printf("%s: %d failure(s)\n", failures ? "FAILED" : "PASSED", failures);
  return failures ? 1 : 0;
}
