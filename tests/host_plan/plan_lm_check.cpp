// The decode plan of casr_beam_lm's caller (csrc/decode_plan.h PLAN_BEAM_LM) on the host, as a program
// of its own under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_decode_plan_lm_host.py
// builds and runs it): at every shape, option and blob it is casr_beam's plan with the caller changed
// and the select never fused, so the decode steps are casr_beam's at that shape and only the select
// differs.  (That casr_beam's own plans are unchanged is plan_check.cpp's business.)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "decode_plan.h"

using namespace casr;

#define CHECK(c)                                                              \
  do {                                                                        \
    if (!(c)) {                                                               \
      fprintf(stderr, "plan_lm_check: %s failed (line %d)\n", #c, __LINE__);  \
      exit(2);                                                                \
    }                                                                         \
  } while (0)

int main() {
  const AttnStaticLds lds{336, 336, 336, 336, 336};
  int plans = 0, folded = 0, unfused = 0;
  for (int V : {5004, 5003, 6000})
    for (float temperature : {1.0f, 0.5f})
      for (int B : {1, 6, 128, 256})
        for (int k : {0, 1, 2, 4, 8, 16, 17})
          for (int Tp : {33, 266})
            for (const BlobFacts& blob : {BlobFacts{1, 1, 1, 1}, BlobFacts{0, 1, 1, 1}, BlobFacts{1, 1, 0, 1}})
              for (int fuse : {0, 1})
                for (int kpb : {0, 4, 8}) {
                  casr_config cfg{};
                  cfg.vocab = V;
                  cfg.max_len = 40;
                  cfg.temperature = temperature;
                  Tuning t;
                  t.v[CASR_OPT_FUSE_SELECT] = fuse;
                  t.v[CASR_OPT_ATTN_KPB] = kpb;
                  const int VP = (V + 63) / 64 * 64;
                  const DecodePlan beam = plan_decode(PLAN_BEAM, B, Tp, k, false, cfg, VP, t, blob, lds);
                  const DecodePlan lm = plan_decode(PLAN_BEAM_LM, B, Tp, k, false, cfg, VP, t, blob, lds);
                  ++plans;
                  CHECK(lm.caller == PLAN_BEAM_LM && beam.caller == PLAN_BEAM);
                  CHECK(lm.status == beam.status);
                  CHECK((k < 1 || k > KMAX_BEAM) == (lm.status == PLAN_BAD_K));
                  CHECK(lm.fuse_select == 0);
                  DecodePlan same = lm;  // everything else: casr_beam's plan, byte for byte
                  same.caller = PLAN_BEAM;
                  same.fuse_select = beam.fuse_select;
                  CHECK(memcmp(&same, &beam, sizeof same) == 0);
                  folded += lm.fold;
                  unfused += beam.fuse_select;
                }
  CHECK(folded > 0 && unfused > 0);  // the folded step, and shapes where casr_beam fuses its select, occurred
  printf("plan_lm_check ok (%d plans, %d folded, %d where casr_beam fuses the select)\n", plans, folded, unfused);
  return 0;
}
