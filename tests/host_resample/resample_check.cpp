// Stand-alone host check of chinese-asr_amd/csrc/resample_design.h (built from that header alone,
// under AddressSanitizer + UndefinedBehaviorSanitizer, by tests/test_convert_host.py): every rate's
// plan and table, the table built into a heap buffer of exactly L x taps floats (so a write past a
// row or the table is caught), the row sums, the tile span the kernel stages against the span its
// outputs really read, and an FNV-1a checksum of each table that the test compares with the
// library's casr_resample_filter.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>

#include "resample_design.h"

using namespace casr;

static int fails = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      ++fails;                           \
      printf("FAIL %s: ", #cond);        \
      printf(__VA_ARGS__);               \
      printf("\n");                      \
    }                                    \
  } while (0)

static uint64_t fnv1a(const void* p, size_t n) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

int main(int argc, char** argv) {
  const int rates[] = {8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 96000, 4000, 384000, 16000};
  for (int rate : rates) {
    ResamplePlan p;
    const int rc = resample_plan(rate, &p);
    CHECK(rc == RS_OK, "rate %d rc %d", rate, rc);
    if (rc != RS_OK) continue;
    CHECK(p.L * (int64_t)rate == p.M * (int64_t)RS_RATE_OUT, "rate %d L %d M %d", rate, p.L, p.M);
    CHECK(p.taps == 2 * p.K && p.K >= p.hw && p.K - 1 < p.hw, "rate %d K %d hw %g", rate, p.K, p.hw);
    const size_t nf = p.table_floats();
    std::unique_ptr<float[]> tab(new float[nf]);  // exact size
    resample_filter(p, tab.get());
    for (int ph = 0; ph < p.L; ++ph) {
      double s = 0;
      for (int i = 0; i < p.taps; ++i) s += tab[(size_t)ph * p.taps + i];
      CHECK(fabs(s - 1.0) < 2e-6, "rate %d phase %d sum %.9g", rate, ph, s);
    }
    // the span a tile stages covers what its outputs read, wherever the tile starts
    const int span = resample_span(p);
    for (int64_t m0 : {(int64_t)0, (int64_t)RS_TILE, (int64_t)7 * RS_TILE, (int64_t)1 << 30}) {
      const int64_t lo = (m0 * p.M) / p.L - p.K + 1;
      const int64_t hi = ((m0 + RS_TILE - 1) * p.M) / p.L + p.K;
      CHECK(hi - lo + 1 <= span, "rate %d m0 %lld needs %lld > span %d", rate, (long long)m0, (long long)(hi - lo + 1), span);
      // the 32-bit form of a lane's position (convert.hip): p0 + dm M = q L + ph
      const int64_t base0 = (m0 * p.M) / p.L;
      const uint32_t p0 = (uint32_t)(m0 * p.M - base0 * p.L);
      for (int dm : {0, 1, RS_TILE / 2, RS_TILE - 1}) {
        const uint32_t d = p0 + (uint32_t)dm * (uint32_t)p.M;
        const int64_t pos = (m0 + dm) * p.M;
        CHECK(base0 + d / (uint32_t)p.L == pos / p.L && d % (uint32_t)p.L == (uint32_t)(pos % p.L), "rate %d m %lld", rate,
              (long long)(m0 + dm));
      }
    }
    CHECK(resample_lds_bytes(p) <= 64 * 1024, "rate %d lds %zu", rate, resample_lds_bytes(p));
    CHECK(resample_frames(0, p) == 0 && resample_frames(1, p) == (p.L + p.M - 1) / p.M, "rate %d frames", rate);
    printf("table %d %d %d %d %016llx\n", rate, p.L, p.M, p.taps, (unsigned long long)fnv1a(tab.get(), nf * sizeof(float)));
  }
  ResamplePlan q;
  CHECK(resample_plan(3999, &q) == RS_BAD_RATE, "3999");
  CHECK(resample_plan(384001, &q) == RS_BAD_RATE, "384001");
  CHECK(resample_plan(44101, &q) == RS_TABLE_TOO_LARGE && q.L == 16000, "44101 L %d", q.L);
  CHECK(fabs(bessel_i0(0.0) - 1.0) == 0.0 && fabs(bessel_i0(9.0) / 1093.5883545113745 - 1.0) < 1e-13, "I0(9) = %.16g",
        bessel_i0(9.0));
  (void)argc;
  (void)argv;
  if (fails) {
    printf("resample_check: %d failures\n", fails);
    return 1;
  }
  printf("resample_check ok\n");
  return 0;
}
