// csrc/align_plan.h under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU: a program of its
// own (tests/test_align_host_sanitizer.py builds and runs it).  Every utterance's weights are read into
// a heap buffer of exactly the values the case file holds for it ([n][T], row-major), so a read past
// a length is a heap-buffer-overflow.  Case file: int32 cases, then per case int32 L, T, n, int64
// count, float a[count].  Output: one text line per case: score, then first, last, peak [L].
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "align_plan.h"

using namespace casr;

template <class T>
static T* read_exact(FILE* f, size_t n) {
  T* p = static_cast<T*>(std::malloc(n ? n * sizeof(T) : 1));
  if (n && std::fread(p, sizeof(T), n, f) != n) {
    std::fprintf(stderr, "align_check: short case file\n");
    std::exit(2);
  }
  return p;
}

template <class T>
static T read_one(FILE* f) {
  T* p = read_exact<T>(f, 1);
  const T v = *p;
  std::free(p);
  return v;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  FILE* o = std::fopen(argv[2], "w");
  if (!f || !o) return 2;
  const int32_t cases = read_one<int32_t>(f);
  for (int32_t i = 0; i < cases; ++i) {
    const int32_t L = read_one<int32_t>(f), T = read_one<int32_t>(f), n = read_one<int32_t>(f);
    const int64_t count = read_one<int64_t>(f);
    float* a = read_exact<float>(f, (size_t)count);
    int32_t* out = static_cast<int32_t*>(std::malloc(sizeof(int32_t) * 3 * (size_t)L));
    const int32_t s = align_path_utterance(a, (size_t)T, 1, T, n, L, out, out + L, out + 2 * L);
    std::fprintf(o, "%d", s);
    for (int32_t j = 0; j < 3 * L; ++j) std::fprintf(o, " %d", out[j]);
    std::fprintf(o, "\n");
    std::free(a);
    std::free(out);
  }
  // the plan's arithmetic at its corners (UBSan: no overflow), and the limit the header states
  const AlignPlan big = align_plan(1 << 30, ALIGN_MAX_L, ALIGN_MAX_TP, 0);
  const AlignPlan usual = align_plan(256, 41, 266, 0);
  const AlignPlan asked = align_plan(256, 41, 266, ALIGN_GROUP_MAX);
  if (big.group != 1 || !big.raise_lds || big.lds_bytes > ALIGN_LDS_LIMIT) return 3;
  if (usual.group != ALIGN_GROUP_DEFAULT || usual.grid != 64 || usual.raise_lds) return 3;
  if (asked.group != ALIGN_GROUP_MAX || asked.grid != 16 || !asked.raise_lds || asked.lds_bytes > ALIGN_LDS_LIMIT) return 3;
  if (align_plan(1, 1, ALIGN_MAX_TP + 1, 0).group || align_plan(1, ALIGN_MAX_L + 1, 1, 0).group ||
      align_plan(1, 1, 1, 3).group || align_plan(0, 1, 1, 0).group)
    return 3;
  if ((int64_t)3072 * (ALIGN_MAX_L + 2 * ALIGN_MAX_TP) >= -(int64_t)ALIGN_NEG) return 3;
  std::fclose(f);
  std::fclose(o);
  std::printf("align_check ok\n");
  return 0;
}
