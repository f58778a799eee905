// csrc/edit_plan.h under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU: a program of its
// own (tests/test_edit_host_sanitizer.py builds and runs it).  Every row is read into a heap buffer of
// exactly the symbols the case file holds for it, so a read past a row's length is a
// heap-buffer-overflow.  Case file: int32 pairs, then per pair int32 m, n, int64 na, a[na], int64 nb,
// b[nb]; then int32 sets, per set int32 L, k, three doubles (scale, lm_weight, length_weight) and the
// arrays tokens [L k][L], score, valid, lm [L k].  Output: one text line per case.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "edit_plan.h"

using namespace casr;

template <class T>
static T* read_exact(FILE* f, size_t n) {
  T* p = static_cast<T*>(std::malloc(n ? n * sizeof(T) : 1));
  if (n && std::fread(p, sizeof(T), n, f) != n) {
    std::fprintf(stderr, "edit_check: short case file\n");
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
  const int32_t pairs = read_one<int32_t>(f);
  for (int32_t i = 0; i < pairs; ++i) {
    const int32_t m = read_one<int32_t>(f), n = read_one<int32_t>(f);
    const int64_t na = read_one<int64_t>(f);
    int32_t* a = read_exact<int32_t>(f, (size_t)na);
    const int64_t nb = read_one<int64_t>(f);
    int32_t* b = read_exact<int32_t>(f, (size_t)nb);
    int32_t ops[3] = {-1, -1, -1};
    const int32_t d = edit_distance_rows(a, m, b, n, ops);
    const int32_t d2 = edit_distance_rows(a, m, b, n, nullptr);
    std::fprintf(o, "P %d %d %d %d %d\n", d, d2, ops[0], ops[1], ops[2]);
    std::free(a);
    std::free(b);
  }
  const int32_t sets = read_one<int32_t>(f);
  for (int32_t i = 0; i < sets; ++i) {
    const int32_t L = read_one<int32_t>(f), k = read_one<int32_t>(f);
    const double scale = read_one<double>(f), lmw = read_one<double>(f), lw = read_one<double>(f);
    const size_t LK = (size_t)L * k;
    int32_t* tok = read_exact<int32_t>(f, LK * L);
    float* score = read_exact<float>(f, LK);
    uint8_t* valid = read_exact<uint8_t>(f, LK);
    float* lm = read_exact<float>(f, LK);
    double* risk = static_cast<double*>(std::malloc(LK * sizeof(double)));
    const int32_t best = mbr_utterance_host(tok, score, valid, lm, L, k, scale, lmw, lw, risk);
    std::fprintf(o, "M %d", best);
    for (size_t j = 0; j < LK; ++j) std::fprintf(o, " %a", risk[j]);
    std::fprintf(o, "\n");
    std::free(tok);
    std::free(score);
    std::free(valid);
    std::free(lm);
    std::free(risk);
  }
  // the plan's arithmetic at its corners (UBSan: no overflow)
  const EditPlan p = edit_plan_pairs(EDIT_MAX_LEN, EDIT_MAX_LEN, 1 << 30, true);
  const EditPlan q = edit_plan_mbr(EDIT_MBR_MAX_LEN, 1 << 20, 0);
  if (p.form != EDIT_FORM_WAVE || !p.raise_lds || q.form != EDIT_FORM_NONE) return 3;
  std::fclose(f);
  std::fclose(o);
  std::printf("edit_check ok\n");
  return 0;
}
