// csrc/confusion_plan.h under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU: a program of its
// own (tests/test_confusion_host_sanitizer.py builds and runs it).  Every array sits in a heap buffer of
// exactly its size; the token array ends with the last token of the last valid record, so a read past a
// record's length there is a heap-buffer-overflow.  Case file: int32 cases, then per case int32 L, k, V, M,
// N, pivot, three doubles (scale, lm_weight, length_weight), int64 ntok, tokens [ntok], valid [L k], unit
// [L k] int64, score [L k], lm [L k].  Output: three text lines per case (C, U, N).
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "confusion_plan.h"

using namespace casr;

template <class T>
static T* read_exact(FILE* f, size_t n) {
  T* p = static_cast<T*>(std::malloc(n ? n * sizeof(T) : 1));
  if (n && std::fread(p, sizeof(T), n, f) != n) {
    std::fprintf(stderr, "confusion_check: short case file\n");
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

template <class T>
static T* heap(size_t n) {
  return static_cast<T*>(std::malloc(n ? n * sizeof(T) : 1));
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  FILE* o = std::fopen(argv[2], "w");
  if (!f || !o) return 2;
  const int32_t cases = read_one<int32_t>(f);
  for (int32_t ci = 0; ci < cases; ++ci) {
    const int32_t L = read_one<int32_t>(f), k = read_one<int32_t>(f), V = read_one<int32_t>(f);
    const int32_t M = read_one<int32_t>(f), N = read_one<int32_t>(f), pivot = read_one<int32_t>(f);
    const double scale = read_one<double>(f), lmw = read_one<double>(f), lw = read_one<double>(f);
    const size_t LK = (size_t)L * k, SM = (size_t)cn_slots(L);
    const int64_t ntok = read_one<int64_t>(f);
    int32_t* tok = read_exact<int32_t>(f, (size_t)ntok);
    uint8_t* valid = read_exact<uint8_t>(f, LK);
    int64_t* unit = read_exact<int64_t>(f, LK);
    float* score = read_exact<float>(f, LK);
    float* lm = read_exact<float>(f, LK);
    int32_t* st = heap<int32_t>(SM * M);
    int64_t* sm = heap<int64_t>(SM * M);
    int64_t* pm = heap<int64_t>(L);
    int64_t total = -1;
    const int32_t ns = cn_confusion_utterance_host(tok, valid, unit, pivot, L, k, V, M, st, sm, pm, &total);
    std::fprintf(o, "C %d %lld", ns, (long long)total);
    for (size_t e = 0; e < SM * M; ++e) std::fprintf(o, " %d %lld", st[e], (long long)sm[e]);
    for (int i = 0; i < L; ++i) std::fprintf(o, " %lld", (long long)pm[i]);
    std::fprintf(o, "\n");
    int64_t* u = heap<int64_t>(LK);
    const int64_t U = cn_units_utterance_host(score, valid, lm, L, k, scale, lmw, lw, u);
    std::fprintf(o, "U %lld", (long long)U);
    for (size_t i = 0; i < LK; ++i) std::fprintf(o, " %lld", (long long)u[i]);
    std::fprintf(o, "\n");
    int32_t* ni = heap<int32_t>(N);
    int32_t* nt = heap<int32_t>((size_t)N * L);
    int32_t* nl = heap<int32_t>(N);
    double* nc = heap<double>(N);
    cn_nbest_utterance_host(tok, score, valid, lm, L, k, N, lmw, lw, ni, nt, nl, nc);
    std::fprintf(o, "N");
    for (int r = 0; r < N; ++r) std::fprintf(o, " %d %d %a", ni[r], nl[r], nc[r]);
    for (size_t e = 0; e < (size_t)N * L; ++e) std::fprintf(o, " %d", nt[e]);
    std::fprintf(o, "\n");
    for (void* p : {(void*)tok, (void*)valid, (void*)unit, (void*)score, (void*)lm, (void*)st, (void*)sm, (void*)pm,
                    (void*)u, (void*)ni, (void*)nt, (void*)nl, (void*)nc})
      std::free(p);
  }
  // the plan's arithmetic at its corners (UBSan: no overflow), and its limits
  const ConfusionPlan a = confusion_plan(256, 40, 16, 5056, true);
  const ConfusionPlan b = confusion_plan(65535, CN_MAX_LEN, CN_MAX_K, 16000, true);
  const ConfusionPlan c = confusion_plan(1, CN_MAX_LEN + 1, 1, 10, false);
  const ConfusionPlan d = confusion_plan(1, 10, 4, CN_MAX_VOCAB, false);
  if (!a.ok || a.lanes != CN_WAVE || a.align_groups != 10 || a.align_lds > EDIT_LDS_DEFAULT ||
      a.votes_bytes != (size_t)2 * 256 * 81 * 640 || a.ws_bytes < a.votes_bytes)
    return 3;
  if (!b.ok || b.lanes < 1 || b.lanes >= CN_WAVE || b.align_lds > EDIT_LDS_LIMIT || !b.align_raise || !b.reduce_raise)
    return 4;
  if (c.ok || d.ok) return 5;
  std::fclose(f);
  std::fclose(o);
  std::printf("confusion_check ok\n");
  return 0;
}
