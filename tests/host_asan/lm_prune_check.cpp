// csrc/lm_prune_plan.h under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU
// (tests/test_lm_prune_host_sanitizer.py).  A program of its own: it includes the header, runs a few
// built-in edge cases, then reads a model and two sweeps from a file into exact-size heap buffers,
// prunes the model and writes what it found, which the test compares with the library's host entry and
// with the Python restatement bit for bit.
//   lm_prune_check <in> <out>
//   in : int32 order, V; float64 theta; per order: int64 count, int64 have (= count n, or one less for
//        the check that the sanitizer is live), int32 ids [have], float32 prob [count], float32 backoff
//        [count]; int64 nx, float64 x [nx]; int64 ny, float64 y [ny]
//   out: float64 tau; int64 removed_any, n_degenerate; per order: int64 count, uint64 key, float64 delta,
//        uint8 kept, float64 b64, float32 backoff (each [count]); float64 exp10(x) [nx]; float64 log(y) [ny]
#include <stdio.h>
#include <stdlib.h>

#include <memory>

#include "lm_prune_plan.h"

using namespace casr;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "lm_prune_check: %s (line %d)\n", #c, __LINE__); \
      exit(2);                                                    \
    }                                                             \
  } while (0)

template <class T>
static std::unique_ptr<T[]> take(FILE* f, size_t n) {
  std::unique_ptr<T[]> p(new T[n]);  // exact size: one element past is the sanitizer's
  CHECK(fread(p.get(), sizeof(T), n, f) == n);
  return p;
}
template <class T>
static void put(FILE* f, const T* p, size_t n) {
  CHECK(fwrite(p, sizeof(T), n, f) == n);
}

static void edge_cases() {
  CHECK(lmp_exp10(0.0) == 1.0 && lmp_exp10(-400.0) == 0.0 && lmp_exp10(400.0) > 1e308);
  CHECK(lmp_log(1.0) == 0.0 && lmp_log(0.0) != lmp_log(0.0) && lmp_log(-1.0) != lmp_log(-1.0));
  CHECK(lmp_log(4.9e-324) < -744.0 && lmp_log(4.9e-324) > -745.0);  // a subnormal
  double s[LMP_LANES] = {};
  CHECK(lmp_tree(s) == 0.0);
  CHECK(lmp_backoff(1.0, 0.5) == 0.0 && lmp_backoff(0.5, 1.5) == 0.0 && lmp_backoff(0.0, 0.0) == 1.0);
  const double inf = lmp_from_bits(0x7ff0000000000000ull);
  CHECK(lmp_delta(1.0, 0.0, 0.1, 1.0, 0.5, 0.5) == inf && lmp_delta(1.0, 0.1, 0.1, 1.0, -0.2, 0.5) == inf);
  // an order-1 model: nothing to decide, everything comes back
  const int32_t ids[3] = {0, 1, 2};
  const float prob[3] = {-0.5f, -0.4f, -0.6f}, back[3] = {-0.1f, 0.f, -0.2f};
  const int64_t count[1] = {3};
  const int32_t* idp[1] = {ids};
  const float *pp[1] = {prob}, *bp[1] = {back};
  NgramTables t;
  NgramSuccTables st;
  CHECK(ngram_build(1, 3, count, idp, pp, bp, &t, nullptr) == NGRAM_OK);
  ngram_succ_build(t, count, idp, pp, &st);
  LmpResult r;
  CHECK(lmp_prune_host(t, st, lmp_dims(t, st, count, false), 0.1, &r));
  CHECK(!r.removed_any && r.count_out[0] == 3 && r.key[0].size() == 3);
}

int main(int argc, char** argv) {
  CHECK(argc == 3);
  edge_cases();
  FILE* f = fopen(argv[1], "rb");
  CHECK(f);
  const auto head = take<int32_t>(f, 2);
  const int order = head[0], V = head[1];
  CHECK(order >= 1 && order <= NGRAM_MAX_ORDER);
  const double theta = take<double>(f, 1)[0];
  int64_t count[NGRAM_MAX_ORDER] = {};
  std::unique_ptr<int32_t[]> ids[NGRAM_MAX_ORDER];
  std::unique_ptr<float[]> prob[NGRAM_MAX_ORDER], back[NGRAM_MAX_ORDER];
  const int32_t* idp[NGRAM_MAX_ORDER] = {};
  const float *pp[NGRAM_MAX_ORDER] = {}, *bp[NGRAM_MAX_ORDER] = {};
  bool unk = false;
  for (int n = 1; n <= order; ++n) {
    count[n - 1] = take<int64_t>(f, 1)[0];
    // the id array may have been written one id short: the build must then read past it
    const int64_t have = take<int64_t>(f, 1)[0];
    ids[n - 1] = take<int32_t>(f, (size_t)have);
    prob[n - 1] = take<float>(f, (size_t)count[n - 1]);
    back[n - 1] = take<float>(f, (size_t)count[n - 1]);
    idp[n - 1] = ids[n - 1].get();
    pp[n - 1] = prob[n - 1].get();
    bp[n - 1] = back[n - 1].get();
  }
  const int64_t nx = take<int64_t>(f, 1)[0];
  const auto xs = take<double>(f, (size_t)nx);
  const int64_t ny = take<int64_t>(f, 1)[0];
  const auto ys = take<double>(f, (size_t)ny);
  fclose(f);
  NgramTables t;
  NgramSuccTables st;
  CHECK(ngram_build(order, V, count, idp, pp, bp, &t, nullptr) == NGRAM_OK);
  ngram_succ_build(t, count, idp, pp, &st);
  for (int64_t i = 0; i < count[0]; ++i) unk = unk || ids[0][i] == V + 2;
  const LmpDims d = lmp_dims(t, st, count, unk);
  LmpResult r;
  CHECK(lmp_prune_host(t, st, d, theta, &r));
  FILE* o = fopen(argv[2], "wb");
  CHECK(o);
  put(o, &r.tau, 1);
  const int64_t two[2] = {r.removed_any ? 1 : 0, r.n_degenerate};
  put(o, two, 2);
  for (int n = 1; n <= order; ++n) {
    const int64_t c = (int64_t)r.key[n - 1].size();
    put(o, &c, 1);
    put(o, r.key[n - 1].data(), (size_t)c);
    put(o, r.delta[n - 1].data(), (size_t)c);
    put(o, r.kept[n - 1].data(), (size_t)c);
    put(o, r.out_b64[n - 1].data(), (size_t)c);
    put(o, r.out_backoff[n - 1].data(), (size_t)c);
  }
  for (int64_t i = 0; i < nx; ++i) {
    const double v = lmp_exp10(xs[i]);
    put(o, &v, 1);
  }
  for (int64_t i = 0; i < ny; ++i) {
    const double v = lmp_log(ys[i]);
    put(o, &v, 1);
  }
  fclose(o);
  printf("lm_prune_check ok\n");
  return 0;
}
