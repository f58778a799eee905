// csrc/ngram_table.h under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (host
// code only; tests/test_ngram_host_sanitizer.py builds and runs it).  Every input array lives in a heap
// buffer of exactly the size the file states, so a read past what the build or a query may touch is a
// sanitizer report.
//   ngram_check <model.bin> <scores.bin>
// model.bin: int32 order, vocab; per order int64 count, then three arrays (ids, prob, backoff), each
// int64 element count + the elements; then int32 n, L, bos, tokens [n][L] int32, lens [n] int32.
// scores.bin: the n sentence scores (float32).  Built-in edge cases run first.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "ngram_table.h"

using namespace casr;

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "ngram_check: %s failed (line %d)\n", #c, __LINE__); \
      exit(2);                                                     \
    }                                                              \
  } while (0)

template <class T>
static std::unique_ptr<T[]> read_array(FILE* f, int64_t* n) {
  CHECK(fread(n, sizeof *n, 1, f) == 1);
  std::unique_ptr<T[]> p(new T[(size_t)*n]);  // exact size: no slack behind the data
  if (*n) CHECK(fread(p.get(), sizeof(T), (size_t)*n, f) == (size_t)*n);
  return p;
}

// exact-size copies of small literal arrays
template <class T>
static std::unique_ptr<T[]> heap(std::initializer_list<T> v) {
  std::unique_ptr<T[]> p(new T[v.size()]);
  size_t i = 0;
  for (T x : v) p[i++] = x;
  return p;
}

static void edge_cases() {
  const int V = 5004;
  // one n-gram at every order above 1; ids V - 1, V (<s>), V + 1 (</s>), V + 2 (<unk>) inside n-grams
  auto u = heap<int32_t>({7, V - 1, V, V + 1});
  auto up = heap<float>({-1.f, -2.f, -0.5f, -1.5f});
  auto ub = heap<float>({-0.25f, -0.125f, -0.5f, 0.f});
  auto b2 = heap<int32_t>({V, V - 1});
  auto p2 = heap<float>({-0.75f});
  auto k2 = heap<float>({-1.f});
  auto b3 = heap<int32_t>({V, V - 1, V + 2});
  auto p3 = heap<float>({-0.375f});
  auto k3 = heap<float>({-2.f});
  auto b4 = heap<int32_t>({V, V - 1, V + 2, V + 1});
  auto p4 = heap<float>({-0.0625f});
  const int64_t count[4] = {4, 1, 1, 1};
  const int32_t* ids[4] = {u.get(), b2.get(), b3.get(), b4.get()};
  const float* prob[4] = {up.get(), p2.get(), p3.get(), p4.get()};
  const float* back[4] = {ub.get(), k2.get(), k3.get(), nullptr};
  NgramTables t;
  std::string why;
  CHECK(ngram_build(4, V, count, ids, prob, back, &t, &why) == NGRAM_OK);
  CHECK(t.tab[0].size() == 2 && t.tab[1].size() == 2 && t.tab[2].size() == 2);
  const NgramView m = t.view();
  auto s1 = heap<int32_t>({V - 1, 9});  // "<s> V-1 <unk> </s>": bigram, trigram and 4-gram hits
  // t(V-1 | <s>) = -0.75; t(<unk> | <s> V-1) = -0.375; t(</s> | <s> V-1 <unk>) = -0.0625
  CHECK(ngram_sentence(m, s1.get(), 2, 1) == (-0.75f + -0.375f) + -0.0625f);
  // empty sentence, both bos values: P(</s>) + bo(<s>), and P(</s>)
  CHECK(ngram_sentence(m, s1.get(), 0, 1) == -1.5f + -0.5f);
  CHECK(ngram_sentence(m, s1.get(), 0, 0) == -1.5f);
  // an id outside [0, V + 3) scores as <unk> (default -100, backoff 0)
  auto s2 = heap<int32_t>({-5});
  CHECK(ngram_sentence(m, s2.get(), 1, 0) == -100.f + (-1.5f + 0.f));

  // a count that is exactly a power of two: 1,024 bigrams in 2,048 slots, every one found again
  const int n = 1024;
  std::unique_ptr<int32_t[]> ui(new int32_t[64]);
  std::unique_ptr<float[]> uz(new float[64]);
  for (int i = 0; i < 64; ++i) {
    ui[i] = i;
    uz[i] = -1.f;
  }
  std::unique_ptr<int32_t[]> bi(new int32_t[2 * n]);
  std::unique_ptr<float[]> bp(new float[n]);
  for (int i = 0; i < n; ++i) {
    bi[2 * i] = i / 32;
    bi[2 * i + 1] = i % 32;
    bp[i] = -(float)i;
  }
  const int64_t c2[2] = {64, n};
  const int32_t* i2[2] = {ui.get(), bi.get()};
  const float* q2[2] = {uz.get(), bp.get()};
  const float* z2[2] = {uz.get(), nullptr};
  CHECK(ngram_build(2, V, c2, i2, q2, z2, &t, &why) == NGRAM_OK);
  CHECK(t.tab[0].size() == 2048);
  const NgramView m2 = t.view();
  for (int i = 0; i < n; ++i) {
    const int c[1] = {i / 32};
    CHECK(ngram_term(m2, c, 1, i % 32) == -(float)i);
  }
  const int c[1] = {40};
  CHECK(ngram_term(m2, c, 1, 3) == -1.f + -1.f);  // absent bigram: unigram + backoff

  // refusals
  CHECK(ngram_build(5, V, count, ids, prob, back, &t, &why) == NGRAM_ERR_UNSUPPORTED);
  CHECK(ngram_build(1, 65533, count, ids, prob, back, &t, &why) == NGRAM_ERR_UNSUPPORTED);
  auto dup = heap<int32_t>({V, V - 1, V, V - 1});
  auto dp = heap<float>({-1.f, -1.f});
  const int64_t c3[2] = {4, 2};
  const int32_t* i3[2] = {u.get(), dup.get()};
  const float* q3[2] = {up.get(), dp.get()};
  CHECK(ngram_build(2, V, c3, i3, q3, z2, &t, &why) == NGRAM_ERR_ARG && why.find("duplicate") != std::string::npos);
  auto bad = heap<int32_t>({V, V + 3});
  const int64_t c4[2] = {4, 1};
  const int32_t* i4[2] = {u.get(), bad.get()};
  CHECK(ngram_build(2, V, c4, i4, q3, z2, &t, &why) == NGRAM_ERR_ARG);
  auto inf = heap<float>({-1.f, -HUGE_VALF, -1.f, -1.f});
  const float* q5[1] = {inf.get()};
  CHECK(ngram_build(1, V, count, ids, q5, back, &t, &why) == NGRAM_ERR_ARG && why.find("non-finite") != std::string::npos);
}

int main(int argc, char** argv) {
  edge_cases();
  if (argc < 3) {
    printf("ngram_check ok (edge cases only)\n");
    return 0;
  }
  FILE* f = fopen(argv[1], "rb");
  CHECK(f);
  int32_t head[2];
  CHECK(fread(head, sizeof head, 1, f) == 1);
  const int order = head[0], vocab = head[1];
  CHECK(order >= 1 && order <= NGRAM_MAX_ORDER);
  int64_t count[NGRAM_MAX_ORDER] = {};
  std::unique_ptr<int32_t[]> ids[NGRAM_MAX_ORDER];
  std::unique_ptr<float[]> prob[NGRAM_MAX_ORDER], back[NGRAM_MAX_ORDER];
  const int32_t* idp[NGRAM_MAX_ORDER] = {};
  const float *pp[NGRAM_MAX_ORDER] = {}, *bp[NGRAM_MAX_ORDER] = {};
  for (int n = 0; n < order; ++n) {
    int64_t sz;
    CHECK(fread(&count[n], sizeof(int64_t), 1, f) == 1);
    ids[n] = read_array<int32_t>(f, &sz);
    prob[n] = read_array<float>(f, &sz);
    back[n] = read_array<float>(f, &sz);
    idp[n] = ids[n].get();
    pp[n] = prob[n].get();
    bp[n] = back[n].get();
  }
  int32_t dims[3];
  CHECK(fread(dims, sizeof dims, 1, f) == 1);
  const int n = dims[0], L = dims[1], bos = dims[2];
  int64_t sz;
  auto tokens = read_array<int32_t>(f, &sz);
  CHECK(sz == (int64_t)n * L);
  auto lens = read_array<int32_t>(f, &sz);
  CHECK(sz == n);
  fclose(f);
  NgramTables t;
  std::string why;
  const int rc = ngram_build(order, vocab, count, idp, pp, bp, &t, &why);
  if (rc != NGRAM_OK) {
    fprintf(stderr, "ngram_build: %s\n", why.c_str());
    return 3;
  }
  const NgramView m = t.view();
  std::unique_ptr<float[]> q(new float[(size_t)n]);
  for (int i = 0; i < n; ++i) {
    std::unique_ptr<int32_t[]> row(new int32_t[(size_t)lens[i]]);  // exactly the sentence's words
    if (lens[i]) memcpy(row.get(), tokens.get() + (size_t)i * L, sizeof(int32_t) * (size_t)lens[i]);
    q[i] = ngram_sentence(m, row.get(), lens[i], bos);
  }
  FILE* o = fopen(argv[2], "wb");
  CHECK(o);
  CHECK(fwrite(q.get(), sizeof(float), (size_t)n, o) == (size_t)n);
  fclose(o);
  printf("ngram_check ok\n");
  return 0;
}
