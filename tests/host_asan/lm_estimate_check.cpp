// csrc/lm_estimate_plan.h under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own
// (host code only; tests/test_lm_estimate_host_sanitizer.py builds and runs it).  The corpus lives in
// heap buffers of exactly the sizes the file states, so a read past what the estimator may touch is a
// sanitizer report.
//   lm_estimate_check <corpus.bin> <out.bin>
// corpus.bin: int32 order, vocab; tokens (int64 element count + int32 elements); offsets (int64 element
// count + int64 elements).  out.bin: int64 positions, n_types; double D[4][3]; int32 fallback[4]; then
// per order int64 count and the arrays key (u64), raw, adjusted (u32), p, gamma (f64), prob, backoff
// (f32), each [count].  Built-in edge cases run first.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "lm_estimate_plan.h"

using namespace casr;

#define CHECK(c)                                                                 \
  do {                                                                           \
    if (!(c)) {                                                                  \
      fprintf(stderr, "lm_estimate_check: %s failed (line %d)\n", #c, __LINE__); \
      exit(2);                                                                   \
    }                                                                            \
  } while (0)

template <class T>
static std::unique_ptr<T[]> read_array(FILE* f, int64_t* n) {
  CHECK(fread(n, sizeof *n, 1, f) == 1);
  std::unique_ptr<T[]> p(new T[(size_t)*n]);  // exact size: no slack behind the data
  if (*n) CHECK(fread(p.get(), sizeof(T), (size_t)*n, f) == (size_t)*n);
  return p;
}

template <class T>
static std::unique_ptr<T[]> heap(std::initializer_list<T> v) {
  std::unique_ptr<T[]> p(new T[v.size()]);
  size_t i = 0;
  for (T x : v) p[i++] = x;
  return p;
}

static void edge_cases() {
  const int V = 5003;
  // the window key is ngram_key's packing
  const int32_t g[4] = {V, 0, V - 1, V + 2};
  for (int n = 1; n <= 4; ++n) {
    uint64_t key = 0;
    for (int e = 0; e < n; ++e) key |= est_key_field(g[n - 1 - e], e);
    CHECK(key == ngram_key(g, n) && est_key_order(key) == n && est_key_first(key, n) == V);
    int32_t back[4];
    est_key_ids(key, n, back);
    CHECK(memcmp(back, g, sizeof(int32_t) * n) == 0);
    if (n > 1) CHECK(est_key_prefix(key) == ngram_key(g, n - 1) && est_key_suffix(key, n) == ngram_key(g + 1, n - 1));
  }
  // a full table refuses instead of spinning: 2 slots, 3 keys
  std::unique_ptr<EstSlot[]> tab(new EstSlot[2]);
  memset(tab.get(), 0, 2 * sizeof(EstSlot));
  CHECK(est_insert<EstHostOps>(tab.get(), 1u, 11, 1));
  CHECK(est_insert<EstHostOps>(tab.get(), 1u, 12, 1));
  CHECK(est_insert<EstHostOps>(tab.get(), 1u, 11, 2));
  CHECK(!est_insert<EstHostOps>(tab.get(), 1u, 13, 1));
  CHECK(est_find(tab.get(), 1u, 13) == -1 && est_find(tab.get(), 1u, 11) >= 0);
  CHECK(tab[est_find(tab.get(), 1u, 11)].count == 3);
  // the plan
  CHECK(est_capacity(2, 1) == 2 && est_capacity(2, 1024) == 2048 && est_capacity(2, 1025) == 4096);
  CHECK(est_capacity(1, 1) == 4 && est_capacity(1, EST_MAX_POSITIONS) == 131072);
  CHECK(est_workspace_bytes(4, EST_MAX_POSITIONS) > 0 && est_workspace_bytes(4, EST_MAX_POSITIONS + 1) == -1);
  CHECK(est_workspace_bytes(0, 5) == -1 && est_workspace_bytes(5, 5) == -1 && est_workspace_bytes(1, 0) == -1);
  // the discount rule: estimated, and the three ways into the fallback
  double D[3];
  const uint32_t t_ok[4] = {100, 40, 20, 10}, t_zero[4] = {100, 40, 20, 0}, t_neg[4] = {10, 10, 100, 10};
  CHECK(!est_discounts(t_ok, D) && D[0] > 0 && D[0] <= 1 && D[2] <= 3);
  CHECK(est_discounts(t_zero, D) && D[0] == 0.5 && D[1] == 1.0 && D[2] == 1.5);
  CHECK(est_discounts(t_neg, D) && D[0] == 0.5);
  // one empty sentence (no token is read: a null corpus is fine), every order
  auto off = heap<int64_t>({0, 0});
  for (int order = 1; order <= 4; ++order) {
    EstResult r;
    std::string why;
    CHECK(est_estimate_host(order, V, nullptr, off.get(), 1, &r, &why) == NGRAM_OK);
    CHECK(r.positions == 1 && r.key[0].size() == 3 && (order < 2 || r.key[1].size() == 1));
    CHECK(r.n_types == 2 && r.p[0][1] + r.p[0][2] == 1.0);  // </s> and <unk> share the mass
  }
  // ids 0, V - 1 and <unk>; a sentence of one word; refusals
  auto tok = heap<int32_t>({0, V - 1, V + 2, 0});
  auto off2 = heap<int64_t>({0, 3, 3, 4});
  EstResult r;
  std::string why;
  CHECK(est_estimate_host(4, V, tok.get(), off2.get(), 3, &r, &why) == NGRAM_OK);
  CHECK(r.positions == 7 && r.key[3].size() == 2);  // <s> 0 V-1 <unk>, 0 V-1 <unk> </s>
  CHECK(est_estimate_host(0, V, tok.get(), off2.get(), 3, &r, &why) == NGRAM_ERR_ARG);
  CHECK(est_estimate_host(5, V, tok.get(), off2.get(), 3, &r, &why) == NGRAM_ERR_ARG);
  CHECK(est_estimate_host(2, V, tok.get(), off2.get(), 0, &r, &why) == NGRAM_ERR_ARG);
  CHECK(est_estimate_host(2, 65533, tok.get(), off2.get(), 3, &r, &why) == NGRAM_ERR_UNSUPPORTED);
  CHECK(est_estimate_host(2, V - 1, tok.get(), off2.get(), 3, &r, &why) == NGRAM_ERR_ARG);  // V - 1 is now <s>
  auto off3 = heap<int64_t>({0, 3, 2, 4});
  CHECK(est_estimate_host(2, V, tok.get(), off3.get(), 3, &r, &why) == NGRAM_ERR_ARG && why.find("descend") != std::string::npos);
  auto off4 = heap<int64_t>({0, EST_MAX_POSITIONS});
  CHECK(est_estimate_host(2, V, tok.get(), off4.get(), 1, &r, &why) == NGRAM_ERR_UNSUPPORTED);
}

template <class T>
static void put(FILE* o, const std::vector<T>& v) {
  if (!v.empty()) CHECK(fwrite(v.data(), sizeof(T), v.size(), o) == v.size());
}

int main(int argc, char** argv) {
  edge_cases();
  if (argc < 3) {
    printf("lm_estimate_check ok (edge cases only)\n");
    return 0;
  }
  FILE* f = fopen(argv[1], "rb");
  CHECK(f);
  int32_t head[2];
  CHECK(fread(head, sizeof head, 1, f) == 1);
  const int order = head[0], vocab = head[1];
  int64_t n_tok, n_off;
  auto tokens = read_array<int32_t>(f, &n_tok);
  auto offsets = read_array<int64_t>(f, &n_off);
  fclose(f);
  CHECK(n_off >= 2);
  EstResult r;
  std::string why;
  const int rc = est_estimate_host(order, vocab, tokens.get(), offsets.get(), n_off - 1, &r, &why);
  if (rc != NGRAM_OK) {
    fprintf(stderr, "est_estimate_host: %s\n", why.c_str());
    return 3;
  }
  FILE* o = fopen(argv[2], "wb");
  CHECK(o);
  const int64_t head2[2] = {r.positions, r.n_types};
  CHECK(fwrite(head2, sizeof head2, 1, o) == 1);
  CHECK(fwrite(r.D, sizeof r.D, 1, o) == 1);
  CHECK(fwrite(r.fallback, sizeof r.fallback, 1, o) == 1);
  for (int n = 1; n <= order; ++n) {
    const int64_t c = (int64_t)r.key[n - 1].size();
    CHECK(fwrite(&c, sizeof c, 1, o) == 1);
    std::vector<float> prob((size_t)c), back((size_t)c);
    for (size_t i = 0; i < (size_t)c; ++i) {
      prob[i] = est_stored_prob(r, n, i);
      back[i] = est_stored_backoff(r, n, i);
    }
    put(o, r.key[n - 1]);
    put(o, r.count[n - 1]);
    put(o, r.adjusted[n - 1]);
    put(o, r.p[n - 1]);
    put(o, r.gamma[n - 1]);
    put(o, prob);
    put(o, back);
  }
  fclose(o);
  printf("lm_estimate_check ok\n");
  return 0;
}
