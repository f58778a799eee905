// csrc/ngram_succ.h (the successor lists' build and the per-row term query, the text the kernel runs
// too) under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (host code only;
// tests/test_lm_terms_sanitizer.py builds and runs it).  Seeded random models of every order live in
// exact-size heap buffers; for many contexts the whole term row must equal the per-word query
// (ngram_term) bit for bit.
//   ngram_terms_check [seed]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <set>
#include <string>
#include <vector>

#include "ngram_succ.h"

using namespace casr;

#define CHECK(c)                                                                 \
  do {                                                                           \
    if (!(c)) {                                                                  \
      fprintf(stderr, "ngram_terms_check: %s failed (line %d)\n", #c, __LINE__); \
      exit(2);                                                                   \
    }                                                                            \
  } while (0)

static uint64_t g_state = 1;
static uint32_t rnd(uint32_t n) {  // splitmix64 stream
  g_state += 0x9e3779b97f4a7c15ull;
  return (uint32_t)(ngram_mix(g_state) >> 33) % n;
}
static float rnd_val(float lo) { return lo * (float)(rnd(1 << 20) + 1) / (float)(1 << 20); }

template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {  // no slack behind the data
  std::unique_ptr<T[]> p(new T[v.size()]);
  if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

static uint32_t bits(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
}

// a random model: unigrams for about 3/4 of the V ASR ids plus <s>, </s> (and <unk> when with_unk); per
// higher order n_high n-grams, half of them extensions of an n-gram of the order below, one in eight
// with a word that has no unigram (stored as given, never reachable); and under the context (1 2 3)
// word 4 at every order, <unk> and </s> as successors, and every unigram id after context (1)
static void one_model(int order, int V, int n_high, bool with_unk) {
  const int NI = V + 3;
  std::vector<int32_t> ids[4];
  std::vector<float> prob[4], back[4];
  std::vector<uint8_t> has(NI, 0);
  for (int i = 0; i < NI; ++i) {
    const bool u = i < V ? (i <= 4 || rnd(4) != 0) : (i != V + 2 || with_unk);
    if (!u) continue;
    has[i] = 1;
    ids[0].push_back(i);
    prob[0].push_back(rnd_val(-6.f));
    back[0].push_back(rnd(8) ? rnd_val(-2.f) : 0.f);
  }
  std::set<std::vector<int32_t>> seen[4];
  auto add = [&](const std::vector<int32_t>& g) {
    const int n = (int)g.size();
    if (n > order || !seen[n - 1].insert(g).second) return;
    ids[n - 1].insert(ids[n - 1].end(), g.begin(), g.end());
    prob[n - 1].push_back(rnd_val(-6.f));
    back[n - 1].push_back(n < order && rnd(8) ? rnd_val(-2.f) : 0.f);
  };
  auto word = [&](bool any) {
    for (;;) {
      const int w = (int)rnd(NI);
      if (any || has[w]) return w;
    }
  };
  add({3, 4});
  add({2, 3, 4});
  add({1, 2, 3, 4});
  add({3, V + 2});
  add({2, 3, V + 1});
  add({1, 2, 3, V + 2});
  add({1, 2, 3, V + 1});
  for (int w = 0; w < NI; ++w)
    if (has[w] && w != V) add({1, w});
  for (int n = 2; n <= order; ++n)
    for (int i = 0; i < n_high; ++i) {
      std::vector<int32_t> g;
      const size_t below = prob[n - 2].size();
      if (n > 2 && below && rnd(2)) {
        const size_t at = rnd((uint32_t)below);
        g.assign(ids[n - 2].begin() + at * (n - 1), ids[n - 2].begin() + (at + 1) * (n - 1));
      } else {
        for (int e = 0; e < n - 1; ++e) g.push_back(word(rnd(8) == 0));
      }
      g.push_back(word(rnd(8) == 0));
      add(g);
    }
  int64_t count[4] = {};
  std::unique_ptr<int32_t[]> idb[4];
  std::unique_ptr<float[]> pb[4], bb[4];
  const int32_t* idp[4] = {};
  const float *pp[4] = {}, *bp[4] = {};
  for (int n = 0; n < order; ++n) {
    count[n] = (int64_t)prob[n].size();
    idb[n] = exact(ids[n]);
    pb[n] = exact(prob[n]);
    bb[n] = exact(back[n]);
    idp[n] = idb[n].get();
    pp[n] = pb[n].get();
    bp[n] = bb[n].get();
  }
  NgramTables t;
  std::string why;
  CHECK(ngram_build(order, V, count, idp, pp, bp, &t, &why) == NGRAM_OK);
  NgramSuccTables st;
  ngram_succ_build(t, count, idp, pp, &st);
  const NgramView m = t.view();
  const NgramSuccView sv = st.view();
  // the lists: ascending in w per context, every listed word with a unigram
  for (int n = 2; n <= NGRAM_MAX_ORDER; ++n) CHECK(n <= order || st.list[n - 2].empty());
  if (order >= 2) {
    const NgramSuccRange r = ngram_succ_find(sv, 2, 1 + 1);
    size_t uni = 0;
    for (int w = 0; w < NI; ++w) uni += has[w] && w != V;
    CHECK(r.count >= uni);
    for (uint32_t i = 1; i < r.count; ++i) CHECK(st.list[0][r.offset + i - 1].w < st.list[0][r.offset + i].w);
  }
  std::unique_ptr<float[]> row(new float[(size_t)V]);  // exactly one row
  const int eos_token = 2;
  for (int q = 0; q < 300; ++q) {
    std::unique_ptr<int32_t[]> ctx(new int32_t[3]);
    int nc = (int)rnd(4);
    if (q < 4) {  // the constructed context, at every length
      ctx[0] = 3, ctx[1] = 2, ctx[2] = 1;
      nc = q;
    } else if (q % 3 == 0 && order >= 2) {  // the leading words of one of the model's n-grams
      const int n = 2 + (int)rnd((uint32_t)(order - 1));
      const size_t at = rnd((uint32_t)prob[n - 1].size());
      for (int e = 0; e < 3; ++e) ctx[e] = e < n - 1 ? ids[n - 1][at * n + (n - 2 - e)] : (int32_t)rnd(NI);
      nc = n - 1;
    } else {
      for (int e = 0; e < 3; ++e) ctx[e] = (int32_t)rnd(NI + 2) - 1;  // -1 and V + 3 among them
    }
    if (q == 7) nc = -3;
    if (q == 8) nc = 17;
    bool bad = false;
    const int eos = q & 1 ? eos_token : -1;
    ngram_terms_row(m, sv, ctx.get(), nc, eos, row.get(), &bad);
    bool want_bad = nc < 0 || nc > order - 1;
    const int ncc = nc < 0 ? 0 : nc > order - 1 ? order - 1 : nc;
    int c[3] = {0, 0, 0};
    for (int e = 0; e < ncc; ++e) c[e] = ngram_lm_id(m, ctx[e], NI, &want_bad);
    CHECK(bad == want_bad);
    for (int v = 0; v < V; ++v) {
      const int w = v == eos ? m.redirect[V + 1] : m.redirect[v];
      CHECK(bits(row[v]) == bits(ngram_term(m, c, ncc, w)));
    }
  }
}

int main(int argc, char** argv) {
  g_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  for (int order = 1; order <= 4; ++order) {
    one_model(order, 37, 200, true);
    one_model(order, 700, 3000, order & 1);
  }
  printf("ngram_terms_check ok\n");
  return 0;
}
