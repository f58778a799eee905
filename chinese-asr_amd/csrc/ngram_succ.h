// Successor lists of the backoff n-gram LM (ngram_table.h) and the per-row term query of
// casr_lm_terms / casr_beam_lm (include/casr.h): the term of EVERY vocabulary word under one context.
// Almost every word backs off to its unigram under the same row-constant backoffs; only the context's
// listed successors differ.  So a row is the dense chain over the unigram array plus the successor
// lists of its context, read sequentially, instead of a hash query per word.
// Pure C++ (no HIP runtime): tests/host_asan/ngram_terms_check.cpp builds from this header and
// ngram_table.h alone.  The row-constant part (ngram_row_prepare) and the per-entry values are
// __host__ __device__: the host row (ngram_terms_row) and the kernel (lm_terms.hip) run one text and
// differ only in who walks the vocabulary.
#pragma once
#include <algorithm>

#include "ngram_table.h"

namespace casr {

// one successor of a context: the n-gram (context, w) has log10 probability prob
struct NgramSucc {
  int32_t w;
  float prob;
};
// where a context's successors lie in its order's list (ascending in w)
struct NgramSuccRange {
  uint32_t offset, count;
};
// one slot of a context table (orders 3, 4): the key of the (n - 1)-word context as ngram_key packs
// it; key 0 = empty.  Independent of NgramView::tab: a context with successors need not be an n-gram
struct alignas(16) NgramCtxEntry {
  uint64_t key;
  uint32_t offset, count;
};

struct NgramSuccView {
  const NgramSucc* list[NGRAM_MAX_ORDER - 1];     // orders 2..4: list[n - 2]
  const NgramSuccRange* dir;                      // order 2: [V + 3], by the context word
  const NgramCtxEntry* ctab[NGRAM_MAX_ORDER - 2]; // orders 3, 4: ctab[n - 3], cmask[n - 3] + 1 slots
  uint32_t cmask[NGRAM_MAX_ORDER - 2];
};

// the successors of the context with key kc (n - 1 words, all redirected) at order n = 2..4
CASR_NGRAM_HD inline NgramSuccRange ngram_succ_find(const NgramSuccView& s, int n, uint64_t kc) {
  if (n == 2) return s.dir[(int)kc - 1];
  const NgramCtxEntry* t = s.ctab[n - 3];
  const uint32_t mask = s.cmask[n - 3];
  uint32_t at = (uint32_t)ngram_mix(kc) & mask;
  for (uint32_t i = 0; i <= mask; ++i) {
    const NgramCtxEntry e = t[at];
    if (e.key == kc) return NgramSuccRange{e.offset, e.count};
    if (e.key == 0) break;
    at = (at + 1) & mask;
  }
  return NgramSuccRange{0u, 0u};
}

// What every word of one row shares: the redirected context, its backoffs, its successor lists and
// the two scalars many words share or are remapped to.
struct NgramRow {
  int nc;                                  // context length in effect (clamped to [0, order - 1])
  int c[NGRAM_MAX_ORDER - 1];              // redirected LM ids, nearest first
  float bo[NGRAM_MAX_ORDER - 1];           // bo[j - 1]: backoff of the j-word context, where has[j - 1]
  bool has[NGRAM_MAX_ORDER - 1];
  NgramSuccRange succ[NGRAM_MAX_ORDER - 1];  // succ[n - 2]: successors at order n (count 0 past nc + 1)
  float unk, eos;                          // ngram_term of <unk> and of </s> under this context
  bool bad;                                // an id outside [0, limit) or an nc outside range
};

// ctx: up to three LM ids, nearest first (only the first nc are read); ids outside [0, limit) score
// as <unk>.  Every lookup of the row happens here, once.
CASR_NGRAM_HD inline void ngram_row_prepare(const NgramView& m, const NgramSuccView& s, const int32_t* ctx, int nc,
                                            int limit, NgramRow* r) {
  bool bad = false;
  if (nc < 0 || nc > m.order - 1) {
    bad = true;
    nc = nc < 0 ? 0 : m.order - 1;
  }
  r->nc = nc;
  uint64_t kc = 0;
  for (int j = 1; j < NGRAM_MAX_ORDER; ++j) {
    r->c[j - 1] = 0;
    r->bo[j - 1] = 0.f;
    r->has[j - 1] = false;
    r->succ[j - 1] = NgramSuccRange{0u, 0u};
    if (j > nc) continue;
    const int id = ngram_lm_id(m, ctx[j - 1], limit, &bad);
    r->c[j - 1] = id;
    kc |= (uint64_t)(uint32_t)(id + 1) << (16 * (j - 1));
    if (j == 1) {  // the unigram of c[0]: always in the model
      r->has[0] = true;
      r->bo[0] = m.uni[id].backoff;
    } else {
      NgramProbe q;
      float pp;
      ngram_probe_start(q, m.tab[j - 2], m.mask[j - 2], kc);
      r->has[j - 1] = ngram_probe_finish(q, &pp, &r->bo[j - 1]);
    }
    r->succ[j - 1] = ngram_succ_find(s, j + 1, kc);
  }
  r->unk = ngram_term(m, r->c, nc, m.V + 2);
  r->eos = ngram_term(m, r->c, nc, m.redirect[m.V + 1]);
  r->bad = bad;
}

// the term of a word whose largest n-gram under the row's context has order mo and probability p:
// p plus the backoffs of the contexts of mo .. nc words that exist, in that order (f32 adds)
CASR_NGRAM_HD inline float ngram_row_value(const NgramRow& r, int mo, float p) {
  for (int j = mo; j <= r.nc; ++j)
    if (r.has[j - 1]) p = p + r.bo[j - 1];
  return p;
}

// the dense value of ASR token v: </s>'s term for the eos token, <unk>'s for a token without a
// unigram, else the m = 1 chain.  A listed successor overwrites it (ngram_row_takes)
CASR_NGRAM_HD inline float ngram_row_dense(const NgramView& m, const NgramRow& r, int v, int eos_token) {
  if (v == eos_token) return r.eos;
  if (m.redirect[v] != v) return r.unk;
  return ngram_row_value(r, 1, m.uni[v].prob);
}
// whether a successor entry writes the row: an ASR token other than the eos token (<s>, </s> and
// <unk> as words are the scalars' business; a listed word always has a unigram, see ngram_succ_build)
CASR_NGRAM_HD inline bool ngram_row_takes(const NgramView& m, int w, int eos_token) {
  return w < m.V && w != eos_token;
}

// terms[v], v in [0, V): the host row.  Orders ascending, so the highest order wins.
inline void ngram_terms_row(const NgramView& m, const NgramSuccView& s, const int32_t* ctx, int nc, int eos_token,
                            float* terms, bool* bad) {
  NgramRow r;
  ngram_row_prepare(m, s, ctx, nc, m.V + 3, &r);
  if (r.bad) *bad = true;
  for (int v = 0; v < m.V; ++v) terms[v] = ngram_row_dense(m, r, v, eos_token);
  for (int n = 2; n <= r.nc + 1; ++n) {
    const NgramSucc* e = s.list[n - 2] + r.succ[n - 2].offset;
    for (uint32_t i = 0; i < r.succ[n - 2].count; ++i)
      if (ngram_row_takes(m, e[i].w, eos_token)) terms[e[i].w] = ngram_row_value(r, n, e[i].prob);
  }
}

// ---------------------------------------------------------------- build (host)
struct NgramSuccTables {
  std::vector<NgramSucc> list[NGRAM_MAX_ORDER - 1];
  std::vector<NgramSuccRange> dir;
  std::vector<NgramCtxEntry> ctab[NGRAM_MAX_ORDER - 2];
  NgramSuccView view() const {
    NgramSuccView v{};
    for (int i = 0; i < NGRAM_MAX_ORDER - 1; ++i) v.list[i] = list[i].data();
    v.dir = dir.data();
    for (int i = 0; i < NGRAM_MAX_ORDER - 2; ++i) {
      v.ctab[i] = ctab[i].data();
      v.cmask[i] = ctab[i].empty() ? 0u : (uint32_t)(ctab[i].size() - 1);
    }
    return v;
  }
};

// From the arrays ngram_build accepted (t: its result).  An n-gram any of whose words has no unigram
// is left out: queries are always redirected and n-grams are stored as given, so no query reaches it.
inline void ngram_succ_build(const NgramTables& t, const int64_t* count, const int32_t* const* ids,
                             const float* const* prob, NgramSuccTables* out) {
  struct Item {
    uint64_t key;
    int32_t w;
    float prob;
  };
  NgramSuccTables s;
  s.dir.assign((size_t)t.V + 3, NgramSuccRange{0u, 0u});
  for (int n = 2; n <= NGRAM_MAX_ORDER; ++n) {
    std::vector<Item> items;
    if (n <= t.order) {
      items.reserve((size_t)count[n - 1]);
      for (int64_t i = 0; i < count[n - 1]; ++i) {
        const int32_t* g = ids[n - 1] + i * n;
        bool reachable = true;
        for (int e = 0; e < n; ++e) reachable = reachable && t.redirect[g[e]] == g[e];
        if (reachable) items.push_back(Item{ngram_key(g, n - 1), g[n - 1], prob[n - 1][i]});
      }
      std::sort(items.begin(), items.end(),
                [](const Item& a, const Item& b) { return a.key != b.key ? a.key < b.key : a.w < b.w; });
    }
    std::vector<NgramSucc>& list = s.list[n - 2];
    list.resize(items.size());
    size_t contexts = 0;
    for (size_t i = 0; i < items.size(); ++i) {
      list[i] = NgramSucc{items[i].w, items[i].prob};
      if (i == 0 || items[i].key != items[i - 1].key) ++contexts;
    }
    if (n >= 3) s.ctab[n - 3].assign(ngram_capacity((int64_t)contexts), NgramCtxEntry{0, 0u, 0u});
    const uint32_t mask = n >= 3 ? (uint32_t)(s.ctab[n - 3].size() - 1) : 0u;
    for (size_t i = 0; i < items.size();) {
      size_t e = i;
      while (e < items.size() && items[e].key == items[i].key) ++e;
      const NgramSuccRange rg{(uint32_t)i, (uint32_t)(e - i)};
      if (n == 2) {
        s.dir[(size_t)items[i].key - 1] = rg;
      } else {
        NgramCtxEntry* tab = s.ctab[n - 3].data();
        uint32_t at = (uint32_t)ngram_mix(items[i].key) & mask;
        while (tab[at].key != 0) at = (at + 1) & mask;
        tab[at] = NgramCtxEntry{items[i].key, rg.offset, rg.count};
      }
      i = e;
    }
  }
  *out = std::move(s);
}

}  // namespace casr
