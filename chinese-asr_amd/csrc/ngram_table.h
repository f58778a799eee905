// The backoff n-gram language model of casr_lm_* and casr_beam_rescore (include/casr.h): the tables,
// their build from id arrays, and the query.  The operation is defined by the formulas in casr.h (the
// textbook ARPA backoff query), not by any other tool's output.
// Pure C++ (no HIP runtime): tests/host_asan/ngram_check.cpp builds from this header alone.  The
// query functions are __host__ __device__ under hipcc, so the kernels (ngram.hip) and the host entry
// points (casr_capi.hip) run one text.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#if defined(__HIPCC__)
#define CASR_NGRAM_HD __host__ __device__
#else
#define CASR_NGRAM_HD
#endif

namespace casr {

constexpr int NGRAM_MAX_ORDER = 4;
constexpr int NGRAM_MAX_IDS = 65535;       // V + 3 ids: id + 1 fits a 16-bit key field
constexpr float NGRAM_UNK_PROB = -100.0f;  // an ARPA file without <unk>: (prob -100, backoff 0)

// status of ngram_build: the CASR_ERR_* values of include/casr.h
enum { NGRAM_OK = 0, NGRAM_ERR_ARG = 1, NGRAM_ERR_UNSUPPORTED = 4 };

struct NgramUni {
  float prob, backoff;
};
// one slot of an open-addressing table; key 0 = empty
struct alignas(16) NgramEntry {
  uint64_t key;
  float prob, backoff;
};

// What a query reads (plain pointers: host arrays, or their device copies as a kernel argument).
// LM ids: 0 .. V - 1 the ASR token ids, V = <s>, V + 1 = </s>, V + 2 = <unk>.
struct NgramView {
  int order, V;
  const NgramUni* uni;        // [V + 3]
  const int32_t* redirect;    // [V + 3]: the id itself, or V + 2 for an id without a unigram
  const NgramEntry* tab[NGRAM_MAX_ORDER - 1];  // orders 2..4: tab[n - 2], mask[n - 2] + 1 slots
  uint32_t mask[NGRAM_MAX_ORDER - 1];
};

// The key of an n-gram (w_1 .. w_n): field i (bits 16 i .. 16 i + 15) holds w_{n - i} + 1, the last
// word in field 0.  Exact (two different n-grams of one order never share a key) and never 0.
inline uint64_t ngram_key(const int32_t* ids, int n) {
  uint64_t k = 0;
  for (int i = 0; i < n; ++i) k |= (uint64_t)(uint32_t)(ids[n - 1 - i] + 1) << (16 * i);
  return k;
}

// slot of a key before masking: the splitmix64 finaliser (Steele, Lea, Flood 2014)
CASR_NGRAM_HD inline uint64_t ngram_mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

// One lookup, in two halves so that a term can have the first read of all its lookups in flight at
// once: start() reads the key's own slot, finish() compares and probes on linearly while it must.  A
// table always has an empty slot (capacity >= 2 count, >= 1).
struct NgramProbe {
  const NgramEntry* t;
  uint32_t mask, s;
  uint64_t key;
  NgramEntry e;
};
CASR_NGRAM_HD inline void ngram_probe_start(NgramProbe& q, const NgramEntry* t, uint32_t mask, uint64_t key) {
  q.t = t;
  q.mask = mask;
  q.key = key;
  q.s = (uint32_t)ngram_mix(key) & mask;
  q.e = t[q.s];
}
CASR_NGRAM_HD inline bool ngram_probe_finish(NgramProbe& q, float* prob, float* backoff) {
  for (uint32_t i = 0; i <= q.mask; ++i) {
    if (q.e.key == q.key) {
      *prob = q.e.prob;
      *backoff = q.e.backoff;
      return true;
    }
    if (q.e.key == 0) return false;
    q.s = (q.s + 1) & q.mask;
    q.e = q.t[q.s];
  }
  return false;
}

// The term of word w after the context c[0 .. nc): LM ids, nearest predecessor first, nc <= order - 1,
// all already redirected.  m = the largest order whose n-gram (c[m - 2] .. c[0], w) is in the model,
// p = prob_m, then for j = m .. nc: p = p + backoff(c[j - 1] .. c[0]) where that j-gram is in the
// model.  f32 adds in that order.  The lookups do not depend on one another, so the first read of
// every one (up to three n-grams ending in w, up to two contexts) is issued before any is examined,
// and the choice is made afterwards: the random reads overlap instead of following one another.
CASR_NGRAM_HD inline float ngram_term(const NgramView& m, const int32_t* c, int nc, int w) {
  uint64_t kw = (uint64_t)(uint32_t)(w + 1), kc = 0;
  NgramProbe qw[NGRAM_MAX_ORDER - 1], qc[NGRAM_MAX_ORDER - 1];  // qw[j - 1]: the (j + 1)-gram; qc[j - 1]: the j-gram context
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 1; j < NGRAM_MAX_ORDER; ++j) {
    if (j > nc) break;
    const uint64_t f = (uint64_t)(uint32_t)(c[j - 1] + 1);
    kc |= f << (16 * (j - 1));
    kw |= f << (16 * j);
    ngram_probe_start(qw[j - 1], m.tab[j - 1], m.mask[j - 1], kw);
    if (j >= 2) ngram_probe_start(qc[j - 1], m.tab[j - 2], m.mask[j - 2], kc);
  }
  float p = m.uni[w].prob;
  int mo = 1;
  float bo[NGRAM_MAX_ORDER - 1] = {0.f, 0.f, 0.f};
  bool has[NGRAM_MAX_ORDER - 1] = {false, false, false};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 1; j < NGRAM_MAX_ORDER; ++j) {
    if (j > nc) break;
    float pp, bb;
    if (ngram_probe_finish(qw[j - 1], &pp, &bb)) {  // the largest order found wins
      p = pp;
      mo = j + 1;
    }
    if (j == 1) {  // the unigram of c[0]: always in the model
      has[0] = true;
      bo[0] = m.uni[c[0]].backoff;
    } else {
      has[j - 1] = ngram_probe_finish(qc[j - 1], &pp, &bo[j - 1]);
    }
  }
  for (int j = mo; j <= nc; ++j)
    if (has[j - 1]) p = p + bo[j - 1];
  return p;
}

// LM id of a token of a sentence: redirected, and <unk> (with *bad set) outside [0, limit)
CASR_NGRAM_HD inline int ngram_lm_id(const NgramView& m, int t, int limit, bool* bad) {
  if ((unsigned)t >= (unsigned)limit) {
    *bad = true;
    return m.V + 2;
  }
  return m.redirect[t];
}

// Term t_p of position p of a sentence of len tokens (LM ids in [0, V + 3)): p < len the word at p,
// p == len the closing </s>; the context is the up to order - 1 ids before it, <s> first when bos.
CASR_NGRAM_HD inline float ngram_position_term(const NgramView& m, const int32_t* tok, int len, int bos, int p,
                                               bool* bad) {
  const int w = p < len ? ngram_lm_id(m, tok[p], m.V + 3, bad) : m.redirect[m.V + 1];
  int c[NGRAM_MAX_ORDER - 1] = {0, 0, 0};
  int nc = 0;
  for (int i = 1; i < m.order; ++i) {
    const int at = p - i;
    if (at >= 0) {
      c[nc++] = ngram_lm_id(m, tok[at], m.V + 3, bad);
    } else {
      if (bos) c[nc++] = m.redirect[m.V];
      break;
    }
  }
  return ngram_term(m, c, nc, w);
}

// q = (..((t_0 + t_1) + t_2).. + t_len): f32 adds, ascending, t_0 taken as is
inline float ngram_sentence(const NgramView& m, const int32_t* tok, int len, int bos) {
  bool bad = false;
  float q = 0.f;
  for (int p = 0; p <= len; ++p) {
    const float t = ngram_position_term(m, tok, len, bos, p, &bad);
    q = p == 0 ? t : q + t;
  }
  return q;
}

// ---------------------------------------------------------------- build (host)
struct NgramTables {
  int order = 0, V = 0;
  std::vector<NgramUni> uni;
  std::vector<int32_t> redirect;
  std::vector<NgramEntry> tab[NGRAM_MAX_ORDER - 1];
  NgramView view() const {
    NgramView v{};
    v.order = order;
    v.V = V;
    v.uni = uni.data();
    v.redirect = redirect.data();
    for (int i = 0; i < NGRAM_MAX_ORDER - 1; ++i) {
      v.tab[i] = tab[i].data();
      v.mask[i] = tab[i].empty() ? 0u : (uint32_t)(tab[i].size() - 1);
    }
    return v;
  }
};

// slots of a table of count n-grams: the power of two >= 2 count (1 for an empty order)
inline size_t ngram_capacity(int64_t count) {
  size_t cap = 1;
  while (cap < 2 * (size_t)count) cap <<= 1;
  return cap;
}

// Per order n = 1 .. order: count[n - 1] n-grams, ids[n - 1] [count][n] LM ids, prob[n - 1] [count]
// log10 probabilities, backoff[n - 1] [count] or null (zeros; the top order's is never read).
// NGRAM_ERR_UNSUPPORTED: order > 4 or V + 3 > 65,535.  NGRAM_ERR_ARG: order < 1, vocab < 1, a null
// array, a negative count, an id outside [0, V + 3), a duplicate n-gram, a non-finite value.
// *why (may be null) says which.
inline int ngram_build(int order, int vocab, const int64_t* count, const int32_t* const* ids,
                       const float* const* prob, const float* const* backoff, NgramTables* out, std::string* why) {
  auto fail = [&](int code, const std::string& s) {
    if (why) *why = s;
    return code;
  };
  if (order > NGRAM_MAX_ORDER) return fail(NGRAM_ERR_UNSUPPORTED, "order " + std::to_string(order) + " > 4");
  if (order < 1 || vocab < 1) return fail(NGRAM_ERR_ARG, "order < 1 or vocab < 1");
  if ((int64_t)vocab + 3 > NGRAM_MAX_IDS)
    return fail(NGRAM_ERR_UNSUPPORTED, "vocab + 3 = " + std::to_string((int64_t)vocab + 3) + " > 65535");
  if (!count || !ids || !prob || !out) return fail(NGRAM_ERR_ARG, "null argument");
  const int NI = vocab + 3;
  for (int n = 1; n <= order; ++n) {
    if (count[n - 1] < 0) return fail(NGRAM_ERR_ARG, "negative count at order " + std::to_string(n));
    if (count[n - 1] > 0 && (!ids[n - 1] || !prob[n - 1]))
      return fail(NGRAM_ERR_ARG, "null ids or prob at order " + std::to_string(n));
    if ((uint64_t)count[n - 1] > (1ull << 30))
      return fail(NGRAM_ERR_UNSUPPORTED, "more than 2^30 n-grams at order " + std::to_string(n));
  }
  NgramTables t;
  t.order = order;
  t.V = vocab;
  t.uni.assign(NI, NgramUni{NGRAM_UNK_PROB, 0.f});
  t.redirect.assign(NI, vocab + 2);
  std::vector<uint8_t> seen(NI, 0);
  for (int n = 1; n <= order; ++n) {
    const int64_t cnt = count[n - 1];
    const float* bo = (backoff && n < order) ? backoff[n - 1] : nullptr;
    if (n >= 2) t.tab[n - 2].assign(ngram_capacity(cnt), NgramEntry{0, 0.f, 0.f});
    const uint32_t mask = n >= 2 ? (uint32_t)(t.tab[n - 2].size() - 1) : 0u;
    for (int64_t i = 0; i < cnt; ++i) {
      const int32_t* g = ids[n - 1] + i * n;
      const std::string at = " (order " + std::to_string(n) + ", n-gram " + std::to_string(i) + ")";
      for (int e = 0; e < n; ++e)
        if (g[e] < 0 || g[e] >= NI) return fail(NGRAM_ERR_ARG, "id " + std::to_string(g[e]) + " outside [0, V + 3)" + at);
      const float p = prob[n - 1][i], b = bo ? bo[i] : 0.f;
      if (!isfinite(p) || !isfinite(b)) return fail(NGRAM_ERR_ARG, "non-finite value" + at);
      if (n == 1) {
        if (seen[g[0]]) return fail(NGRAM_ERR_ARG, "duplicate n-gram" + at);
        seen[g[0]] = 1;
        t.uni[g[0]] = NgramUni{p, b};
        t.redirect[g[0]] = g[0];
        continue;
      }
      const uint64_t key = ngram_key(g, n);
      NgramEntry* tab = t.tab[n - 2].data();
      uint32_t s = (uint32_t)ngram_mix(key) & mask;
      while (tab[s].key != 0) {
        if (tab[s].key == key) return fail(NGRAM_ERR_ARG, "duplicate n-gram" + at);
        s = (s + 1) & mask;
      }
      tab[s] = NgramEntry{key, p, b};
    }
  }
  for (int n = order + 1; n <= NGRAM_MAX_ORDER; ++n) t.tab[n - 2].assign(1, NgramEntry{0, 0.f, 0.f});
  // an id without a unigram scores and matches as <unk> (which always has one: the default above)
  t.redirect[vocab + 2] = vocab + 2;
  for (int i = 0; i < NI; ++i)
    if (t.redirect[i] != i) t.uni[i] = t.uni[vocab + 2];
  *out = std::move(t);
  return NGRAM_OK;
}

}  // namespace casr
