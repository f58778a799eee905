// Estimation of an interpolated modified-Kneser-Ney n-gram model (orders 1..4) from a token corpus:
// casr_lm_estimate_host and casr_lm_estimate (include/casr.h, which has the definition).  This header
// is the one text both run: the window key, the bounded insert and lookup of the counting tables, the
// per-slot stage bodies, the discount rule with its fallback, gamma, u and the interpolation step, the
// size plan, and the host estimator built from them.  The kernels (lm_estimate.hip) call the same stage
// bodies with atomic operations in place of the plain ones; every accumulated quantity is an integer,
// so the order of the additions does not matter, and every float64 operation is one IEEE operation in
// a stated order with contraction off, so the device and the host give the same bits.
// Pure C++ (no HIP runtime): tests/host_asan/lm_estimate_check.cpp builds from this header alone.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "ngram_table.h"

#define CASR_EST_HD CASR_NGRAM_HD

namespace casr {

constexpr int64_t EST_MAX_POSITIONS = 1ll << 28;  // counts and S in 32 bits
constexpr int EST_FLAG_BAD_INPUT = 1;  // an id or an offset was clamped (the handle's guard bit 1)
constexpr int EST_FLAG_FULL = 2;       // a table proved full, or a prefix / suffix was missing: refused

// one slot of a counting table; key 0 = empty.  count: the raw count c_n; ext: the number of distinct
// left extensions (the (n + 1)-gram types whose suffix this is)
struct alignas(16) EstSlot {
  uint64_t key;
  uint32_t count, ext;
};
// what an n-gram gathers as the CONTEXT of order n + 1: n[0] = S = sum of a_{n+1}(c w) over w, n[k] =
// N_k = the number of w with min(a_{n+1}(c w), 3) = k
struct alignas(16) EstCtx {
  uint32_t n[4];
};

// The tables of one call: per order n = 1..order, mask[n - 1] + 1 slots with, beside each slot, its
// context statistics, its p and the gamma it carries as a context (orders below the top one).
struct EstView {
  int order, V;
  EstSlot* slot[NGRAM_MAX_ORDER];
  EstCtx* ctx[NGRAM_MAX_ORDER];
  double* p[NGRAM_MAX_ORDER];
  double* gamma[NGRAM_MAX_ORDER];
  uint32_t mask[NGRAM_MAX_ORDER];
};

// sums over a whole order (device: through block partials)
struct EstTotals {
  uint32_t occupied[NGRAM_MAX_ORDER];  // n-grams of the order (the unigram <s> included)
  uint32_t t[NGRAM_MAX_ORDER][4];      // t_{n,k}, k = 1..4
  uint32_t ctx0[4];                    // the empty context's S, N_1, N_2, N_3
  uint32_t out[NGRAM_MAX_ORDER];       // compaction cursors
  uint32_t flags;                      // EST_FLAG_*
  uint32_t unk_seen;                   // the corpus holds <unk>
  uint32_t pad[2];
};

struct EstDiscounts {
  double D[NGRAM_MAX_ORDER][3];
  double gamma0;  // gamma_1 of the empty context
  uint32_t S0;    // S_1 of the empty context
  uint32_t W;     // |W|: unigram types other than <s> and <unk>, plus 1
};

// ---------------------------------------------------------------- keys
// ngram_key's packing, one word at a time: the key of (w_1 .. w_n) holds w_{n - i} + 1 in field i (bits
// 16 i .. 16 i + 15).  A window ending at a position is built backwards from its last word: the word e
// places before the last goes to field e.
CASR_EST_HD inline uint64_t est_key_field(int id, int e) { return (uint64_t)(uint32_t)(id + 1) << (16 * e); }
// order of a key: its non-zero fields (every field of an n-gram is id + 1 >= 1)
CASR_EST_HD inline int est_key_order(uint64_t key) {
  return (key >> 48) ? 4 : (key >> 32) ? 3 : (key >> 16) ? 2 : 1;
}
CASR_EST_HD inline int est_key_first(uint64_t key, int n) { return (int)((key >> (16 * (n - 1))) & 0xffff) - 1; }
CASR_EST_HD inline uint64_t est_key_suffix(uint64_t key, int n) { return key & ((1ull << (16 * (n - 1))) - 1); }
CASR_EST_HD inline uint64_t est_key_prefix(uint64_t key) { return key >> 16; }
inline void est_key_ids(uint64_t key, int n, int32_t* ids) {
  for (int e = 0; e < n; ++e) ids[e] = (int32_t)((key >> (16 * (n - 1 - e))) & 0xffff) - 1;
}

// LM id of a corpus token: itself in [0, V) and for V + 2 = <unk>; anything else counts as <unk>
CASR_EST_HD inline int est_clean_id(int t, int V, bool* bad) {
  if ((unsigned)t < (unsigned)V || t == V + 2) return t;
  *bad = true;
  return V + 2;
}
// id at place j of the padded sentence <s> w_1 .. w_len </s> (j = 0 .. len + 1)
CASR_EST_HD inline int est_padded_id(const int32_t* tok, int64_t len, int64_t j, int V, bool* bad) {
  if (j == 0) return V;
  if (j == len + 1) return V + 1;
  return est_clean_id(tok[j - 1], V, bad);
}
// The sentence a pair of offsets names inside tokens [0, total): clamped, *bad where that changed it
CASR_EST_HD inline void est_sentence_range(int64_t o0, int64_t o1, int64_t total, int64_t* start, int64_t* len,
                                           bool* bad) {
  int64_t s = o0 < 0 ? 0 : (o0 > total ? total : o0);
  int64_t e = o1 < s ? s : (o1 > total ? total : o1);
  if (s != o0 || e != o1) *bad = true;
  *start = s;
  *len = e - s;
}

// ---------------------------------------------------------------- tables
struct EstHostOps {
  static uint64_t load_key(const uint64_t* p) { return *p; }
  static uint64_t cas_key(uint64_t* p, uint64_t v) {  // the value before; stores v where that was 0
    const uint64_t o = *p;
    if (o == 0) *p = v;
    return o;
  }
  static void add(uint32_t* p, uint32_t v) { *p += v; }
};

// count += add in the slot of key, claiming an empty one.  The probe is bounded by the capacity: false
// when the table is full (it never is at the planned capacity: >= 2 windows)
template <class Ops>
CASR_EST_HD inline bool est_insert(EstSlot* tab, uint32_t mask, uint64_t key, uint32_t add) {
  uint32_t s = (uint32_t)ngram_mix(key) & mask;
  for (uint32_t i = 0; i <= mask; ++i) {
    uint64_t k = Ops::load_key(&tab[s].key);
    if (k == 0) k = Ops::cas_key(&tab[s].key, key);
    if (k == 0 || k == key) {
      Ops::add(&tab[s].count, add);
      return true;
    }
    s = (s + 1) & mask;
  }
  return false;
}

// slot of a key in a finished table, -1 where it has none; bounded as ngram_probe_finish is
CASR_EST_HD inline int64_t est_find(const EstSlot* tab, uint32_t mask, uint64_t key) {
  uint32_t s = (uint32_t)ngram_mix(key) & mask;
  for (uint32_t i = 0; i <= mask; ++i) {
    const uint64_t k = tab[s].key;
    if (k == key) return s;
    if (k == 0) return -1;
    s = (s + 1) & mask;
  }
  return -1;
}

// ---------------------------------------------------------------- stage bodies (one slot each)
// count: the windows ending at place j >= 1 of a padded sentence, orders 1 .. min(order, j + 1);
// emit(key) once per window
template <class Emit>
CASR_EST_HD inline void est_windows(const int32_t* tok, int64_t len, int64_t j, int order, int V, bool* bad,
                                    Emit&& emit) {
  uint64_t key = 0;
  for (int e = 0; e < order && j - e >= 0; ++e) {
    key |= est_key_field(est_padded_id(tok, len, j - e, V, bad), e);
    emit(key);
  }
}

// extensions: an (n >= 2)-gram adds 1 to its suffix in order n - 1.  false: the suffix is missing
template <class Ops>
CASR_EST_HD inline bool est_extend(const EstView& v, int n, uint32_t s) {
  const uint64_t key = v.slot[n - 1][s].key;
  if (key == 0) return true;
  const int64_t f = est_find(v.slot[n - 2], v.mask[n - 2], est_key_suffix(key, n));
  if (f < 0) return false;
  Ops::add(&v.slot[n - 2][f].ext, 1u);
  return true;
}

// the adjusted count a_n of an occupied slot
CASR_EST_HD inline uint32_t est_adjusted(const EstView& v, int n, const EstSlot& e) {
  return (n == v.order || est_key_first(e.key, n) == v.V) ? e.count : e.ext;
}

// does the slot hold an n-gram the estimate predicts (occupied, and not the unigram <s>)
CASR_EST_HD inline bool est_predicted(const EstView& v, int n, const EstSlot& e) {
  return e.key != 0 && !(n == 1 && e.key == (uint64_t)(v.V + 1));
}

// context statistics: an (n >= 2)-gram adds its a and its N_k increment to its prefix in order n - 1
template <class Ops>
CASR_EST_HD inline bool est_ctx_add(const EstView& v, int n, uint32_t s) {
  const EstSlot e = v.slot[n - 1][s];
  if (e.key == 0) return true;
  const int64_t f = est_find(v.slot[n - 2], v.mask[n - 2], est_key_prefix(e.key));
  if (f < 0) return false;
  const uint32_t a = est_adjusted(v, n, e);
  Ops::add(&v.ctx[n - 2][f].n[0], a);
  Ops::add(&v.ctx[n - 2][f].n[a < 3 ? a : 3], 1u);
  return true;
}

// ---------------------------------------------------------------- the arithmetic (float64, no contraction)
// D_n(k) = k - ((k + 1) Y) t_{k+1} / t_k with Y = t1 / (t1 + 2 t2); the order falls back to (0.5, 1, 1.5)
// unless t1..t4 are all positive and 0 < D(k) <= k for every k.  Returns the fallback flag.
CASR_EST_HD inline bool est_discounts(const uint32_t t[4], double D[3]) {
#pragma clang fp contract(off)
  bool ok = t[0] > 0 && t[1] > 0 && t[2] > 0 && t[3] > 0;
  if (ok) {
    const double Y = (double)t[0] / ((double)t[0] + 2.0 * (double)t[1]);
    for (int k = 1; k <= 3; ++k) {
      D[k - 1] = (double)k - (((double)(k + 1) * Y) * (double)t[k]) / (double)t[k - 1];
      ok = ok && D[k - 1] > 0.0 && D[k - 1] <= (double)k;
    }
  }
  if (!ok) {
    D[0] = 0.5;
    D[1] = 1.0;
    D[2] = 1.5;
  }
  return !ok;
}

// gamma(c) = ((D(1) N_1 + D(2) N_2) + D(3) N_3) / S
CASR_EST_HD inline double est_gamma(const double D[3], const EstCtx& c) {
#pragma clang fp contract(off)
  const double a = D[0] * (double)c.n[1];
  const double b = D[1] * (double)c.n[2];
  const double d = D[2] * (double)c.n[3];
  return ((a + b) + d) / (double)c.n[0];
}

// u = (a - D(min(a, 3))) / S; 0 for a = 0 (the never seen <unk>)
CASR_EST_HD inline double est_u(uint32_t a, const double D[3], uint32_t S) {
#pragma clang fp contract(off)
  if (a == 0) return 0.0;
  return ((double)a - D[(a < 3 ? a : 3) - 1]) / (double)S;
}

// p_1 = u + gamma_1 / |W|
CASR_EST_HD inline double est_p1(double u, double gamma0, uint32_t W) {
#pragma clang fp contract(off)
  const double q = gamma0 / (double)W;
  return u + q;
}

// p_n = u + gamma p_{n-1}: a multiplication, then an addition
CASR_EST_HD inline double est_interp(double u, double gamma, double lower) {
#pragma clang fp contract(off)
  const double q = gamma * lower;
  return u + q;
}

// probabilities: slot s of order n writes the gamma it carries as a context (orders below the top one;
// 0 where nothing follows it) and, once order n - 1 is done, its p.  false: prefix or suffix missing
CASR_EST_HD inline bool est_prob(const EstView& v, const EstDiscounts& d, int n, uint32_t s) {
  const EstSlot e = v.slot[n - 1][s];
  if (e.key == 0) return true;
  if (n < v.order) {
    const EstCtx c = v.ctx[n - 1][s];
    v.gamma[n - 1][s] = c.n[0] > 0 ? est_gamma(d.D[n], c) : 0.0;
  }
  if (!est_predicted(v, n, e)) {
    v.p[n - 1][s] = 0.0;
    return true;
  }
  const uint32_t a = est_adjusted(v, n, e);
  if (n == 1) {
    v.p[0][s] = est_p1(est_u(a, d.D[0], d.S0), d.gamma0, d.W);
    return true;
  }
  const int64_t fc = est_find(v.slot[n - 2], v.mask[n - 2], est_key_prefix(e.key));
  const int64_t fs = est_find(v.slot[n - 2], v.mask[n - 2], est_key_suffix(e.key, n));
  if (fc < 0 || fs < 0) return false;
  const EstCtx c = v.ctx[n - 2][fc];
  v.p[n - 1][s] = est_interp(est_u(a, d.D[n - 1], c.n[0]), est_gamma(d.D[n - 1], c), v.p[n - 2][fs]);
  return true;
}

// the discounts of every order and the empty context's gamma, from the totals
inline void est_plan_discounts(const EstView& v, const EstTotals& t, EstDiscounts* d, int32_t fallback[NGRAM_MAX_ORDER]) {
  *d = EstDiscounts{};
  for (int n = 1; n <= NGRAM_MAX_ORDER; ++n) fallback[n - 1] = 0;
  for (int n = 1; n <= v.order; ++n) fallback[n - 1] = est_discounts(t.t[n - 1], d->D[n - 1]) ? 1 : 0;
  EstCtx c0;
  for (int i = 0; i < 4; ++i) c0.n[i] = t.ctx0[i];
  d->S0 = t.ctx0[0];
  d->gamma0 = est_gamma(d->D[0], c0);
  // |W|: the unigram types but <s> (always one) and <unk> (where seen), plus 1 for <unk>
  d->W = t.occupied[0] - 1 - (t.unk_seen ? 1 : 0) + 1;
}

// ---------------------------------------------------------------- the size plan
// slots of order n's table for a corpus of P positions (every window ends at one): the power of two
// >= 2 P, and for the unigrams >= 2 (the ids there can be), so there is always an empty slot
inline size_t est_capacity(int n, int64_t P) {
  return ngram_capacity(n == 1 ? std::min<int64_t>(P + 1, NGRAM_MAX_IDS) : P);
}
inline size_t est_slot_bytes(int n, int order) {
  return sizeof(EstSlot) + sizeof(double) + (n < order ? sizeof(EstCtx) + sizeof(double) : 0);
}
// bytes of the tables and totals of one call (each array 256-byte aligned); -1 for what is refused
inline int64_t est_workspace_bytes(int order, int64_t P) {
  if (order < 1 || order > NGRAM_MAX_ORDER || P < 1 || P > EST_MAX_POSITIONS) return -1;
  int64_t b = 256;  // EstTotals
  for (int n = 1; n <= order; ++n) b += (int64_t)est_capacity(n, P) * (int64_t)est_slot_bytes(n, order) + 4 * 256;
  return b;
}
// the view over a zeroed workspace of est_workspace_bytes (host or device memory)
inline EstView est_carve(void* ws, int order, int V, int64_t P, EstTotals** totals) {
  EstView v{};
  v.order = order;
  v.V = V;
  char* p = static_cast<char*>(ws);
  *totals = reinterpret_cast<EstTotals*>(p);
  p += 256;
  auto take = [&](size_t bytes) {
    char* q = p;
    p += (bytes + 255) / 256 * 256;
    return q;
  };
  for (int n = 1; n <= order; ++n) {
    const size_t cap = est_capacity(n, P);
    v.mask[n - 1] = (uint32_t)(cap - 1);
    v.slot[n - 1] = reinterpret_cast<EstSlot*>(take(cap * sizeof(EstSlot)));
    v.p[n - 1] = reinterpret_cast<double*>(take(cap * sizeof(double)));
    if (n < order) {
      v.ctx[n - 1] = reinterpret_cast<EstCtx*>(take(cap * sizeof(EstCtx)));
      v.gamma[n - 1] = reinterpret_cast<double*>(take(cap * sizeof(double)));
    }
  }
  return v;
}

// ---------------------------------------------------------------- the result (both entries)
struct EstResult {
  int order = 0, V = 0;
  int64_t positions = 0, n_types = 0;
  double D[NGRAM_MAX_ORDER][3] = {};
  int32_t fallback[NGRAM_MAX_ORDER] = {};
  double gamma0 = 0.0;
  // per order, dense: key, raw and adjusted count, p and the gamma carried as a context (0: none)
  std::vector<uint64_t> key[NGRAM_MAX_ORDER];
  std::vector<uint32_t> count[NGRAM_MAX_ORDER], adjusted[NGRAM_MAX_ORDER];
  std::vector<double> p[NGRAM_MAX_ORDER], gamma[NGRAM_MAX_ORDER];
  double stage_ms[8] = {};  // device entry: count, extend, stats, prob, compact, copy, 0, total
};

// What both entries do after their tables are dense: the header facts, and the unigram <unk> where the
// corpus never had it (a = 0, u = 0, p = gamma_1 / |W|)
inline void est_finish(EstResult* r, const EstDiscounts& d, const int32_t fallback[NGRAM_MAX_ORDER]) {
  for (int n = 0; n < NGRAM_MAX_ORDER; ++n) {
    for (int k = 0; k < 3; ++k) r->D[n][k] = n < r->order ? d.D[n][k] : 0.0;
    r->fallback[n] = n < r->order ? fallback[n] : 0;
  }
  r->gamma0 = d.gamma0;
  r->n_types = d.W;
  const uint64_t unk = (uint64_t)(r->V + 3);
  if (std::find(r->key[0].begin(), r->key[0].end(), unk) == r->key[0].end()) {
    r->key[0].push_back(unk);
    r->count[0].push_back(0);
    r->adjusted[0].push_back(0);
    r->p[0].push_back(est_p1(0.0, d.gamma0, d.W));
    r->gamma[0].push_back(0.0);
  }
}

// sort every order by key (ascending key order is ascending id-tuple order)
inline void est_sort(EstResult* r) {
  for (int n = 0; n < r->order; ++n) {
    const size_t m = r->key[n].size();
    std::vector<size_t> ix(m);
    std::iota(ix.begin(), ix.end(), (size_t)0);
    const std::vector<uint64_t>& k = r->key[n];
    std::sort(ix.begin(), ix.end(), [&](size_t a, size_t b) { return k[a] < k[b]; });
    auto gather = [&](auto& vec) {
      auto old = vec;
      for (size_t i = 0; i < m; ++i) vec[i] = old[ix[i]];
    };
    gather(r->count[n]);
    gather(r->adjusted[n]);
    gather(r->p[n]);
    gather(r->gamma[n]);
    gather(r->key[n]);
  }
}

// what the stored model holds for entry i of order n: prob = f32(log10 p) (-99 for the unigram <s>),
// backoff = f32(log10 gamma) where the n-gram is a context, else 0
inline float est_stored_prob(const EstResult& r, int n, size_t i) {
  if (n == 1 && r.key[0][i] == (uint64_t)(r.V + 1)) return -99.0f;
  return (float)log10(r.p[n - 1][i]);
}
inline float est_stored_backoff(const EstResult& r, int n, size_t i) {
  const double g = r.gamma[n - 1][i];
  return (n < r.order && g > 0.0) ? (float)log10(g) : 0.0f;
}

// ---------------------------------------------------------------- the host estimator
// tokens [offsets[n]] LM ids, offsets [n + 1] ascending from 0.  NGRAM_ERR_ARG: order outside 1..4,
// n < 1, vocab < 1, a null argument, offsets that do not ascend from 0, an id neither in [0, V) nor
// V + 2.  NGRAM_ERR_UNSUPPORTED: V + 3 > 65,535, more than 2^28 positions.  Within an order the n-grams
// come out in ascending key order.
inline int est_estimate_host(int order, int vocab, const int32_t* tokens, const int64_t* offsets, int64_t n,
                             EstResult* out, std::string* why) {
  auto fail = [&](int code, const std::string& s) {
    if (why) *why = s;
    return code;
  };
  if (order < 1 || order > NGRAM_MAX_ORDER) return fail(NGRAM_ERR_ARG, "order " + std::to_string(order) + " outside 1..4");
  if (n < 1 || vocab < 1) return fail(NGRAM_ERR_ARG, "n < 1 or vocab < 1");
  if (!offsets || !out) return fail(NGRAM_ERR_ARG, "null argument");
  if ((int64_t)vocab + 3 > NGRAM_MAX_IDS)
    return fail(NGRAM_ERR_UNSUPPORTED, "vocab + 3 = " + std::to_string((int64_t)vocab + 3) + " > 65535");
  if (n > EST_MAX_POSITIONS) return fail(NGRAM_ERR_UNSUPPORTED, "more than 2^28 positions");
  if (offsets[0] != 0) return fail(NGRAM_ERR_ARG, "offsets[0] is not 0");
  for (int64_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) return fail(NGRAM_ERR_ARG, "offsets descend at sentence " + std::to_string(i));
  const int64_t total = offsets[n], P = total + n;
  if (P > EST_MAX_POSITIONS) return fail(NGRAM_ERR_UNSUPPORTED, "more than 2^28 positions");
  if (total > 0 && !tokens) return fail(NGRAM_ERR_ARG, "null argument");
  for (int64_t i = 0; i < total; ++i)
    if (!((unsigned)tokens[i] < (unsigned)vocab || tokens[i] == vocab + 2))
      return fail(NGRAM_ERR_ARG, "id " + std::to_string(tokens[i]) + " at token " + std::to_string(i) +
                                     " is neither in [0, V) nor V + 2");
  std::vector<char> ws((size_t)est_workspace_bytes(order, P) + 256, 0);
  EstTotals* t;
  void* base = ws.data() + (256 - reinterpret_cast<uintptr_t>(ws.data()) % 256) % 256;
  const EstView v = est_carve(base, order, vocab, P, &t);
  bool bad = false, ok = true;
  // 1. raw counts
  ok = est_insert<EstHostOps>(v.slot[0], v.mask[0], (uint64_t)(vocab + 1), (uint32_t)n) && ok;
  for (int64_t i = 0; i < n; ++i) {
    const int32_t* tok = tokens + offsets[i];
    const int64_t len = offsets[i + 1] - offsets[i];
    for (int64_t j = 1; j <= len + 1; ++j)
      est_windows(tok, len, j, order, vocab, &bad, [&](uint64_t key) {
        const int m = est_key_order(key);
        ok = est_insert<EstHostOps>(v.slot[m - 1], v.mask[m - 1], key, 1u) && ok;
      });
  }
  // 2. extensions, 4. context statistics, 3. counts of counts
  for (int m = 2; m <= order; ++m)
    for (uint32_t s = 0; s <= v.mask[m - 1]; ++s) ok = est_extend<EstHostOps>(v, m, s) && ok;
  for (int m = 1; m <= order; ++m)
    for (uint32_t s = 0; s <= v.mask[m - 1]; ++s) {
      const EstSlot e = v.slot[m - 1][s];
      if (e.key == 0) continue;
      ++t->occupied[m - 1];
      if (m == 1 && e.key == (uint64_t)(vocab + 3)) t->unk_seen = 1;
      if (!est_predicted(v, m, e)) continue;
      const uint32_t a = est_adjusted(v, m, e);
      if (a >= 1 && a <= 4) ++t->t[m - 1][a - 1];
      if (m == 1) {
        t->ctx0[0] += a;
        ++t->ctx0[a < 3 ? a : 3];
      } else {
        ok = est_ctx_add<EstHostOps>(v, m, s) && ok;
      }
    }
  if (!ok || bad) return fail(NGRAM_ERR_ARG, "the counting tables are inconsistent");
  EstDiscounts d;
  int32_t fallback[NGRAM_MAX_ORDER];
  est_plan_discounts(v, *t, &d, fallback);
  // 5. probabilities, orders ascending
  for (int m = 1; m <= order; ++m)
    for (uint32_t s = 0; s <= v.mask[m - 1]; ++s) ok = est_prob(v, d, m, s) && ok;
  if (!ok) return fail(NGRAM_ERR_ARG, "the counting tables are inconsistent");
  // compaction
  EstResult r;
  r.order = order;
  r.V = vocab;
  r.positions = P;
  for (int m = 1; m <= order; ++m)
    for (uint32_t s = 0; s <= v.mask[m - 1]; ++s) {
      const EstSlot e = v.slot[m - 1][s];
      if (e.key == 0) continue;
      r.key[m - 1].push_back(e.key);
      r.count[m - 1].push_back(e.count);
      r.adjusted[m - 1].push_back(est_adjusted(v, m, e));
      r.p[m - 1].push_back(v.p[m - 1][s]);
      r.gamma[m - 1].push_back(m < order ? v.gamma[m - 1][s] : 0.0);
    }
  est_finish(&r, d, fallback);
  est_sort(&r);
  *out = std::move(r);
  return NGRAM_OK;
}

}  // namespace casr
