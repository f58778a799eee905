// Relative-entropy pruning (Stolcke 1998) of a backoff n-gram LM: casr_lm_prune_host and casr_lm_prune
// (include/casr.h, which has the definition).  This header is the one text both run: lmp_exp10 and
// lmp_log, the order of a sum, the linear query (of the model as given, or of the pruned one through a
// keep bit and a renewed backoff per slot), the context probability, the decision, the backoff rule,
// the per-slot and per-lane stage bodies, the size plan, and the host entry built from them.  The
// kernels (lm_prune.hip) call the same bodies, one wave where the host loops 64 lanes.  Every float64
// operation is one IEEE + - * / in a stated order with contraction off, and exp10 and log are written
// out here instead of taken from a libm, so the device, the host and tests/lm_prune_ref.py give the
// same bits.
// Pure C++ (no HIP runtime): tests/host_asan/lm_prune_check.cpp builds from this header alone.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "ngram_succ.h"

#define CASR_LMP_HD CASR_NGRAM_HD

namespace casr {

constexpr int LMP_LANES = 64;
constexpr uint32_t LMP_NO_SLOT = 0xffffffffu;
constexpr uint32_t LMP_FLAG_INCONSISTENT = 1;  // a listed successor is not in its order's table: refused

// ---------------------------------------------------------------- exp10 and the natural log
CASR_LMP_HD inline uint64_t lmp_bits(double x) {
  uint64_t u;
  __builtin_memcpy(&u, &x, 8);
  return u;
}
CASR_LMP_HD inline double lmp_from_bits(uint64_t u) {
  double x;
  __builtin_memcpy(&x, &u, 8);
  return x;
}
CASR_LMP_HD inline bool lmp_pos_finite(double x) { return x > 0.0 && x < lmp_from_bits(0x7ff0000000000000ull); }

// 10^x.  k = the integer nearest x log2(10) (halves away from zero), r = (x - k HI) - k LO with HI + LO
// = log10(2) and k HI exact, z = r ln(10) (|z| <= 0.35), then the Taylor polynomial of e^z to z^13 in
// Horner form, scaled by 2^k through the exponent bits.  0 below -307, +inf above 308, NaN for NaN.
CASR_LMP_HD inline double lmp_exp10(double x) {
#pragma clang fp contract(off)
  if (!(x == x)) return x;
  if (x > 308.0) return lmp_from_bits(0x7ff0000000000000ull);
  if (x < -307.0) return 0.0;
  const double t = x * 0x1.a934f0979a371p+1;
  const int64_t k = (int64_t)(t < 0.0 ? t - 0.5 : t + 0.5);
  const double kd = (double)k;
  const double r = (x - kd * 0x1.3441350800000p-2) - kd * 0x1.f79fef311f12bp-34;
  const double z = r * 0x1.26bb1bbb55516p+1;
  double p = 0x1.6124613a86d09p-33;  // 1 / 13!
  p = p * z + 0x1.1eed8eff8d898p-29;
  p = p * z + 0x1.ae64567f544e4p-26;
  p = p * z + 0x1.27e4fb7789f5cp-22;
  p = p * z + 0x1.71de3a556c734p-19;
  p = p * z + 0x1.a01a01a01a01ap-16;
  p = p * z + 0x1.a01a01a01a01ap-13;
  p = p * z + 0x1.6c16c16c16c17p-10;
  p = p * z + 0x1.1111111111111p-7;
  p = p * z + 0x1.5555555555555p-5;
  p = p * z + 0x1.5555555555555p-3;
  p = p * z + 0.5;
  p = p * z + 1.0;
  p = p * z + 1.0;
  return p * lmp_from_bits((uint64_t)(k + 1023) << 52);
}

// ln x.  x = 2^e m with m in (sqrt(1/2), sqrt(2)] from the bits (a subnormal is scaled by 2^54 first),
// s = (m - 1) / (m + 1), ln m = 2 s (1 + s^2 / 3 + .. + s^22 / 23) in Horner form, and e ln 2 added as
// e HI + (ln m + e LO).  NaN for x <= 0 and NaN, +inf for +inf.
CASR_LMP_HD inline double lmp_log(double x) {
#pragma clang fp contract(off)
  if (!(x > 0.0)) return lmp_from_bits(0x7ff8000000000000ull);
  uint64_t u = lmp_bits(x);
  if (u >= 0x7ff0000000000000ull) return x;
  int64_t e = 0;
  if (u < 0x0010000000000000ull) {
    x = x * 0x1p54;
    u = lmp_bits(x);
    e = -54;
  }
  e += (int64_t)(u >> 52) - 1023;
  double m = lmp_from_bits((u & 0x000fffffffffffffull) | 0x3ff0000000000000ull);
  if (m > 0x1.6a09e667f3bcdp+0) {
    m = m * 0.5;
    e += 1;
  }
  const double f = m - 1.0;
  const double s = f / (2.0 + f);
  const double z = s * s;
  double p = 0x1.642c8590b2164p-5;  // 1 / 23
  p = p * z + 0x1.8618618618618p-5;
  p = p * z + 0x1.af286bca1af28p-5;
  p = p * z + 0x1.e1e1e1e1e1e1ep-5;
  p = p * z + 0x1.1111111111111p-4;
  p = p * z + 0x1.3b13b13b13b14p-4;
  p = p * z + 0x1.745d1745d1746p-4;
  p = p * z + 0x1.c71c71c71c71cp-4;
  p = p * z + 0x1.2492492492492p-3;
  p = p * z + 0x1.999999999999ap-3;
  p = p * z + 0x1.5555555555555p-2;
  p = p * z + 1.0;
  const double ed = (double)e;
  return ed * 0x1.62e42fec00000p-1 + ((2.0 * s) * p + ed * 0x1.d1cf79abc9e3bp-32);
}

// ---------------------------------------------------------------- the order of a sum
// sum(x_0 .. x_{m-1}): 64 partials s_l = x_l + x_{l+64} + .. ascending (lmp_*_sums below), then this
// tree.  A wave does the same with one partial per lane.
CASR_LMP_HD inline double lmp_tree(double* s) {
#pragma clang fp contract(off)
  for (int d = LMP_LANES / 2; d >= 1; d >>= 1)
    for (int l = 0; l < d; ++l) s[l] = s[l] + s[l + d];
  return s[0];
}

// ---------------------------------------------------------------- the tables of one call
// Per order n (index n - 1): one value per slot of the LM's own table (order 1: per LM id).  P, B: the
// linear values of the model as given; Bn: the renewed backoff (1 until the renew stage writes it);
// delta: the decision's relative entropy (NaN: takes no part); keep, protect: bytes.  Per order n >= 2
// (index n - 2) and entry of its successor list: the n-gram's slot and its lower-order query q.
struct LmpView {
  NgramView m;
  NgramSuccView s;
  double* P[NGRAM_MAX_ORDER];
  double* B[NGRAM_MAX_ORDER];
  double* Bn[NGRAM_MAX_ORDER];
  double* delta[NGRAM_MAX_ORDER];
  uint8_t* keep[NGRAM_MAX_ORDER];
  uint8_t* protect[NGRAM_MAX_ORDER];
  uint32_t* sslot[NGRAM_MAX_ORDER - 1];
  double* qv[NGRAM_MAX_ORDER - 1];
};

struct LmpTotals {
  uint32_t removed[NGRAM_MAX_ORDER];
  uint32_t out[NGRAM_MAX_ORDER];  // compaction cursors
  uint32_t flags;                 // LMP_FLAG_*
  uint32_t pad[7];
};

// what the model has, as the size plan and the entries need it
struct LmpDims {
  int order, V;
  uint32_t cap[NGRAM_MAX_ORDER - 1];      // slots of tab[n - 2]
  int64_t list_len[NGRAM_MAX_ORDER - 1];  // entries of list[n - 2]
  int64_t count[NGRAM_MAX_ORDER];         // n-grams per order as given to casr_lm_create
  bool unk_given;                         // the <unk> unigram was given (else it is the default, not listed)
};
CASR_LMP_HD inline uint32_t lmp_slots(const LmpDims& d, int n) { return n == 1 ? (uint32_t)d.V + 3u : d.cap[n - 2]; }

// every occupied slot of an order >= 2, dense (the compact stage's output)
struct LmpDense {
  uint64_t* key;
  double *bn, *delta;
  float *prob, *backoff;
  uint8_t* kept;
  uint32_t room;
};

// The workspace: totals, the per-slot and per-entry arrays, the dense output.  base == null: the size only.
inline int64_t lmp_carve(void* base, const LmpDims& d, LmpView* v, LmpDense* dense, LmpTotals** tot) {
  size_t off = 0;
  auto take = [&](size_t bytes) -> char* {
    char* p = base ? static_cast<char*>(base) + off : nullptr;
    off += (bytes + 255) / 256 * 256;
    return p;
  };
  LmpTotals* t = reinterpret_cast<LmpTotals*>(take(sizeof(LmpTotals)));
  if (tot) *tot = t;
  LmpView w{};
  LmpDense dn[NGRAM_MAX_ORDER] = {};
  for (int n = 1; n <= d.order; ++n) {
    const size_t slots = lmp_slots(d, n);
    w.protect[n - 1] = reinterpret_cast<uint8_t*>(take(slots));  // (first: the part lmp_zeroed_bytes covers)
    w.keep[n - 1] = reinterpret_cast<uint8_t*>(take(slots));
  }
  for (int n = 1; n <= d.order; ++n) {
    const size_t slots = lmp_slots(d, n);
    w.P[n - 1] = reinterpret_cast<double*>(take(8 * slots));
    w.B[n - 1] = reinterpret_cast<double*>(take(8 * slots));
    w.Bn[n - 1] = reinterpret_cast<double*>(take(8 * slots));
    w.delta[n - 1] = reinterpret_cast<double*>(take(8 * slots));
    if (n >= 2) {
      const size_t len = (size_t)d.list_len[n - 2], c = (size_t)d.count[n - 1];
      w.sslot[n - 2] = reinterpret_cast<uint32_t*>(take(4 * len));
      w.qv[n - 2] = reinterpret_cast<double*>(take(8 * len));
      dn[n - 1].room = (uint32_t)c;
      dn[n - 1].key = reinterpret_cast<uint64_t*>(take(8 * c));
      dn[n - 1].bn = reinterpret_cast<double*>(take(8 * c));
      dn[n - 1].delta = reinterpret_cast<double*>(take(8 * c));
      dn[n - 1].prob = reinterpret_cast<float*>(take(4 * c));
      dn[n - 1].backoff = reinterpret_cast<float*>(take(4 * c));
      dn[n - 1].kept = reinterpret_cast<uint8_t*>(take(c));
    }
  }
  if (v) {
    const NgramView m = v->m;
    const NgramSuccView s = v->s;
    *v = w;
    v->m = m;
    v->s = s;
  }
  if (dense)
    for (int n = 0; n < NGRAM_MAX_ORDER; ++n) dense[n] = dn[n];
  return (int64_t)off;
}
// the leading part the device entry zeroes: totals, protect, keep
inline int64_t lmp_zeroed_bytes(const LmpDims& d) {
  size_t off = (sizeof(LmpTotals) + 255) / 256 * 256;
  for (int n = 1; n <= d.order; ++n) off += 2 * (((size_t)lmp_slots(d, n) + 255) / 256 * 256);
  return (int64_t)off;
}

// ---------------------------------------------------------------- lookups
// slot of a key in tab[n - 2] (n >= 2), -1 where the model has no such n-gram; bounded by the capacity
CASR_LMP_HD inline int64_t lmp_find(const NgramView& m, int n, uint64_t key) {
  NgramProbe q;
  float pp, bb;
  ngram_probe_start(q, m.tab[n - 2], m.mask[n - 2], key);
  return ngram_probe_finish(q, &pp, &bb) ? (int64_t)q.s : -1;
}

// Q(w | c) in the linear domain: c[0 .. nc) LM ids with a unigram, nearest predecessor first, nc <= order
// - 1.  m = the largest order whose n-gram (c[m - 2] .. c[0], w) is present, the value starts from P_m
// and is multiplied by B(c[j - 1] .. c[0]) for j = m .. nc where that j-gram is present.  pruned: present
// means kept, and B is the renewed backoff.  ngram_term's probe structure: the first read of every
// lookup is issued before any is examined.
CASR_LMP_HD inline double lmp_query(const LmpView& v, bool pruned, const int32_t* c, int nc, int w) {
#pragma clang fp contract(off)
  const NgramView& m = v.m;
  uint64_t kw = (uint64_t)(uint32_t)(w + 1), kc = 0;
  NgramProbe qw[NGRAM_MAX_ORDER - 1], qc[NGRAM_MAX_ORDER - 1];
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
  double* const* Bv = pruned ? v.Bn : v.B;
  double p = v.P[0][w];
  int mo = 1;
  double bo[NGRAM_MAX_ORDER - 1] = {1.0, 1.0, 1.0};
  bool has[NGRAM_MAX_ORDER - 1] = {false, false, false};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 1; j < NGRAM_MAX_ORDER; ++j) {
    if (j > nc) break;
    float pp, bb;
    if (ngram_probe_finish(qw[j - 1], &pp, &bb) && (!pruned || v.keep[j][qw[j - 1].s])) {
      p = v.P[j][qw[j - 1].s];
      mo = j + 1;
    }
    if (j == 1) {
      has[0] = true;
      bo[0] = Bv[0][c[0]];
    } else if (ngram_probe_finish(qc[j - 1], &pp, &bb) && (!pruned || v.keep[j - 1][qc[j - 1].s])) {
      has[j - 1] = true;
      bo[j - 1] = Bv[j - 1][qc[j - 1].s];
    }
  }
  for (int j = mo; j <= nc; ++j)
    if (has[j - 1]) p = p * bo[j - 1];
  return p;
}

// ph(h) of the context c[0 .. L) (nearest first, so h_i = c[L - i]): the product over i = 1 .. L,
// ascending, of Q(h_i | h_1 .. h_{i-1}), with P_1(</s>) in place of the factor of <s>
CASR_LMP_HD inline double lmp_ph(const LmpView& v, const int32_t* c, int L) {
#pragma clang fp contract(off)
  double ph = 1.0;
  for (int i = 1; i <= L; ++i) {
    const int w = c[L - i];
    const double f = w == v.m.V ? v.P[0][v.m.V + 1] : lmp_query(v, false, c + (L - i + 1), i - 1, w);
    ph = ph * f;
  }
  return ph;
}

// ---------------------------------------------------------------- stage: linearise (one per slot)
CASR_LMP_HD inline bool lmp_key_reachable(const NgramView& m, uint64_t key, int n) {
  bool ok = true;
  for (int e = 0; e < n; ++e) {
    const int id = (int)((key >> (16 * e)) & 0xffff) - 1;
    ok = ok && m.redirect[id] == id;
  }
  return ok;
}
// P, B, Bn = 1, delta = NaN, keep = 1 for an n-gram of the model.  An n-gram holding a word without a
// unigram takes no further part; as a kept n-gram it protects its prefix
CASR_LMP_HD inline void lmp_linearise(const LmpView& v, int n, uint32_t s) {
  float prob, backoff;
  if (n == 1) {
    prob = v.m.uni[s].prob;
    backoff = v.m.uni[s].backoff;
  } else {
    const NgramEntry e = v.m.tab[n - 2][s];
    if (e.key == 0) return;  // (keep stays 0)
    prob = e.prob;
    backoff = e.backoff;
    if (n >= 3 && !lmp_key_reachable(v.m, e.key, n)) {
      const int64_t hs = lmp_find(v.m, n - 1, e.key >> 16);
      if (hs >= 0) v.protect[n - 2][hs] = 1;
    }
  }
  v.P[n - 1][s] = lmp_exp10((double)prob);
  v.B[n - 1][s] = lmp_exp10((double)backoff);
  v.Bn[n - 1][s] = 1.0;
  v.delta[n - 1][s] = lmp_from_bits(0x7ff8000000000000ull);
  v.keep[n - 1][s] = 1;
}

// ---------------------------------------------------------------- stage: decide (one wave per context)
// a context h of order-n successors: its words nearest first, its own slot in order n - 1 (the id at
// n = 2; -1 where the model has no such n-gram), a = B(h), ph(h)
struct LmpCtx {
  int n;
  uint64_t kc;
  NgramSuccRange rg;
  int32_t c[NGRAM_MAX_ORDER - 1];
  int64_t hslot;
};
// work items of order n: LM ids at n = 2, the slots of the context table above
CASR_LMP_HD inline uint32_t lmp_ctx_items(const LmpView& v, int n) { return n == 2 ? (uint32_t)v.m.V + 3u : v.s.cmask[n - 3] + 1u; }
// false: the item holds no context
CASR_LMP_HD inline bool lmp_ctx_prepare(const LmpView& v, int n, uint32_t item, LmpCtx* x) {
  x->n = n;
  if (n == 2) {
    x->kc = (uint64_t)item + 1;
    x->rg = v.s.dir[item];
  } else {
    const NgramCtxEntry e = v.s.ctab[n - 3][item];
    x->kc = e.key;
    x->rg = NgramSuccRange{e.offset, e.count};
    if (e.key == 0) return false;
  }
  if (x->rg.count == 0) return false;
  for (int j = 0; j < NGRAM_MAX_ORDER - 1; ++j) x->c[j] = j < n - 1 ? (int32_t)((x->kc >> (16 * j)) & 0xffff) - 1 : 0;
  x->hslot = n == 2 ? (int64_t)item : lmp_find(v.m, n - 1, x->kc);
  return true;
}

// lane's partials of sum P_n(h v) and sum Q(v | h'); every successor's slot and q are written for the
// stages after.  *bad: a listed successor is not in the table
CASR_LMP_HD inline void lmp_decide_sums(const LmpView& v, const LmpCtx& x, int lane, double* sp, double* sq, bool* bad) {
#pragma clang fp contract(off)
  const int n = x.n;
  double a = 0.0, b = 0.0;
  for (uint32_t i = (uint32_t)lane; i < x.rg.count; i += LMP_LANES) {
    const size_t at = (size_t)x.rg.offset + i;
    const int w = v.s.list[n - 2][at].w;
    const int64_t slot = lmp_find(v.m, n, (x.kc << 16) | (uint64_t)(uint32_t)(w + 1));
    if (slot < 0) {
      *bad = true;
      v.sslot[n - 2][at] = LMP_NO_SLOT;
      v.qv[n - 2][at] = 0.0;
      continue;
    }
    const double q = lmp_query(v, false, x.c, n - 2, w);
    v.sslot[n - 2][at] = (uint32_t)slot;
    v.qv[n - 2][at] = q;
    a = a + v.P[n - 1][slot];
    b = b + q;
  }
  *sp = a;
  *sq = b;
}

// the relative entropy of removing one n-gram; +inf where a precondition fails (never removable)
CASR_LMP_HD inline double lmp_delta(double ph, double p, double q, double a, double num, double den) {
#pragma clang fp contract(off)
  const double np = num + p, dq = den + q;
  if (!(lmp_pos_finite(p) && lmp_pos_finite(q) && lmp_pos_finite(a) && lmp_pos_finite(np) && lmp_pos_finite(dq)))
    return lmp_from_bits(0x7ff0000000000000ull);
  const double a1 = np / dq;
  const double la1 = lmp_log(a1);
  const double t0 = p * ((lmp_log(q) + la1) - lmp_log(p));
  const double t1 = num * (la1 - lmp_log(a));
  return -ph * (t0 + t1);
}

// lane's n-grams of the context: delta and the keep bit.  Returns whether it kept one; *removed += the
// others
CASR_LMP_HD inline bool lmp_decide_lane(const LmpView& v, const LmpCtx& x, int lane, double a, double ph, double num,
                                        double den, double tau, uint32_t* removed) {
  const int n = x.n;
  bool any = false;
  for (uint32_t i = (uint32_t)lane; i < x.rg.count; i += LMP_LANES) {
    const size_t at = (size_t)x.rg.offset + i;
    const uint32_t slot = v.sslot[n - 2][at];
    if (slot == LMP_NO_SLOT) continue;
    const double d = lmp_delta(ph, v.P[n - 1][slot], v.qv[n - 2][at], a, num, den);
    const bool keep = v.protect[n - 1][slot] != 0 || !(d < tau);
    v.delta[n - 1][slot] = d;
    v.keep[n - 1][slot] = keep ? 1 : 0;
    any = any || keep;
    if (!keep) ++*removed;
  }
  return any;
}

// ---------------------------------------------------------------- stage: renew (one wave per context)
// whether the context is a kept n-gram (unigrams always are): only then is there a backoff to renew
CASR_LMP_HD inline bool lmp_renew_wanted(const LmpView& v, const LmpCtx& x) {
  return x.hslot >= 0 && (x.n == 2 || v.keep[x.n - 2][x.hslot] != 0);
}
// lane's partials over the kept successors; each successor keeps its place in the list, a removed one
// adds nothing
CASR_LMP_HD inline void lmp_renew_sums(const LmpView& v, const LmpCtx& x, int lane, double* sp, double* sq) {
#pragma clang fp contract(off)
  const int n = x.n;
  double a = 0.0, b = 0.0;
  for (uint32_t i = (uint32_t)lane; i < x.rg.count; i += LMP_LANES) {
    const size_t at = (size_t)x.rg.offset + i;
    const uint32_t slot = v.sslot[n - 2][at];
    if (slot == LMP_NO_SLOT || !v.keep[n - 1][slot]) continue;
    a = a + v.P[n - 1][slot];
    b = b + lmp_query(v, true, x.c, n - 2, v.s.list[n - 2][at].w);
  }
  *sp = a;
  *sq = b;
}
// B' = num' / den'; 0 marks a degenerate context (stored as -99)
CASR_LMP_HD inline double lmp_backoff(double sp, double sq) {
#pragma clang fp contract(off)
  const double num = 1.0 - sp, den = 1.0 - sq;
  if (!(lmp_pos_finite(num) && lmp_pos_finite(den))) return 0.0;
  const double b = num / den;
  return lmp_pos_finite(b) ? b : 0.0;
}

// ---------------------------------------------------------------- the result
struct LmpResult {
  int order = 0, V = 0;
  double theta = 0.0, tau = 0.0;
  bool removed_any = false;
  // every n-gram of the model as given, per order
  std::vector<uint64_t> key[NGRAM_MAX_ORDER];
  std::vector<float> prob[NGRAM_MAX_ORDER], backoff[NGRAM_MAX_ORDER];
  std::vector<double> bn[NGRAM_MAX_ORDER], delta[NGRAM_MAX_ORDER];
  std::vector<uint8_t> kept[NGRAM_MAX_ORDER];
  // lmp_finish: the stored and the float64 backoff of every n-gram (read for the kept ones)
  std::vector<float> out_backoff[NGRAM_MAX_ORDER];
  std::vector<double> out_b64[NGRAM_MAX_ORDER];
  int64_t count_out[NGRAM_MAX_ORDER] = {}, n_protected[NGRAM_MAX_ORDER] = {}, n_degenerate = 0;
  double stage_ms[8] = {};  // linearise, decide, renew, compact, copy, -, -, all (the device entry)
};

inline void lmp_key_ids(uint64_t key, int n, int32_t* ids) {
  for (int e = 0; e < n; ++e) ids[e] = (int32_t)((key >> (16 * (n - 1 - e))) & 0xffff) - 1;
}

// the unigrams of the result: every id with a unigram (<unk> only where it was given)
inline void lmp_result_unigrams(const NgramTables& t, const LmpDims& d, const double* bn, LmpResult* r) {
  const double nan = lmp_from_bits(0x7ff8000000000000ull);
  for (int id = 0; id < t.V + 3; ++id) {
    if (t.redirect[id] != id || (id == t.V + 2 && !d.unk_given)) continue;
    r->key[0].push_back((uint64_t)id + 1);
    r->prob[0].push_back(t.uni[id].prob);
    r->backoff[0].push_back(t.uni[id].backoff);
    r->bn[0].push_back(bn[id]);
    r->delta[0].push_back(nan);
    r->kept[0].push_back(1);
  }
}

// Nothing removed: the backoffs as given.  Else 0 at the top order, the given one for an n-gram that
// takes no part, f32(log10 B') for every other (-99 for a degenerate context).  log10 is the host's,
// for both entries.
inline void lmp_finish(LmpResult* r) {
  r->n_degenerate = 0;
  for (int n = 1; n <= r->order; ++n) {
    const size_t c = r->key[n - 1].size();
    r->out_backoff[n - 1].resize(c);
    r->out_b64[n - 1].resize(c);
    r->count_out[n - 1] = r->n_protected[n - 1] = 0;
    for (size_t i = 0; i < c; ++i) {
      const bool kept = r->kept[n - 1][i] != 0;
      const double d = r->delta[n - 1][i];
      if (kept) ++r->count_out[n - 1];
      if (kept && d < r->tau) ++r->n_protected[n - 1];
      float b = r->backoff[n - 1][i];
      double b64 = lmp_exp10((double)b);
      if (r->removed_any && n == r->order) {
        b = 0.0f;
        b64 = 1.0;
      } else if (r->removed_any && (n == 1 || d == d)) {
        b64 = r->bn[n - 1][i];
        if (b64 > 0.0) {
          b = (float)log10(b64);
        } else {
          b = -99.0f;
          if (kept) ++r->n_degenerate;
        }
      }
      r->out_backoff[n - 1][i] = b;
      r->out_b64[n - 1][i] = b64;
    }
  }
}

// ---------------------------------------------------------------- the host entry
inline LmpDims lmp_dims(const NgramTables& t, const NgramSuccTables& st, const int64_t* count, bool unk_given) {
  LmpDims d{};
  d.order = t.order;
  d.V = t.V;
  for (int i = 0; i < NGRAM_MAX_ORDER - 1; ++i) {
    d.cap[i] = (uint32_t)t.tab[i].size();
    d.list_len[i] = (int64_t)st.list[i].size();
  }
  for (int i = 0; i < NGRAM_MAX_ORDER; ++i) d.count[i] = i < t.order ? count[i] : 0;
  d.unk_given = unk_given;
  return d;
}

// theta >= 0 and finite (the caller has checked).  false: the object is inconsistent (cannot happen
// for one casr_lm_create built).  Within an order the n-grams come out in ascending key order.
inline bool lmp_prune_host(const NgramTables& t, const NgramSuccTables& st, const LmpDims& d, double theta, LmpResult* out) {
  const int N = t.order;
  std::vector<char> ws((size_t)lmp_carve(nullptr, d, nullptr, nullptr, nullptr), 0);
  LmpView v{};
  v.m = t.view();
  v.s = st.view();
  LmpDense dense[NGRAM_MAX_ORDER];
  LmpTotals* tot = nullptr;
  lmp_carve(ws.data(), d, &v, dense, &tot);
  LmpResult r;
  r.order = N;
  r.V = t.V;
  r.theta = theta;
  r.tau = lmp_log(1.0 + theta);
  for (int n = 1; n <= N; ++n)
    for (uint32_t s = 0; s < lmp_slots(d, n); ++s) lmp_linearise(v, n, s);
  bool bad = false;
  double sp[LMP_LANES], sq[LMP_LANES];
  for (int n = N; n >= 2; --n) {
    for (uint32_t item = 0; item < lmp_ctx_items(v, n); ++item) {
      LmpCtx x;
      if (!lmp_ctx_prepare(v, n, item, &x)) continue;
      for (int l = 0; l < LMP_LANES; ++l) lmp_decide_sums(v, x, l, &sp[l], &sq[l], &bad);
      const double num = 1.0 - lmp_tree(sp), den = 1.0 - lmp_tree(sq);
      const double a = x.hslot >= 0 ? v.B[n - 2][x.hslot] : 1.0;
      const double ph = lmp_ph(v, x.c, n - 1);
      bool any = false;
      for (int l = 0; l < LMP_LANES; ++l) any = lmp_decide_lane(v, x, l, a, ph, num, den, r.tau, &tot->removed[n - 1]) || any;
      if (any && n >= 3 && x.hslot >= 0) v.protect[n - 2][x.hslot] = 1;
    }
  }
  if (bad) return false;
  for (int n = 2; n <= N; ++n) r.removed_any = r.removed_any || tot->removed[n - 1] != 0;
  if (r.removed_any) {
    for (int n = 2; n <= N; ++n) {
      for (uint32_t item = 0; item < lmp_ctx_items(v, n); ++item) {
        LmpCtx x;
        if (!lmp_ctx_prepare(v, n, item, &x) || !lmp_renew_wanted(v, x)) continue;
        for (int l = 0; l < LMP_LANES; ++l) lmp_renew_sums(v, x, l, &sp[l], &sq[l]);
        const double a = lmp_tree(sp), b = lmp_tree(sq);
        v.Bn[n - 2][x.hslot] = lmp_backoff(a, b);
      }
    }
  }
  lmp_result_unigrams(t, d, v.Bn[0], &r);
  for (int n = 2; n <= N; ++n) {
    std::vector<uint32_t> slots;
    for (uint32_t s = 0; s < d.cap[n - 2]; ++s)
      if (t.tab[n - 2][s].key != 0) slots.push_back(s);
    std::sort(slots.begin(), slots.end(),
              [&](uint32_t a, uint32_t b) { return t.tab[n - 2][a].key < t.tab[n - 2][b].key; });
    for (uint32_t s : slots) {
      const NgramEntry& e = t.tab[n - 2][s];
      r.key[n - 1].push_back(e.key);
      r.prob[n - 1].push_back(e.prob);
      r.backoff[n - 1].push_back(e.backoff);
      r.bn[n - 1].push_back(v.Bn[n - 1][s]);
      r.delta[n - 1].push_back(v.delta[n - 1][s]);
      r.kept[n - 1].push_back(v.keep[n - 1][s]);
    }
  }
  lmp_finish(&r);
  *out = std::move(r);
  return true;
}

}  // namespace casr
