// N-best lists and confusion networks over a beam's finished hypotheses (include/casr.h
// casr_posterior_units_host, casr_nbest_host, casr_confusion*, casr_beam_nbest, casr_beam_confusion): the
// unit rule, the N-best order, the vote walk, the slot order and the plan of a call, once, as plain C++
// that the kernels (confusion.hip), the host entry points and the sanitizer program
// (tests/host_asan/confusion_check.cpp) all compile.  The cell rule, the direction code and the layout
// of its bits are edit_plan.h's; the formulas are casr.h's and tests/confusion_ref.py restates them.
#pragma once
#include "edit_plan.h"

namespace casr {

constexpr int CN_EPS = CASR_CN_EPS;    // the vote "nothing here"
constexpr int CN_NONE = CASR_CN_NONE;  // an unused entry of a slot
constexpr int CN_MAX_M = CASR_CN_MAX_M;
constexpr int CN_MAX_N = CASR_NBEST_MAX_N;
constexpr int CN_MAX_LEN = EDIT_MBR_MAX_LEN;  // D's cells are bytes
constexpr int CN_MAX_K = 16;
constexpr int CN_MAX_VOCAB = 32767;  // votes are int16
constexpr int CN_WAVE = 64;
// reduce workgroups per utterance: each takes every 32nd slot.  CASR_CN_REDUCE_GROUPS: diagnostic builds
// only (the A/B of DESIGN.md 3.10; 511 is one wave per slot)
#ifndef CASR_CN_REDUCE_GROUPS
#define CASR_CN_REDUCE_GROUPS 32
#endif
constexpr int CN_REDUCE_GROUPS = CASR_CN_REDUCE_GROUPS;
constexpr int64_t CN_UNIT_ONE = (int64_t)1 << 32;

// ---------------------------------------------------------------- the unit rule
// u = (int64) floor(w 2^32), 0 for a NaN; w = mbr_weight(..) lies in [0, 1], the clamp is for the rest
CASR_EDIT_HD inline int64_t cn_unit(double w) {
  if (!(w == w)) return 0;
  const double x = floor(w * 4294967296.0);
  return x <= 0.0 ? 0 : x >= 4294967296.0 ? CN_UNIT_ONE : (int64_t)x;
}

// a unit handed in (casr_confusion*): clamped into [0, 2^32], so that no sum can overflow
CASR_EDIT_HD inline int64_t cn_unit_clamp(int64_t u) { return u < 0 ? 0 : u > CN_UNIT_ONE ? CN_UNIT_ONE : u; }

// a token id outside [0, V) is 0 before anything else
CASR_EDIT_HD inline int32_t cn_token(int32_t t, int V) { return (uint32_t)t >= (uint32_t)V ? 0 : t; }

// ---------------------------------------------------------------- the N-best order
// a c that is no NaN before a NaN, then the larger c, then the lower flat index.  A total order: a
// record's rank is the number of records before it
CASR_EDIT_HD inline bool cn_before(double ca, int ia, double cb, int ib) {
  const bool na = ca != ca, nb = cb != cb;
  if (na != nb) return nb;
  if (!na && ca != cb) return ca > cb;
  return ia < ib;
}

// ---------------------------------------------------------------- the slot order
// the larger mass, then the smaller token (EPS = -1 first)
CASR_EDIT_HD inline bool cn_slot_before(int64_t ma, int32_t ta, int64_t mb, int32_t tb) {
  return ma != mb ? ma > mb : ta < tb;
}

CASR_EDIT_HD inline int cn_slots(int m) { return 2 * m + 1; }

// ---------------------------------------------------------------- the vote walk
// The backtrace of the script turning the pivot a[0 .. m) into b[0 .. n), edit_backtrace's rules in
// edit_backtrace's order, row by row from m down: dir(i, j) is the direction code of interior cell
// (i, j), 0-based; tok(j) is b[j]; put(slot, token) receives exactly one vote for every slot, from slot
// 2m down to 0.  At row i the inserts come first (the last one met, the smallest j, stands in gap 2i),
// then the move that leaves the row votes at slot 2i - 1; what is left of b at row 0 are inserts into
// gap 0, of which b[0] stands.
template <class Dir, class Tok, class Put>
CASR_EDIT_HD inline void cn_walk(int m, int n, Dir dir, Tok tok, Put put) {
  int j = n;
  for (int i = m; i > 0; --i) {
    int32_t gap = CN_EPS;
    int d = EDIT_DELETE;  // the first column: only deletes are left
    while (j > 0) {
      d = dir(i - 1, j - 1);
      if (d != EDIT_INSERT) break;
      gap = tok(j - 1);
      --j;
      d = EDIT_DELETE;
    }
    put(2 * i, gap);
    if (d == EDIT_DELETE) {
      put(2 * i - 1, CN_EPS);
    } else {
      put(2 * i - 1, tok(j - 1));
      --j;
    }
  }
  put(0, j > 0 ? tok(0) : CN_EPS);
}

// ---------------------------------------------------------------- one utterance on the host
// On the expanded records of casr_beam_records: tokens [L k][L], score, valid, lm (or null) [L k]; flat
// index = step k + rank, a record at step l holds l tokens; nothing past a record's length is read.

// unit [L k] (0 where there is no record); returns U
inline int64_t cn_units_utterance_host(const float* score, const uint8_t* valid, const float* lm, int L, int k,
                                       double scale, double lm_weight, double length_weight, int64_t* unit) {
  const int LK = L * k;
  double cmax = NAN;
  for (int i = 0; i < LK; ++i)
    if (valid[i]) cmax = mbr_cmax(cmax, mbr_comb(score[i], lm ? lm[i] : 0.f, i / k, lm_weight, length_weight));
  int64_t total = 0;
  for (int i = 0; i < LK; ++i) {
    unit[i] = 0;
    if (!valid[i]) continue;
    const double c = mbr_comb(score[i], lm ? lm[i] : 0.f, i / k, lm_weight, length_weight);
    unit[i] = cn_unit(mbr_weight(scale, c, cmax));
    total += unit[i];
  }
  return total;
}

// index [N], toks [N][L], len [N], comb [N]
inline void cn_nbest_utterance_host(const int32_t* tokens, const float* score, const uint8_t* valid, const float* lm,
                                    int L, int k, int N, double lm_weight, double length_weight, int32_t* index,
                                    int32_t* toks, int32_t* len, double* comb) {
  const int LK = L * k;
  for (int r = 0; r < N; ++r) {
    index[r] = -1;
    len[r] = 0;
    comb[r] = 0.0;
    for (int s = 0; s < L; ++s) toks[(size_t)r * L + s] = -1;
  }
  std::vector<int32_t> list;
  std::vector<double> c;
  for (int i = 0; i < LK; ++i)
    if (valid[i]) {
      list.push_back(i);
      c.push_back(mbr_comb(score[i], lm ? lm[i] : 0.f, i / k, lm_weight, length_weight));
    }
  const int n = (int)list.size();
  for (int p = 0; p < n; ++p) {
    int rank = 0;
    for (int q = 0; q < n && rank < N; ++q) rank += q != p && cn_before(c[q], list[q], c[p], list[p]);
    if (rank >= N) continue;
    const int l = list[p] / k;
    index[rank] = list[p];
    len[rank] = l;
    comb[rank] = c[p];
    for (int s = 0; s < l; ++s) toks[(size_t)rank * L + s] = tokens[(size_t)list[p] * L + s];
  }
}

// The direction bits of pivot a[0 .. m) against b[0 .. n), edit_plan.h's layout, column by column as a
// lane of the kernel fills them: col rolls D[.][j] over j
inline void cn_fill_bits(const int32_t* a, int m, const int32_t* b, int n, std::vector<uint32_t>& bits,
                         std::vector<int32_t>& col) {
  const int stride = edit_bits_stride(m);
  bits.assign(edit_bits_words(m, n), 0u);
  col.resize((size_t)m + 1);
  for (int i = 0; i <= m; ++i) col[i] = i;
  for (int j = 0; j < n; ++j) {
    int diag = col[0], up = j + 1;
    col[0] = up;
    const int32_t bj = b[j];
    for (int i = 0; i < m; ++i) {
      const int left = col[i + 1];
      const bool match = a[i] == bj;
      const int d = edit_cell(match, diag, up, left);
      bits[edit_bits_word(i, j, stride)] |= (uint32_t)edit_dir(match, d, diag, up) << edit_bits_shift(i);
      col[i + 1] = d;
      diag = left;
      up = d;
    }
  }
}

// unit [L k] is an input; pivot a flat index.  slot_token / slot_mass [2 L + 1][M], pivot_mass [L].
// Returns n_slots; *total = U (also without a pivot)
inline int32_t cn_confusion_utterance_host(const int32_t* tokens, const uint8_t* valid, const int64_t* unit,
                                           int32_t pivot, int L, int k, int V, int M, int32_t* slot_token,
                                           int64_t* slot_mass, int64_t* pivot_mass, int64_t* total) {
  const int LK = L * k, SM = cn_slots(L);
  for (int e = 0; e < SM * M; ++e) {
    slot_token[e] = CN_NONE;
    slot_mass[e] = 0;
  }
  for (int i = 0; i < L; ++i) pivot_mass[i] = 0;
  std::vector<int32_t> list;
  int64_t U = 0;
  for (int i = 0; i < LK; ++i)
    if (valid[i]) {
      list.push_back(i);
      U += cn_unit_clamp(unit[i]);
    }
  *total = U;
  if (pivot < 0 || pivot >= LK || !valid[pivot]) return 0;
  const int n = (int)list.size(), m = pivot / k, S = cn_slots(m);
  std::vector<int32_t> a((size_t)m), b;
  for (int i = 0; i < m; ++i) a[i] = cn_token(tokens[(size_t)pivot * L + i], V);
  std::vector<int32_t> votes((size_t)n * S);
  std::vector<uint32_t> bits;
  std::vector<int32_t> col;
  for (int p = 0; p < n; ++p) {
    const int l = list[p] / k, stride = edit_bits_stride(m);
    b.resize((size_t)l);
    for (int j = 0; j < l; ++j) b[j] = cn_token(tokens[(size_t)list[p] * L + j], V);
    cn_fill_bits(a.data(), m, b.data(), l, bits, col);
    int32_t* v = votes.data() + (size_t)p * S;
    cn_walk(
        m, l, [&](int i, int j) { return (int)((bits[edit_bits_word(i, j, stride)] >> edit_bits_shift(i)) & 3); },
        [&](int j) { return b[j]; }, [&](int s, int32_t t) { v[s] = t; });
  }
  // per slot: masses by bin = token + 1 (EPS in bin 0), the touched bins, M rounds of the arg-max
  std::vector<int64_t> hist((size_t)V + 1, 0);
  std::vector<int32_t> touched;
  for (int s = 0; s < S; ++s) {
    touched.clear();
    for (int p = 0; p < n; ++p) {
      const int64_t u = cn_unit_clamp(unit[list[p]]);
      if (u == 0) continue;
      const int bin = votes[(size_t)p * S + s] + 1;
      if (hist[bin] == 0) touched.push_back(bin);
      hist[bin] += u;
    }
    if (s & 1) pivot_mass[s >> 1] = hist[a[s >> 1] + 1];
    for (int r = 0; r < M; ++r) {
      int best = -1;
      for (int32_t bin : touched)
        if (hist[bin] > 0 && (best < 0 || cn_slot_before(hist[bin], bin - 1, hist[best], best - 1))) best = bin;
      if (best < 0) break;
      slot_token[s * M + r] = best - 1;
      slot_mass[s * M + r] = hist[best];
      hist[best] = 0;
    }
    for (int32_t bin : touched) hist[bin] = 0;
  }
  return S;
}

// ---------------------------------------------------------------- the plan
// align: one wave per workgroup, a lane per record (the pivot's tokens uniform).  A lane's LDS, all of it
// [.][lane]: its record's tokens as int16 [L], a rolling column of D as bytes [L + 1], and the direction
// bits of L x L cells, edit_plan.h's words.  Shared by the wave: the pivot's tokens [L] int32 and, read
// off the beam tree (casr_beam_confusion), the tree's back-pointers and tokens [L k] int32 each.  Where
// 64 lanes do not fit the 160 KB of a CU fewer lanes work (down to 1).
// reduce: one wave per workgroup; int64 masses over V + 1 bins, the touched bins' list [L k] int32.
struct ConfusionPlan {
  bool ok;
  int lanes;             // records per align workgroup
  int align_groups;      // align workgroups per utterance: ceil(L k / lanes)
  size_t align_lds;
  bool align_raise;      // past the 64 KB a kernel gets without asking
  int reduce_groups;     // reduce workgroups per utterance
  size_t reduce_lds;
  bool reduce_raise;
  size_t votes_bytes;    // [B][2 L + 1][L k] int16, slot-major
  size_t ws_bytes;       // the whole handle-owned workspace (confusion.hip carve_confusion)
};

CASR_EDIT_HD inline size_t cn_lane_bytes(int L) {
  return sizeof(int16_t) * (size_t)L + (size_t)(L + 1) + sizeof(uint32_t) * edit_bits_words(L, L);
}
CASR_EDIT_HD inline size_t cn_align_fixed_bytes(int L, int k, bool tree) {
  return sizeof(int32_t) * ((size_t)L + (tree ? 2 * (size_t)L * k : 0));
}
CASR_EDIT_HD inline size_t cn_round256(size_t x) { return (x + 255) & ~(size_t)255; }

inline ConfusionPlan confusion_plan(int B, int L, int k, int V, bool tree) {
  ConfusionPlan p{};
  if (B < 1 || L < 1 || L > CN_MAX_LEN || k < 1 || k > CN_MAX_K || V < 1 || V > CN_MAX_VOCAB) return p;
  const size_t LK = (size_t)L * k, fixed = cn_align_fixed_bytes(L, k, tree), lane = cn_lane_bytes(L);
  if (fixed + lane > EDIT_LDS_LIMIT) return p;
  const size_t fit = (EDIT_LDS_LIMIT - fixed) / lane;
  p.lanes = fit >= CN_WAVE ? CN_WAVE : (int)fit;
  p.align_groups = (int)((LK + p.lanes - 1) / p.lanes);
  p.align_lds = fixed + lane * p.lanes;
  p.align_raise = p.align_lds > EDIT_LDS_DEFAULT;
  p.reduce_lds = sizeof(int64_t) * ((size_t)V + 1) + sizeof(int32_t) * LK;
  if (p.reduce_lds + 64 > EDIT_LDS_LIMIT) return p;  // (+ the kernel's static words)
  p.reduce_raise = p.reduce_lds > EDIT_LDS_DEFAULT;
  p.reduce_groups = cn_slots(L) < CN_REDUCE_GROUPS ? cn_slots(L) : CN_REDUCE_GROUPS;
  p.votes_bytes = sizeof(int16_t) * (size_t)B * cn_slots(L) * LK;
  // c [B][L k] double | unit [B][L k] int64 | list [B][L k] | count, pivot position [B] | pivot tokens
  // [B][L] | votes, each piece on a 256-byte boundary
  p.ws_bytes = 2 * cn_round256(8 * (size_t)B * LK) + cn_round256(4 * (size_t)B * LK) + 2 * cn_round256(4 * (size_t)B) +
               cn_round256(4 * (size_t)B * L) + cn_round256(p.votes_bytes);
  p.ok = true;
  return p;
}

}  // namespace casr
