// Edit distance, its operation counts and the minimum-Bayes-risk choice (include/casr.h
// casr_edit_distance*, casr_mbr_host, casr_beam_mbr): the cell rule, the 2-bit direction code and its
// backtrace, the total order of the MBR reduction and the plan of a call, once, as plain C++ that the
// kernels (edit.hip), the host entry points and the sanitizer program (tests/host_asan/edit_check.cpp)
// all compile.  The formulas are casr.h's; tests/edit_ref.py restates the MBR ones in numpy and
// casr/results.py's edit_distance / edit_ops are the reference of the distances and the counts.
//
// Cells.  D is (m + 1) x (n + 1); cell (i, j), 0-based, is D[i + 1][j + 1].  Nothing keeps D: a cell
// needs its diagonal, upper and left neighbours only, and the rule the backtrace would take at a cell
// is known when the cell is filled (edit_dir), so two bits per interior cell are all the backtrace
// reads.  The bits are stored column-major, 16 rows per 32-bit word (edit_bits_stride words per
// column): a lane of the wave form owns a column and writes a finished word once, with no
// read-modify-write.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "casr.h"

#if defined(__HIPCC__)
#define CASR_EDIT_HD __host__ __device__
#else
#define CASR_EDIT_HD
#endif

namespace casr {

constexpr int EDIT_MAX_LEN = CASR_EDIT_MAX_LEN;  // longest row of the device entry
constexpr int EDIT_WAVE = 64;                    // columns per strip of the wave form
constexpr int EDIT_MBR_MAX_LEN = 255;            // casr_beam_mbr keeps its distances as bytes
constexpr size_t EDIT_LDS_LIMIT = 160 * 1024;    // LDS of a gfx950 CU
constexpr size_t EDIT_LDS_DEFAULT = 64 * 1024;   // beyond it a kernel must raise its dynamic LDS limit

enum { EDIT_DIAG = 0, EDIT_REPLACE = 1, EDIT_DELETE = 2, EDIT_INSERT = 3 };

// ---------------------------------------------------------------- the cell rule
CASR_EDIT_HD inline int edit_min3(int a, int b, int c) {
  const int ab = a < b ? a : b;
  return ab < c ? ab : c;
}

// D[i][j] from match = (a[i-1] == b[j-1]), diag = D[i-1][j-1], up = D[i-1][j], left = D[i][j-1]
CASR_EDIT_HD inline int edit_cell(bool match, int diag, int up, int left) {
  return match ? diag : 1 + edit_min3(diag, up, left);
}

// the backtrace's rule at an interior cell whose value is d: the first that applies of match
// (diagonal), replace (d == diag + 1), delete (d == up + 1), insert
CASR_EDIT_HD inline int edit_dir(bool match, int d, int diag, int up) {
  return match ? EDIT_DIAG : d == diag + 1 ? EDIT_REPLACE : d == up + 1 ? EDIT_DELETE : EDIT_INSERT;
}

// ---------------------------------------------------------------- direction bits and the backtrace
CASR_EDIT_HD inline int edit_bits_stride(int m) { return (m + 15) >> 4; }  // words per column
CASR_EDIT_HD inline size_t edit_bits_words(int m, int n) { return (size_t)n * edit_bits_stride(m); }
CASR_EDIT_HD inline size_t edit_bits_word(int i, int j, int stride) { return (size_t)j * stride + (i >> 4); }
CASR_EDIT_HD inline int edit_bits_shift(int i) { return 2 * (i & 15); }

// (insert, delete, replace) of the script turning a into b, from (m, n) back to (0, 0).  On the first
// row only inserts are left, on the first column only deletes (rule 3 holds there: D[i][0] = i)
CASR_EDIT_HD inline void edit_backtrace(const uint32_t* bits, int m, int n, int32_t* ops) {
  const int stride = edit_bits_stride(m);
  int i = m, j = n, ins = 0, del = 0, rep = 0;
  while (i > 0 || j > 0) {
    if (i > 0 && j > 0) {
      const int dir = (bits[edit_bits_word(i - 1, j - 1, stride)] >> edit_bits_shift(i - 1)) & 3;
      if (dir == EDIT_DIAG || dir == EDIT_REPLACE) {
        rep += dir == EDIT_REPLACE;
        --i;
        --j;
      } else if (dir == EDIT_DELETE) {
        ++del;
        --i;
      } else {
        ++ins;
        --j;
      }
    } else if (i > 0) {
      ++del;
      --i;
    } else {
      ++ins;
      --j;
    }
  }
  ops[0] = ins;
  ops[1] = del;
  ops[2] = rep;
}

// One pair on the host: a row of D rolls over i; a[0 .. m) and b[0 .. n) are read and nothing past them.
inline int32_t edit_distance_rows(const int32_t* a, int m, const int32_t* b, int n, int32_t* ops) {
  std::vector<int32_t> row((size_t)n + 1);
  for (int j = 0; j <= n; ++j) row[j] = j;
  const int stride = edit_bits_stride(m);
  std::vector<uint32_t> bits;
  if (ops) bits.assign(edit_bits_words(m, n), 0u);
  for (int i = 0; i < m; ++i) {
    int diag = row[0], left = i + 1;
    row[0] = left;
    const int32_t ai = a[i];
    for (int j = 0; j < n; ++j) {
      const int up = row[j + 1];
      const bool match = ai == b[j];
      const int d = edit_cell(match, diag, up, left);
      if (ops) bits[edit_bits_word(i, j, stride)] |= (uint32_t)edit_dir(match, d, diag, up) << edit_bits_shift(i);
      row[j + 1] = d;
      diag = up;
      left = d;
    }
  }
  if (ops) edit_backtrace(bits.data(), m, n, ops);
  return row[n];
}

// ---------------------------------------------------------------- MBR
// comb of casr_beam_rescore: (s + lm_weight q) + length_weight l, each one IEEE double operation
CASR_EDIT_HD inline double mbr_comb(float s, float q, int l, double lm_weight, double length_weight) {
#pragma clang fp contract(off)
  const double t = lm_weight * (double)q;
  const double u = (double)s + t;
  const double v = length_weight * (double)l;
  return u + v;
}

// c_max: the largest c that is not a NaN (NaN when there is none), starting from acc = NaN: the
// outcome does not depend on the order in which the values arrive
CASR_EDIT_HD inline double mbr_cmax(double acc, double c) { return (c == c && (acc != acc || c > acc)) ? c : acc; }

// w = exp(scale (c - c_max)): the difference and the product rounded on their own
CASR_EDIT_HD inline double mbr_weight(double scale, double c, double cmax) {
#pragma clang fp contract(off)
  const double d = c - cmax;
  const double x = scale * d;
  return exp(x);
}

// risk += w d, the product rounded before the add
CASR_EDIT_HD inline double mbr_risk_add(double risk, double w, int d) {
#pragma clang fp contract(off)
  const double p = w * (double)d;
  return risk + p;
}

// The choice: a risk that is no NaN beats a NaN, then the smaller risk, then the lower index (an index
// below 0 is no candidate).  A total order, so any reduction tree gives the same winner.
CASR_EDIT_HD inline bool mbr_better(double ra, int ia, double rb, int ib) {
  if (ia < 0) return false;
  if (ib < 0) return true;
  const bool na = ra != ra, nb = rb != rb;
  if (na != nb) return nb;
  if (!na && ra != rb) return ra < rb;
  return ia < ib;
}

// One utterance on the host, on the expanded records of casr_beam_records: tokens [L k][L], score,
// valid, lm (or null) [L k]; flat index = step k + rank, a record at step l holds l tokens.  Returns
// the choice's flat index (-1 without a record); risk (or null) [L k] gets 0 where there is no record.
inline int32_t mbr_utterance_host(const int32_t* tokens, const float* score, const uint8_t* valid, const float* lm,
                                  int L, int k, double scale, double lm_weight, double length_weight, double* risk) {
  const int LK = L * k;
  std::vector<int32_t> list;
  for (int i = 0; i < LK; ++i) {
    if (risk) risk[i] = 0.0;
    if (valid[i]) list.push_back(i);
  }
  const int n = (int)list.size();
  std::vector<double> w((size_t)n);
  double cmax = NAN;
  for (int p = 0; p < n; ++p) {
    w[p] = mbr_comb(score[list[p]], lm ? lm[list[p]] : 0.f, list[p] / k, lm_weight, length_weight);
    cmax = mbr_cmax(cmax, w[p]);
  }
  for (int p = 0; p < n; ++p) w[p] = mbr_weight(scale, w[p], cmax);
  std::vector<uint8_t> tri;  // distances of p > q at p (p - 1) / 2 + q; as int32 past a byte's range
  std::vector<int32_t> tri32;
  const bool wide = L > EDIT_MBR_MAX_LEN;
  const size_t pairs = (size_t)n * (n > 0 ? n - 1 : 0) / 2;
  if (wide) tri32.resize(pairs); else tri.resize(pairs);
  for (int p = 1; p < n; ++p)
    for (int q = 0; q < p; ++q) {
      const int32_t d = edit_distance_rows(tokens + (size_t)list[p] * L, list[p] / k, tokens + (size_t)list[q] * L,
                                           list[q] / k, nullptr);
      const size_t at = (size_t)p * (p - 1) / 2 + q;
      if (wide) tri32[at] = d; else tri[at] = (uint8_t)d;
    }
  double br = 0.0;
  int bi = -1;
  for (int p = 0; p < n; ++p) {
    double r = 0.0;
    for (int q = 0; q < n; ++q) {
      const size_t at = p > q ? (size_t)p * (p - 1) / 2 + q : (size_t)q * (q - 1) / 2 + p;
      const int d = p == q ? 0 : (wide ? tri32[at] : (int32_t)tri[at]);
      r = mbr_risk_add(r, w[q], d);
    }
    if (risk) risk[list[p]] = r;
    if (mbr_better(r, p, br, bi)) {
      br = r;
      bi = p;
    }
  }
  return bi < 0 ? -1 : list[bi];
}

// ---------------------------------------------------------------- the plan
// Which kernel form a call takes and the LDS of one of its workgroups (one wave each).
//   EDIT_FORM_WAVE  one wave per pair: lane = column, the anti-diagonals of a strip of 64 columns in
//                   turn; a lane keeps its own previous value and its left neighbour's last two, the
//                   strip's last column goes to the next strip through LDS (carry).
//   EDIT_FORM_LANE  one lane per pair (all-pairs only): one record's tokens are uniform across the wave
//                   and each lane rolls a row of D, as bytes in LDS, against a record of its own.
// Pairs (casr_edit_distance) always take the wave form; the all-pairs call (casr_beam_mbr) takes the
// form CASR_OPT_MBR_MAP names, or at 0 the default below.
enum { EDIT_FORM_NONE = 0, EDIT_FORM_WAVE = 1, EDIT_FORM_LANE = 2 };
constexpr int EDIT_MBR_DEFAULT_FORM = EDIT_FORM_LANE;
constexpr int EDIT_MBR_ROWS_PER_UTT = 128;  // workgroups per utterance of the all-pairs kernels

struct EditPlan {
  int form;          // EDIT_FORM_*; NONE: unsupported
  int strips;        // strips of 64 columns (wave form)
  int grid;          // workgroups (pairs: n; all-pairs: per utterance)
  size_t lds_bytes;  // dynamic LDS of a workgroup
  bool raise_lds;    // past the 64 KB a kernel gets without asking
};

// pairs: a [La] tokens, carry [La + 1], and with ops the direction words of La x Lb cells
inline EditPlan edit_plan_pairs(int La, int Lb, int n, bool ops) {
  EditPlan p{EDIT_FORM_NONE, 0, 0, 0, false};
  if (La < 1 || Lb < 1 || La > EDIT_MAX_LEN || Lb > EDIT_MAX_LEN || n < 0) return p;
  p.form = EDIT_FORM_WAVE;
  p.strips = (Lb + EDIT_WAVE - 1) / EDIT_WAVE;
  p.grid = n;
  p.lds_bytes = sizeof(int32_t) * ((size_t)La + La + 1) + (ops ? sizeof(uint32_t) * edit_bits_words(La, Lb) : 0);
  p.raise_lds = p.lds_bytes > EDIT_LDS_DEFAULT;
  if (p.lds_bytes > EDIT_LDS_LIMIT) p.form = EDIT_FORM_NONE;
  return p;
}

// all pairs of an utterance's records: the beam tree (back-pointers and tokens, [L k] each), then the
// wave form's two token rows and carry, or the lane form's uniform row and 64 rolling rows of bytes
inline EditPlan edit_plan_mbr(int L, int k, int map) {
  EditPlan p{EDIT_FORM_NONE, 0, 0, 0, false};
  if (L < 1 || k < 1 || L > EDIT_MBR_MAX_LEN || map < 0 || map > 2) return p;
  p.form = map ? map : EDIT_MBR_DEFAULT_FORM;
  p.strips = (L + EDIT_WAVE - 1) / EDIT_WAVE;
  p.grid = EDIT_MBR_ROWS_PER_UTT;
  const size_t tree = sizeof(int32_t) * 2 * (size_t)L * k;
  p.lds_bytes = tree + (p.form == EDIT_FORM_WAVE ? sizeof(int32_t) * ((size_t)3 * L + 1)
                                                 : sizeof(int32_t) * (size_t)L + (size_t)(L + 1) * EDIT_WAVE);
  if (p.lds_bytes > EDIT_LDS_DEFAULT) p.form = EDIT_FORM_NONE;
  return p;
}

}  // namespace casr
