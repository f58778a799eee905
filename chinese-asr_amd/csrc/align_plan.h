// The monotone path through an attention matrix (include/casr.h casr_align_path*): the integer
// weight, the move code and its tie order, where the move bits live, the backtrack, the order that
// picks a token's peak frame and the plan of a launch, once, as plain C++ that the kernel (align.hip),
// the host entry and the sanitizer program (tests/host_asan/align_check.cpp) all compile.  The
// formulas are casr.h's; tests/align_ref.py restates them in numpy.
//
// Cells.  Row l is a token, column t an encoder frame; q[l][t] <= 0 is the cell's weight and D[l][t]
// the best sum of a path from (0, 0) to (l, t).  Nothing keeps D past the row above: the move a cell
// takes is known when the cell is filled, and two bits per cell are all the backtrack reads.  The bits
// are two planes of 64 cells each (a wave's two ballots): words [row][chunk][plane], chunk = t / 64.
//
// Range.  |q| <= 3072, a path has at most L + Tp - 1 cells, and the scan form (align.hip) subtracts a
// prefix sum of a row from a row's entry values: every intermediate is inside 3072 (L + 2 Tp), which
// must stay clear of the sentinel -2^30.  At L = 512 and Tp = ALIGN_MAX_TP that is 7.9 million.
#pragma once
#include <stdint.h>

#include <vector>

#include "casr.h"

#if defined(__HIPCC__)
#define CASR_ALIGN_HD __host__ __device__
#else
#define CASR_ALIGN_HD
#endif

namespace casr {

constexpr int ALIGN_MAX_TP = CASR_ALIGN_MAX_TP;  // longest row of the device entry
constexpr int ALIGN_MAX_L = 512;
constexpr int ALIGN_WAVE = 64;                    // cells per chunk of a row
constexpr int ALIGN_GROUP_MAX = 16;               // utterances (waves) per workgroup: 64 contiguous bytes per cell
constexpr int ALIGN_GROUP_DEFAULT = 4;            // the measured choice: 16-byte runs, 4 x the workgroups
constexpr int ALIGN_Q_FLOOR = -3072;              // 2^-24 in 1/128 octave
constexpr int32_t ALIGN_NEG = -(1 << 30);         // "no such predecessor"
constexpr size_t ALIGN_LDS_LIMIT = 160 * 1024;    // LDS of a gfx950 CU
constexpr size_t ALIGN_LDS_DEFAULT = 64 * 1024;   // beyond it a kernel must raise its dynamic LDS limit

enum { ALIGN_DIAG = 0, ALIGN_VERT = 1, ALIGN_STAY = 2 };

// ---------------------------------------------------------------- (a) the weight
// The f32's upper 16 bits are sign, exponent and 7 mantissa bits: minus 127 << 7 they are a
// piecewise-linear log2 in 1/128 octave.  Zero, negatives and NaN take the floor (denormals reach it
// through the clamp), x >= 1 gives 0.
CASR_ALIGN_HD inline int32_t align_quant(float x) {
  if (!(x > 0.f)) return ALIGN_Q_FLOOR;
  uint32_t u;
  __builtin_memcpy(&u, &x, sizeof(u));
  const int32_t q = (int32_t)(u >> 16) - (127 << 7);
  return q < ALIGN_Q_FLOOR ? ALIGN_Q_FLOOR : q > 0 ? 0 : q;
}

// ---------------------------------------------------------------- (b) the move of a cell
// what a row takes from the row above at column t: the diagonal on equal values
CASR_ALIGN_HD inline int align_enter_move(int64_t diag, int64_t vert) { return diag >= vert ? ALIGN_DIAG : ALIGN_VERT; }

// ---------------------------------------------------------------- move bits and (c) the backtrack
CASR_ALIGN_HD inline int align_chunks(int T) { return (T + ALIGN_WAVE - 1) / ALIGN_WAVE; }
CASR_ALIGN_HD inline size_t align_bits_words(int rows, int chunks) { return (size_t)rows * chunks * 2; }

// first[l], last[l] of the n tokens, from (n - 1, T - 1) back to (0, 0); n, T >= 1.  A run of stays
// is crossed in one step per chunk: STAY is the only code with the upper plane's bit, so the nearest
// cell at or before t that does not stay is the highest clear bit of that plane.  Row 0 only stays and
// column 0 only climbs, whatever their bits say.  FT: int32_t or int16_t rows.
template <class FT>
CASR_ALIGN_HD inline void align_backtrack(const uint64_t* bits, int chunks, int n, int T, FT* first, FT* last) {
  int l = n - 1, t = T - 1;
  last[l] = (FT)t;
  while (l > 0) {
    const uint64_t* w = bits + ((size_t)l * chunks + (t >> 6)) * 2;
    const int pos = t & 63;
    const uint64_t upto = pos == 63 ? ~(uint64_t)0 : (((uint64_t)1 << (pos + 1)) - 1);
    const uint64_t leave = ~w[1] & upto;
    int mv = ALIGN_VERT;
    if (leave) {
      t = (t & ~63) + 63 - __builtin_clzll(leave);
      if (t > 0) mv = (int)((w[0] >> (t & 63)) & 1);
    } else if (t >= ALIGN_WAVE) {
      t = (t & ~63) - 1;  // the whole chunk up to t stays
      continue;
    } else {
      t = 0;
    }
    first[l] = (FT)t;
    --l;
    t -= mv == ALIGN_DIAG;
    last[l] = (FT)t;
  }
  first[0] = 0;
}

// the peak of a span: the larger weight, then the smaller frame (a frame below 0 is no candidate).  A
// total order, so any reduction tree gives the same frame.
CASR_ALIGN_HD inline bool align_peak_better(int qa, int ta, int qb, int tb) {
  if (ta < 0) return false;
  if (tb < 0) return true;
  return qa != qb ? qa > qb : ta < tb;
}

// the same order as one integer for t < 1024 (the device entry's rows): the larger key is the better
CASR_ALIGN_HD inline int align_peak_key(int q, int t) { return ((q - ALIGN_Q_FLOOR) << 10) | (1023 - t); }
CASR_ALIGN_HD inline int align_peak_frame(int key) { return 1023 - (key & 1023); }
static_assert(CASR_ALIGN_MAX_TP <= 1024, "align_peak_key keeps the frame in 10 bits");

// (d) a length outside its range is clamped; returns whether it was
CASR_ALIGN_HD inline bool align_clamp(int& v, int hi) {
  if (v < 0 || v > hi) {
    v = v < 0 ? 0 : hi;
    return true;
  }
  return false;
}

// ---------------------------------------------------------------- one utterance on the host
// The sequential recurrence, the definition.  a(l, t) = align[l * stride_l + t * stride_t]; cells with
// l < n and t < T are read and nothing else.  first, last, peak [L] get -1 past n.  64-bit sums: the
// values of the int32 definition wherever that does not overflow.
inline int32_t align_path_utterance(const float* align, size_t stride_l, size_t stride_t, int T, int n, int L,
                                    int32_t* first, int32_t* last, int32_t* peak) {
  for (int l = 0; l < L; ++l) first[l] = last[l] = peak[l] = -1;
  if (n <= 0 || T <= 0) return 0;
  const int chunks = align_chunks(T);
  std::vector<uint64_t> bits(align_bits_words(n, chunks), 0);
  std::vector<int64_t> row((size_t)T);
  for (int l = 0; l < n; ++l) {
    int64_t diag = 0, left = 0;  // D[l - 1][t - 1], D[l][t - 1]
    for (int t = 0; t < T; ++t) {
      const int64_t q = align_quant(align[l * stride_l + t * stride_t]);
      const int64_t vert = row[t];
      int mv;
      int64_t best;
      if (l == 0) {
        mv = t == 0 ? ALIGN_DIAG : ALIGN_STAY;
        best = t == 0 ? 0 : left;
      } else if (t == 0) {
        mv = ALIGN_VERT;
        best = vert;
      } else {
        mv = align_enter_move(diag, vert);
        best = mv == ALIGN_DIAG ? diag : vert;
        if (left > best) {
          mv = ALIGN_STAY;
          best = left;
        }
      }
      uint64_t* w = bits.data() + ((size_t)l * chunks + (t >> 6)) * 2;
      w[0] |= (uint64_t)(mv & 1) << (t & 63);
      w[1] |= (uint64_t)(mv >> 1) << (t & 63);
      diag = vert;
      left = row[t] = q + best;
    }
  }
  align_backtrack(bits.data(), chunks, n, T, first, last);
  for (int l = 0; l < n; ++l) {
    int bq = 0, bt = -1;
    for (int t = first[l]; t <= last[l]; ++t) {
      const int q = align_quant(align[l * stride_l + t * stride_t]);
      if (align_peak_better(q, t, bq, bt)) {
        bq = q;
        bt = t;
      }
    }
    peak[l] = bt;
  }
  return (int32_t)row[T - 1];
}

// ---------------------------------------------------------------- the plan
// A workgroup takes `group` adjacent utterances, one wave each.  Its LDS, in this order:
//   move bits  uint64 [group][L][chunks][2]
//   D rows     int32  [group][2][dw], dw = max(Tp, L): after the last row the backtrack's first and
//              last [L] take the place of the two rows
//   q tiles    int16  [2][group][qstride]: the row being scanned and the one being loaded; qstride is
//              twice an odd number of 32-bit words, so the 16 utterances of a frame fall in 16 banks
//   T, n       int32  [2][group]
// group is ALIGN_GROUP_DEFAULT, or the power of two up to ALIGN_GROUP_MAX asked for, halved until the
// LDS fits a CU.
struct AlignPlan {
  int group;  // 0: unsupported
  int chunks, dw, qstride;
  int grid;
  size_t lds_bytes;
  bool raise_lds;
};

inline size_t align_lds_bytes(int group, int L, int Tp) {
  const int chunks = align_chunks(Tp), dw = Tp > L ? Tp : L, qstride = 2 * (((Tp + 1) / 2) | 1);
  return (size_t)group * (sizeof(uint64_t) * align_bits_words(L, chunks) + sizeof(int32_t) * 2 * dw +
                          sizeof(int16_t) * 2 * qstride + sizeof(int32_t) * 2);
}

inline AlignPlan align_plan(int B, int L, int Tp, int group) {
  AlignPlan p{0, 0, 0, 0, 0, 0, false};
  if (B < 1 || L < 1 || L > ALIGN_MAX_L || Tp < 1 || Tp > ALIGN_MAX_TP) return p;
  if (group < 0 || group > ALIGN_GROUP_MAX || (group & (group - 1))) return p;
  int g = group ? group : ALIGN_GROUP_DEFAULT;
  while (g > 1 && align_lds_bytes(g, L, Tp) > ALIGN_LDS_LIMIT) g >>= 1;
  if (align_lds_bytes(g, L, Tp) > ALIGN_LDS_LIMIT) return p;
  p.group = g;
  p.chunks = align_chunks(Tp);
  p.dw = Tp > L ? Tp : L;
  p.qstride = 2 * (((Tp + 1) / 2) | 1);
  p.grid = (B + g - 1) / g;
  p.lds_bytes = align_lds_bytes(g, L, Tp);
  p.raise_lds = p.lds_bytes > ALIGN_LDS_DEFAULT;
  return p;
}

}  // namespace casr
