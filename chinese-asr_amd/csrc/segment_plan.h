// casr_segment (include/casr.h): the decision text of stages (b) to (e), once, as plain C++ that the
// decision kernel (segment.hip) and casr_segment_host both compile, with the level formula of stage (a)
// and the host's whole-row driver.  The formulas are casr.h's; tests/segment_ref.py restates them.
//
// Stages (c) to (e) run as ONE left-to-right walk over the active runs of A0, with O(1) state (SegWalk):
//   seg_run      takes the active runs [s, e) of A0 in ascending order.  A run that starts where the
//                previous one ended continues it: a maximal run may arrive in pieces, which is how a run
//                that crosses a tile boundary of the kernel is put together again;
//   close_run    A1 drops a maximal run shorter than min_speech; A2 joins a kept run to the open island
//                when the quiet stretch between them is shorter than min_pause (every frame between two
//                kept runs is inactive in A1, so that stretch is one maximal inactive run), else the open
//                island is complete;
//   island       widens a complete island by pad and splits it (d); every cut is an arg-minimum over a
//                window of q, which the caller's Io computes (a serial loop on the host, a reduction
//                over lanes on the device).  Its total order, smaller cost then larger c, is one 64-bit
//                key (seg_cut_key), so the winner does not depend on the order of the reduction;
//   piece        the greedy merge (e); a complete segment goes to Io::emit.
// Io supplies  uint64_t best_cut(int32_t lo, int32_t hi)  (the smallest seg_cut_key over c in [lo, hi])
// and  void emit(int32_t index, int32_t start, int32_t len).
#pragma once
#include <stdint.h>

#include <vector>

#include "casr.h"

#if defined(__HIPCC__)
#define CASR_SEG_HD __host__ __device__
#else
#define CASR_SEG_HD
#endif

namespace casr {

constexpr int SEG_BINS = 512;   // levels of q
constexpr int SEG_LANES = 16;   // partial sums (lanes) per frame in stage (a)

inline casr_segment_params segment_default_params() { return casr_segment_params{800, 200, 20, 5, 8, 100, 10, 95, 90, 12}; }

CASR_SEG_HD inline bool segment_params_valid(const casr_segment_params& p) {
  return p.min_speech >= 1 && p.pad >= 0 && (int64_t)p.min_pause > 2 * (int64_t)p.pad && p.min_frames >= 1 &&
         2 * (int64_t)p.min_frames <= (int64_t)p.max_frames && p.max_gap >= 0 && 0 <= p.pct_lo &&
         p.pct_lo <= p.pct_hi && p.pct_hi <= 100 && 0 <= p.rel_q8 && p.rel_q8 <= 256 && p.rise_min >= 0;
}

// (T + min_pause) / (min_speech + min_pause) + T / min_frames; -1: invalid, or it does not fit an int
inline int64_t segment_bound(int T, const casr_segment_params& p) {
  if (T < 0 || !segment_params_valid(p)) return -1;
  const int64_t b = ((int64_t)T + p.min_pause) / ((int64_t)p.min_speech + p.min_pause) + (int64_t)T / p.min_frames;
  return b > INT32_MAX ? -1 : b;
}

// ---------------------------------------------------------------- (a) level
// q of a frame from p_0 of the halving tree: E = p_0 (1 / n_mels), q = clamp(floor((E + 24) 8), 0, 511),
// NaN -> 0.  The product is rounded on its own (no fma with the add)
CASR_SEG_HD inline int seg_level_bin(float p0, float inv_mels) {
#pragma clang fp contract(off)
  const float e = p0 * inv_mels;
  const float x = (e + 24.f) * 8.f;
  return x >= 512.f ? SEG_BINS - 1 : (x > 0.f ? (int)x : 0);  // a NaN fails both comparisons
}

// one frame on the host: the 16 partial sums in ascending order, then the halving tree
inline int seg_frame_bin_host(const float* row, int n_mels) {
#pragma clang fp contract(off)
  float p[SEG_LANES];
  for (int j = 0; j < SEG_LANES; ++j) p[j] = row[j];
  for (int k = SEG_LANES; k < n_mels; k += SEG_LANES)
    for (int j = 0; j < SEG_LANES; ++j) p[j] = p[j] + row[k + j];
  for (int h = SEG_LANES / 2; h >= 1; h >>= 1)
    for (int j = 0; j < h; ++j) p[j] = p[j] + p[j + h];
  return seg_level_bin(p[0], 1.0f / (float)n_mels);
}

// ---------------------------------------------------------------- (b) threshold
// the smallest v with sum_{u <= v} hist[u] >= max(1, (n pct + 99) div 100)
CASR_SEG_HD inline int seg_percentile(const uint32_t* hist, int n, int pct) {
  int64_t need = ((int64_t)n * pct + 99) / 100;
  if (need < 1) need = 1;
  int64_t cum = 0;
  for (int v = 0; v < SEG_BINS; ++v) {
    cum += hist[v];
    if (cum >= need) return v;
  }
  return SEG_BINS - 1;  // (a histogram of fewer than n frames: not reached with hist of q[0..n))
}

CASR_SEG_HD inline int32_t seg_threshold(const uint32_t* hist, int n, const casr_segment_params& p) {
  if (n <= 0) return 0;
  const int lo = seg_percentile(hist, n, p.pct_lo), hi = seg_percentile(hist, n, p.pct_hi);
  const int64_t rel = ((int64_t)(hi - lo) * p.rel_q8 + 128) >> 8;
  const int64_t thr = lo + (rel > p.rise_min ? rel : (int64_t)p.rise_min);
  return thr > INT32_MAX ? INT32_MAX : (int32_t)thr;
}

// ---------------------------------------------------------------- (c) to (e) the walk
// the split's total order as one key: smaller cost first, then the larger c
CASR_SEG_HD inline uint64_t seg_cut_key(uint32_t cost, int32_t c) {
  return ((uint64_t)cost << 32) | (uint32_t)(INT32_MAX - c);
}
CASR_SEG_HD inline int32_t seg_key_cut(uint64_t key) { return INT32_MAX - (int32_t)(uint32_t)(key & 0xffffffffu); }

struct SegWalk {
  int32_t n;             // frames of the recording
  int32_t run_s, run_e;  // the open run of A0 (run_s < 0: none)
  int32_t isl_s, isl_e;  // the open island of A2, not yet widened (isl_s < 0: none)
  int32_t seg_s, seg_e;  // the open segment (seg_s < 0: none)
  int32_t count;         // segments emitted
};

CASR_SEG_HD inline void seg_walk_init(SegWalk& w, int32_t n) {
  w.n = n;
  w.run_s = w.run_e = w.isl_s = w.isl_e = w.seg_s = w.seg_e = -1;
  w.count = 0;
}

template <class Io>
CASR_SEG_HD inline void seg_close_segment(SegWalk& w, Io& io) {
  if (w.seg_s < 0) return;
  io.emit(w.count, w.seg_s, w.seg_e - w.seg_s);
  ++w.count;
  w.seg_s = -1;
}

// (e): piece [s, e) joins the open segment, or closes it and opens the next
template <class Io>
CASR_SEG_HD inline void seg_piece(SegWalk& w, const casr_segment_params& p, Io& io, int32_t s, int32_t e) {
  if (w.seg_s >= 0 && (int64_t)s - w.seg_e <= p.max_gap && (int64_t)e - w.seg_s <= p.max_frames) {
    w.seg_e = e;
    return;
  }
  seg_close_segment(w, io);
  w.seg_s = s;
  w.seg_e = e;
}

// (c) widening and (d): the complete island [a, b) of A2
template <class Io>
CASR_SEG_HD inline void seg_island(SegWalk& w, const casr_segment_params& p, Io& io, int32_t a, int32_t b) {
  int64_t s = (int64_t)a - p.pad, e = (int64_t)b + p.pad;
  if (s < 0) s = 0;
  if (e > w.n) e = w.n;
  while (e - s > p.max_frames) {
    // 2 min_frames <= max_frames < e - s: lo <= hi, q[lo - 1] and q[hi] are frames of the recording
    const int64_t lo = s + p.min_frames;
    const int64_t hi = s + p.max_frames < e - p.min_frames ? s + p.max_frames : e - p.min_frames;
    int64_t c = seg_key_cut(io.best_cut((int32_t)lo, (int32_t)hi));
    c = c < lo ? lo : (c > hi ? hi : c);  // (a reduction's result is never followed out of its window)
    seg_piece(w, p, io, (int32_t)s, (int32_t)c);
    s = c;
  }
  seg_piece(w, p, io, (int32_t)s, (int32_t)e);
}

// the open run is maximal now: A1, then A2 against the open island
template <class Io>
CASR_SEG_HD inline void seg_close_run(SegWalk& w, const casr_segment_params& p, Io& io) {
  if (w.run_s < 0) return;
  const int32_t s = w.run_s, e = w.run_e;
  w.run_s = -1;
  if (e - s < p.min_speech) return;  // A1
  if (w.isl_s >= 0) {
    if (s - w.isl_e < p.min_pause) {  // A2: the pause is filled
      w.isl_e = e;
      return;
    }
    seg_island(w, p, io, w.isl_s, w.isl_e);
  }
  w.isl_s = s;
  w.isl_e = e;
}

// the next active run [s, e) of A0, ascending; s == the previous run's end continues that run
template <class Io>
CASR_SEG_HD inline void seg_run(SegWalk& w, const casr_segment_params& p, Io& io, int32_t s, int32_t e) {
  if (w.run_s >= 0 && s == w.run_e) {
    w.run_e = e;
    return;
  }
  seg_close_run(w, p, io);
  w.run_s = s;
  w.run_e = e;
}

// after the last run: everything open is complete.  w.count is the recording's segment count
template <class Io>
CASR_SEG_HD inline void seg_finish(SegWalk& w, const casr_segment_params& p, Io& io) {
  seg_close_run(w, p, io);
  if (w.isl_s >= 0) seg_island(w, p, io, w.isl_s, w.isl_e);
  w.isl_s = -1;
  seg_close_segment(w, io);
}

// ---------------------------------------------------------------- the host's driver
struct SegHostIo {
  const uint16_t* q;
  int32_t* start;
  int32_t* len;
  int s_max;
  uint64_t best_cut(int32_t lo, int32_t hi) const {
    uint64_t best = ~uint64_t(0);
    for (int64_t c = lo; c <= hi; ++c) {
      const uint64_t k = seg_cut_key((uint32_t)q[c - 1] + q[c], (int32_t)c);
      best = k < best ? k : best;
    }
    return best;
  }
  void emit(int32_t i, int32_t s, int32_t l) const {
    if (i < s_max) {
      start[i] = s;
      len[i] = l;
    }
  }
};

// one recording: rows [0, n) of fb [..][n_mels] -> its segments (at most s_max written), the true
// count, and thr.  p valid, n >= 0, n_mels a positive multiple of 16.  chunk > 0 hands the runs over
// clipped to chunks of that many frames, as the kernel's tiles do (the same segments)
inline void segment_row_host(const float* fb, int32_t n, int n_mels, const casr_segment_params& p, int s_max,
                             int32_t* start, int32_t* len, int32_t* n_seg, int32_t* thr, int32_t chunk = 0) {
  std::vector<uint16_t> q((size_t)n);
  std::vector<uint32_t> hist(SEG_BINS, 0u);
  for (int32_t t = 0; t < n; ++t) {
    q[(size_t)t] = (uint16_t)seg_frame_bin_host(fb + (size_t)t * n_mels, n_mels);
    ++hist[q[(size_t)t]];
  }
  const int32_t th = seg_threshold(hist.data(), n, p);
  if (thr) *thr = th;
  SegWalk w;
  seg_walk_init(w, n);
  SegHostIo io{q.data(), start, len, s_max};
  int32_t s = -1;  // start of the open active stretch
  for (int32_t t = 0; t < n; ++t) {
    const bool act = (int32_t)q[(size_t)t] >= th;
    if (act && s < 0) s = t;
    const bool last = t + 1 == n || (chunk > 0 && (t + 1) % chunk == 0);
    if (s >= 0 && (!act || last)) {
      seg_run(w, p, io, s, act ? t + 1 : t);
      s = -1;
    }
  }
  seg_finish(w, p, io);
  *n_seg = w.count;
}

}  // namespace casr
