// How a kernel reads the tree a beam search left (beam_state.h BeamTree), once: the executed steps,
// the plain beam's unfinished fallback, the back-pointer walk over both layouts, the staging of one
// utterance into LDS and a record's start slot.  Plain C++ that is also device code: the kernels
// (decoder.hip, beam_lm.hip, ngram.hip, edit.hip, confusion.hip) and the sanitizer program
// (tests/host_plan/beam_tree_check.cpp) compile this text.  Nothing here reports: a function says that
// it clamped and the caller raises CASR_DEV_BAD_BACKPTR, at once or from a flag at its end.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "beam_state.h"

#if defined(__HIPCC__)
#define CASR_TREE_HD __host__ __device__
#else
#define CASR_TREE_HD
#endif

namespace casr {

// executed loop steps: the step at which the cumulative count of newdone reached `total`, + 1 (else L)
CASR_TREE_HD inline int beam_executed_steps(const int32_t* newdone, int L, int total) {
  int cum = 0;
  for (int s = 0; s < L; ++s) {
    cum += newdone[s];
    if (cum >= total) return s + 1;
  }
  return L;
}

// casr_beam's unfinished fallback (model.py:961-972): without a record, the first maximum over the k
// live rows of the last executed step; returns the row, its score to *score.  The select of step l
// writes score[(l + 1) & 1] and the last executed step is steps - 1, so the parity of steps picks the
// buffer.  Every reader that falls back calls this with the beam's own weights: the same bits.
CASR_TREE_HD inline int beam_live_row(const BeamTree& t, int b, float lm_weight, float length_weight, int steps,
                                      float* score) {
  const float* score_final = t.score[steps & 1];
  const float lw = (float)((double)length_weight * (double)steps);
  int bj = 0;
  float bsv = 0.f;
  for (int j = 0; j < t.k; ++j) {
    const float s = (score_final[b * t.k + j] + lm_weight * 0.f) + lw;
    if (j == 0 || s > bsv) {
      bsv = s;
      bj = j;
    }
  }
  *score = bsv;
  return bj;
}

// Where node (step, slot) of one utterance lies, and whether a pointer read there may be outside [0, k)
// (checked): in the workspaces, [step][B k] at utterance b ...
struct TreeGlobal {
  static constexpr bool checked = true;
  const int32_t* bp;
  const int32_t* tk;
  int R, row0;  // B k, b k
  CASR_TREE_HD TreeGlobal(const BeamTree& t, int b) : bp(t.bp), tk(t.tk), R(t.B * t.k), row0(b * t.k) {}
  CASR_TREE_HD size_t at(int st, int slot) const { return (size_t)st * R + row0 + slot; }
};
// ... or staged by beam_stage_tree<CLAMP>, [step][k]
template <bool CLAMP>
struct TreeStaged {
  static constexpr bool checked = !CLAMP;
  const int32_t* bp;
  const int32_t* tk;
  int k;
  CASR_TREE_HD int at(int st, int slot) const { return st * k + slot; }
};

// one hop: the token of node (st, *slot), *slot to its predecessor at step st - 1
template <class Tree>
CASR_TREE_HD inline int32_t beam_hop(const Tree& t, int st, int* slot) {
  const auto ix = t.at(st, *slot);
  *slot = t.bp[ix];
  return t.tk[ix];
}

// The walk from node (from, slot) to step 0: put(st, token) for st = from .. 0 (nothing at from < 0).
// The start slot and, in a checked tree, every pointer the walk follows (step 0's is not) are taken as 0
// where outside [0, k); returns whether that happened.
template <class Tree, class Put>
CASR_TREE_HD inline bool beam_walk(const Tree& t, int k, int slot, int from, Put&& put) {
  bool clamped = from >= 0 && (unsigned)slot >= (unsigned)k;
  if (clamped) slot = 0;
  for (int st = from; st >= 0; --st) {
    put(st, beam_hop(t, st, &slot));
    if (Tree::checked && st > 0 && (unsigned)slot >= (unsigned)k) {
      clamped = true;
      slot = 0;
    }
  }
  return clamped;
}

// Thread tid of nthreads stages the nodes i = st k + slot of the first `steps` steps of utterance b into
// sbp / stk and calls node(i, token) for each of its own (the caller's token check, or what else it
// stages beside).  CLAMP: a back-pointer outside [0, k) is staged as 0 and, at a step >= 1, returned as
// true (step 0 has no predecessor node: its pointer is never followed); TreeStaged<true> then needs no
// check per hop.  Without CLAMP the pointers are staged as they are, for a walk (TreeStaged<false>) that
// reports only the pointers it follows.
template <bool CLAMP, class Node>
CASR_TREE_HD inline bool beam_stage_tree(const BeamTree& t, int b, int steps, int32_t* sbp, int32_t* stk, int tid,
                                         int nthreads, Node&& node) {
  const TreeGlobal g(t, b);
  bool bad = false;
  for (int i = tid; i < steps * t.k; i += nthreads) {
    const int st = i / t.k;
    const size_t ix = g.at(st, i - st * t.k);
    int p = g.bp[ix];
    if (CLAMP && (unsigned)p >= (unsigned)t.k) {
      bad |= st > 0;
      p = 0;
    }
    const int32_t tok = g.tk[ix];
    sbp[i] = p;
    stk[i] = tok;
    node(i, tok);
  }
  return bad;
}

// the slot the walk of record ri = (b L + l) k + rank starts from (step l - 1): rec_src, taken as 0
// outside [0, k) and then, unless the record is empty, *bad set
CASR_TREE_HD inline int beam_record_slot(const BeamTree& t, size_t ri, int l, bool* bad) {
  const int slot = t.rec_src[ri];
  if ((unsigned)slot < (unsigned)t.k) return slot;
  if (l > 0) *bad = true;
  return 0;
}

}  // namespace casr
