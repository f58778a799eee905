// Device text that the kernels over a beam's finished records share (edit.hip: casr_beam_mbr;
// confusion.hip: casr_beam_nbest, casr_beam_confusion): the arguments and the list of an utterance's valid
// records with c and c_max.  How the tree is read (executed steps, staging, walks) is beam_tree.h's.
#pragma once
#include "beam_tree.h"
#include "casr_internal.h"
#include "edit_plan.h"

namespace casr {

constexpr int MBR_THREADS = 256;

struct MbrArgs {
  BeamTree t;
  double scale, lm_weight, length_weight;
  float beam_lm_weight, beam_length_weight;  // casr_beam's (the unfinished fallback)
  const float* rec_lm;  // or null
  MbrBufs w;
  int32_t* best_tokens;
  int32_t* best_len;
  float* best_score;
  int32_t* best_index;  // or null
  double* best_risk;    // or null
  double* rec_risk;     // or null
};

// A workgroup of MBR_THREADS: the flat indices i < nn with valid[i], ascending, into list; returns their
// count.  wcount: LDS [MBR_THREADS / 64]
__device__ __forceinline__ int mbr_list_records(const uint8_t* valid, int nn, int LK, int32_t* list, int* wcount) {
  const int tid = threadIdx.x;
  int base = 0;
  for (int i0 = 0; i0 < LK; i0 += MBR_THREADS) {
    const int i = i0 + tid;
    const bool v = i < nn && valid[i];
    const unsigned long long bal = __ballot(v);
    const int lane = tid & 63, wv = tid >> 6;
    if (lane == 0) wcount[wv] = __popcll(bal);
    __syncthreads();
    int off = base, tot = 0;
    for (int u = 0; u < MBR_THREADS / 64; ++u) {
      if (u < wv) off += wcount[u];
      tot += wcount[u];
    }
    if (v) list[off + __popcll(bal & ((1ull << lane) - 1ull))] = i;
    base += tot;
    __syncthreads();
  }
  return base;
}

// c of the listed records of utterance b into c[0 .. n); returns c_max.  red: LDS [MBR_THREADS] doubles
__device__ __forceinline__ double mbr_comb_records(const MbrArgs& a, int b, int n, const int32_t* list, double* c,
                                                   double* red) {
  const int tid = threadIdx.x, k = a.t.k, LK = a.t.L * k;
  double cm = NAN;
  for (int p = tid; p < n; p += MBR_THREADS) {
    const int i = list[p];
    const size_t ri = (size_t)b * LK + i;
    const double v = mbr_comb(a.t.rec_score[ri], a.rec_lm ? a.rec_lm[ri] : 0.f, i / k, a.lm_weight, a.length_weight);
    c[p] = v;
    cm = mbr_cmax(cm, v);
  }
  red[tid] = cm;
  __syncthreads();
  for (int o = MBR_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] = mbr_cmax(red[tid], red[tid + o]);
    __syncthreads();
  }
  return red[0];
}

// stage the executed steps of utterance b (beam_tree.h) for a workgroup; a token outside [0, V) is kept
// as it is and reported, as a clamped back-pointer is
__device__ __forceinline__ void mbr_stage_tree(const BeamTree& t, int b, int32_t* sbp, int32_t* stk) {
  bool bad_tok = false;
  const int steps = beam_executed_steps(t.newdone, t.L, t.B);
  const bool bad_bp = beam_stage_tree<true>(t, b, steps, sbp, stk, threadIdx.x, blockDim.x,
                                            [&](int, int32_t tok) { bad_tok |= (unsigned)tok >= (unsigned)t.V; });
  if (blockIdx.y == 0) {
    if (bad_tok) atomicOr(t.err, CASR_DEV_BAD_TOKEN);
    if (bad_bp) atomicOr(t.err, CASR_DEV_BAD_BACKPTR);
  }
}

}  // namespace casr
