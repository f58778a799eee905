// Device text that the kernels over a beam's finished records share (edit.hip: casr_beam_mbr;
// confusion.hip: casr_beam_nbest, casr_beam_confusion): the arguments, the executed steps, the list of an
// utterance's valid records with c and c_max, and the beam tree staged in LDS.
#pragma once
#include "casr_internal.h"
#include "edit_plan.h"

namespace casr {

constexpr int MBR_THREADS = 256;

// executed loop steps: the step at which the cumulative count of newdone reached `total`, + 1 (else L)
__device__ __forceinline__ int mbr_executed_steps(const int32_t* newdone, int L, int total) {
  int cum = 0;
  for (int s = 0; s < L; ++s) {
    cum += newdone[s];
    if (cum >= total) return s + 1;
  }
  return L;
}

struct MbrArgs {
  int B, k, L;
  double scale, lm_weight, length_weight;
  float beam_lm_weight, beam_length_weight;  // casr_beam's (the unfinished fallback)
  const float* score0;
  const float* score1;
  const int32_t* bp;
  const int32_t* tk;
  const float* rec_score;
  const int32_t* rec_src;
  const uint8_t* rec_valid;
  const int32_t* newdone;
  const float* rec_lm;  // or null
  MbrBufs w;
  int V;
  int32_t* best_tokens;
  int32_t* best_len;
  float* best_score;
  int32_t* best_index;  // or null
  double* best_risk;    // or null
  double* rec_risk;     // or null
  int32_t* err;
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
  const int tid = threadIdx.x, k = a.k, LK = a.L * k;
  double cm = NAN;
  for (int p = tid; p < n; p += MBR_THREADS) {
    const int i = list[p];
    const size_t ri = (size_t)b * LK + i;
    const double v = mbr_comb(a.rec_score[ri], a.rec_lm ? a.rec_lm[ri] : 0.f, i / k, a.lm_weight, a.length_weight);
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

// stage the beam tree of utterance b (beam_finalize's layout: [step][slot]); a back-pointer outside
// [0, k) is clamped, a token outside [0, V) is kept as it is; both are reported
__device__ __forceinline__ void mbr_stage_tree(const MbrArgs& a, int b, int nn, int32_t* sbp, int32_t* stk) {
  const int k = a.k, R = a.B * k;
  bool bad_tok = false, bad_bp = false;
  for (int i = threadIdx.x; i < nn; i += blockDim.x) {
    const int st = i / k, c = i - st * k;
    const size_t ix = (size_t)st * R + b * k + c;
    int p = a.bp[ix];
    if ((unsigned)p >= (unsigned)k) {
      if (st > 0) bad_bp = true;  // (step 0 has no predecessor node: its pointer is never followed)
      p = 0;
    }
    const int t = a.tk[ix];
    if ((unsigned)t >= (unsigned)a.V) bad_tok = true;
    sbp[i] = p;
    stk[i] = t;
  }
  if (blockIdx.y == 0) {
    if (bad_tok) atomicOr(a.err, CASR_DEV_BAD_TOKEN);
    if (bad_bp) atomicOr(a.err, CASR_DEV_BAD_BACKPTR);
  }
}

// the slot a record's walk starts from (step l - 1), clamped
__device__ __forceinline__ int mbr_record_slot(const MbrArgs& a, size_t ri, int l, int k) {
  int slot = a.rec_src[ri];
  if ((unsigned)slot >= (unsigned)k) {
    if (l > 0) atomicOr(a.err, CASR_DEV_BAD_BACKPTR);
    slot = 0;
  }
  return slot;
}

}  // namespace casr
