// Hotword biasing on the device (include/casr.h casr_bias_score, casr_bias_rows, casr_beam_bias): the
// sentence walk, the dense gain row of an automaton state (one workgroup per row), the biased beam's
// final choice and its records' bias.  The automaton, its transition and the row rule are bias_plan.h's,
// the text the host entries run; the select is beam_lm.hip's with its BIAS switch (decoder.hip
// run_beam_bias drives the steps).
//
// The gain rows go through a workspace [R][V] as the LM's term rows do: bias_rows_kernel writes a row
// once, the select reads it beside the logits row.  A row is assembled in LDS, so the chain's scattered
// overwrites never leave the CU and the row goes out in one coalesced pass.
#include "beam_select.h"
#include "casr_internal.h"

namespace casr {

// ------------------------------------------------------------------ sentences
__global__ void bias_score_kernel(BiasView m, const int32_t* __restrict__ tokens, const int32_t* __restrict__ lens,
                                  int n, int L, int32_t* __restrict__ full, int32_t* __restrict__ tail,
                                  int32_t* __restrict__ state, int32_t* __restrict__ err) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int l = lens[i];
  if (l < 0 || l > L) {
    atomicOr(err, CASR_DEV_BAD_TOKEN);
    l = l < 0 ? 0 : L;
  }
  int32_t f, t, s;
  bias_sentence(m, tokens + (size_t)i * L, l, &f, &t, &s);
  if (full) full[i] = f;
  if (tail) tail[i] = t;
  if (state) state[i] = s;
}

hipError_t launch_bias_score(const BiasView& m, const int32_t* tokens, const int32_t* lens, int n, int L,
                             int32_t* full, int32_t* tail, int32_t* state, int32_t* err, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(bias_score_kernel, dim3((n + 63) / 64), dim3(64), 0, s, m, tokens, lens, n, L, full, tail, state,
                     err);
  return hipGetLastError();
}

// ------------------------------------------------------------------ gain rows
constexpr int BR_THREADS = 256;

// One workgroup per row.  tree == 0: row i's state is state[i].  tree == 1: row i = b k + j of decode
// step l, its state the one the select of step l - 1 left (the root at step 0), and the workgroup leaves
// at once where the select of step l would not run or not read the row (lm_terms_kernel's early exit).
// LDS: gain [V], then next [V] when next is asked for.
__global__ __launch_bounds__(BR_THREADS) void bias_rows_kernel(BiasView m, BiasRowsSrc src, int32_t* __restrict__ gain,
                                                               int32_t* __restrict__ next, int32_t* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) int32_t brow[];
  __shared__ int32_t chain[BIAS_MAX_LEN];
  __shared__ int nchain;
  const int i = blockIdx.x, tid = threadIdx.x, V = m.V;
  if (src.tree) {
    if (done_before(src.newdone, src.l) >= src.B) return;
    if (src.l == 0 && i % src.k != 0) return;
  }
  int32_t* grow = brow;
  int32_t* nrow = brow + V;  // (touched only with next)
  if (tid == 0) {
    bool bad = false;
    const int s = (src.tree && src.l == 0) ? 0 : bias_clamp_state(m, src.state[i], &bad);
    if (bad) atomicOr(err, CASR_DEV_BAD_TOKEN);
    nchain = bias_chain(m, s, chain);
  }
  for (int v = tid; v < V; v += BR_THREADS) {
    grow[v] = m.root_gain[v];
    if (next) nrow[v] = m.root_next[v];
  }
  __syncthreads();
  // from the node nearest the root to the state itself, a barrier between: the deepest wins (a node
  // holds a token once)
  for (int c = nchain - 1; c >= 0; --c) {
    const BiasNode nd = m.node[chain[c]];
    for (int e = tid; e < nd.child_cnt; e += BR_THREADS) {
      const int t = m.ctok[nd.child_off + e], nx = m.cnext[nd.child_off + e];
      if ((unsigned)t < (unsigned)V) {  // (the builder's ids are; an LDS write is never unchecked)
        grow[t] = bias_gain_of(m, nx);
        if (next) nrow[t] = nx;
      }
    }
    __syncthreads();
  }
  int32_t* og = gain + (size_t)i * V;
  for (int v = tid; v < V; v += BR_THREADS) og[v] = grow[v];
  if (next) {
    int32_t* on = next + (size_t)i * V;
    for (int v = tid; v < V; v += BR_THREADS) on[v] = nrow[v];
  }
}

bool bias_rows_supported(int V) { return (size_t)V * 2 * sizeof(int32_t) <= BIAS_ROWS_LDS_BYTES; }

hipError_t launch_bias_rows(const BiasView& m, const BiasRowsSrc& src, int n, int32_t* gain, int32_t* next,
                            int32_t* err, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(bias_rows_kernel, dim3(n), dim3(BR_THREADS), (size_t)m.V * (next ? 2 : 1) * sizeof(int32_t), s, m,
                     src, gain, next, err);
  return hipGetLastError();
}

// ------------------------------------------------------------------ the final choice
__device__ __forceinline__ float bias_of(int c) { return __int2float_rn(c) * (1.f / 256.f); }

// ((am + lm_weight lm) + bias_weight bias) + len_l; without LM the lm term is left out
__device__ __forceinline__ float bias_comb(float am, bool has_lm, float lm, float bias, float lmw, float bw, float lenw,
                                           int l) {
  const float len_l = (float)((double)lenw * (double)(l + 1));
  float r = am;
  if (has_lm) r = __fadd_rn(r, __fmul_rn(lmw, lm));
  return __fadd_rn(__fadd_rn(r, __fmul_rn(bw, bias)), len_l);
}

struct BiasFinArgs {
  int B, k, L;
  float lmw, bw, lenw;
  const float* score[2];
  const float* g[2];  // null without LM
  const int32_t* st[2];
  const int32_t* full[2];
  const int32_t* bp;
  const int32_t* tk;
  const float* rec_score;
  const float* rec_lm;  // null without LM
  const int32_t* rec_full;
  const int32_t* rec_src;
  const uint8_t* rec_valid;
  const int32_t* newdone;
};

// One thread per utterance, as beam_lm_finalize_kernel: the first maximum of the expression over its
// valid records in (step, rank) order (bias_closed), or without a record the first maximum over the k
// live rows of the last executed step (bias_open: C + tail(s)); tokens by walking the back-pointers.
__global__ void beam_bias_finalize_kernel(BiasFinArgs a, BiasView m, int32_t* __restrict__ best_tokens,
                                          int32_t* __restrict__ best_len, float* __restrict__ best_score,
                                          float* __restrict__ best_lm, float* __restrict__ best_bias,
                                          int32_t* __restrict__ steps_out, int32_t* __restrict__ err) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const int B = a.B, k = a.k, L = a.L;
  const int steps = lmf_executed_steps(a.newdone, L, B);
  if (b == 0) steps_out[0] = steps;
  if (b >= B) return;
  const bool has_lm = a.rec_lm != nullptr;
  const int R = B * k;
  int bl = -1, bc = -1;
  float bv = 0.f, bs = 0.f, bq = 0.f, bb = 0.f;
  for (int l = 0; l < steps; ++l)
    for (int c = 0; c < k; ++c) {
      const size_t ri = ((size_t)b * L + l) * k + c;
      if (!a.rec_valid[ri]) continue;
      const float lm = has_lm ? a.rec_lm[ri] : 0.f, bias = bias_of(a.rec_full[ri]);
      const float v = bias_comb(a.rec_score[ri], has_lm, lm, bias, a.lmw, a.bw, a.lenw, l);
      if (bl < 0 || v > bv) {
        bl = l;
        bc = c;
        bv = v;
        bs = a.rec_score[ri];
        bq = lm;
        bb = bias;
      }
    }
  int32_t* out = best_tokens + (size_t)b * L;
  int len, slot, from;
  if (bl >= 0) {
    len = bl;
    slot = a.rec_src[((size_t)b * L + bl) * k + bc];
    from = bl - 1;
  } else {  // the select of step l writes buffer (l + 1) & 1; the last executed step is steps - 1
    const int w = steps & 1, ll = steps - 1;
    int bj = 0;
    for (int j = 0; j < k; ++j) {
      const int rw = b * k + j;
      bool sbad = false;
      const int s = bias_clamp_state(m, a.st[w][rw], &sbad);
      if (sbad) atomicOr(err, CASR_DEV_BAD_TOKEN);
      const float lm = has_lm ? a.g[w][rw] : 0.f, bias = bias_of(a.full[w][rw] + m.node[s].tail);
      const float v = bias_comb(a.score[w][rw], has_lm, lm, bias, a.lmw, a.bw, a.lenw, ll);
      if (j == 0 || v > bv) {
        bv = v;
        bj = j;
        bs = a.score[w][rw];
        bq = lm;
        bb = bias;
      }
    }
    len = ll + 1;
    slot = bj;
    from = ll;
  }
  for (int s = from; s >= 0; --s) {
    if ((unsigned)slot >= (unsigned)k) {
      atomicOr(err, CASR_DEV_BAD_BACKPTR);
      slot = 0;
    }
    const size_t ix = (size_t)s * R + b * k + slot;
    out[s] = a.tk[ix];
    slot = a.bp[ix];
  }
  for (int s = len; s < L; ++s) out[s] = -1;
  best_len[b] = len;
  best_score[b] = bs;
  if (best_lm) best_lm[b] = bq;
  best_bias[b] = bb;
}

hipError_t launch_beam_bias_finalize(const DecodeArgs& a, const DecodeBufs& d, const BeamLmBufs* lw,
                                     const BeamBiasBufs& w, const BiasView& m, float bias_weight, float lm_weight,
                                     float length_weight, int32_t* best_tokens, int32_t* best_len, float* best_score,
                                     float* best_lm, float* best_bias, int32_t* steps, hipStream_t s) {
  const BiasFinArgs f{a.B, a.k, a.max_len, lm_weight, bias_weight, length_weight,
                      {d.score[0], d.score[1]},
                      {lw ? lw->g[0] : nullptr, lw ? lw->g[1] : nullptr},
                      {w.st[0], w.st[1]},
                      {w.full[0], w.full[1]},
                      d.bp, d.tk, d.rec_score, lw ? lw->rec_lm : nullptr, w.rec_full, d.rec_src, d.rec_valid,
                      d.newdone};
  hipLaunchKernelGGL(beam_bias_finalize_kernel, dim3((a.B + 63) / 64), dim3(64), 0, s, f, m, best_tokens, best_len,
                     best_score, best_lm, best_bias, steps, d.err);
  return hipGetLastError();
}

// bias_closed of the valid records of the executed steps, 0 elsewhere
__global__ void beam_record_bias_kernel(int B, int k, int L, const int32_t* __restrict__ rec_full,
                                        const uint8_t* __restrict__ rec_valid, const int32_t* __restrict__ newdone,
                                        float* __restrict__ out) {
  const size_t n = (size_t)B * L * k;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int steps = lmf_executed_steps(newdone, L, B);
  const int l = (int)((i / k) % L);
  out[i] = (l < steps && rec_valid[i]) ? bias_of(rec_full[i]) : 0.f;
}

hipError_t run_beam_record_bias(const BeamTree& t, const BeamBiasBufs& w, float* rec_bias, hipStream_t s) {
  const size_t n = (size_t)t.B * t.L * t.k;
  hipLaunchKernelGGL(beam_record_bias_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, t.B, t.k, t.L,
                     w.rec_full, t.rec_valid, t.newdone, rec_bias);
  return hipGetLastError();
}

}  // namespace casr
