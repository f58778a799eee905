// Grammar-constrained decoding on the device (include/casr.h casr_grammar_accept, casr_grammar_rows,
// casr_beam_grammar): the sentence walk (one thread per sentence) and the mask row of a grammar state (one
// wave per row).  The acceptor, its transition and the row rule are grammar_plan.h's, the text the host
// entries run; the select and the final choice are beam_lm.hip's with their GRAM switch (decoder.hip
// run_beam_grammar drives the steps).
//
// The mask rows go through a workspace [R][GW] as the bias path's gain rows do, one bit per token where
// those hold an int32: gram_rows_kernel writes a row once, the select reads it beside the logits row.  A
// row is assembled in LDS, so the arcs' scattered bits never leave the CU and the row goes out in one
// coalesced pass.
#include "beam_select.h"
#include "casr_internal.h"

namespace casr {

// ------------------------------------------------------------------ sentences
__global__ void gram_accept_kernel(GrammarView m, const int32_t* __restrict__ tokens,
                                   const int32_t* __restrict__ lens, int n, int L, int32_t* __restrict__ consumed,
                                   int32_t* __restrict__ state, uint8_t* __restrict__ accepted,
                                   int32_t* __restrict__ err) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int l = lens[i];
  if (l < 0 || l > L) {
    atomicOr(err, CASR_DEV_BAD_TOKEN);
    l = l < 0 ? 0 : L;
  }
  int32_t c, s;
  uint8_t ok;
  gram_sentence(m, tokens + (size_t)i * L, l, &c, &s, &ok);
  if (consumed) consumed[i] = c;
  if (state) state[i] = s;
  if (accepted) accepted[i] = ok;
}

hipError_t launch_gram_accept(const GrammarView& m, const int32_t* tokens, const int32_t* lens, int n, int L,
                              int32_t* consumed, int32_t* state, uint8_t* accepted, int32_t* err, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(gram_accept_kernel, dim3((n + 63) / 64), dim3(64), 0, s, m, tokens, lens, n, L, consumed, state,
                     accepted, err);
  return hipGetLastError();
}

// ------------------------------------------------------------------ mask rows
constexpr int GR_THREADS = 256, GR_ROWS = GR_THREADS / 64;

// One wave per row, GR_ROWS rows per workgroup.  tree == 0: row i's state and budget are state[i] and
// budget[i].  tree == 1: row i = b k + j of decode step l, its state the one the select of step l - 1
// left (the start state at step 0), its budget budget_l; the workgroup leaves at once where the select of
// step l would not run, and a wave sits out where it would not read the row (bias_rows_kernel's early exit).
// LDS: GR_ROWS rows of GW words; a wave touches its own row only, the barriers are the workgroup's.
__global__ __launch_bounds__(GR_THREADS) void gram_rows_kernel(GrammarView m, GramRowsSrc src, int n,
                                                               uint32_t* __restrict__ mask,
                                                               int32_t* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) uint32_t grow[];
  const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6, V = m.V, GW = gram_mask_words(V);
  const int i = blockIdx.x * GR_ROWS + wv;
  if (src.tree && done_before(src.newdone, src.l) >= src.B) return;
  const bool live = i < n && !(src.tree && src.l == 0 && i % src.k != 0);
  uint32_t* row = grow + (size_t)wv * GW;
  for (int w = ln; w < GW; w += 64) row[w] = 0u;
  __syncthreads();
  if (live) {
    const int s = src.state[i];
    const int budget = src.tree ? src.budget_l : src.budget[i];
    if ((unsigned)s < (unsigned)m.n_states) {
      const int lo = m.arc_off[s], hi = m.arc_off[s + 1];
      for (int q = lo + ln; q < hi; q += 64) {
        const int t = m.arc_tok[q];  // (two coalesced reads per arc: its token and its target's dist)
        // (the builder's ids are in range; an LDS write is never unchecked)
        if ((unsigned)t < (unsigned)V && m.arc_dist[q] <= budget) atomicOr(&row[t >> 5], 1u << (t & 31));
      }
      if (ln == 0 && m.is_final[s] && (unsigned)m.eos < (unsigned)V) atomicOr(&row[m.eos >> 5], 1u << (m.eos & 31));
    } else if (s != GRAM_DEAD && ln == 0) {
      atomicOr(err, CASR_DEV_BAD_TOKEN);
    }
  }
  __syncthreads();
  if (live) {
    uint32_t* out = mask + (size_t)i * GW;
    for (int w = ln; w < GW; w += 64) out[w] = row[w];
  }
}

bool gram_rows_supported(int V) { return (size_t)GR_ROWS * gram_mask_words(V) * sizeof(uint32_t) <= GRAM_ROWS_LDS_BYTES; }

hipError_t launch_gram_rows(const GrammarView& m, const GramRowsSrc& src, int n, uint32_t* mask, int32_t* err,
                            hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(gram_rows_kernel, dim3((n + GR_ROWS - 1) / GR_ROWS), dim3(GR_THREADS),
                     (size_t)GR_ROWS * gram_mask_words(m.V) * sizeof(uint32_t), s, m, src, n, mask, err);
  return hipGetLastError();
}

// ------------------------------------------------------------------ the rows' states before step 0
__global__ void gram_start_kernel(const int32_t* __restrict__ start, int R, int k, int32_t* __restrict__ state) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < R) state[i] = start ? start[i / k] : 0;
}

hipError_t launch_gram_start(const int32_t* start, int B, int k, int32_t* state, hipStream_t s) {
  const int R = B * k;
  if (R <= 0) return hipSuccess;
  hipLaunchKernelGGL(gram_start_kernel, dim3((R + 255) / 256), dim3(256), 0, s, start, R, k, state);
  return hipGetLastError();
}

}  // namespace casr
