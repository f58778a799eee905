// Hotword biasing on the device (include/casr.h casr_bias_score, casr_bias_rows, casr_beam_bias): the
// sentence walk and the dense gain row of an automaton state (one workgroup per row).  The automaton, its
// transition and the row rule are bias_plan.h's, the text the host entries run; the select, the final
// choice and the records' bias are beam_lm.hip's with their BIAS switch (decoder.hip run_beam_bias drives
// the steps).
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

}  // namespace casr
