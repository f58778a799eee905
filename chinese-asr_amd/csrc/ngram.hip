// Backoff n-gram LM on the device (include/casr.h casr_lm_score, casr_beam_rescore): sentence scoring
// and the second-pass selection over the beam tree casr_beam leaves in the handle.  The query itself
// is ngram_table.h's, the same text the host runs.
//
// The probes are dependent random 16-byte reads of tables far larger than an L2, so the kernels are
// shaped for few dependent round trips, not for bandwidth: every lookup of a term is issued
// unconditionally (ngram_term: up to three n-gram and two context probes, independent of each other),
// and the rescore computes one term per beam-tree NODE, not per record token: a word's term depends
// only on its at most three predecessors, which every hypothesis through that node shares.  An
// utterance has at most steps x k nodes and as many records, so it makes at most 2 steps k queries.
#include "beam_tree.h"
#include "casr_internal.h"

namespace casr {

// ------------------------------------------------------------------ sentence scoring
// One workgroup (one wave) per sentence; one work item per position for the terms, 64 positions at a
// time, then lane 0 adds the chunk's terms in ascending order: q = (..(t_0 + t_1).. + t_len).
__global__ __launch_bounds__(64) void lm_score_kernel(NgramView m, const int32_t* __restrict__ tokens,
                                                      const int32_t* __restrict__ lens, int L, int bos,
                                                      float* __restrict__ q, int32_t* __restrict__ err) {
  __shared__ float term[64];
  const int i = blockIdx.x, ln = threadIdx.x;
  const int32_t* tok = tokens + (size_t)i * L;
  int len = lens[i];
  bool bad = false;
  if (len < 0 || len > L) {
    bad = true;
    len = len < 0 ? 0 : L;
  }
  float acc = 0.f;
  for (int p0 = 0; p0 <= len; p0 += 64) {
    const int p = p0 + ln;
    if (p <= len) term[ln] = ngram_position_term(m, tok, len, bos, p, &bad);
    __syncthreads();
    if (ln == 0) {
      const int n = min(64, len + 1 - p0);
      for (int e = 0; e < n; ++e) acc = (p0 + e == 0) ? term[e] : acc + term[e];
    }
    __syncthreads();
  }
  if (ln == 0) q[i] = acc;
  if (__ballot(bad) && ln == 0) atomicOr(err, CASR_DEV_BAD_TOKEN);
}

hipError_t launch_lm_score(const NgramView& m, const int32_t* tokens, const int32_t* lens, int n, int L, int bos,
                           float* q, int32_t* err, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(lm_score_kernel, dim3(n), dim3(64), 0, s, m, tokens, lens, L, bos, q, err);
  return hipGetLastError();
}

// ------------------------------------------------------------------ second pass over the beam tree
constexpr int LMR_THREADS = 256;

// first-max / first-NaN (np.argmax): a NaN beats every number, a larger number a smaller one, and of
// two equals (or two NaNs) the lower index wins.  A total order, so any reduction tree gives the
// same winner.
__device__ __forceinline__ bool lmr_better(double ca, int ia, double cb, int ib) {
  if (ia < 0) return false;
  if (ib < 0) return true;
  const bool na = ca != ca, nb = cb != cb;
  if (na != nb) return na;
  if (!na && ca != cb) return ca > cb;
  return ia < ib;
}

struct RescoreArgs {
  NgramView m;
  BeamTree t;
  double lm_weight, length_weight;  // the second pass's
  float beam_lm_weight, beam_length_weight;  // casr_beam's (the unfinished fallback)
  int32_t* best_tokens;
  int32_t* best_len;
  float* best_score;
  float* best_lm;  // or null
  float* rec_lm;   // or null
};

// LDS of one workgroup: back-pointers, tokens, LM ids and prefix sums [L k] each, then the reduction
inline size_t rescore_lds_bytes(int L, int k) {
  return (size_t)L * k * 4 * sizeof(int32_t) + LMR_THREADS * (sizeof(double) + sizeof(int32_t));
}

// One workgroup per utterance.
__global__ __launch_bounds__(LMR_THREADS) void lm_rescore_kernel(RescoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) int32_t rsm[];
  const BeamTree& t = a.t;
  const int b = blockIdx.x, tid = threadIdx.x, k = t.k, L = t.L, LK = L * k;
  double* redc = reinterpret_cast<double*>(rsm);  // first: 8-byte aligned
  int32_t* redi = reinterpret_cast<int32_t*>(redc + LMR_THREADS);
  int32_t* sbp = redi + LMR_THREADS;
  int32_t* stk = sbp + LK;
  int32_t* sid = stk + LK;
  float* pre = reinterpret_cast<float*>(sid + LK);
  const NgramView& m = a.m;
  const int steps = beam_executed_steps(t.newdone, L, t.B);
  const int n = steps * k;
  bool bad_tok = false;

  // stage the executed steps (beam_tree.h: [step][slot], back-pointers clamped) with the tokens' LM ids
  // beside; a token outside [0, V) scores as <unk>; both are reported
  bool bad_bp = beam_stage_tree<true>(t, b, steps, sbp, stk, tid, LMR_THREADS,
                                      [&](int i, int32_t tok) { sid[i] = ngram_lm_id(m, tok, m.V, &bad_tok); });
  __syncthreads();

  // node terms: the word of node (st, c) after its at most order - 1 ancestors, <s> before step 0
  const int bos_id = m.redirect[m.V], eos_id = m.redirect[m.V + 1];
  for (int i = tid; i < n; i += LMR_THREADS) {
    int st = i / k, slot = i - st * k;
    const int w = sid[i];
    int c[NGRAM_MAX_ORDER - 1] = {0, 0, 0};
    int nc = 0;
    for (int j = 1; j < m.order; ++j) {
      slot = sbp[st * k + slot];
      --st;
      if (st < 0) {
        c[nc++] = bos_id;
        break;
      }
      c[nc++] = sid[st * k + slot];
    }
    pre[i] = ngram_term(m, c, nc, w);
  }
  __syncthreads();

  // prefix sums down the tree, one barrier per step: exactly the ascending f32 sentence sum
  for (int st = 1; st < steps; ++st) {
    if (tid < k) pre[st * k + tid] = pre[(st - 1) * k + sbp[st * k + tid]] + pre[st * k + tid];
    __syncthreads();
  }

  // records in (step, rank) order: q = prefix of the parent node + the term of </s> after it
  double bc = 0.0;
  int bi = -1;
  float bq = 0.f;
  for (int i = tid; i < LK; i += LMR_THREADS) {
    const size_t ri = (size_t)b * LK + i;
    const bool valid = i < n && t.rec_valid[ri];
    float q = 0.f;
    if (valid) {
      const int l = i / k;
      int slot = beam_record_slot(t, ri, l, &bad_bp);
      int c[NGRAM_MAX_ORDER - 1] = {0, 0, 0};
      int nc = 0, st = l - 1;
      const int src = slot;
      for (int j = 1; j < m.order; ++j) {
        if (st < 0) {
          c[nc++] = bos_id;
          break;
        }
        c[nc++] = sid[st * k + slot];
        slot = sbp[st * k + slot];
        --st;
      }
      const float te = ngram_term(m, c, nc, eos_id);
      q = l == 0 ? te : pre[(l - 1) * k + src] + te;
      // comb = (logp + lm_w q) + len_w l, each one IEEE double operation (never contracted to an fma)
      const double comb = __dadd_rn(__dadd_rn((double)t.rec_score[ri], __dmul_rn(a.lm_weight, (double)q)),
                                    __dmul_rn(a.length_weight, (double)l));
      if (lmr_better(comb, i, bc, bi)) {
        bc = comb;
        bi = i;
        bq = q;
      }
    }
    if (a.rec_lm) a.rec_lm[ri] = q;
  }
  redc[tid] = bc;
  redi[tid] = bi;
  __syncthreads();
  for (int o = LMR_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o && lmr_better(redc[tid + o], redi[tid + o], redc[tid], redi[tid])) {
      redc[tid] = redc[tid + o];
      redi[tid] = redi[tid + o];
    }
    __syncthreads();
  }
  const int win = redi[0];
  __syncthreads();  // (redi[0] is rewritten below as the length)

  // the winner's owner (or thread 0 for the unfinished fallback) walks the back-pointers in LDS
  int32_t* out = a.best_tokens + (size_t)b * L;
  if (win >= 0 ? (bi == win) : (tid == 0)) {
    int len, slot;
    float bs;
    if (win >= 0) {
      const size_t ri = (size_t)b * LK + win;
      len = win / k;
      slot = t.rec_src[ri];
      bs = t.rec_score[ri];
    } else {  // no record: casr_beam's unfinished fallback with its weights, LM sum 0
      len = steps;
      slot = beam_live_row(t, b, a.beam_lm_weight, a.beam_length_weight, steps, &bs);
      bq = 0.f;
    }
    bad_bp |= beam_walk(TreeStaged<true>{sbp, stk, k}, k, slot, len - 1, [&](int st, int32_t tok) { out[st] = tok; });
    a.best_len[b] = len;
    a.best_score[b] = bs;
    if (a.best_lm) a.best_lm[b] = bq;
    redi[0] = len;
  }
  __syncthreads();
  const int len = redi[0];
  for (int st = len + tid; st < L; st += LMR_THREADS) out[st] = -1;
  if (bad_tok) atomicOr(t.err, CASR_DEV_BAD_TOKEN);
  if (bad_bp) atomicOr(t.err, CASR_DEV_BAD_BACKPTR);
}

bool rescore_supported(int max_len, int k) { return rescore_lds_bytes(max_len, k) <= 64 * 1024; }

hipError_t run_beam_rescore(const BeamTree& t, const NgramView& m, double lm_weight, double length_weight,
                            float beam_lm_weight, float beam_length_weight, int32_t* best_tokens, int32_t* best_len,
                            float* best_score, float* best_lm, float* rec_lm, hipStream_t s) {
  RescoreArgs r{m, t, lm_weight, length_weight, beam_lm_weight, beam_length_weight,
                best_tokens, best_len, best_score, best_lm, rec_lm};
  hipLaunchKernelGGL(lm_rescore_kernel, dim3(t.B), dim3(LMR_THREADS), rescore_lds_bytes(t.L, t.k), s, r);
  return hipGetLastError();
}

}  // namespace casr
