// Teacher-forced scoring of given transcripts on the last encode (casr_score, include/casr.h):
// the reference's training-time forward (model.py:405-469: decoder steps with compute_logit =
// False, one batched proj_linear over every step's [h | attn] rows) and the terms of its
// label-smoothed loss (util.py:265-279), on the decode kernels.
//   1. score_prep_kernel   targets [B][L] -> the step loop's token feed [L][B] and the clamped
//                          targets [L][B] (row order of the batched GEMM, i = l B + b)
//   2. score_steps         decoder.hip: L x (LSTMCell GEMM, attention), state slabs kept
//   3. score_project       decoder.hip: one projection GEMM over L B rows, ScoreEpi partials
//   4. score_rows_kernel   one wave per row: logsumexp, argmax, target and mean log-probability
//   5. score_total_kernel  one thread per utterance: the sum over its scored positions, ascending
#include "casr_common.h"
#include "casr_internal.h"

namespace casr {

static size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// history + partials + target logits + feed + clamped targets, each 256-byte aligned
size_t score_workspace_bytes(int B, int L) {
  const size_t R = (size_t)L * B;
  return align256((size_t)(L + 1) * B * ST * sizeof(float)) + 4 * align256(R * GP_NB * sizeof(float)) +
         3 * align256(R * sizeof(float));
}

ScoreBufs score_carve(void* base, int B, int L) {
  const size_t R = (size_t)L * B;
  char* p = reinterpret_cast<char*>(base);
  auto take = [&](size_t bytes) {
    char* q = p;
    p += align256(bytes);
    return q;
  };
  ScoreBufs sb{};
  sb.hist = reinterpret_cast<float*>(take((size_t)(L + 1) * B * ST * sizeof(float)));
  sb.part.mx = reinterpret_cast<float*>(take(R * GP_NB * sizeof(float)));
  sb.part.se = reinterpret_cast<float*>(take(R * GP_NB * sizeof(float)));
  sb.part.ix = reinterpret_cast<int32_t*>(take(R * GP_NB * sizeof(int32_t)));
  sb.part.tmx = nullptr;
  sb.xsum = reinterpret_cast<float*>(take(R * GP_NB * sizeof(float)));
  sb.tl = reinterpret_cast<float*>(take(R * sizeof(float)));
  sb.feed = reinterpret_cast<int32_t*>(take(R * sizeof(int32_t)));
  sb.tgt = reinterpret_cast<int32_t*>(take(R * sizeof(int32_t)));
  return sb;
}

// one thread per (b, l).  Position l of utterance b is scored when l < tgt_len[b] (clamped to
// 0..L); only then is targets[b][l] read: an id outside [0, V) becomes 0 and raises
// CASR_DEV_BAD_TOKEN, as the decode kernels' own clamp does.  Step l + 1 feeds the clamped id;
// past the scored positions it feeds eos, so padding entries never reach any output.
__global__ void score_prep_kernel(const int32_t* __restrict__ targets, const int32_t* __restrict__ tgt_len, int B, int L,
                                  int V, int sos, int eos, int32_t* __restrict__ feed, int32_t* __restrict__ tgt,
                                  int32_t* __restrict__ err) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * L) return;
  const int b = i / L, l = i - b * L;
  const int n = min(max(tgt_len[b], 0), L);
  int t = -1;
  if (l < n) {
    t = targets[i];
    if ((unsigned)t >= (unsigned)V) {
      atomicOr(err, CASR_DEV_BAD_TOKEN);
      t = 0;
    }
  }
  tgt[(size_t)l * B + b] = t;
  if (l == 0) feed[b] = sos;
  if (l + 1 < L) feed[(size_t)(l + 1) * B + b] = t >= 0 ? t : eos;
}

// One wave per GEMM row i = l B + b; lane j holds column block j's partials.  The row's maximum,
// first-index argmax and sum of exp(x - max) are combined exactly as greedy_select_part_kernel
// forms a row's logsumexp (decoder.hip); the block sums of the logits by the same shuffle tree.
// Outputs are [B][L]; a position at l >= tgt_len[b] gets 0 (best_token: -1).
__global__ __launch_bounds__(256) void score_rows_kernel(GreedyPart gp, const float* __restrict__ xsum,
                                                         const float* __restrict__ tl, const int32_t* __restrict__ tgt,
                                                         int nbp, int V, int B, int L, float* __restrict__ token_logp,
                                                         int32_t* __restrict__ best_token, float* __restrict__ best_logp,
                                                         float* __restrict__ mean_logp, int32_t* __restrict__ err) {
  const int ln = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= B * L) return;
  const int l = i / B, b = i - l * B;
  const size_t o = (size_t)b * L + l;
  const int t = tgt[i];
  if (t < 0) {  // wave-uniform
    if (ln == 0) {
      token_logp[o] = 0.f;
      if (best_token) best_token[o] = -1;
      if (best_logp) best_logp[o] = 0.f;
      if (mean_logp) mean_logp[o] = 0.f;
    }
    return;
  }
  float m = -INFINITY, se = 0.f, sx = 0.f;
  int mi = 0x7fffffff;
  if (ln < nbp) {
    m = gp.mx[(size_t)i * GP_NB + ln];
    se = gp.se[(size_t)i * GP_NB + ln];
    mi = gp.ix[(size_t)i * GP_NB + ln];
    sx = xsum[(size_t)i * GP_NB + ln];
  }
  float gm = m;
  int gi = mi;
  wave_best(gm, gi);
  const float s = wave_sum((se > 0.f) ? se * expf(m - gm) : 0.f);
  const float xs = wave_sum(sx);
  if (ln != 0) return;
  const float lse = logf(s) + gm;
  if ((unsigned)gi >= (unsigned)V) {  // no finite maximum (NaN row)
    atomicOr(err, CASR_DEV_NAN_LOGITS);
    gi = 0;
  }
  token_logp[o] = tl[i] - lse;
  if (best_token) best_token[o] = gi;
  if (best_logp) best_logp[o] = gm - lse;
  if (mean_logp) mean_logp[o] = xs / (float)V - lse;
}

// total_logp[b] = sum of token_logp[b][l] over l < tgt_len[b], added in ascending l
__global__ void score_total_kernel(const float* __restrict__ token_logp, const int32_t* __restrict__ tgt_len, int B,
                                   int L, float* __restrict__ total_logp) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int n = min(max(tgt_len[b], 0), L);
  float acc = 0.f;
  for (int l = 0; l < n; ++l) acc = acc + token_logp[(size_t)b * L + l];
  total_logp[b] = acc;
}

hipError_t run_score(const DecodeArgs& a, DecodeBufs& d, const ScoreBufs& sb, const int32_t* targets,
                     const int32_t* tgt_len, int L, float* token_logp, float* total_logp, int32_t* best_token,
                     float* best_logp, float* mean_logp, float* align, hipStream_t s) {
  const int B = a.B, R = L * B;
  hipLaunchKernelGGL(score_prep_kernel, dim3((R + 255) / 256), dim3(256), 0, s, targets, tgt_len, B, L, a.V, a.sos,
                     a.eos, sb.feed, sb.tgt, d.err);
  hipError_t e = score_steps(a, d, sb, L, align, s);
  if (e != hipSuccess) return e;
  e = score_project(a, d, sb, L, s);
  if (e != hipSuccess) return e;
  {
    ProfScope ps(a.prof, CASR_K_SELECT, s);
    hipLaunchKernelGGL(score_rows_kernel, dim3((R + 3) / 4), dim3(256), 0, s, sb.part, sb.xsum, sb.tl, sb.tgt,
                       a.plan.nbp, a.V, B, L, token_logp, best_token, best_logp, mean_logp, d.err);
    hipLaunchKernelGGL(score_total_kernel, dim3((B + 63) / 64), dim3(64), 0, s, token_logp, tgt_len, B, L, total_logp);
  }
  return hipGetLastError();
}

}  // namespace casr
