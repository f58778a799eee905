// Edit distance on the device (include/casr.h casr_edit_distance, casr_beam_mbr): batches of
// independent pairs with their operation counts (the WER of an evaluation), and every pair of an
// utterance's finished beam records for the minimum-Bayes-risk choice.  The cell rule, the direction
// bits, the backtrace, the total order and the plan are edit_plan.h's, the text the host compiles too.
//
// Every workgroup here is ONE wave (64 threads): its barriers order that wave's LDS traffic only.
#include "casr_internal.h"
#include "edit_plan.h"
#include "mbr_device.h"

namespace casr {

// ------------------------------------------------------------------ the wave form
// D[m][n] of a[0 .. m) (LDS) against b[0 .. n), lane = column, one anti-diagonal per step.  At step t
// lane c of a strip fills row i = t - c: up is its own previous value, left its left neighbour's value of
// the step before (one cross-lane move), diag that neighbour's value of two steps before, which is the
// left it fetched a step ago.  Lane 0 takes left from carry, the previous strip's last column, and the
// strip's last lane overwrites carry behind it (it writes entry i + 1 - (cols - 1) <= what lane 0 reads).
// OPS: a lane collects the direction codes of its column, 16 rows to a word (edit_plan.h layout).
template <bool OPS>
__device__ __forceinline__ int edit_wave_sweep(const int32_t* sa, int m, const int32_t* b, int n, int32_t* carry,
                                               uint32_t* bits) {
  const int ln = threadIdx.x;
  if (m == 0) return n;  // (uniform)
  if (n == 0) return m;
  const int stride = edit_bits_stride(m);
  for (int i = ln; i <= m; i += EDIT_WAVE) carry[i] = i;  // D[i][0]
  __syncthreads();
  int result = 0;
  for (int j0 = 0; j0 < n; j0 += EDIT_WAVE) {
    const int cols = min(EDIT_WAVE, n - j0), j = j0 + ln;
    const bool on = ln < cols;
    const int32_t bj = on ? b[j] : 0;
    int v = j + 1;   // D[0][j + 1]
    int diag = j;    // D[0][j]
    uint32_t acc = 0;
    const int T = m + cols - 1;
    for (int t = 0; t < T; ++t) {
      const int i = t - ln;
      const bool act = on && i >= 0 && i < m;
      int left = __shfl_up(v, 1);
      if (act) {
        if (ln == 0) left = carry[i + 1];
        const bool match = sa[i] == bj;
        const int d = edit_cell(match, diag, v, left);
        if (OPS) {
          acc |= (uint32_t)edit_dir(match, d, diag, v) << edit_bits_shift(i);
          if ((i & 15) == 15 || i == m - 1) {
            bits[edit_bits_word(i, j, stride)] = acc;
            acc = 0;
          }
        }
        v = d;
        if (ln == cols - 1) carry[i + 1] = d;
      }
      diag = left;
    }
    if (j0 + EDIT_WAVE >= n) result = __shfl(v, n - 1 - j0);
    __syncthreads();
  }
  return result;
}

struct EditPairsArgs {
  const int32_t* a;
  const int32_t* a_len;
  const int32_t* b;
  const int32_t* b_len;
  int La, Lb;
  int32_t* dist;
  int32_t* ops;  // or null
  int32_t* err;
};

// One workgroup per pair.  LDS: a [La], carry [La + 1], then the direction words (OPS)
template <bool OPS>
__global__ __launch_bounds__(EDIT_WAVE) void edit_pairs_kernel(EditPairsArgs p) {
  extern __shared__ __attribute__((aligned(16))) int32_t esm[];
  const size_t pair = blockIdx.x;
  const int ln = threadIdx.x;
  int m = p.a_len[pair], n = p.b_len[pair];
  bool bad = false;
  if (m < 0 || m > p.La) {
    bad = true;
    m = m < 0 ? 0 : p.La;
  }
  if (n < 0 || n > p.Lb) {
    bad = true;
    n = n < 0 ? 0 : p.Lb;
  }
  int32_t* sa = esm;
  int32_t* carry = sa + p.La;
  uint32_t* bits = reinterpret_cast<uint32_t*>(carry + p.La + 1);
  const int32_t* a = p.a + pair * p.La;
  for (int i = ln; i < m; i += EDIT_WAVE) sa[i] = a[i];
  __syncthreads();
  const int d = edit_wave_sweep<OPS>(sa, m, p.b + pair * p.Lb, n, carry, bits);
  if (OPS) __syncthreads();
  if (ln == 0) {
    p.dist[pair] = d;
    if (OPS) edit_backtrace(bits, m, n, p.ops + pair * 3);
    if (bad) atomicOr(p.err, CASR_DEV_BAD_TOKEN);
  }
}

hipError_t launch_edit_pairs(const int32_t* a, const int32_t* a_len, int La, const int32_t* b, const int32_t* b_len,
                             int Lb, int n, int32_t* dist, int32_t* ops, int32_t* err, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const EditPlan pl = edit_plan_pairs(La, Lb, n, ops != nullptr);
  if (pl.form != EDIT_FORM_WAVE) return hipErrorInvalidValue;
  const EditPairsArgs p{a, a_len, b, b_len, La, Lb, dist, ops, err};
  if (ops) {
    if (pl.raise_lds) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(edit_pairs_kernel<true>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(edit_pairs_kernel<true>, dim3(pl.grid), dim3(EDIT_WAVE), pl.lds_bytes, s, p);
  } else {
    hipLaunchKernelGGL(edit_pairs_kernel<false>, dim3(pl.grid), dim3(EDIT_WAVE), pl.lds_bytes, s, p);
  }
  return hipGetLastError();
}

// ------------------------------------------------------------------ all pairs of a beam's records
// One workgroup per utterance: the valid records' flat indices in (step, rank) order (list, count) and
// their weights w = exp(scale (c - c_max)).  LDS: reduction [MBR_THREADS] doubles, wave counts
__global__ __launch_bounds__(MBR_THREADS) void mbr_prepare_kernel(MbrArgs a) {
  __shared__ double red[MBR_THREADS];
  __shared__ int wcount[MBR_THREADS / 64];
  const BeamTree& t = a.t;
  const int b = blockIdx.x, tid = threadIdx.x, LK = t.L * t.k;
  const int steps = beam_executed_steps(t.newdone, t.L, t.B);
  int32_t* list = a.w.list + (size_t)b * LK;
  double* w = a.w.w + (size_t)b * LK;
  const int n = mbr_list_records(t.rec_valid + (size_t)b * LK, steps * t.k, LK, list, wcount);
  if (tid == 0) a.w.count[b] = n;
  // c of every record (kept in w), c_max over the workgroup
  const double cmax = mbr_comb_records(a, b, n, list, w, red);
  for (int p = tid; p < n; p += MBR_THREADS) w[p] = mbr_weight(a.scale, w[p], cmax);
}

// Distances d(p, q), q < p, as bytes at dist[b][p][q] (p, q positions in the utterance's list).  Grid
// (B, rows): workgroup y takes the records p = 1 + y, 1 + y + rows, ..  One wave per workgroup.
//   FORM lane: record p's tokens, LAST FIRST, are uniform across the wave (every lane walks the tree
//        and writes the same words: no hand-off between lanes); lane q rolls a row of D, as bytes
//        [column][lane] in LDS, down its own record, read last token first off the back-pointers, one
//        hop per row (the distance of two reversed rows is that of the rows).
//   FORM wave: both records expanded in LDS, then the anti-diagonal sweep of the pairs kernel.
template <int FORM>
__global__ __launch_bounds__(EDIT_WAVE) void mbr_dist_kernel(MbrArgs a) {
  extern __shared__ __attribute__((aligned(16))) int32_t esm[];
  const BeamTree& t = a.t;
  const int b = blockIdx.x, ln = threadIdx.x, k = t.k, L = t.L, LK = L * k;
  const int n = a.w.count[b];
  if (n < 2) return;  // (uniform)
  int32_t* sbp = esm;
  int32_t* stk = sbp + LK;
  int32_t* ua = stk + LK;  // record p's tokens [L]
  mbr_stage_tree(t, b, sbp, stk);
  __syncthreads();
  const TreeStaged<true> tree{sbp, stk, k};
  bool bad_bp = false;  // a record's start slot outside [0, k) (the staged pointers are clamped)
  const int32_t* list = a.w.list + (size_t)b * LK;
  uint8_t* dist = a.w.dist + (size_t)b * LK * LK;
  for (int p = 1 + blockIdx.y; p < n; p += gridDim.y) {
    const int fp = list[p], lp = fp / k;
    const int slot = t.rec_src[(size_t)b * LK + fp];
    if (FORM == EDIT_FORM_LANE) {
      uint8_t* row = reinterpret_cast<uint8_t*>(ua + L);  // [L + 1][64]
      bad_bp |= beam_walk(tree, k, slot, lp - 1, [&](int st, int32_t tok) { ua[lp - 1 - st] = tok; });
      for (int q = ln; q < p; q += EDIT_WAVE) {
        const int fq = list[q], lq = fq / k;
        int sq = beam_record_slot(t, (size_t)b * LK + fq, lq, &bad_bp);
        for (int c = 0; c <= lp; ++c) row[c * EDIT_WAVE + ln] = (uint8_t)c;
        for (int r = 1; r <= lq; ++r) {
          const int32_t tok = beam_hop(tree, lq - r, &sq);
          int diag = row[ln], left = r;
          row[ln] = (uint8_t)r;
          for (int c = 1; c <= lp; ++c) {
            const int up = row[c * EDIT_WAVE + ln];
            const int d = edit_cell(tok == ua[c - 1], diag, up, left);
            row[c * EDIT_WAVE + ln] = (uint8_t)d;
            diag = up;
            left = d;
          }
        }
        dist[(size_t)p * LK + q] = row[lp * EDIT_WAVE + ln];
      }
    } else {
      int32_t* ub = ua + L;
      int32_t* carry = ub + L;  // [L + 1]
      bad_bp |= beam_walk(tree, k, slot, lp - 1, [&](int st, int32_t tok) { ua[st] = tok; });
      for (int q = 0; q < p; ++q) {
        const int fq = list[q], lq = fq / k;
        bad_bp |= beam_walk(tree, k, t.rec_src[(size_t)b * LK + fq], lq - 1,
                            [&](int st, int32_t tok) { ub[st] = tok; });
        __syncthreads();
        const int d = edit_wave_sweep<false>(ua, lp, ub, lq, carry, nullptr);
        if (ln == 0) dist[(size_t)p * LK + q] = (uint8_t)d;
        __syncthreads();
      }
    }
  }
  if (bad_bp) atomicOr(t.err, CASR_DEV_BAD_BACKPTR);
}

// One workgroup per utterance: risk_p = sum_q w_q d(p, q) in ascending q, the winner by mbr_better, its
// tokens off the tree; without a record casr_beam's unfinished fallback, as the rescore keeps it.
__global__ __launch_bounds__(MBR_THREADS) void mbr_reduce_kernel(MbrArgs a) {
  __shared__ double redr[MBR_THREADS];
  __shared__ int32_t redi[MBR_THREADS];
  const BeamTree& t = a.t;
  const int b = blockIdx.x, tid = threadIdx.x, k = t.k, L = t.L, LK = L * k;
  const int n = a.w.count[b];
  const int32_t* list = a.w.list + (size_t)b * LK;
  const double* w = a.w.w + (size_t)b * LK;
  const uint8_t* dist = a.w.dist + (size_t)b * LK * LK;
  if (a.rec_risk) {
    for (int i = tid; i < LK; i += MBR_THREADS) a.rec_risk[(size_t)b * LK + i] = 0.0;
    __syncthreads();
  }
  double br = 0.0;
  int bi = -1;
  for (int p = tid; p < n; p += MBR_THREADS) {
    double r = 0.0;
    for (int q = 0; q < n; ++q) {
      const int d = q == p ? 0 : (q < p ? dist[(size_t)p * LK + q] : dist[(size_t)q * LK + p]);
      r = mbr_risk_add(r, w[q], d);
    }
    if (a.rec_risk) a.rec_risk[(size_t)b * LK + list[p]] = r;
    if (mbr_better(r, p, br, bi)) {
      br = r;
      bi = p;
    }
  }
  redr[tid] = br;
  redi[tid] = bi;
  __syncthreads();
  for (int o = MBR_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o && mbr_better(redr[tid + o], redi[tid + o], redr[tid], redi[tid])) {
      redr[tid] = redr[tid + o];
      redi[tid] = redi[tid + o];
    }
    __syncthreads();
  }
  const int win = redi[0];
  __syncthreads();  // (redi[0] is rewritten below as the length)
  int32_t* out = a.best_tokens + (size_t)b * L;
  if (win >= 0 ? (bi == win) : (tid == 0)) {
    int len, slot;
    float bs;
    if (win >= 0) {
      const int fi = list[win];
      const size_t ri = (size_t)b * LK + fi;
      len = fi / k;
      slot = t.rec_src[ri];
      bs = t.rec_score[ri];
      if (a.best_index) a.best_index[b] = fi;
      if (a.best_risk) a.best_risk[b] = br;
    } else {  // no record: casr_beam's unfinished fallback with its weights
      len = beam_executed_steps(t.newdone, L, t.B);
      slot = beam_live_row(t, b, a.beam_lm_weight, a.beam_length_weight, len, &bs);
      if (a.best_index) a.best_index[b] = -1;
      if (a.best_risk) a.best_risk[b] = 0.0;
    }
    const bool bad_bp = beam_walk(TreeGlobal(t, b), k, slot, len - 1, [&](int st, int32_t tok) { out[st] = tok; });
    a.best_len[b] = len;
    a.best_score[b] = bs;
    redi[0] = len;
    if (bad_bp) atomicOr(t.err, CASR_DEV_BAD_BACKPTR);
  }
  __syncthreads();
  const int len = redi[0];
  for (int st = len + tid; st < L; st += MBR_THREADS) out[st] = -1;
}

// the byte matrix as a full symmetric one: out [B][L k][L k], 0 on the diagonal and past the count
__global__ __launch_bounds__(MBR_THREADS) void mbr_expand_kernel(MbrBufs w, int LK, uint8_t* out, int32_t* n_rec) {
  const int b = blockIdx.x, n = w.count[b];
  const uint8_t* dist = w.dist + (size_t)b * LK * LK;
  uint8_t* o = out + (size_t)b * LK * LK;
  for (int i = threadIdx.x; i < LK * LK; i += MBR_THREADS) {
    const int p = i / LK, q = i - p * LK;
    o[i] = (p < n && q < n && p != q) ? (q < p ? dist[(size_t)p * LK + q] : dist[(size_t)q * LK + p]) : 0;
  }
  if (threadIdx.x == 0 && n_rec) n_rec[b] = n;
}

bool mbr_supported(int max_len, int k) {
  return edit_plan_mbr(max_len, k, EDIT_FORM_WAVE).form != EDIT_FORM_NONE &&
         edit_plan_mbr(max_len, k, EDIT_FORM_LANE).form != EDIT_FORM_NONE;
}

size_t carve_mbr(void* base, int B, int L, int k, MbrBufs& w) {
  Carver c(base);
  const size_t LK = (size_t)L * k;
  w.w = c.take<double>((size_t)B * LK);
  w.list = c.take<int32_t>((size_t)B * LK);
  w.count = c.take<int32_t>(B);
  w.dist = c.take<uint8_t>((size_t)B * LK * LK);
  return c.bytes(256);
}

hipError_t run_beam_mbr(const BeamTree& t, const MbrBufs& w, int map, double scale, const float* rec_lm,
                        double lm_weight, double length_weight, float beam_lm_weight, float beam_length_weight,
                        int32_t* best_tokens, int32_t* best_len, float* best_score, int32_t* best_index,
                        double* best_risk, double* rec_risk, hipStream_t s) {
  const EditPlan pl = edit_plan_mbr(t.L, t.k, map);
  if (pl.form == EDIT_FORM_NONE) return hipErrorInvalidValue;
  const MbrArgs m{t, scale, lm_weight, length_weight, beam_lm_weight, beam_length_weight, rec_lm, w,
                  best_tokens, best_len, best_score, best_index, best_risk, rec_risk};
  hipLaunchKernelGGL(mbr_prepare_kernel, dim3(t.B), dim3(MBR_THREADS), 0, s, m);
  if (pl.form == EDIT_FORM_LANE)
    hipLaunchKernelGGL(mbr_dist_kernel<EDIT_FORM_LANE>, dim3(t.B, pl.grid), dim3(EDIT_WAVE), pl.lds_bytes, s, m);
  else
    hipLaunchKernelGGL(mbr_dist_kernel<EDIT_FORM_WAVE>, dim3(t.B, pl.grid), dim3(EDIT_WAVE), pl.lds_bytes, s, m);
  hipLaunchKernelGGL(mbr_reduce_kernel, dim3(t.B), dim3(MBR_THREADS), 0, s, m);
  return hipGetLastError();
}

hipError_t run_mbr_distances(const BeamTree& t, const MbrBufs& w, uint8_t* dist, int32_t* n_rec, hipStream_t s) {
  hipLaunchKernelGGL(mbr_expand_kernel, dim3(t.B), dim3(MBR_THREADS), 0, s, w, t.L * t.k, dist, n_rec);
  return hipGetLastError();
}

}  // namespace casr
