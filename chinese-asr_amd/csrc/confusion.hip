// N-best lists and confusion networks over a beam's finished records on the device (include/casr.h
// casr_confusion, casr_beam_nbest, casr_beam_confusion).  The unit rule, the N-best order, the vote walk,
// the slot order and the plan are confusion_plan.h's, the text the host compiles too; the list of an
// utterance's records, c and c_max are mbr_device.h's, shared with casr_beam_mbr; the tree is read by
// beam_tree.h's rules.
//
// Three kernels: prepare (one workgroup per utterance), align (one wave per workgroup, a lane per record)
// and reduce (one wave per workgroup, a slot at a time).  After the units everything is integer
// arithmetic, and the only atomics are integer adds in LDS: no result depends on scheduling.
#include "casr_internal.h"
#include "confusion_plan.h"
#include "mbr_device.h"

namespace casr {

struct CnArgs {
  MbrArgs m;   // the tree (without one: B, k, L, V, rec_valid, err), the weights
  CnBufs w;
  bool tree;   // the records are the handle's beam tree; else the expanded rec_tokens with units given
  int lanes;   // records per align workgroup
  int N, M;    // 0: no N-best / no confusion network
  const int32_t* rec_tokens;  // [B][L k][L] (!tree)
  const int64_t* unit_in;     // [B][L k] (!tree)
  const int32_t* pivot;       // [B] flat indices, or null (tree): the top of the N-best order
  int32_t* nbest_index;
  int32_t* nbest_tokens;
  int32_t* nbest_len;
  double* nbest_comb;
  int32_t* n_slots;
  int32_t* slot_token;
  int64_t* slot_mass;
  int64_t* pivot_mass;
  int64_t* total;
  int64_t* rec_unit;  // or null
};

// ------------------------------------------------------------------ prepare
// One workgroup per utterance: the list, c and c_max (mbr_device.h), then u, U and rec_unit, a record's
// rank as the number of records before it under cn_before (all pairs inside the workgroup), the N best
// walked off the tree, and the pivot's position in the list.
__global__ __launch_bounds__(MBR_THREADS) void cn_prepare_kernel(CnArgs a) {
  __shared__ double red[MBR_THREADS];
  __shared__ int wcount[MBR_THREADS / 64];
  __shared__ unsigned long long usum;
  __shared__ int spos;
  const BeamTree& t = a.m.t;
  const int b = blockIdx.x, tid = threadIdx.x, k = t.k, L = t.L, LK = L * k;
  const int nn = a.tree ? beam_executed_steps(t.newdone, L, t.B) * k : LK;
  int32_t* list = a.w.list + (size_t)b * LK;
  double* c = a.w.c + (size_t)b * LK;
  if (tid == 0) {
    usum = 0;
    spos = -1;
  }
  if (a.M > 0 && a.rec_unit)
    for (int i = tid; i < LK; i += MBR_THREADS) a.rec_unit[(size_t)b * LK + i] = 0;
  const int n = mbr_list_records(t.rec_valid + (size_t)b * LK, nn, LK, list, wcount);
  if (tid == 0) a.w.count[b] = n;
  double cmax = NAN;
  if (a.tree) cmax = mbr_comb_records(a.m, b, n, list, c, red);
  __syncthreads();
  if (a.M > 0) {
    int64_t* u = a.w.unit + (size_t)b * LK;
    int64_t part = 0;
    for (int p = tid; p < n; p += MBR_THREADS) {
      const int64_t v = a.tree ? cn_unit(mbr_weight(a.m.scale, c[p], cmax))
                               : cn_unit_clamp(a.unit_in[(size_t)b * LK + list[p]]);
      u[p] = v;
      part += v;
      if (a.rec_unit) a.rec_unit[(size_t)b * LK + list[p]] = v;
    }
    if (part) atomicAdd(&usum, (unsigned long long)part);
  }
  const bool top = a.M > 0 && !a.pivot;
  if (a.tree && (a.N > 0 || top)) {
    const int lim = a.N > 0 ? a.N : 1;
    for (int r = (n < a.N ? n : a.N) + tid; r < a.N; r += MBR_THREADS) {
      const size_t o = (size_t)b * a.N + r;
      a.nbest_index[o] = -1;
      a.nbest_len[o] = 0;
      a.nbest_comb[o] = 0.0;
      for (int s = 0; s < L; ++s) a.nbest_tokens[o * L + s] = -1;
    }
    for (int p = tid; p < n; p += MBR_THREADS) {
      const double cp = c[p];
      const int fp = list[p];
      int rank = 0;
      for (int q = 0; q < n && rank < lim; ++q) rank += q != p && cn_before(c[q], list[q], cp, fp);
      if (rank == 0 && top) spos = p;
      if (rank >= a.N) continue;
      const size_t o = (size_t)b * a.N + rank;
      const int l = fp / k;
      a.nbest_index[o] = fp;
      a.nbest_len[o] = l;
      a.nbest_comb[o] = cp;
      int32_t* out = a.nbest_tokens + o * L;
      if (beam_walk(TreeGlobal(t, b), k, t.rec_src[(size_t)b * LK + fp], l - 1,
                    [&](int st, int32_t tok) { out[st] = tok; }))
        atomicOr(t.err, CASR_DEV_BAD_BACKPTR);
      for (int st = l; st < L; ++st) out[st] = -1;
    }
  }
  if (a.M > 0 && a.pivot) {
    const int pv = a.pivot[b];
    for (int p = tid; p < n; p += MBR_THREADS)
      if (list[p] == pv) spos = p;
  }
  __syncthreads();
  if (a.M > 0 && tid == 0) {
    a.total[b] = (int64_t)usum;
    a.w.ppos[b] = spos;
    a.n_slots[b] = spos < 0 ? 0 : cn_slots(list[spos] / k);
  }
}

// ------------------------------------------------------------------ align
// Grid (B, plan.align_groups), one wave: workgroup g takes the records at list positions g lanes ..  The
// pivot's tokens are uniform (LDS ua); a lane expands its own record into LDS as int16, rolls a column
// of D as bytes over its record's tokens, keeps the direction code of every cell (edit_plan.h's words,
// all [.][lane]) and walks them back by cn_walk: the lanes leave a row together, so their stores to a
// slot's votes [B][2 L + 1][L k] are adjacent.
template <bool TREE>
__global__ __launch_bounds__(CN_WAVE) void cn_align_kernel(CnArgs a) {
  extern __shared__ __attribute__((aligned(16))) int32_t csm[];
  const BeamTree& t = a.m.t;
  const int b = blockIdx.x, g = blockIdx.y, ln = threadIdx.x, k = t.k, L = t.L, LK = L * k, V = t.V;
  const int lanes = a.lanes, n = a.w.count[b], ppos = a.w.ppos[b];
  if (ppos < 0 || g * lanes >= n) return;  // (uniform)
  int32_t* ua = csm;  // the pivot [L]
  int32_t* sbp = ua + L;
  int32_t* stk = sbp + LK;
  uint32_t* bits = reinterpret_cast<uint32_t*>(ua + L + (TREE ? 2 * LK : 0));
  int16_t* tokl = reinterpret_cast<int16_t*>(bits + edit_bits_words(L, L) * lanes);
  uint8_t* col = reinterpret_cast<uint8_t*>(tokl + (size_t)L * lanes);
  if (TREE) {
    mbr_stage_tree(t, b, sbp, stk);
    __syncthreads();
  }
  const TreeStaged<true> tree{sbp, stk, k};
  const int32_t* list = a.w.list + (size_t)b * LK;
  const int fp = list[ppos], m = fp / k;
  bool bad = false, bad_bp = false;  // (bad_bp: a record's start slot; the staged pointers are clamped)
  if (TREE) {
    if (ln == 0)
      bad_bp = beam_walk(tree, k, t.rec_src[(size_t)b * LK + fp], m - 1,
                         [&](int st, int32_t tok) { ua[st] = cn_token(tok, V); });
  } else {
    const int32_t* row = a.rec_tokens + ((size_t)b * LK + fp) * L;
    for (int i = ln; i < m; i += CN_WAVE) {
      const int32_t t = row[i];
      bad |= (uint32_t)t >= (uint32_t)V;
      ua[i] = cn_token(t, V);
    }
  }
  __syncthreads();
  if (g == 0)
    for (int i = ln; i < m; i += CN_WAVE) a.w.ptok[(size_t)b * L + i] = ua[i];
  const int p = g * lanes + ln;
  if (ln < lanes && p < n) {
    const int fq = list[p], lq = fq / k;
    if (TREE) {
      bad_bp |= beam_walk(tree, k, t.rec_src[(size_t)b * LK + fq], lq - 1,
                          [&](int st, int32_t tok) { tokl[st * lanes + ln] = (int16_t)cn_token(tok, V); });
    } else {
      const int32_t* row = a.rec_tokens + ((size_t)b * LK + fq) * L;
      for (int j = 0; j < lq; ++j) {
        const int32_t t = row[j];
        bad |= (uint32_t)t >= (uint32_t)V;
        tokl[j * lanes + ln] = (int16_t)cn_token(t, V);
      }
    }
    const int stride = edit_bits_stride(m);
    for (int i = 0; i <= m; ++i) col[i * lanes + ln] = (uint8_t)i;
    for (int j = 0; j < lq; ++j) {
      const int32_t bj = tokl[j * lanes + ln];
      int diag = col[ln], up = j + 1;
      col[ln] = (uint8_t)up;
      uint32_t acc = 0;
      for (int i = 0; i < m; ++i) {
        const int left = col[(i + 1) * lanes + ln];
        const bool match = ua[i] == bj;
        const int d = edit_cell(match, diag, up, left);
        acc |= (uint32_t)edit_dir(match, d, diag, up) << edit_bits_shift(i);
        if ((i & 15) == 15 || i == m - 1) {
          bits[edit_bits_word(i, j, stride) * lanes + ln] = acc;
          acc = 0;
        }
        col[(i + 1) * lanes + ln] = (uint8_t)d;
        diag = left;
        up = d;
      }
    }
    int16_t* v = a.w.votes + (size_t)b * cn_slots(L) * LK + p;
    cn_walk(
        m, lq,
        [&](int i, int j) { return (int)((bits[edit_bits_word(i, j, stride) * lanes + ln] >> edit_bits_shift(i)) & 3); },
        [&](int j) { return (int32_t)tokl[j * lanes + ln]; }, [&](int s, int32_t t) { v[(size_t)s * LK] = (int16_t)t; });
  }
  if (bad) atomicOr(t.err, CASR_DEV_BAD_TOKEN);
  if (bad_bp) atomicOr(t.err, CASR_DEV_BAD_BACKPTR);
}

// ------------------------------------------------------------------ reduce
// Grid (B, plan.reduce_groups), one wave: workgroup y takes the slots y, y + groups, ..  LDS: int64 masses
// over V + 1 bins (bin = token + 1, EPS in bin 0), zeroed once, then the touched bins' list.  Per slot the
// lanes read the votes and the units coalesced and add with LDS integer atomics; the lane that finds a
// bin at 0 lists it (every unit added is positive, so exactly one does).  M rounds of the arg-max under
// cn_slot_before over the list, each winner zeroed as it is written; the rest is cleared afterwards.
__global__ __launch_bounds__(CN_WAVE) void cn_reduce_kernel(CnArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long hist[];
  __shared__ int ntouched;
  const int b = blockIdx.x, y = blockIdx.y, ln = threadIdx.x, k = a.m.t.k, L = a.m.t.L, LK = L * k, V = a.m.t.V, M = a.M;
  const int SM = cn_slots(L), n = a.w.count[b], ppos = a.w.ppos[b];
  const int S = ppos < 0 ? 0 : cn_slots(a.w.list[(size_t)b * LK + ppos] / k);
  for (int s = y; s < SM; s += gridDim.y)
    if (s >= S)
      for (int e = ln; e < M; e += CN_WAVE) {
        a.slot_token[((size_t)b * SM + s) * M + e] = CN_NONE;
        a.slot_mass[((size_t)b * SM + s) * M + e] = 0;
      }
  if (y == 0)
    for (int i = ln; i < L; i += CN_WAVE)
      if (2 * i + 1 >= S) a.pivot_mass[(size_t)b * L + i] = 0;
  if (S == 0) return;  // (uniform)
  int32_t* touched = reinterpret_cast<int32_t*>(hist + V + 1);
  for (int i = ln; i <= V; i += CN_WAVE) hist[i] = 0;
  if (ln == 0) ntouched = 0;
  __syncthreads();
  const int64_t* u = a.w.unit + (size_t)b * LK;
  for (int s = y; s < S; s += gridDim.y) {
    const int16_t* row = a.w.votes + ((size_t)b * SM + s) * LK;
    for (int p = ln; p < n; p += CN_WAVE) {
      const int64_t v = u[p];
      if (v <= 0) continue;
      int bin = row[p] + 1;
      if ((unsigned)bin > (unsigned)V) bin = 0;  // (never: align wrote every vote of a slot below S)
      if (atomicAdd(&hist[bin], (unsigned long long)v) == 0) touched[atomicAdd(&ntouched, 1)] = bin;
    }
    __syncthreads();
    const int nt = ntouched;
    if ((s & 1) && ln == 0) a.pivot_mass[(size_t)b * L + (s >> 1)] = (int64_t)hist[a.w.ptok[(size_t)b * L + (s >> 1)] + 1];
    __syncthreads();
    for (int r = 0; r < M; ++r) {
      int64_t bm = 0;
      int bb = -1;
      for (int t = ln; t < nt; t += CN_WAVE) {
        const int bin = touched[t];
        const int64_t mm = (int64_t)hist[bin];
        if (mm > 0 && (bb < 0 || cn_slot_before(mm, bin - 1, bm, bb - 1))) {
          bm = mm;
          bb = bin;
        }
      }
      for (int o = CN_WAVE / 2; o > 0; o >>= 1) {
        const int64_t om = __shfl_xor(bm, o);
        const int ob = __shfl_xor(bb, o);
        if (ob >= 0 && (bb < 0 || cn_slot_before(om, ob - 1, bm, bb - 1))) {
          bm = om;
          bb = ob;
        }
      }
      __syncthreads();  // every lane has read the masses of this round
      if (ln == 0) {
        a.slot_token[((size_t)b * SM + s) * M + r] = bb < 0 ? CN_NONE : bb - 1;
        a.slot_mass[((size_t)b * SM + s) * M + r] = bb < 0 ? 0 : bm;
        if (bb >= 0) hist[bb] = 0;
      }
      __syncthreads();
    }
    for (int t = ln; t < nt; t += CN_WAVE) hist[touched[t]] = 0;
    if (ln == 0) ntouched = 0;
    __syncthreads();
  }
}

// ------------------------------------------------------------------ host side
bool confusion_supported(int B, int max_len, int k, int V, bool tree) {
  return confusion_plan(B, max_len, k, V, tree).ok;
}

// votes: the confusion network's kernels follow (casr_beam_nbest needs the list and c only)
size_t carve_confusion(void* base, int B, int L, int k, bool votes, CnBufs& w) {
  Carver c(base);
  const size_t LK = (size_t)L * k;
  w.c = c.take<double>((size_t)B * LK, 256);
  w.unit = c.take<int64_t>((size_t)B * LK, 256);
  w.list = c.take<int32_t>((size_t)B * LK, 256);
  w.count = c.take<int32_t>(B, 256);
  w.ppos = c.take<int32_t>(B, 256);
  w.ptok = c.take<int32_t>((size_t)B * L, 256);
  w.votes = votes ? c.take<int16_t>((size_t)B * cn_slots(L) * LK, 256) : nullptr;
  return cn_round256(c.bytes());
}

static CnArgs cn_beam_args(const BeamTree& t, const CnBufs& w, double scale, const float* rec_lm, double lm_weight,
                           double length_weight) {
  CnArgs c{};  // (what is not named stays null: the MBR's outputs and workspace are not read here)
  c.m.t = t;
  c.m.scale = scale;
  c.m.lm_weight = lm_weight;
  c.m.length_weight = length_weight;
  c.m.rec_lm = rec_lm;
  c.w = w;
  c.tree = true;
  return c;
}

template <class K>
static hipError_t cn_raise(K kernel, bool raise, size_t bytes) {
  if (!raise) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)bytes);
}

// prepare, align and reduce.  Both LDS limits are raised before the first launch: a call that fails has
// launched nothing
static hipError_t cn_launch_network(CnArgs& c, const ConfusionPlan& pl, hipStream_t s) {
  c.lanes = pl.lanes;
  const dim3 ga(c.m.t.B, pl.align_groups), gr(c.m.t.B, pl.reduce_groups);
  hipError_t e = c.tree ? cn_raise(cn_align_kernel<true>, pl.align_raise, pl.align_lds)
                        : cn_raise(cn_align_kernel<false>, pl.align_raise, pl.align_lds);
  if (e != hipSuccess) return e;
  if ((e = cn_raise(cn_reduce_kernel, pl.reduce_raise, pl.reduce_lds)) != hipSuccess) return e;
  hipLaunchKernelGGL(cn_prepare_kernel, dim3(c.m.t.B), dim3(MBR_THREADS), 0, s, c);
  if (c.tree)
    hipLaunchKernelGGL(cn_align_kernel<true>, ga, dim3(CN_WAVE), pl.align_lds, s, c);
  else
    hipLaunchKernelGGL(cn_align_kernel<false>, ga, dim3(CN_WAVE), pl.align_lds, s, c);
  hipLaunchKernelGGL(cn_reduce_kernel, gr, dim3(CN_WAVE), pl.reduce_lds, s, c);
  return hipGetLastError();
}

hipError_t run_beam_nbest(const BeamTree& t, const CnBufs& w, int N, const float* rec_lm, double lm_weight,
                          double length_weight, int32_t* nbest_index, int32_t* nbest_tokens, int32_t* nbest_len,
                          double* nbest_comb, hipStream_t s) {
  CnArgs c = cn_beam_args(t, w, 0.0, rec_lm, lm_weight, length_weight);
  c.N = N;
  c.nbest_index = nbest_index;
  c.nbest_tokens = nbest_tokens;
  c.nbest_len = nbest_len;
  c.nbest_comb = nbest_comb;
  hipLaunchKernelGGL(cn_prepare_kernel, dim3(t.B), dim3(MBR_THREADS), 0, s, c);
  return hipGetLastError();
}

hipError_t run_beam_confusion(const BeamTree& t, const CnBufs& w, int M, double scale, const float* rec_lm,
                              double lm_weight, double length_weight, const int32_t* pivot, int32_t* n_slots,
                              int32_t* slot_token, int64_t* slot_mass, int64_t* pivot_mass, int64_t* total,
                              int64_t* rec_unit, hipStream_t s) {
  const ConfusionPlan pl = confusion_plan(t.B, t.L, t.k, t.V, true);
  if (!pl.ok) return hipErrorInvalidValue;
  CnArgs c = cn_beam_args(t, w, scale, rec_lm, lm_weight, length_weight);
  c.M = M;
  c.pivot = pivot;
  c.n_slots = n_slots;
  c.slot_token = slot_token;
  c.slot_mass = slot_mass;
  c.pivot_mass = pivot_mass;
  c.total = total;
  c.rec_unit = rec_unit;
  return cn_launch_network(c, pl, s);
}

hipError_t run_confusion(const CnBufs& w, const int32_t* rec_tokens, const uint8_t* rec_valid, const int64_t* rec_unit,
                         const int32_t* pivot, int B, int L, int k, int V, int M, int32_t* n_slots,
                         int32_t* slot_token, int64_t* slot_mass, int64_t* pivot_mass, int64_t* total, int32_t* err,
                         hipStream_t s) {
  const ConfusionPlan pl = confusion_plan(B, L, k, V, false);
  if (!pl.ok) return hipErrorInvalidValue;
  CnArgs c{};
  c.m.t.B = B;
  c.m.t.k = k;
  c.m.t.L = L;
  c.m.t.V = V;
  c.m.t.rec_valid = rec_valid;
  c.m.t.err = err;
  c.w = w;
  c.tree = false;
  c.M = M;
  c.rec_tokens = rec_tokens;
  c.unit_in = rec_unit;
  c.pivot = pivot;
  c.n_slots = n_slots;
  c.slot_token = slot_token;
  c.slot_mass = slot_mass;
  c.pivot_mass = pivot_mass;
  c.total = total;
  return cn_launch_network(c, pl, s);
}

}  // namespace casr
