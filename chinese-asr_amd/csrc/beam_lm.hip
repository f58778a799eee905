// Shallow fusion of the backoff n-gram LM into the beam search's first pass (include/casr.h
// casr_lm_terms, casr_beam_lm): the term row of a context (ngram_succ.h's row query, one workgroup
// per row), the select that ranks by (am + lm_weight lm) + len_l and carries am and lm separately,
// and the final choice; with their BIAS switch the select and the final choice are casr_beam_bias's too.
// The decode steps are run_beam's (decoder.hip run_beam_lm, run_beam_bias drive them).
//
// The term rows go through a workspace [R][V]: lm_terms_kernel writes a row once, the select reads
// it beside the logits row.  A row is assembled in LDS (4 V bytes), so the successors' scattered
// overwrites never leave the CU and the row goes out in one coalesced pass.
#include "beam_select.h"
#include "beam_tree.h"
#include "casr_internal.h"

namespace casr {

// ------------------------------------------------------------------ term rows
constexpr int LMT_THREADS = 256;

// One workgroup per row.  tree == 0: row i's context is ctx[i][0..3) / nc[i] (LM ids in [0, V + 3)).
// tree == 1: row i = b k + j of decode step l; its context is read off the beam tree (the tokens
// before, <s> before step 0), and the workgroup leaves at once where the select of step l would not
// run or not read the row (the early exit; step 0 ranks beam 0 only).
__global__ __launch_bounds__(LMT_THREADS) void lm_terms_kernel(NgramView m, NgramSuccView s, LmTermsSrc src,
                                                               int eos_token, float* __restrict__ terms,
                                                               int32_t* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) float trow[];
  __shared__ NgramRow row;
  __shared__ int flags;
  const int i = blockIdx.x, tid = threadIdx.x, V = m.V;
  if (src.tree) {
    if (done_before(src.newdone, src.l) >= src.B) return;
    if (src.l == 0 && i % src.k != 0) return;
  }
  if (tid == 0) {
    int32_t c[NGRAM_MAX_ORDER - 1] = {0, 0, 0};
    int nc = 0, fl = 0;
    if (src.tree) {
      const int b = i / src.k;
      int slot = i - b * src.k, st = src.l - 1;
      for (int j = 1; j < m.order; ++j) {
        if (st < 0) {
          c[nc++] = V;  // <s>
          break;
        }
        const size_t ix = (size_t)st * src.R + b * src.k + slot;
        const int t = src.tk[ix];
        if ((unsigned)t >= (unsigned)V) fl |= CASR_DEV_BAD_TOKEN;
        c[nc++] = (unsigned)t < (unsigned)V ? t : V + 2;
        int p = src.bp[ix];
        if ((unsigned)p >= (unsigned)src.k) {
          if (st > 0) fl |= CASR_DEV_BAD_BACKPTR;  // (step 0 has no predecessor node)
          p = 0;
        }
        slot = p;
        --st;
      }
    } else {
      nc = src.nc[i];
      for (int j = 0; j < NGRAM_MAX_ORDER - 1; ++j) c[j] = src.ctx[(size_t)i * (NGRAM_MAX_ORDER - 1) + j];
    }
    NgramRow r;
    ngram_row_prepare(m, s, c, nc, V + 3, &r);
    if (r.bad) fl |= CASR_DEV_BAD_TOKEN;
    row = r;
    flags = fl;
  }
  __syncthreads();
  for (int v = tid; v < V; v += LMT_THREADS) trow[v] = ngram_row_dense(m, row, v, eos_token);
  // orders ascending, a barrier between: the highest order wins (a list holds a word once)
  for (int n = 2; n <= row.nc + 1; ++n) {
    __syncthreads();
    const NgramSucc* e = s.list[n - 2] + row.succ[n - 2].offset;
    const uint32_t cnt = row.succ[n - 2].count;
    for (uint32_t q = tid; q < cnt; q += LMT_THREADS) {
      const NgramSucc x = e[q];
      if (ngram_row_takes(m, x.w, eos_token)) trow[x.w] = ngram_row_value(row, n, x.prob);
    }
  }
  __syncthreads();
  float* out = terms + (size_t)i * V;
  for (int v = tid; v < V; v += LMT_THREADS) out[v] = trow[v];
  if (tid == 0 && flags) atomicOr(err, flags);
}

bool lm_terms_supported(int V) { return (size_t)V * sizeof(float) <= LM_TERMS_LDS_BYTES; }

hipError_t launch_lm_terms(const NgramView& m, const NgramSuccView& sv, const LmTermsSrc& src, int n, int eos_token,
                           float* terms, int32_t* err, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(lm_terms_kernel, dim3(n), dim3(LMT_THREADS), (size_t)m.V * sizeof(float), s, m, sv, src,
                     eos_token, terms, err);
  return hipGetLastError();
}

// ------------------------------------------------------------------ the fused select
// LDS of one select: the rows' sorted lists and log-sum-exps, the utterance's list, and per wave its
// threshold candidates
// (GRAM: per row its candidate count; an empty base elsewhere, so the other selects' LDS is unchanged)
template <int NR, bool GRAM>
struct BeamGramSelLds {};
template <int NR>
struct BeamGramSelLds<NR, true> {
  int ncand[NR];
};

template <int K2, int NR, int NWV, bool GRAM = false>
struct BeamLmSelLds : BeamGramSelLds<NR, GRAM> {
  float rv[NR][K2];
  int ri[NR][K2];
  float lse[NR];
  float cv[K2];
  int ci[K2];
  float cvs[NWV][BS_CAP];
  int cis[NWV][BS_CAP];
  int cnt[NWV];
};

// One block per utterance, one wave per beam row (rows j = w, w + 8), as beam_select_block.  Per row:
// its log-sum-exp formed exactly as beam_select_block forms it at the same plan (from the projection's
// partials, or from the row), then every candidate's
//   am = (x / T - lse) + a,  lm = l == 0 ? term : g + term,  val = (am + lm_weight lm) + len_l
// (each operation rounded on its own) ranked to the row's top 2k: a lane computes its vals once and
// holds them; a threshold is found (the 2k-th largest of the lanes' two best), the candidates at or
// above it are collected, and those are ranked by counting.  The rows' lists are ranked the same way into the utterance's top 2k.  The
// bookkeeping is beam_select_block's on that ranking; the chosen candidates pass on am and lm, which
// their lane recomputes from the same operands (the same bits).
// LM / BIAS: which scorers take part (casr_beam_lm: LM alone; casr_beam_bias: BIAS, with or without LM).
// With BIAS the row's gain row (bias.hip) is read beside the logits, row r carries (s_r, C_r), and
//   bias = (float)(v == eos ? C_r : C_r + gain[v]) / 256,  val = ((am + lm_weight lm) + bias_weight bias) + len_l
// (without LM the lm_weight lm term is left out); the bookkeeping lanes walk the automaton for the
// chosen candidates' delta and out_sum (bias_plan.h) and pass on (delta, C_r + out_sum).
// GRAM (casr_beam_grammar, never with BIAS; the third operand is then BeamGramArgs): row r carries a grammar
// state s_r (-1: a dead row) and its mask row (grammar.hip) is read beside the logits.  Only the pairs
// whose bit is set are candidates: the others are never ranked, whatever their value, so a row's list
// and the utterance's may be shorter than 2k or empty, and then tau is -inf and it is the bit, not the
// threshold, that keeps a pair out.  lse is over the whole row.  The bookkeeping lanes get the chosen
// candidates' successor states with gram_next (grammar_plan.h); the slots no candidate takes are dead rows.
template <bool GRAM>
using BeamSideArgs = std::conditional_t<GRAM, BeamGramArgs, BeamBiasArgs>;

template <int K2, bool UNIT_T, bool LM, bool BIAS, bool GRAM = false>
__global__ __launch_bounds__(64 * bs_waves<K2>()) void beam_lm_select_kernel(BeamSelArgs a, BeamLmArgs g,
                                                                             BeamSideArgs<GRAM> sd) {
  static_assert(!(GRAM && BIAS), "the grammar select takes no bias");
  constexpr int NWV = bs_waves<K2>(), NTH = 64 * NWV;
  __shared__ BeamLmSelLds<K2, KMAX_BEAM, NWV, GRAM> S;
  if (done_before(a.newdone, a.l) >= a.B) return;
  const auto& hb = sd;  // BIAS
  const auto& gr = sd;  // GRAM
  const float* __restrict__ logits = a.logits;
  const float* __restrict__ terms = g.terms;
  const int32_t* __restrict__ gains = nullptr;
  float bw = 0.f;
  if constexpr (!GRAM) {
    gains = hb.gain;
    bw = hb.bias_weight;
  }
  [[maybe_unused]] const int GW = gram_mask_words(a.V);
  const int V = a.V, B = a.B, k = a.k, l = a.l, L = a.L, eos = a.eos, b = blockIdx.x;
  const float temperature = a.temperature;
  const GreedyPart& gp = a.gp;
  const int nbp = a.nbp;
  const int tid = threadIdx.x, ln = tid & 63, wv = tid >> 6;
  const int R = B * k;
  const int nrows = (l == 0) ? 1 : k;  // step 0 ranks beam 0 only
  const int n2k = 2 * k;
  const bool vec = (V & 3) == 0;
  const float lmw = g.lm_weight, len_l = g.len_l;
  auto xt = [&](float x) { return UNIT_T ? x : x / temperature; };

  for (int j = wv; j < nrows; j += NWV) {
    const size_t row = (size_t)(b * k + j);
    const float* x = logits + row * V;
    const float* t = LM ? terms + row * V : x;  // (without LM: never read)
    const int32_t* gn = BIAS ? gains + row * V : nullptr;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const float4* t4 = reinterpret_cast<const float4*>(t);
    const int4* gn4 = reinterpret_cast<const int4*>(gn);
    const float sc = a.score_cur[row];
    const float gc = (!LM || l == 0) ? 0.f : g.g_cur[row];
    int Cc = 0;
    if constexpr (BIAS) Cc = l == 0 ? 0 : hb.full_cur[row];
    const uint32_t* mk = nullptr;  // GRAM: the row's mask
    if constexpr (GRAM) {
      mk = gr.mask + row * GW;
      if (gr.st_cur[row] < 0) {  // a dead row offers nothing
        if (ln < n2k) {
          S.rv[j][ln] = -INFINITY;
          S.ri[j][ln] = 0x7fffffff;
        }
        if (ln == 0) {
          S.lse[j] = 0.f;
          S.ncand[j] = 0;
        }
        continue;
      }
      int nb = 0;
      for (int w = ln; w < GW; w += 64) nb += __popc(mk[w]);
      for (int o = 32; o > 0; o >>= 1) nb += __shfl_xor(nb, o);
      if (ln == 0) S.ncand[j] = nb;
    }
    auto allowed = [&](int v) { return GRAM ? ((mk[v >> 5] >> (v & 31)) & 1u) != 0 : true; };
    float lse;
    if (UNIT_T && nbp > 0 && gp.tmx && vec) {  // beam_select_block's first form: from the partials
      float mb = -INFINITY, sb = 0.f;
      if (ln < nbp) {
        mb = gp.mx[row * GP_NB + ln];
        sb = gp.se[row * GP_NB + ln];
      }
      const float M = wave_max(mb);
      const float s = wave_sum((sb > 0.f) ? sb * expf(mb - M) : 0.f);
      lse = logf(s) + M;
    } else {  // ... and its second: from the row
      float lm = -INFINITY;
      if (vec) {
#pragma unroll 4
        for (int i = ln; i < V / 4; i += 64) {
          const float4 q = x4[i];
          lm = fmaxf(lm, fmaxf(fmaxf(xt(q.x), xt(q.y)), fmaxf(xt(q.z), xt(q.w))));
        }
      } else {
        for (int v = ln; v < V; v += 64) lm = fmaxf(lm, xt(x[v]));
      }
      const float mm = wave_max(lm);
      float s = 0.f;
      if (vec) {
#pragma unroll 4
        for (int i = ln; i < V / 4; i += 64) {
          const float4 q = x4[i];
          s += expf(xt(q.x) - mm) + expf(xt(q.y) - mm) + expf(xt(q.z) - mm) + expf(xt(q.w) - mm);
        }
      } else {
        for (int v = ln; v < V; v += 64) s += expf(xt(x[v]) - mm);
      }
      s = wave_sum(s);
      lse = logf(s) + mm;
    }
    if (ln == 0) S.lse[j] = lse;
    auto val = [&](float xv, float tv, int gv, int v) {
      float r = (xt(xv) - lse) + sc;  // am
      if constexpr (LM) {
        const float lm = l == 0 ? tv : __fadd_rn(gc, tv);
        r = __fadd_rn(r, __fmul_rn(lmw, lm));
      }
      if constexpr (BIAS) {
        const float bias = __int2float_rn(v == eos ? Cc : Cc + gv) * (1.f / 256.f);  // (exact)
        r = __fadd_rn(r, __fmul_rn(bw, bias));
      }
      return __fadd_rn(r, len_l);
    };
    auto val_at = [&](int v) { return val(x[v], LM ? t[v] : 0.f, BIAS ? gn[v] : 0, v); };
    // this lane's largest and second-largest candidate values (distinct elements), then tau = the
    // 2k-th largest of the lanes' values: a lower bound of the row's 2k-th best
    float lt = -INFINITY, lt2 = -INFINITY;
    auto top2 = [&](float y) {
      lt2 = fmaxf(lt2, fminf(lt, y));
      lt = fmaxf(lt, y);
    };
    // a row of at most 64 x LMS_QB float4 (V <= 5,120): the lane's vals stay in registers between the
    // two passes, so the logits row and the term row are read once
    constexpr int LMS_QB = 20;
    const bool held = vec && V <= 4 * 64 * LMS_QB;
    float vq[LMS_QB][4];
    // GRAM: float4 i's four bits are nibble (i & 7) of mask word i >> 3; LMS_QB nibbles, 8 to a word
    [[maybe_unused]] uint32_t nib[(LMS_QB + 7) / 8] = {};
    auto nib_at = [&](int u, int e) { return GRAM ? ((nib[u >> 3] >> (4 * (u & 7) + e)) & 1u) != 0 : true; };
    if (held) {
#pragma unroll
      for (int u = 0; u < LMS_QB; ++u) {
        const int i = ln + 64 * u;
        if (i < V / 4) {
          const float4 xq = x4[i], w4 = LM ? t4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
          const int4 g4 = BIAS ? gn4[i] : make_int4(0, 0, 0, 0);
          vq[u][0] = val(xq.x, w4.x, g4.x, 4 * i);
          vq[u][1] = val(xq.y, w4.y, g4.y, 4 * i + 1);
          vq[u][2] = val(xq.z, w4.z, g4.z, 4 * i + 2);
          vq[u][3] = val(xq.w, w4.w, g4.w, 4 * i + 3);
          if constexpr (GRAM) nib[u >> 3] |= ((mk[i >> 3] >> (4 * (i & 7))) & 15u) << (4 * (u & 7));
        } else {
          vq[u][0] = vq[u][1] = vq[u][2] = vq[u][3] = -INFINITY;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (nib_at(u, e)) top2(vq[u][e]);
      }
    } else {
      for (int v = ln; v < V; v += 64)  // (a longer or unaligned row: two passes)
        if (allowed(v)) top2(val_at(v));
    }
    float tau = -INFINITY;
    for (int c = 0; c < n2k; ++c) {
      const float mx = wave_max(lt);
      tau = mx;
      const unsigned long long hit = __ballot(lt == mx);
      if (hit && ln == __ffsll((long long)hit) - 1) {
        lt = lt2;
        lt2 = -INFINITY;
      }
    }
    if (ln == 0) S.cnt[wv] = 0;
    __builtin_amdgcn_wave_barrier();
    // (an integer LDS counter hands out the slots; their order varies, the ranking below does not)
    auto offer = [&](float v, int idx) {
      if (v >= tau) {
        const int slot = atomicAdd(&S.cnt[wv], 1);
        if (slot < BS_CAP) {
          S.cvs[wv][slot] = v;
          S.cis[wv][slot] = idx;
        }
      }
    };
    if (held) {
#pragma unroll
      for (int u = 0; u < LMS_QB; ++u) {
        const int i = ln + 64 * u;
        if (i < V / 4) {  // (the padding never qualifies, whatever tau is)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (nib_at(u, e)) offer(vq[u][e], j * V + 4 * i + e);
        }
      }
    } else {
      for (int v = ln; v < V; v += 64)
        if (allowed(v)) offer(val_at(v), j * V + v);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    const int nc = S.cnt[wv];
    if (nc <= BS_CAP) {
      // a candidate's slot is the number of candidates better than it (better(): value, then lower
      // flat index; indices are distinct, so ranks are); unreached slots keep the sentinel
      if (ln < n2k) {
        S.rv[j][ln] = -INFINITY;
        S.ri[j][ln] = 0x7fffffff;
      }
      __builtin_amdgcn_wave_barrier();
      for (int p = ln; p < nc; p += 64) {
        const float pv = S.cvs[wv][p];
        const int pi = S.cis[wv][p];
        int rank = 0;
        for (int q = 0; q < nc; ++q) rank += better(S.cvs[wv][q], S.cis[wv][q], pv, pi) ? 1 : 0;
        if (rank < n2k) {
          S.rv[j][rank] = pv;
          S.ri[j][rank] = pi;
        }
      }
    } else {  // more ties at tau than the buffer holds: every element through sorted lane lists
      TopList<K2> tl;
      tl.init();
      for (int v = ln; v < V; v += 64)
        if (allowed(v)) tl.insert(val_at(v), j * V + v);
      wave_merge<K2>(tl, n2k, S.rv[j], S.ri[j]);
    }
  }
  if (tid < n2k) {
    S.cv[tid] = -INFINITY;
    S.ci[tid] = 0x7fffffff;
  }
  __syncthreads();  // every row's sorted list is in S.rv / S.ri
  // the utterance's top 2k: one thread per list entry (at most 16 x 32 = NTH), its slot the number
  // of entries of all lists better than it; sentinels write nothing
  for (int e = tid; e < nrows * n2k; e += NTH) {
    const int j = e / n2k, p = e - j * n2k;
    const float pv = S.rv[j][p];
    const int pi = S.ri[j][p];
    if (pi == 0x7fffffff) continue;
    int rank = 0;
    for (int jj = 0; jj < nrows; ++jj)
      for (int q = 0; q < n2k; ++q) rank += better(S.rv[jj][q], S.ri[jj][q], pv, pi) ? 1 : 0;
    if (rank < n2k) {
      S.cv[rank] = pv;
      S.ci[rank] = pi;
    }
  }
  __syncthreads();

  // bookkeeping (beam_select_block's, on the val ranking), one lane of wave 0 per ranked candidate
  if (wv == 0) {
    const int c = ln;
    const bool inr = c < n2k;
    int cc = inr ? S.ci[c] : 0;
    const bool bad = inr && (unsigned)cc >= (unsigned)(nrows * V);  // NaN rows leave empty slots
    if (bad) cc = 0;
    if constexpr (GRAM) {
      // an empty slot is a fault only where the utterance had more candidates than were ranked (NaN)
      int want = 0;
      for (int j = 0; j < nrows; ++j) want += S.ncand[j];
      want = want < n2k ? want : n2k;
      if (__popcll(__ballot(inr && !bad)) < want && ln == 0) atomicOr(a.err, CASR_DEV_BAD_CAND);
    } else {
      if (__ballot(bad) && ln == 0) atomicOr(a.err, CASR_DEV_BAD_CAND);
    }
    const bool has = GRAM ? inr && !bad : inr;  // this lane holds a ranked candidate
    const int beam = cc / V, tok = cc - beam * V;
    const bool f = has && tok == eos;
    const size_t srow = (size_t)(b * k + beam);
    float am = 0.f, lm = 0.f;
    int bs = 0, bC = 0;  // BIAS: the candidate's successor state and its full; GRAM: its successor state
    if (has) {
      am = (xt(logits[srow * V + tok]) - S.lse[beam]) + a.score_cur[srow];
      if constexpr (LM) {
        const float tv = terms[srow * V + tok];
        lm = l == 0 ? tv : __fadd_rn(g.g_cur[srow], tv);
      }
      if constexpr (BIAS) {
        bool sbad = false;
        bs = l == 0 ? 0 : bias_clamp_state(hb.m, hb.st_cur[srow], &sbad);
        bC = l == 0 ? 0 : hb.full_cur[srow];
        if (sbad) atomicOr(a.err, CASR_DEV_BAD_TOKEN);
        if (!f) bias_advance(hb.m, tok, &bs, &bC);  // (eos: the record keeps C_r, bias_closed)
      }
      if constexpr (GRAM) {
        const int s = gr.st_cur[srow];  // (a state: the row's mask had the candidate's bit)
        bs = (!f && (unsigned)s < (unsigned)gr.m.n_states) ? gram_next(gr.m, s, tok) : GRAM_DEAD;
      }
    }
    if (c < k) {  // finished hypotheses among the first k candidates
      const size_t ri = ((size_t)b * L + l) * k + c;
      a.rec_valid[ri] = f;
      if (f) {
        a.rec_score[ri] = am;
        if constexpr (LM) g.rec_lm[ri] = lm;
        if constexpr (BIAS) hb.rec_full[ri] = bC;
        a.rec_src[ri] = beam;
      }
    }
    if (ln == 0 && !a.topfin[b] && (tok == eos || !has)) {  // candidate 0 (GRAM: or an empty list)
      a.topfin[b] = 1;
      atomicAdd(&a.newdone[l], 1);
    }
    // active = first k non-EOS candidates in rank order, then EOS ones
    const unsigned long long ne = __ballot(has && !f), eo = __ballot(f);
    const unsigned long long below = (1ull << c) - 1ull;
    const int slot = f ? __popcll(ne) + __popcll(eo & below) : __popcll(ne & below);
    if constexpr (GRAM) {
      // the non-eos candidates alone; the slots they leave are dead rows, every word of the tree in range
      const int rw = b * k + c;
      if (c < k && c >= __popcll(ne)) {
        a.tok_next[rw] = eos;
        a.src_next[rw] = b * k;
        a.score_next[rw] = 0.f;
        if constexpr (LM) g.g_next[rw] = 0.f;
        gr.st_next[rw] = GRAM_DEAD;
        a.bp[(size_t)l * R + rw] = 0;
        a.tk[(size_t)l * R + rw] = eos;
      }
    }
    if (has && (GRAM ? !f : true) && slot < k) {
      const int rw = b * k + slot;
      a.tok_next[rw] = tok;
      a.src_next[rw] = b * k + beam;
      a.score_next[rw] = am;
      if constexpr (LM) g.g_next[rw] = lm;
      if constexpr (BIAS) {
        hb.st_next[rw] = bs;
        hb.full_next[rw] = bC;
      }
      if constexpr (GRAM) gr.st_next[rw] = bs;
      a.bp[(size_t)l * R + rw] = beam;
      a.tk[(size_t)l * R + rw] = tok;
    }
  }
}

template <int K2, bool LM, bool BIAS>
static void launch_beam_lm_select_k(const BeamSelArgs& a, const BeamLmArgs& g, const BeamBiasArgs& q, hipStream_t s) {
  auto kern = a.temperature == 1.0f ? beam_lm_select_kernel<K2, true, LM, BIAS>
                                    : beam_lm_select_kernel<K2, false, LM, BIAS>;
  hipLaunchKernelGGL(kern, dim3(a.B), dim3(64 * bs_waves<K2>()), 0, s, a, g, q);
}

template <bool LM, bool BIAS>
static hipError_t launch_beam_lm_select_of(const BeamSelArgs& a, const BeamLmArgs& g, const BeamBiasArgs& q, int K2,
                                           hipStream_t s) {
  switch (K2) {
    case 4: launch_beam_lm_select_k<4, LM, BIAS>(a, g, q, s); break;
    case 8: launch_beam_lm_select_k<8, LM, BIAS>(a, g, q, s); break;
    case 16: launch_beam_lm_select_k<16, LM, BIAS>(a, g, q, s); break;
    default: launch_beam_lm_select_k<32, LM, BIAS>(a, g, q, s);
  }
  return hipGetLastError();
}

hipError_t launch_beam_lm_select(const BeamSelArgs& a, const BeamLmArgs& g, int K2, hipStream_t s) {
  return launch_beam_lm_select_of<true, false>(a, g, BeamBiasArgs{}, K2, s);
}

hipError_t launch_beam_bias_select(const BeamSelArgs& a, const BeamLmArgs& g, const BeamBiasArgs& q, int K2,
                                   hipStream_t s) {
  return g.terms ? launch_beam_lm_select_of<true, true>(a, g, q, K2, s)
                 : launch_beam_lm_select_of<false, true>(a, g, q, K2, s);
}

template <int K2, bool LM>
static void launch_beam_gram_select_k(const BeamSelArgs& a, const BeamLmArgs& g, const BeamGramArgs& q, hipStream_t s) {
  auto kern = a.temperature == 1.0f ? beam_lm_select_kernel<K2, true, LM, false, true>
                                    : beam_lm_select_kernel<K2, false, LM, false, true>;
  hipLaunchKernelGGL(kern, dim3(a.B), dim3(64 * bs_waves<K2>()), 0, s, a, g, q);
}

template <bool LM>
static hipError_t launch_beam_gram_select_of(const BeamSelArgs& a, const BeamLmArgs& g, const BeamGramArgs& q, int K2,
                                             hipStream_t s) {
  switch (K2) {
    case 4: launch_beam_gram_select_k<4, LM>(a, g, q, s); break;
    case 8: launch_beam_gram_select_k<8, LM>(a, g, q, s); break;
    case 16: launch_beam_gram_select_k<16, LM>(a, g, q, s); break;
    default: launch_beam_gram_select_k<32, LM>(a, g, q, s);
  }
  return hipGetLastError();
}

hipError_t launch_beam_gram_select(const BeamSelArgs& a, const BeamLmArgs& g, const BeamGramArgs& q, int K2,
                                   hipStream_t s) {
  return g.terms ? launch_beam_gram_select_of<true>(a, g, q, K2, s) : launch_beam_gram_select_of<false>(a, g, q, K2, s);
}

// ------------------------------------------------------------------ the final choice
__device__ __forceinline__ float bias_of(int c) { return __int2float_rn(c) * (1.f / 256.f); }

// what the final choice reads beside the tree: the LM sums (LM) and the automaton's states and sums (BIAS)
struct FusedFinArgs {
  BeamTree t;
  float lmw, bw, lenw;
  const float* g[2];
  const float* rec_lm;
  const int32_t* st[2];
  const int32_t* full[2];
  const int32_t* rec_full;
  BiasView m;
  int32_t* best_tokens;
  int32_t* best_len;
  float* best_score;
  float* best_lm;    // or null
  float* best_bias;  // BIAS
  int32_t* steps;
  const int32_t* gst[2];  // GRAM: the rows' grammar states (-1: a dead row)
  uint8_t* complete;      // GRAM: 1 where the choice is a record
};

// (am + lm_weight lm) + len_l, with BIAS ((am [+ lm_weight lm]) + bias_weight bias) + len_l: every
// operation rounded on its own
template <bool LM, bool BIAS>
__device__ __forceinline__ float fused_comb(const FusedFinArgs& a, float am, float lm, float bias, int l) {
  const float len_l = (float)((double)a.lenw * (double)(l + 1));
  float r = am;
  if (LM) r = __fadd_rn(r, __fmul_rn(a.lmw, lm));
  if (BIAS) r = __fadd_rn(r, __fmul_rn(a.bw, bias));
  return __fadd_rn(r, len_l);
}

// One thread per utterance: the first maximum of the combined score over its valid records in (step,
// rank) order (BIAS: bias_closed), or without a record the first maximum over the k live rows of the last
// executed step (BIAS: bias_open, C + tail(s)); tokens by walking the back-pointers.  GRAM
// (casr_beam_grammar): the fallback skips the dead rows, and an utterance with neither a record nor a
// live row gives length 0 and score 0; complete says whether the choice is a record.
template <bool LM, bool BIAS, bool GRAM = false>
__global__ void beam_fused_finalize_kernel(FusedFinArgs a) {
  const BeamTree& t = a.t;
  const int b = blockIdx.x * blockDim.x + threadIdx.x, k = t.k, L = t.L;
  const int steps = beam_executed_steps(t.newdone, L, t.B);
  if (b == 0) a.steps[0] = steps;
  if (b >= t.B) return;
  int bl = -1, bc = -1;
  float bv = 0.f, bs = 0.f, bq = 0.f, bb = 0.f;
  for (int l = 0; l < steps; ++l)
    for (int c = 0; c < k; ++c) {
      const size_t ri = ((size_t)b * L + l) * k + c;
      if (!t.rec_valid[ri]) continue;
      const float lm = LM ? a.rec_lm[ri] : 0.f, bias = BIAS ? bias_of(a.rec_full[ri]) : 0.f;
      const float v = fused_comb<LM, BIAS>(a, t.rec_score[ri], lm, bias, l);
      if (bl < 0 || v > bv) {
        bl = l;
        bc = c;
        bv = v;
        bs = t.rec_score[ri];
        bq = lm;
        bb = bias;
      }
    }
  int32_t* out = a.best_tokens + (size_t)b * L;
  int len, slot;
  if (bl >= 0) {
    len = bl;
    slot = t.rec_src[((size_t)b * L + bl) * k + bc];
  } else {  // the select of step l writes buffer (l + 1) & 1; the last executed step is steps - 1
    const int w = steps & 1;
    len = steps;
    slot = 0;
    [[maybe_unused]] bool any = false;  // GRAM: a live row was seen
    for (int j = 0; j < k; ++j) {
      const int rw = b * k + j;
      if constexpr (GRAM)
        if (a.gst[w][rw] < 0) continue;
      float bias = 0.f;
      if (BIAS) {
        bool sbad = false;
        const int s = bias_clamp_state(a.m, a.st[w][rw], &sbad);
        if (sbad) atomicOr(t.err, CASR_DEV_BAD_TOKEN);
        bias = bias_of(a.full[w][rw] + a.m.node[s].tail);
      }
      const float lm = LM ? a.g[w][rw] : 0.f;
      const float v = fused_comb<LM, BIAS>(a, t.score[w][rw], lm, bias, steps - 1);
      if ((GRAM ? !any : j == 0) || v > bv) {
        bv = v;
        slot = j;
        bs = t.score[w][rw];
        bq = lm;
        bb = bias;
      }
      any = true;
    }
    if constexpr (GRAM)
      if (!any) len = 0;  // (bs and bq are still 0)
  }
  if constexpr (GRAM) a.complete[b] = bl >= 0 ? 1 : 0;
  if (beam_walk(TreeGlobal(t, b), k, slot, len - 1, [&](int s, int32_t tok) { out[s] = tok; }))
    atomicOr(t.err, CASR_DEV_BAD_BACKPTR);
  for (int s = len; s < L; ++s) out[s] = -1;
  a.best_len[b] = len;
  a.best_score[b] = bs;
  if (a.best_lm) a.best_lm[b] = bq;
  if (BIAS) a.best_bias[b] = bb;
}

hipError_t launch_beam_fused_finalize(const BeamTree& t, const BeamLmBufs* lw, const BeamBiasBufs* w,
                                      const BiasView* m, float bias_weight, float lm_weight, float length_weight,
                                      int32_t* best_tokens, int32_t* best_len, float* best_score, float* best_lm,
                                      float* best_bias, int32_t* steps, hipStream_t s) {
  if ((w != nullptr) != (m != nullptr) || (!lw && !w)) return hipErrorInvalidValue;
  FusedFinArgs f{t, lm_weight, bias_weight, length_weight};
  if (lw) {
    f.g[0] = lw->g[0], f.g[1] = lw->g[1];
    f.rec_lm = lw->rec_lm;
  }
  if (w) {
    f.st[0] = w->st[0], f.st[1] = w->st[1];
    f.full[0] = w->full[0], f.full[1] = w->full[1];
    f.rec_full = w->rec_full;
    f.m = *m;
  }
  f.best_tokens = best_tokens, f.best_len = best_len, f.best_score = best_score;
  f.best_lm = best_lm, f.best_bias = best_bias, f.steps = steps;
  const auto kern = !w ? beam_fused_finalize_kernel<true, false>
                       : lw ? beam_fused_finalize_kernel<true, true> : beam_fused_finalize_kernel<false, true>;
  hipLaunchKernelGGL(kern, dim3((t.B + 63) / 64), dim3(64), 0, s, f);
  return hipGetLastError();
}

hipError_t launch_beam_gram_finalize(const BeamTree& t, const BeamLmBufs* lw, const BeamGramBufs& w, float lm_weight,
                                     float length_weight, int32_t* best_tokens, int32_t* best_len, float* best_score,
                                     float* best_lm, uint8_t* complete, int32_t* steps, hipStream_t s) {
  FusedFinArgs f{t, lm_weight, 0.f, length_weight};
  if (lw) {
    f.g[0] = lw->g[0], f.g[1] = lw->g[1];
    f.rec_lm = lw->rec_lm;
  }
  f.best_tokens = best_tokens, f.best_len = best_len, f.best_score = best_score;
  f.best_lm = best_lm, f.best_bias = nullptr, f.steps = steps;
  f.gst[0] = w.st[0], f.gst[1] = w.st[1];
  f.complete = complete;
  const auto kern = lw ? beam_fused_finalize_kernel<true, false, true> : beam_fused_finalize_kernel<false, false, true>;
  hipLaunchKernelGGL(kern, dim3((t.B + 63) / 64), dim3(64), 0, s, f);
  return hipGetLastError();
}

// a per-record term of the fused beams as the API gives it: rec_lm as it is, or (rec_lm null) rec_full
// through bias_of, for the valid records of the executed steps, 0 elsewhere
__global__ void beam_record_term_kernel(BeamTree t, const float* __restrict__ rec_lm,
                                        const int32_t* __restrict__ rec_full, float* __restrict__ out) {
  const size_t n = (size_t)t.B * t.L * t.k;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int steps = beam_executed_steps(t.newdone, t.L, t.B);
  const int l = (int)((i / t.k) % t.L);
  out[i] = !(l < steps && t.rec_valid[i]) ? 0.f : rec_lm ? rec_lm[i] : bias_of(rec_full[i]);
}

static hipError_t run_beam_record_term(const BeamTree& t, const float* rec_lm, const int32_t* rec_full, float* out,
                                       hipStream_t s) {
  const size_t n = (size_t)t.B * t.L * t.k;
  hipLaunchKernelGGL(beam_record_term_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, t, rec_lm, rec_full,
                     out);
  return hipGetLastError();
}

hipError_t run_beam_record_lm(const BeamTree& t, const BeamLmBufs& w, float* rec_lm, hipStream_t s) {
  return run_beam_record_term(t, w.rec_lm, nullptr, rec_lm, s);
}

hipError_t run_beam_record_bias(const BeamTree& t, const BeamBiasBufs& w, float* rec_bias, hipStream_t s) {
  return run_beam_record_term(t, nullptr, w.rec_full, rec_bias, s);
}

}  // namespace casr

