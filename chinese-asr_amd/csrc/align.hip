// The monotone path through an attention matrix on the device (include/casr.h casr_align_path): per
// token the first, last and peak frame of its cells on the best path, and the path's score.  The
// weight, the tie order, the move bits, the backtrack and the plan are align_plan.h's, the text the
// host compiles too; integers throughout, so the scans below give the sequential host's bits.
//
// Mapping.  align is [L][Tp][B]: the B utterances of a cell are adjacent, one utterance's row is
// strided by 4 B bytes.  A workgroup takes `group` adjacent utterances (the plan's choice is 4: 16-byte
// runs of a cell; 16, the whole 64-byte run, measured slower), one wave each: per row l
// it loads the [T][group] tile, quantises, and writes it transposed to LDS as int16 (two tiles: row
// l + 1 is fetched into registers before row l is scanned, and slower waves may still scan the other
// tile; one barrier per row).  A wave scans its utterance's row in chunks of 64 frames.  With
// E[t] = max(diagonal, vertical) from the row above and P the inclusive prefix sum of the row's q,
//   D[l][t] = P[t] + max_{s <= t} (E[s] - P[s - 1]),
// and the cell stays exactly when the maximum over s < t beats the term of s = t: a prefix sum and a
// prefix maximum over the lanes (data-parallel-primitive moves, no LDS), their last lane carried to the
// next chunk.  Two ballots per chunk are the move bits.  After the last row one lane walks the bits
// back, and the wave reads each token's span again for its peak.
#include "align_plan.h"
#include "casr_internal.h"

namespace casr {

// ------------------------------------------------------------------ scans over the 64 lanes
// Data-parallel-primitive moves, no LDS traffic: a lane without a source keeps `old`, the operation's
// identity.  Four shifts inside each row of 16 lanes make the row's inclusive scan; then the last lane
// of rows 0 and 2 goes to every lane of rows 1 and 3, and lane 31 to the upper half.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int align_dpp(int old, int v) {
  return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xf, false);
}
constexpr int DPP_ROW_SHR = 0x110, DPP_WAVE_SHR1 = 0x138, DPP_ROW_BCAST15 = 0x142, DPP_ROW_BCAST31 = 0x143;

__device__ __forceinline__ int wave_scan_add(int v) {
  v += align_dpp<DPP_ROW_SHR + 1, 0xf>(0, v);
  v += align_dpp<DPP_ROW_SHR + 2, 0xf>(0, v);
  v += align_dpp<DPP_ROW_SHR + 4, 0xf>(0, v);
  v += align_dpp<DPP_ROW_SHR + 8, 0xf>(0, v);
  v += align_dpp<DPP_ROW_BCAST15, 0xa>(0, v);
  v += align_dpp<DPP_ROW_BCAST31, 0xc>(0, v);
  return v;
}

__device__ __forceinline__ int wave_scan_max(int v) {
  v = max(v, align_dpp<DPP_ROW_SHR + 1, 0xf>(INT32_MIN, v));
  v = max(v, align_dpp<DPP_ROW_SHR + 2, 0xf>(INT32_MIN, v));
  v = max(v, align_dpp<DPP_ROW_SHR + 4, 0xf>(INT32_MIN, v));
  v = max(v, align_dpp<DPP_ROW_SHR + 8, 0xf>(INT32_MIN, v));
  v = max(v, align_dpp<DPP_ROW_BCAST15, 0xa>(INT32_MIN, v));
  v = max(v, align_dpp<DPP_ROW_BCAST31, 0xc>(INT32_MIN, v));
  return v;
}

constexpr int ALIGN_PF = ALIGN_MAX_TP / ALIGN_WAVE;  // values of a row's tile a thread loads at most
constexpr int ALIGN_PEAK_BATCH = 4;                  // spans whose cells are fetched before any is reduced

struct AlignArgs {
  const float* align;
  const int32_t* enc_len;
  const int32_t* tgt_len;
  int B, Tp, L;
  int gshift;  // log2 of the plan's group
  int chunks, dw, qstride;
  int32_t* first;
  int32_t* last;
  int32_t* peak;
  int32_t* path_score;  // or null
  int32_t* err;
};

__global__ __launch_bounds__(ALIGN_WAVE* ALIGN_GROUP_MAX) void align_path_kernel(AlignArgs p) {
  extern __shared__ __attribute__((aligned(16))) uint64_t asm64[];
  const int G = 1 << p.gshift, tid = threadIdx.x, u = tid >> 6, ln = tid & 63;
  const int b0 = blockIdx.x * G, b = b0 + u;
  const int L = p.L, Tp = p.Tp, chunks = p.chunks;
  uint64_t* bits = asm64 + (size_t)u * align_bits_words(L, chunks);
  int32_t* drows = reinterpret_cast<int32_t*>(asm64 + (size_t)G * align_bits_words(L, chunks));
  int16_t* tiles = reinterpret_cast<int16_t*>(drows + (size_t)G * 2 * p.dw);
  int32_t* sT = reinterpret_cast<int32_t*>(tiles + (size_t)2 * G * p.qstride);
  int32_t* sN = sT + G;
  int32_t* D = drows + (size_t)u * 2 * p.dw;

  // (d) lengths: clamped and reported; an utterance without a cell, and a wave past B, take no part
  if (ln == 0) {
    int T = 0, n = 0;
    if (b < p.B) {
      T = p.enc_len[b];
      n = p.tgt_len[b];
      const bool bad_t = align_clamp(T, Tp), bad_n = align_clamp(n, L);
      if (bad_t || bad_n) atomicOr(p.err, CASR_DEV_BAD_TOKEN);
      if (n == 0 || T == 0) n = T = 0;
    }
    sT[u] = T;
    sN[u] = n;
  }
  __syncthreads();
  const int T = sT[u], n = sN[u];
  int tmax = 0, nmax = 0;
  for (int i = 0; i < G; ++i) {
    tmax = max(tmax, sT[i]);
    nmax = max(nmax, sN[i]);
  }

  // a row's tile: thread -> (frame, utterance), utterance innermost as in memory: a thread keeps its
  // utterance and takes every 64th frame.  The values of row l + 1 are fetched into registers before
  // row l is scanned and quantised into LDS after it.
  float pf[ALIGN_PF];
  const int t0 = tid >> p.gshift, uu = tid & (G - 1), tu = sT[uu], nu = sN[uu];
  const size_t hop = (size_t)ALIGN_WAVE * p.B;  // 64 frames on
  auto fetch = [&](int l) {
    const float* src = p.align + ((size_t)l * Tp + t0) * p.B + b0 + uu;
#pragma unroll
    for (int k = 0; k < ALIGN_PF; ++k) {
      pf[k] = 0.f;
      if (t0 + k * ALIGN_WAVE < tu && l < nu) pf[k] = src[k * hop];
    }
  };
  if (nmax > 0) fetch(0);
  for (int l = 0; l < nmax; ++l) {
    int16_t* tile = tiles + ((size_t)(l & 1) * G + uu) * p.qstride + t0;
#pragma unroll
    for (int k = 0; k < ALIGN_PF; ++k)
      if (t0 + k * ALIGN_WAVE < tmax) tile[k * ALIGN_WAVE] = (int16_t)align_quant(pf[k]);
    if (l + 1 < nmax) fetch(l + 1);
    __syncthreads();
    if (l >= n) continue;  // (uniform in the wave; the barrier above is the row's only one)
    const int16_t* sq = tiles + ((size_t)(l & 1) * G + u) * p.qstride;
    const int32_t* Dp = D + ((l & 1) ^ 1) * p.dw;
    int32_t* Dc = D + (l & 1) * p.dw;
    int Pc = 0, Mc = INT32_MIN;  // the chunks before: the row's prefix sum, and the maximum (compared only)
    for (int c = 0; c * ALIGN_WAVE < T; ++c) {
      const int t = c * ALIGN_WAVE + ln;
      const bool on = t < T;
      const int qv = on ? sq[t] : 0;
      const int P = wave_scan_add(qv) + Pc;
      int E = t == 0 ? 0 : ALIGN_NEG, mv = ALIGN_DIAG;
      if (l > 0) {
        const int vert = on ? Dp[t] : ALIGN_NEG;
        const int diag = (on && t > 0) ? Dp[t - 1] : ALIGN_NEG;
        mv = align_enter_move(diag, vert);
        E = mv == ALIGN_DIAG ? diag : vert;
      }
      const int a = on ? E - (P - qv) : INT32_MIN;
      const int M = max(wave_scan_max(a), Mc);
      const int Mex = align_dpp<DPP_WAVE_SHR1, 0xf>(Mc, M);  // (lane 0: the chunks before)
      const bool stay = Mex > a;
      if (stay) mv = ALIGN_STAY;
      if (on) Dc[t] = P + (stay ? Mex : a);
      const uint64_t w0 = __ballot(on && (mv & 1)), w1 = __ballot(on && (mv >> 1));
      if (ln == 0) {
        bits[((size_t)l * chunks + c) * 2] = w0;
        bits[((size_t)l * chunks + c) * 2 + 1] = w1;
      }
      Pc = __builtin_amdgcn_readlane(P, ALIGN_WAVE - 1);
      Mc = __builtin_amdgcn_readlane(M, ALIGN_WAVE - 1);
    }
  }
  __syncthreads();  // every row and every move bit of this wave is in LDS

  // (c) one lane walks back; first and last take the place of the D rows
  int32_t* sf = D;
  int32_t* sl = D + p.dw;
  if (ln == 0 && n > 0) {
    const int32_t score = D[((n - 1) & 1) * p.dw + T - 1];
    align_backtrack(bits, chunks, n, T, sf, sl);
    if (p.path_score) p.path_score[b] = score;
  }
  if (ln == 0 && n == 0 && b < p.B && p.path_score) p.path_score[b] = 0;
  __syncthreads();
  if (b >= p.B) return;
  int32_t* of = p.first + (size_t)b * L;
  int32_t* ol = p.last + (size_t)b * L;
  int32_t* op = p.peak + (size_t)b * L;
  for (int l = ln; l < L; l += ALIGN_WAVE) {
    of[l] = l < n ? sf[l] : -1;
    ol[l] = l < n ? sl[l] : -1;
    if (l >= n) op[l] = -1;
  }
  // the peak of each span: its cells once more from memory (at most T + n of them in all), a few
  // spans' first 64 cells in flight together; (weight, frame) as one key whose maximum is the peak
  for (int l0 = 0; l0 < n; l0 += ALIGN_PEAK_BATCH) {
    int key[ALIGN_PEAK_BATCH];
#pragma unroll
    for (int k = 0; k < ALIGN_PEAK_BATCH; ++k) {
      const int l = l0 + k;
      key[k] = INT32_MIN;
      if (l < n && sf[l] + ln <= sl[l])
        key[k] = align_peak_key(align_quant(p.align[((size_t)l * Tp + sf[l] + ln) * p.B + b]), sf[l] + ln);
    }
#pragma unroll
    for (int k = 0; k < ALIGN_PEAK_BATCH; ++k) {
      const int l = l0 + k;
      if (l >= n) break;  // (uniform)
      for (int t = sf[l] + ln + ALIGN_WAVE; t <= sl[l]; t += ALIGN_WAVE)
        key[k] = max(key[k], align_peak_key(align_quant(p.align[((size_t)l * Tp + t) * p.B + b]), t));
      const int best = __builtin_amdgcn_readlane(wave_scan_max(key[k]), ALIGN_WAVE - 1);
      if (ln == 0) op[l] = align_peak_frame(best);
    }
  }
}

hipError_t launch_align_path(const float* align, const int32_t* enc_len, const int32_t* tgt_len, int B, int Tp, int L,
                             int group, int32_t* first, int32_t* last, int32_t* peak, int32_t* path_score,
                             int32_t* err, hipStream_t s) {
  const AlignPlan pl = align_plan(B, L, Tp, group);
  if (!pl.group) return hipErrorInvalidValue;
  int gshift = 0;
  while ((1 << gshift) < pl.group) ++gshift;
  const AlignArgs p{align, enc_len, tgt_len, B, Tp, L, gshift, pl.chunks, pl.dw, pl.qstride,
                    first, last, peak, path_score, err};
  if (pl.raise_lds) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(align_path_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(align_path_kernel, dim3(pl.grid), dim3(ALIGN_WAVE * pl.group), pl.lds_bytes, s, p);
  return hipGetLastError();
}

}  // namespace casr
