// casr_segment and casr_gather_segments (include/casr.h): cut the log-mel of long recordings at their
// pauses, and copy the segments into a padded batch.  The work is time-parallel over a few very long
// rows (B small, T up to hours of frames), the opposite shape of every other kernel here.
//   segment_level_kernel   stage (a).  Grid ceil(T / 256) x B, 16 lanes per frame: lane j adds the bins
//       j, 16 + j, .. of its frame in ascending order (a group's 16 lanes read 64 B pieces of the row,
//       a workgroup's 16 groups 16 consecutive rows), then the halving tree as an xor butterfly over
//       the group (f32 adds commute, so every lane holds the tree's bits).  q goes to the handle's
//       uint16 workspace [B][T]; the histogram is kept per workgroup in LDS and added to [B][512] words
//       with integer atomics, so it does not depend on scheduling.
//   segment_decide_kernel  stages (b) to (e), one workgroup per recording.  The threshold comes from
//       the histogram; then q streams through in tiles of 2,048 frames (the next tile's loads in flight
//       under the current tile's work): ballots give the tile's A0 as 32 mask words, every frame flags whether it heads or ends an active run (clipped to the tile),
//       and a prefix over the words' ballot counts compacts the runs into an LDS list.  Wave 0 walks the
//       list through segment_plan.h's seg_run, whose state carries a run, an island and a segment
//       across tiles: a run that crosses a tile boundary arrives as two touching runs and is joined
//       there.  The split's arg-minimum is a strided scan of the window by the wave's 64 lanes and an
//       xor-butterfly minimum of 64-bit keys (cost, then larger c): a total order, so the tree does not
//       matter.  The walk is the serial part: O(runs) steps of a few instructions.
//   gather_segments_kernel a segment's rows are contiguous in fbank and in out: one flat copy of
//       float4 (a row of 80 floats is 20 of them), zeros past the length.
// Every data-dependent index (frames[b], seg_src, seg_start, seg_len, a cut) is clamped and reported as
// guard bit 64, never followed.
#include "casr_common.h"
#include "casr_internal.h"
#include "segment_plan.h"

namespace casr {

namespace {

constexpr int SEG_THREADS = 256;
constexpr int SEG_FT = 256;                // frames per workgroup of the level kernel
constexpr int SEG_DT = 2048;               // frames per tile of the decision kernel
constexpr int SEG_DW = SEG_DT / 64;        // its mask words
constexpr int SEG_DI = SEG_DT / SEG_THREADS;  // frames per thread and tile
constexpr int SEG_RUNS = SEG_DT / 2;       // the most active runs a tile can hold

__device__ __forceinline__ int clamp_frames(int n, int T, bool* bad) {
  *bad = n < 0 || n > T;
  return n < 0 ? 0 : (n > T ? T : n);
}

__global__ __launch_bounds__(SEG_THREADS) void segment_level_kernel(SegmentArgs a) {
  __shared__ uint32_t h[SEG_BINS];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int t0 = blockIdx.x * SEG_FT;
  bool bad;
  const int n = clamp_frames(a.frames[b], a.T, &bad);
  if (blockIdx.x == 0 && tid == 0 && bad) atomicOr(a.err, CASR_DEV_BAD_AUDIO);
  if (t0 >= n) return;  // the whole workgroup: rows past frames[b] are never read
  for (int i = tid; i < SEG_BINS; i += SEG_THREADS) h[i] = 0u;
  __syncthreads();
  const int j = tid & (SEG_LANES - 1), g = tid / SEG_LANES;
  const float inv = 1.0f / (float)a.n_mels;
  const float* __restrict__ fb = a.fbank + (size_t)b * a.T * a.n_mels;
  uint16_t* __restrict__ q = a.q + (size_t)b * a.T;
  for (int i = 0; i < SEG_FT; i += SEG_THREADS / SEG_LANES) {
    const int t = t0 + i + g;
    const bool ok = t < n;
    float p = 0.f;
    if (ok) {
      const float* __restrict__ row = fb + (size_t)t * a.n_mels + j;
      p = row[0];
      for (int k = SEG_LANES; k < a.n_mels; k += SEG_LANES) p = __fadd_rn(p, row[k]);
    }
    // p_j += p_{j+8}, then 4, 2, 1: lane 0's chain is the tree's, and every lane's has its bits
    p = __fadd_rn(p, __shfl_xor(p, 8));
    p = __fadd_rn(p, __shfl_xor(p, 4));
    p = __fadd_rn(p, __shfl_xor(p, 2));
    p = __fadd_rn(p, __shfl_xor(p, 1));
    if (ok && j == 0) {
      const int bin = seg_level_bin(p, inv);
      q[t] = (uint16_t)bin;
      atomicAdd(&h[bin], 1u);
    }
  }
  __syncthreads();
  uint32_t* __restrict__ gh = a.hist + (size_t)b * SEG_BINS;
  for (int i = tid; i < SEG_BINS; i += SEG_THREADS)
    if (h[i]) atomicAdd(&gh[i], h[i]);
}

// the walking wave's Io: every lane runs the walk with the same state; lane 0 writes
struct SegDevIo {
  const uint16_t* __restrict__ q;
  int32_t* start;
  int32_t* len;
  int s_max, lane;
  __device__ uint64_t best_cut(int32_t lo, int32_t hi) const {
    unsigned long long best = ~0ull;
    // (measured: a branch-free form with 16 clamped candidates per lane in flight was 8 to 11 % slower
    // per call than this loop; a default window of 600 frames is 10 steps)
#pragma unroll 4
    for (int64_t c = (int64_t)lo + lane; c <= hi; c += 64) {
      const unsigned long long k = seg_cut_key((uint32_t)q[c - 1] + q[c], (int32_t)c);
      best = k < best ? k : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long k = __shfl_xor(best, o);
      best = k < best ? k : best;
    }
    return best;
  }
  __device__ void emit(int32_t i, int32_t s, int32_t l) const {
    if (lane == 0 && i < s_max) {
      start[i] = s;
      len[i] = l;
    }
  }
};

__global__ __launch_bounds__(SEG_THREADS) void segment_decide_kernel(SegmentArgs a) {
  __shared__ uint32_t hist[SEG_BINS];
  __shared__ unsigned long long mask[SEG_DW];
  __shared__ uint32_t cnt[SEG_DW];  // per mask word: run ends << 16 | run heads (at most 32 each)
  __shared__ int32_t rs[SEG_RUNS], re[SEG_RUNS];
  __shared__ int32_t s_thr;
  constexpr int WPI = SEG_THREADS / 64;  // mask words per step i: word W = i WPI + wave
  const int tid = threadIdx.x, b = blockIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  bool bad;
  const int n = clamp_frames(a.frames[b], a.T, &bad);
  const uint16_t* __restrict__ q = a.q + (size_t)b * a.T;
  // the first tile's levels are in flight while the threshold is found
  uint16_t qv[SEG_DI];
#pragma unroll
  for (int i = 0; i < SEG_DI; ++i) {
    const int t = i * SEG_THREADS + tid;
    qv[i] = t < n ? q[t] : (uint16_t)0;
  }
  for (int i = tid; i < SEG_BINS; i += SEG_THREADS) hist[i] = a.hist[(size_t)b * SEG_BINS + i];
  __syncthreads();
  if (tid == 0) s_thr = seg_threshold(hist, n, a.p);
  __syncthreads();
  const int thr = s_thr;
  if (tid == 0 && a.thr) a.thr[b] = thr;
  SegWalk w;  // wave 0's
  seg_walk_init(w, n);
  SegDevIo io{q, a.seg_start + (size_t)b * a.s_max, a.seg_len + (size_t)b * a.s_max, a.s_max, lane};
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int t0 = 0; t0 < n; t0 += SEG_DT) {  // n is the workgroup's: every barrier below is reached by all
    unsigned long long mine[SEG_DI];
#pragma unroll
    for (int i = 0; i < SEG_DI; ++i) {
      const int t = t0 + i * SEG_THREADS + tid;  // frame `lane` of mask word i WPI + wv
      const bool act = t < n && (int)qv[i] >= thr;
      mine[i] = __ballot(act);
      if (lane == 0) mask[i * WPI + wv] = mine[i];
    }
    // the next tile's levels: in flight during this tile's barriers and walk
#pragma unroll
    for (int i = 0; i < SEG_DI; ++i) {
      const int t = t0 + SEG_DT + i * SEG_THREADS + tid;
      qv[i] = t < n ? q[t] : (uint16_t)0;
    }
    __syncthreads();
    // a frame heads (ends) a run when it is active and its predecessor (successor) in the tile is not;
    // frames past n are inactive, so a run also ends at n
    unsigned long long hb[SEG_DI], tb[SEG_DI];
#pragma unroll
    for (int i = 0; i < SEG_DI; ++i) {
      const int W = i * WPI + wv;
      const bool act = (mine[i] >> lane) & 1ull;
      const bool prev = lane > 0 ? (mine[i] >> (lane - 1)) & 1ull : (W > 0 ? mask[W - 1] >> 63 : 0ull);
      const bool next = lane < 63 ? (mine[i] >> (lane + 1)) & 1ull : (W < SEG_DW - 1 ? mask[W + 1] & 1ull : 0ull);
      hb[i] = __ballot(act && !prev);
      tb[i] = __ballot(act && !next);
      if (lane == 0) cnt[W] = (uint32_t)__popcll(hb[i]) | ((uint32_t)__popcll(tb[i]) << 16);
    }
    __syncthreads();
    // the k-th head and the k-th end of the tile are one run's: compact both by their rank.  `pre` is
    // the packed count of the words before W; from one step to the next it takes the WPI words between
    uint32_t pre = 0;
    for (int u = 0; u < wv; ++u) pre += cnt[u];
#pragma unroll
    for (int i = 0; i < SEG_DI; ++i) {
      const int W = i * WPI + wv;
      const int t = t0 + W * 64 + lane;
      if ((hb[i] >> lane) & 1ull) {
        const int k = (int)(pre & 0xffffu) + __popcll(hb[i] & below);
        if (k < SEG_RUNS) rs[k] = t;
      }
      if ((tb[i] >> lane) & 1ull) {
        const int k = (int)(pre >> 16) + __popcll(tb[i] & below);
        if (k < SEG_RUNS) re[k] = t + 1;
      }
      if (i + 1 < SEG_DI) {
#pragma unroll
        for (int u = 0; u < WPI; ++u) pre += cnt[W + u];  // W + u <= (SEG_DI - 2) WPI + 2 WPI - 2 < SEG_DW
      }
    }
    __syncthreads();
    if (wv == 0) {
      uint32_t all = 0;
#pragma unroll
      for (int u = 0; u < SEG_DW; ++u) all += cnt[u];
      int runs = (int)(all & 0xffffu);
      runs = runs < SEG_RUNS ? runs : SEG_RUNS;
      for (int k = 0; k < runs; ++k) seg_run(w, a.p, io, rs[k], re[k]);
    }
    __syncthreads();  // the masks and the run list are the next tile's
  }
  if (wv == 0) {
    seg_finish(w, a.p, io);
    if (lane == 0) a.n_seg[b] = w.count;
  }
}

__global__ __launch_bounds__(256) void gather_segments_kernel(const float* __restrict__ fbank, int B, int T, int n_mels,
                                                              const int32_t* __restrict__ seg_src,
                                                              const int32_t* __restrict__ seg_start,
                                                              const int32_t* __restrict__ seg_len, int t_seg,
                                                              float* __restrict__ out, int32_t* __restrict__ frames_out,
                                                              int32_t* err) {
  const int s = blockIdx.x;
  int src = seg_src[s], st = seg_start[s], ln = seg_len[s];
  const bool bad = src < 0 || src >= B || st < 0 || st > T || ln < 0 || ln > t_seg || (int64_t)st + ln > T;
  src = src < 0 ? 0 : (src >= B ? B - 1 : src);
  st = st < 0 ? 0 : (st > T ? T : st);
  ln = ln < 0 ? 0 : ln;
  ln = ln > T - st ? T - st : ln;
  ln = ln > t_seg ? t_seg : ln;
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    frames_out[s] = ln;
    if (bad) atomicOr(err, CASR_DEV_BAD_AUDIO);
  }
  const int r4 = n_mels / 4;  // float4 per row
  const float4* __restrict__ in = reinterpret_cast<const float4*>(fbank + ((size_t)src * T + st) * n_mels);
  float4* __restrict__ o = reinterpret_cast<float4*>(out + (size_t)s * t_seg * n_mels);
  const size_t total = (size_t)t_seg * r4, valid = (size_t)ln * r4;
  for (size_t i = (size_t)blockIdx.y * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.y * blockDim.x)
    o[i] = i < valid ? in[i] : make_float4(0.f, 0.f, 0.f, 0.f);
}

}  // namespace

hipError_t launch_segment(const SegmentArgs& a, hipStream_t s) {
  hipError_t e = fill_u32(a.hist, 0u, (size_t)a.B * SEG_BINS, s);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)((a.T + SEG_FT - 1) / SEG_FT), (unsigned)a.B);
  hipLaunchKernelGGL(segment_level_kernel, grid, dim3(SEG_THREADS), 0, s, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(segment_decide_kernel, dim3((unsigned)a.B), dim3(SEG_THREADS), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_gather_segments(const float* fbank, int B, int T, int n_mels, const int32_t* seg_src,
                                  const int32_t* seg_start, const int32_t* seg_len, int S, int t_seg, float* out,
                                  int32_t* frames_out, int32_t* err, hipStream_t s) {
  const size_t total = (size_t)t_seg * (n_mels / 4);
  const unsigned ny = (unsigned)std::min<size_t>((total + 1023) / 1024, 64);
  hipLaunchKernelGGL(gather_segments_kernel, dim3((unsigned)S, ny), dim3(256), 0, s, fbank, B, T, n_mels, seg_src,
                     seg_start, seg_len, t_seg, out, frames_out, err);
  return hipGetLastError();
}

}  // namespace casr
