// Relative-entropy pruning on the device (include/casr.h casr_lm_prune): the stage bodies of
// lm_prune_plan.h, the text the host entry runs too.  Where the host loops 64 lanes over a context's
// successors and then the tree of lmp_tree, a wave holds one partial per lane and adds them in the same
// order with shuffles, so every float64 sum has the host's association.  The only atomics are integer
// adds (the removed counts, the compaction cursors) and a flag; protect flags are plain stores of 1.
//
// Stages, each its own launch per order:
//   linearise  one work item per slot: P, B, Bn = 1, delta = NaN, keep = 1; an n-gram that takes no part
//              protects its prefix.
//   decide     orders N..2, one wave per context (LM ids at order 2, the slots of the context table
//              above): lane l takes successors l, l + 64, ..: slot, p, q, the partial sums; the wave's
//              sums give num and den; a and ph are the context's; then each lane decides its n-grams.
//   renew      orders 2..N, one wave per context that is a kept n-gram: the sums over its kept
//              successors in the pruned model, B' by lane 0.
//   compact    occupied slots of orders 2..N to dense arrays, one cursor add per wave.
// The longest list is one word's successors (at most V + 3), walked by one wave.
#include "casr_internal.h"

namespace casr {

namespace {

constexpr int LMP_THREADS = 256;
constexpr int LMP_WAVES = LMP_THREADS / 64;
constexpr int LMP_MAX_GRID = 8192;

// lmp_tree over the wave's 64 partials; every lane returns s_0
__device__ __forceinline__ double lmp_wave_sum(double s) {
#pragma clang fp contract(off)
  for (int d = 32; d >= 1; d >>= 1) s = s + __shfl_down(s, d);
  return __shfl(s, 0);
}

__global__ __launch_bounds__(LMP_THREADS) void lmp_linearise_kernel(LmpView v, int n, uint32_t slots) {
  for (uint64_t s = (uint64_t)blockIdx.x * LMP_THREADS + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * LMP_THREADS)
    lmp_linearise(v, n, (uint32_t)s);
}

__global__ __launch_bounds__(LMP_THREADS) void lmp_decide_kernel(LmpView v, int n, uint32_t items, double tau,
                                                                 LmpTotals* tot) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  bool bad = false;
  uint32_t removed = 0;
  for (uint64_t item = (uint64_t)blockIdx.x * LMP_WAVES + wave; item < items; item += (uint64_t)gridDim.x * LMP_WAVES) {
    LmpCtx x;
    if (!lmp_ctx_prepare(v, n, (uint32_t)item, &x)) continue;  // (the same for the whole wave)
    double sp, sq;
    lmp_decide_sums(v, x, lane, &sp, &sq, &bad);
    const double num = 1.0 - lmp_wave_sum(sp), den = 1.0 - lmp_wave_sum(sq);
    const double a = x.hslot >= 0 ? v.B[n - 2][x.hslot] : 1.0;
    const double ph = lmp_ph(v, x.c, n - 1);
    const bool any = lmp_decide_lane(v, x, lane, a, ph, num, den, tau, &removed);
    if (any && n >= 3 && x.hslot >= 0) v.protect[n - 2][x.hslot] = 1;
  }
  for (int d = 32; d >= 1; d >>= 1) removed += __shfl_down(removed, d);
  if (lane == 0 && removed) atomicAdd(&tot->removed[n - 1], removed);
  if (bad) atomicOr(&tot->flags, LMP_FLAG_INCONSISTENT);
}

__global__ __launch_bounds__(LMP_THREADS) void lmp_renew_kernel(LmpView v, int n, uint32_t items) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (uint64_t item = (uint64_t)blockIdx.x * LMP_WAVES + wave; item < items; item += (uint64_t)gridDim.x * LMP_WAVES) {
    LmpCtx x;
    if (!lmp_ctx_prepare(v, n, (uint32_t)item, &x) || !lmp_renew_wanted(v, x)) continue;
    double sp, sq;
    lmp_renew_sums(v, x, lane, &sp, &sq);
    const double a = lmp_wave_sum(sp), b = lmp_wave_sum(sq);
    if (lane == 0) v.Bn[n - 2][x.hslot] = lmp_backoff(a, b);
  }
}

__global__ __launch_bounds__(LMP_THREADS) void lmp_compact_kernel(LmpView v, int n, uint32_t cap, LmpDense o,
                                                                  LmpTotals* tot) {
  const int lane = threadIdx.x & 63;
  for (uint64_t base = (uint64_t)blockIdx.x * LMP_THREADS; base < cap; base += (uint64_t)gridDim.x * LMP_THREADS) {
    const uint64_t s = base + threadIdx.x;
    NgramEntry e{0, 0.f, 0.f};
    if (s < cap) e = v.m.tab[n - 2][s];
    const bool occ = e.key != 0;
    const unsigned long long m = __ballot(occ);
    if (!m) continue;
    const int first = __ffsll(m) - 1;
    uint32_t at = 0;
    if (lane == first) at = atomicAdd(&tot->out[n - 1], (uint32_t)__popcll(m));
    at = __shfl(at, first) + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (occ && at < o.room) {  // (room = the n-grams casr_lm_create was given: exactly the occupied slots)
      o.key[at] = e.key;
      o.prob[at] = e.prob;
      o.backoff[at] = e.backoff;
      o.bn[at] = v.Bn[n - 1][s];
      o.delta[at] = v.delta[n - 1][s];
      o.kept[at] = v.keep[n - 1][s];
    }
  }
}

int grid_threads(uint64_t items) { return (int)std::max<uint64_t>(1, std::min<uint64_t>((items + LMP_THREADS - 1) / LMP_THREADS, LMP_MAX_GRID)); }
int grid_waves(uint64_t items) { return (int)std::max<uint64_t>(1, std::min<uint64_t>((items + LMP_WAVES - 1) / LMP_WAVES, LMP_MAX_GRID)); }

}  // namespace

#define LMP_TRY(expr)               \
  do {                              \
    e = (expr);                     \
    if (e != hipSuccess) goto done; \
  } while (0)

hipError_t run_lm_prune(const NgramTables& host, const NgramView& dm, const NgramSuccView& ds, const LmpDims& d,
                        double theta, void* ws, hipStream_t s, LmpResult* out, uint32_t* flags) {
  const int N = d.order;
  LmpView v{};
  v.m = dm;
  v.s = ds;
  LmpDense dense[NGRAM_MAX_ORDER];
  LmpTotals* dtot = nullptr;
  lmp_carve(ws, d, &v, dense, &dtot);
  LmpTotals tot{};
  LmpResult r;
  std::vector<double> bn1((size_t)d.V + 3, 1.0);
  hipEvent_t ev[6] = {};
  hipError_t e = hipSuccess;
  *flags = 0;
  r.order = N;
  r.V = d.V;
  r.theta = theta;
  r.tau = lmp_log(1.0 + theta);
  for (hipEvent_t& x : ev) LMP_TRY(hipEventCreate(&x));
  LMP_TRY(hipMemsetAsync(ws, 0, (size_t)lmp_zeroed_bytes(d), s));
  LMP_TRY(hipEventRecord(ev[0], s));
  for (int n = 1; n <= N; ++n) {
    const uint32_t slots = lmp_slots(d, n);
    hipLaunchKernelGGL(lmp_linearise_kernel, dim3(grid_threads(slots)), dim3(LMP_THREADS), 0, s, v, n, slots);
    LMP_TRY(hipGetLastError());
  }
  LMP_TRY(hipEventRecord(ev[1], s));
  for (int n = N; n >= 2; --n) {
    const uint32_t items = lmp_ctx_items(v, n);
    hipLaunchKernelGGL(lmp_decide_kernel, dim3(grid_waves(items)), dim3(LMP_THREADS), 0, s, v, n, items, r.tau, dtot);
    LMP_TRY(hipGetLastError());
  }
  LMP_TRY(hipMemcpyAsync(&tot, dtot, sizeof tot, hipMemcpyDeviceToHost, s));
  LMP_TRY(hipEventRecord(ev[2], s));
  LMP_TRY(hipStreamSynchronize(s));
  *flags = tot.flags;
  if (tot.flags) goto done;
  for (int n = 2; n <= N; ++n) r.removed_any = r.removed_any || tot.removed[n - 1] != 0;
  if (r.removed_any)
    for (int n = 2; n <= N; ++n) {
      const uint32_t items = lmp_ctx_items(v, n);
      hipLaunchKernelGGL(lmp_renew_kernel, dim3(grid_waves(items)), dim3(LMP_THREADS), 0, s, v, n, items);
      LMP_TRY(hipGetLastError());
    }
  LMP_TRY(hipEventRecord(ev[3], s));
  for (int n = 2; n <= N; ++n) {
    hipLaunchKernelGGL(lmp_compact_kernel, dim3(grid_threads(d.cap[n - 2])), dim3(LMP_THREADS), 0, s, v, n, d.cap[n - 2],
                       dense[n - 1], dtot);
    LMP_TRY(hipGetLastError());
  }
  LMP_TRY(hipMemcpyAsync(&tot, dtot, sizeof tot, hipMemcpyDeviceToHost, s));
  LMP_TRY(hipEventRecord(ev[4], s));
  LMP_TRY(hipMemcpyAsync(bn1.data(), v.Bn[0], 8 * bn1.size(), hipMemcpyDeviceToHost, s));
  for (int n = 2; n <= N; ++n) {
    const size_t c = (size_t)d.count[n - 1];
    r.key[n - 1].resize(c);
    r.prob[n - 1].resize(c);
    r.backoff[n - 1].resize(c);
    r.bn[n - 1].resize(c);
    r.delta[n - 1].resize(c);
    r.kept[n - 1].resize(c);
    if (!c) continue;
    const LmpDense& o = dense[n - 1];
    LMP_TRY(hipMemcpyAsync(r.key[n - 1].data(), o.key, 8 * c, hipMemcpyDeviceToHost, s));
    LMP_TRY(hipMemcpyAsync(r.prob[n - 1].data(), o.prob, 4 * c, hipMemcpyDeviceToHost, s));
    LMP_TRY(hipMemcpyAsync(r.backoff[n - 1].data(), o.backoff, 4 * c, hipMemcpyDeviceToHost, s));
    LMP_TRY(hipMemcpyAsync(r.bn[n - 1].data(), o.bn, 8 * c, hipMemcpyDeviceToHost, s));
    LMP_TRY(hipMemcpyAsync(r.delta[n - 1].data(), o.delta, 8 * c, hipMemcpyDeviceToHost, s));
    LMP_TRY(hipMemcpyAsync(r.kept[n - 1].data(), o.kept, c, hipMemcpyDeviceToHost, s));
  }
  LMP_TRY(hipEventRecord(ev[5], s));
  LMP_TRY(hipStreamSynchronize(s));
  for (int n = 2; n <= N; ++n)
    if ((int64_t)tot.out[n - 1] != d.count[n - 1]) *flags |= LMP_FLAG_INCONSISTENT;
  if (*flags) goto done;
  lmp_result_unigrams(host, d, bn1.data(), &r);
  lmp_finish(&r);
  for (int i = 0; i < 5; ++i) {
    float ms = 0.f;
    LMP_TRY(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
    r.stage_ms[i] = ms;
  }
  {
    float ms = 0.f;
    LMP_TRY(hipEventElapsedTime(&ms, ev[0], ev[5]));
    r.stage_ms[7] = ms;
  }
  *out = std::move(r);
done:
  if (e != hipSuccess) (void)hipStreamSynchronize(s);
  for (hipEvent_t x : ev)
    if (x) (void)hipEventDestroy(x);
  return e;
}

}  // namespace casr
