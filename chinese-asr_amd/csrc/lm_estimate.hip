// Kneser-Ney estimation on the device (include/casr.h casr_lm_estimate): the stage bodies of
// lm_estimate_plan.h, the text the host entry runs too, with atomic operations in place of the plain
// ones.  Everything the kernels accumulate is an integer (counts, extensions, S, N_k, t_{n,k}), so the
// order of the atomics does not show in the result; the float64 values are computed once per slot from
// those integers by est_prob, contraction off.
//
// Stages, each its own launch (per order where an order reads the one below):
//   count     one wave per sentence, one lane per position; every window's key goes into its order's
//             table (64-bit CAS on the key, integer add on the count, probes bounded by the capacity).
//             Equal keys are combined first in a workgroup-wide LDS table of EST_LDS_SLOTS slots that
//             lives for the workgroup's whole share of the corpus and is flushed once: the hot keys
//             (<s>-initial n-grams, frequent characters, </s>) arrive early, stay, and cost one
//             global atomic per workgroup instead of one per occurrence.  A key that finds no LDS slot
//             within EST_LDS_PROBES probes goes to the global table at once.
//   extend    one work item per slot of order n + 1: +1 on its suffix in order n.
//   stats     one per slot: a and the N_k increment onto its prefix; occupancy, t_{n,k} and the empty
//             context's S and N_k through wave ballots and LDS partials, one global atomic per
//             workgroup and counter.
//   prob      orders ascending, one per slot: the context for S and gamma, the suffix for p_{n-1}.
//   compact   occupied slots to dense arrays, one cursor add per wave.
#include "casr_internal.h"

namespace casr {

namespace {

constexpr int EST_THREADS = 256;
constexpr int EST_LDS_SLOTS = 1024;
constexpr int EST_LDS_PROBES = 4;
constexpr int EST_MAX_GRID = 8192;
constexpr int EST_COUNT_GRID = 2048;

struct EstDevOps {
  static __host__ __device__ uint64_t load_key(const uint64_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
  static __host__ __device__ uint64_t cas_key(uint64_t* p, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicCAS(reinterpret_cast<unsigned long long*>(p), 0ull, (unsigned long long)v);
#else
    return EstHostOps::cas_key(p, v);
#endif
  }
  static __host__ __device__ void add(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
  }
};

__device__ __forceinline__ bool est_global_insert(const EstView& v, uint64_t key, uint32_t add) {
  const int m = est_key_order(key);
  return est_insert<EstDevOps>(v.slot[m - 1], v.mask[m - 1], key, add);
}

__global__ __launch_bounds__(EST_THREADS) void est_count_kernel(EstView v, const int32_t* __restrict__ tokens,
                                                                const int64_t* __restrict__ offsets, int64_t n_sent,
                                                                int64_t total, int combine, EstTotals* tot,
                                                                int32_t* err) {
  __shared__ unsigned long long lkey[EST_LDS_SLOTS];
  __shared__ uint32_t lcnt[EST_LDS_SLOTS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < EST_LDS_SLOTS; i += EST_THREADS) {
    lkey[i] = 0ull;
    lcnt[i] = 0u;
  }
  __syncthreads();
  bool bad = false, full = false;
  if (blockIdx.x == 0 && tid == 0) full |= !est_global_insert(v, (uint64_t)(v.V + 1), (uint32_t)n_sent);  // <s>
  constexpr int WAVES = EST_THREADS / 64;
  for (int64_t i = (int64_t)blockIdx.x * WAVES + wave; i < n_sent; i += (int64_t)gridDim.x * WAVES) {
    int64_t start, len;
    est_sentence_range(offsets[i], offsets[i + 1], total, &start, &len, &bad);
    const int32_t* tok = tokens + start;
    for (int64_t j = 1 + lane; j <= len + 1; j += 64)
      est_windows(tok, len, j, v.order, v.V, &bad, [&](uint64_t key) {
        if (combine) {
          uint32_t s = (uint32_t)(ngram_mix(key) >> 40) & (EST_LDS_SLOTS - 1);
          for (int q = 0; q < EST_LDS_PROBES; ++q) {
            const unsigned long long old = atomicCAS(&lkey[s], 0ull, (unsigned long long)key);
            if (old == 0ull || old == key) {
              atomicAdd(&lcnt[s], 1u);
              return;
            }
            s = (s + 1) & (EST_LDS_SLOTS - 1);
          }
        }
        full |= !est_global_insert(v, key, 1u);
      });
  }
  __syncthreads();
  if (combine)
    for (int s = tid; s < EST_LDS_SLOTS; s += EST_THREADS)
      if (lkey[s] != 0ull) full |= !est_global_insert(v, lkey[s], lcnt[s]);
  if (bad) atomicOr(err, CASR_DEV_BAD_TOKEN);
  if (full) atomicOr(&tot->flags, (uint32_t)EST_FLAG_FULL);
}

__global__ __launch_bounds__(EST_THREADS) void est_extend_kernel(EstView v, int n, EstTotals* tot) {
  const uint32_t cap = v.mask[n - 1] + 1;
  bool miss = false;
  for (uint64_t s = (uint64_t)blockIdx.x * EST_THREADS + threadIdx.x; s < cap; s += (uint64_t)gridDim.x * EST_THREADS)
    miss |= !est_extend<EstDevOps>(v, n, (uint32_t)s);
  if (miss) atomicOr(&tot->flags, (uint32_t)EST_FLAG_FULL);
}

// sh: [0] occupied, [1..4] t_{n,1..4}, [5..8] the empty context (order 1), [9] <unk> seen (order 1)
__global__ __launch_bounds__(EST_THREADS) void est_stats_kernel(EstView v, int n, EstTotals* tot) {
  __shared__ uint32_t sh[10];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < 10) sh[tid] = 0u;
  __syncthreads();
  const uint32_t cap = v.mask[n - 1] + 1;
  bool miss = false;
  for (uint64_t base = (uint64_t)blockIdx.x * EST_THREADS; base < cap; base += (uint64_t)gridDim.x * EST_THREADS) {
    const uint64_t s = base + tid;
    EstSlot e{0, 0, 0};
    if (s < cap) e = v.slot[n - 1][s];
    const bool occ = e.key != 0, pred = est_predicted(v, n, e);
    const uint32_t a = pred ? est_adjusted(v, n, e) : 0u;
    const unsigned long long mo = __ballot(occ);
    unsigned long long mk[4];
    for (int k = 1; k <= 4; ++k) mk[k - 1] = __ballot(pred && a == (uint32_t)k);
    if (lane == 0) {
      if (mo) atomicAdd(&sh[0], (uint32_t)__popcll(mo));
      for (int k = 0; k < 4; ++k)
        if (mk[k]) atomicAdd(&sh[1 + k], (uint32_t)__popcll(mk[k]));
    }
    if (pred) {
      if (n == 1) {
        atomicAdd(&sh[5], a);
        atomicAdd(&sh[5 + (a < 3 ? a : 3)], 1u);
      } else {
        miss |= !est_ctx_add<EstDevOps>(v, n, (uint32_t)s);
      }
    }
    if (n == 1 && e.key == (uint64_t)(v.V + 3)) sh[9] = 1u;
  }
  __syncthreads();
  if (tid == 0 && sh[0]) atomicAdd(&tot->occupied[n - 1], sh[0]);
  if (tid >= 1 && tid <= 4 && sh[tid]) atomicAdd(&tot->t[n - 1][tid - 1], sh[tid]);
  if (tid >= 5 && tid <= 8 && sh[tid]) atomicAdd(&tot->ctx0[tid - 5], sh[tid]);
  if (tid == 9 && sh[9]) atomicOr(&tot->unk_seen, 1u);
  if (miss) atomicOr(&tot->flags, (uint32_t)EST_FLAG_FULL);
}

__global__ __launch_bounds__(EST_THREADS) void est_prob_kernel(EstView v, EstDiscounts d, int n, EstTotals* tot) {
  const uint32_t cap = v.mask[n - 1] + 1;
  bool miss = false;
  for (uint64_t s = (uint64_t)blockIdx.x * EST_THREADS + threadIdx.x; s < cap; s += (uint64_t)gridDim.x * EST_THREADS)
    miss |= !est_prob(v, d, n, (uint32_t)s);
  if (miss) atomicOr(&tot->flags, (uint32_t)EST_FLAG_FULL);
}

struct EstDense {
  uint64_t* key;
  uint32_t *count, *adjusted;
  double *p, *gamma;
  uint32_t room;
};

__global__ __launch_bounds__(EST_THREADS) void est_compact_kernel(EstView v, int n, EstDense o, EstTotals* tot) {
  const int lane = threadIdx.x & 63;
  const uint32_t cap = v.mask[n - 1] + 1;
  for (uint64_t base = (uint64_t)blockIdx.x * EST_THREADS; base < cap; base += (uint64_t)gridDim.x * EST_THREADS) {
    const uint64_t s = base + threadIdx.x;
    EstSlot e{0, 0, 0};
    if (s < cap) e = v.slot[n - 1][s];
    const bool occ = e.key != 0;
    const unsigned long long m = __ballot(occ);
    if (!m) continue;
    const int first = __ffsll(m) - 1;
    uint32_t at = 0;
    if (lane == first) at = atomicAdd(&tot->out[n - 1], (uint32_t)__popcll(m));
    at = __shfl(at, first) + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (occ && at < o.room) {  // (room = the occupancy the stats stage counted: always enough)
      o.key[at] = e.key;
      o.count[at] = e.count;
      o.adjusted[at] = est_adjusted(v, n, e);
      o.p[at] = v.p[n - 1][s];
      o.gamma[at] = n < v.order ? v.gamma[n - 1][s] : 0.0;
    }
  }
}

int grid_for(uint64_t items) { return (int)std::min<uint64_t>((items + EST_THREADS - 1) / EST_THREADS, EST_MAX_GRID); }

}  // namespace

#define EST_TRY(expr)                 \
  do {                                \
    e = (expr);                       \
    if (e != hipSuccess) goto done;   \
  } while (0)

hipError_t run_lm_estimate(int order, int V, const int32_t* tokens, const int64_t* offsets, int64_t n, int64_t total,
                           void* ws, int combine, int32_t* err, hipStream_t s, EstResult* out, uint32_t* flags) {
  const int64_t P = total + n;
  const size_t bytes = (size_t)est_workspace_bytes(order, P);
  EstTotals* dtot = nullptr;
  const EstView v = est_carve(ws, order, V, P, &dtot);
  EstTotals tot{};
  EstDiscounts d{};
  int32_t fallback[NGRAM_MAX_ORDER] = {};
  hipEvent_t ev[7] = {};
  void* dense = nullptr;
  EstResult r;
  hipError_t e = hipSuccess;
  *flags = 0;
  for (hipEvent_t& x : ev) EST_TRY(hipEventCreate(&x));
  EST_TRY(hipMemsetAsync(ws, 0, bytes, s));
  EST_TRY(hipEventRecord(ev[0], s));
  hipLaunchKernelGGL(est_count_kernel, dim3((unsigned)std::min<int64_t>((n + 3) / 4, EST_COUNT_GRID)), dim3(EST_THREADS), 0,
                     s, v, tokens, offsets, n, total, combine, dtot, err);
  EST_TRY(hipGetLastError());
  EST_TRY(hipEventRecord(ev[1], s));
  for (int m = 2; m <= order; ++m) {
    hipLaunchKernelGGL(est_extend_kernel, dim3(grid_for((uint64_t)v.mask[m - 1] + 1)), dim3(EST_THREADS), 0, s, v, m, dtot);
    EST_TRY(hipGetLastError());
  }
  EST_TRY(hipEventRecord(ev[2], s));
  for (int m = 1; m <= order; ++m) {
    hipLaunchKernelGGL(est_stats_kernel, dim3(grid_for((uint64_t)v.mask[m - 1] + 1)), dim3(EST_THREADS), 0, s, v, m, dtot);
    EST_TRY(hipGetLastError());
  }
  EST_TRY(hipMemcpyAsync(&tot, dtot, sizeof tot, hipMemcpyDeviceToHost, s));
  EST_TRY(hipStreamSynchronize(s));
  EST_TRY(hipEventRecord(ev[3], s));
  *flags = tot.flags;
  if (tot.flags & EST_FLAG_FULL) goto done;
  est_plan_discounts(v, tot, &d, fallback);
  for (int m = 1; m <= order; ++m) {
    hipLaunchKernelGGL(est_prob_kernel, dim3(grid_for((uint64_t)v.mask[m - 1] + 1)), dim3(EST_THREADS), 0, s, v, d, m, dtot);
    EST_TRY(hipGetLastError());
  }
  EST_TRY(hipEventRecord(ev[4], s));
  r.order = order;
  r.V = V;
  r.positions = P;
  {
    // dense arrays of every order in one allocation: key, p, gamma (8 bytes each), count, adjusted (4 each)
    size_t room = 0;
    for (int m = 0; m < order; ++m) room += ((size_t)tot.occupied[m] + 32) * 32;
    EST_TRY(hipMalloc(&dense, room));
    char* q = static_cast<char*>(dense);
    EstDense o[NGRAM_MAX_ORDER];
    for (int m = 0; m < order; ++m) {
      const size_t c = ((size_t)tot.occupied[m] + 31) / 32 * 32;
      o[m].room = tot.occupied[m];
      o[m].key = reinterpret_cast<uint64_t*>(q);
      o[m].p = reinterpret_cast<double*>(q + 8 * c);
      o[m].gamma = reinterpret_cast<double*>(q + 16 * c);
      o[m].count = reinterpret_cast<uint32_t*>(q + 24 * c);
      o[m].adjusted = reinterpret_cast<uint32_t*>(q + 28 * c);
      q += 32 * c;
      hipLaunchKernelGGL(est_compact_kernel, dim3(grid_for((uint64_t)v.mask[m] + 1)), dim3(EST_THREADS), 0, s, v, m + 1,
                         o[m], dtot);
      EST_TRY(hipGetLastError());
    }
    EST_TRY(hipMemcpyAsync(&tot, dtot, sizeof tot, hipMemcpyDeviceToHost, s));
    EST_TRY(hipEventRecord(ev[5], s));
    for (int m = 0; m < order; ++m) {
      const size_t c = tot.occupied[m];
      r.key[m].resize(c);
      r.p[m].resize(c);
      r.gamma[m].resize(c);
      r.count[m].resize(c);
      r.adjusted[m].resize(c);
      if (!c) continue;
      EST_TRY(hipMemcpyAsync(r.key[m].data(), o[m].key, 8 * c, hipMemcpyDeviceToHost, s));
      EST_TRY(hipMemcpyAsync(r.p[m].data(), o[m].p, 8 * c, hipMemcpyDeviceToHost, s));
      EST_TRY(hipMemcpyAsync(r.gamma[m].data(), o[m].gamma, 8 * c, hipMemcpyDeviceToHost, s));
      EST_TRY(hipMemcpyAsync(r.count[m].data(), o[m].count, 4 * c, hipMemcpyDeviceToHost, s));
      EST_TRY(hipMemcpyAsync(r.adjusted[m].data(), o[m].adjusted, 4 * c, hipMemcpyDeviceToHost, s));
    }
    EST_TRY(hipEventRecord(ev[6], s));
    EST_TRY(hipStreamSynchronize(s));
  }
  *flags = tot.flags;
  for (int m = 0; m < order; ++m)
    if (tot.out[m] != tot.occupied[m]) *flags |= EST_FLAG_FULL;  // (cannot happen: both count the occupied slots)
  if (*flags & EST_FLAG_FULL) goto done;
  est_finish(&r, d, fallback);
  for (int i = 0; i < 6; ++i) {
    float ms = 0.f;
    EST_TRY(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
    r.stage_ms[i] = ms;
  }
  {
    float ms = 0.f;
    EST_TRY(hipEventElapsedTime(&ms, ev[0], ev[6]));
    r.stage_ms[7] = ms;
  }
  *out = std::move(r);
done:
  if (e != hipSuccess) (void)hipStreamSynchronize(s);
  if (dense) (void)hipFree(dense);
  for (hipEvent_t x : ev)
    if (x) (void)hipEventDestroy(x);
  return e;
}

}  // namespace casr
