// casr_convert_audio (include/casr.h): any-rate, any-channel-count float32 PCM -> 16 kHz mono, the
// reference's convert_audio (main.py:19-24: ffmpeg -sample_fmt s16 -ar 16000 -ac 1, sox --norm=-1)
// as four stages defined by formulas (resample_design.h), not by those tools' bits:
//   (a) downmix, (b) polyphase Kaiser-sinc resampling by L / M, (c) s16 quantisation, (d) peak
//   normalisation.
// convert_kernel does (a) to (c): one workgroup takes RS_TILE consecutive outputs of one utterance,
// stages the input span they read (RS_TILE M / L + 2 K samples) into LDS once, downmixing as it
// stages, and every lane runs one f32 fma chain per output over the 2 K taps of the output's phase
// in ascending tap order (the same chain in every form below, so the same bits).  Three forms:
//   L <= 2 (8, 24, 32, 48, 96 kHz)  a lane takes two adjacent outputs; their phases are the same in
//       every lane, so the taps are wave-uniform loads, and the two chains share the staged samples
//       their windows have in common: one LDS read per two fmas (or fewer).  Lanes read 2 M / L
//       apart: conflict-free at 8 and 24 kHz, two-way at 48 kHz, four-way at 32 and 96 kHz;
//   a table of up to RS_TAB_LDS_MAX floats (12 kHz)  copied into LDS, each lane its own phase row;
//   a larger table (160 to 640 phases, at most 256 KB, shared by every workgroup)  read through L2,
//       each lane walking its own phase row 8 bytes at a time.
// The peak of stage (d) is an integer maximum of |q| (or of the bit pattern of |y|, monotone for
// non-negative floats), reduced per workgroup and then by one atomicMax on a word that has its cache
// line to itself, so it does not depend on arrival order; normalise_kernel then scales each utterance
// in place.
#include "casr_common.h"
#include "casr_internal.h"

namespace casr {

namespace {

// stage (c): q = clamp(rint(y 32768), -32768, 32767), ties to even; NaN -> 0
__device__ __forceinline__ float quantise_s16(float y) {
  const float r = fminf(fmaxf(rintf(y * 32768.f), -32768.f), 32767.f);
  return y != y ? 0.f : r;
}

// (a): the f32 sum of the frame's channels in ascending order, times 1 / ch
__device__ __forceinline__ float downmix(const float* __restrict__ frame, int ch, float inv_ch) {
  float s = frame[0];
  for (int c = 1; c < ch; ++c) s += frame[c];
  return s * inv_ch;
}

// MODE 0: the table read through L2, each lane its own phase row; 1: the table copied into LDS; 2: L <= 2
// (8, 24, 32, 48, 96 kHz): a lane takes two ADJACENT outputs, whose phases 0 and M mod L are then the
// same in every lane, so the taps are wave-uniform loads (scalar registers, no LDS traffic) and the two
// outputs share every staged sample their windows have in common (all of them when upsampling)
template <int MODE>
__global__ __launch_bounds__(RS_THREADS) void convert_kernel(ConvertArgs a, const float* __restrict__ tab) {
  extern __shared__ __align__(16) float smem[];
  __shared__ uint32_t wave_peak[RS_THREADS / 64];
  constexpr bool TLDS = MODE == 1;
  const int tid = threadIdx.x, b = blockIdx.y;
  const int m0 = blockIdx.x * RS_TILE;
  int n = a.n_in[b];
  const bool bad = n < 0 || n > a.n_max_in;
  n = n < 0 ? 0 : (n > a.n_max_in ? a.n_max_in : n);
  const bool pass = a.L == a.M;  // 16 kHz in: (a) only, no filter
  const int64_t nout = ((int64_t)n * a.L + a.M - 1) / a.M;  // <= m_max (checked by the host)
  if (blockIdx.x == 0 && tid == 0) {
    a.n_out[b] = (int32_t)nout;
    if (bad) atomicOr(a.err, CASR_DEV_BAD_AUDIO);
    if (!a.norm && a.gain) a.gain[b] = 1.f;
  }
  float* __restrict__ wrow = a.wav + (size_t)b * a.m_max;
  constexpr int OPL = RS_TILE / RS_THREADS;
  if (m0 >= nout) {  // a tile of padding: exactly zero
#pragma unroll
    for (int i = 0; i < OPL; ++i) {
      const int m = m0 + tid + i * RS_THREADS;
      if (m < a.m_max) wrow[m] = 0.f;
    }
    return;
  }
  const float* __restrict__ prow = a.pcm + (size_t)b * a.n_max_in * a.ch;
  float y[OPL];
  if (pass) {
#pragma unroll
    for (int i = 0; i < OPL; ++i) {
      const int m = m0 + tid + i * RS_THREADS;
      y[i] = m < nout ? downmix(prow + (size_t)m * a.ch, a.ch, a.inv_ch) : 0.f;
    }
  } else {
    float* tl = smem;
    float* xs = smem + (TLDS ? a.L * a.taps : 0);
    if (TLDS)
      for (int i = tid; i < a.L * a.taps; i += RS_THREADS) tl[i] = tab[i];
    // the tile's first output: position m0 M = base0 L + p0
    const int64_t pos0 = (int64_t)m0 * a.M;
    const int64_t base0 = pos0 / a.L;
    const uint32_t p0 = (uint32_t)(pos0 - base0 * a.L);
    const int mlast = (int)((int64_t)m0 + RS_TILE - 1 < nout - 1 ? (int64_t)m0 + RS_TILE - 1 : nout - 1);
    const int64_t lo = base0 - a.K + 1;
    const int cnt = (int)(((int64_t)mlast * a.M) / a.L + a.K - lo + 1);  // <= resample_span(): >= taps
    for (int i = tid; i < cnt; i += RS_THREADS) {
      const int64_t idx = lo + i;
      xs[i] = idx >= 0 && idx < n ? downmix(prow + (size_t)idx * a.ch, a.ch, a.inv_ch) : 0.f;  // x = 0 outside [0, n)
    }
    __syncthreads();
    if (MODE == 2) {
      // outputs m0 + 2 tid and m0 + 2 tid + 1.  L divides 2 and RS_TILE, so (m0 + 2 tid) M is a multiple
      // of L: phase 0 at x offset q0 = 2 tid M / L, and the next output has phase M mod L, delta = M div L
      // samples on.  A lane past mlast reads from the span's start (staged or not, never out of the
      // allocation: resample_span) and its sums are dropped
      const int delta = a.M / a.L;
      const float* __restrict__ t0 = tab;
      const float* __restrict__ t1 = tab + (size_t)(a.M % a.L) * a.taps;
      const bool valid = m0 + 2 * tid <= mlast;
      const float* x = xs + (valid ? (uint32_t)(2 * tid) * (uint32_t)a.M / (uint32_t)a.L : 0u);
      float a0 = 0.f, a1 = 0.f;
      int i = 0;
      for (; i < delta; ++i) a0 = fmaf(t0[i], x[i], a0);
#pragma unroll 8
      for (; i < a.taps; ++i) {
        const float xv = x[i];
        a0 = fmaf(t0[i], xv, a0);
        a1 = fmaf(t1[i - delta], xv, a1);
      }
      for (; i < a.taps + delta; ++i) a1 = fmaf(t1[i - delta], x[i], a1);
      y[0] = valid ? a0 : 0.f;
      y[1] = m0 + 2 * tid + 1 <= mlast ? a1 : 0.f;
    } else {
      // a lane's outputs (RS_THREADS apart) run their fma chains side by side; an output past mlast
      // reads phase 0 on the span's first taps samples (all staged) and its sum is dropped
      const float* tp[OPL];
      const float* xp[OPL];
      float acc[OPL];
#pragma unroll
      for (int i = 0; i < OPL; ++i) {
        const int dm = tid + i * RS_THREADS;
        const bool valid = m0 + dm <= mlast;
        const uint32_t d = p0 + (uint32_t)dm * (uint32_t)a.M;  // < 16000 + 512 x 384000
        const uint32_t q = d / (uint32_t)a.L, p = d - q * (uint32_t)a.L;
        tp[i] = (TLDS ? tl : tab) + (valid ? (size_t)p * a.taps : 0);
        xp[i] = xs + (valid ? (int)q : 0);  // base - K + 1 - lo = q
        acc[i] = 0.f;
      }
      for (int j = 0; j < a.taps; j += 2) {
#pragma unroll
        for (int i = 0; i < OPL; ++i) {
          const float2 t = *reinterpret_cast<const float2*>(tp[i] + j);  // taps is even: 8-byte aligned rows
          acc[i] = fmaf(t.x, xp[i][j], acc[i]);
          acc[i] = fmaf(t.y, xp[i][j + 1], acc[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < OPL; ++i) y[i] = m0 + tid + i * RS_THREADS <= mlast ? acc[i] : 0.f;
    }
  }
  uint32_t peak = 0;
#pragma unroll
  for (int i = 0; i < OPL; ++i) {
    const int m = m0 + (MODE == 2 && !pass ? OPL * tid + i : tid + i * RS_THREADS);
    if (m >= a.m_max) continue;
    float v = 0.f;
    if (m < nout) {
      if (a.quantize) {
        const float q = quantise_s16(y[i]);
        peak = max(peak, (uint32_t)fabsf(q));
        v = q * (1.f / 32768.f);
      } else {
        v = y[i];
        if (v == v) peak = max(peak, __float_as_uint(fabsf(v)));  // a NaN sample takes no part in the peak
      }
    }
    wrow[m] = v;
  }
  if (a.norm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) peak = max(peak, (uint32_t)__shfl_xor((int)peak, o));
    // one atomic per workgroup, on a word that has its 128-byte line to itself
    if ((tid & 63) == 0) wave_peak[tid >> 6] = peak;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int w = 1; w < RS_THREADS / 64; ++w) peak = max(peak, wave_peak[w]);
      if (peak) atomicMax(a.peak + (size_t)b * RS_PEAK_STRIDE, peak);
    }
  }
}

// stage (d) in place on wav [B][m_max]: gain = target / peak, one correctly rounded f32 division
__global__ __launch_bounds__(256) void normalise_kernel(float* __restrict__ wav, const int32_t* __restrict__ n_out,
                                                        int m_max, const uint32_t* __restrict__ peak, int quantize,
                                                        float target, float* __restrict__ gain) {
  const int b = blockIdx.y;
  const uint32_t pk = peak[(size_t)b * RS_PEAK_STRIDE];
  float g = 1.f;  // silence, or no samples
  if (pk) g = __fdiv_rn(target, quantize ? (float)pk : __uint_as_float(pk));
  if (blockIdx.x == 0 && threadIdx.x == 0 && gain) gain[b] = g;
  if (!pk) return;
  int nout = n_out[b];
  nout = nout < m_max ? nout : m_max;
  float* __restrict__ w = wav + (size_t)b * m_max;
  for (int m = blockIdx.x * blockDim.x + threadIdx.x; m < nout; m += gridDim.x * blockDim.x) {
    const float v = w[m];
    if (quantize) {
      const float r = rintf(__fmul_rn(v * 32768.f, g));
      w[m] = fminf(fmaxf(r, -32768.f), 32767.f) * (1.f / 32768.f);
    } else {
      w[m] = __fmul_rn(v, g);
    }
  }
}

}  // namespace

hipError_t launch_convert(const ConvertArgs& a, int B, const ResamplePlan& p, float target, hipStream_t s) {
  if (a.norm) {
    hipError_t e = fill_u32(a.peak, 0u, (size_t)B * RS_PEAK_STRIDE, s);
    if (e != hipSuccess) return e;
  }
  const dim3 grid((unsigned)((a.m_max + RS_TILE - 1) / RS_TILE), (unsigned)B);
  const bool pass = p.L == p.M;
  const size_t lds = pass ? 0 : resample_lds_bytes(p);
  if (!pass && resample_uniform_phases(p))
    hipLaunchKernelGGL(convert_kernel<2>, grid, dim3(RS_THREADS), lds, s, a, a.tab);
  else if (!pass && resample_tab_in_lds(p))
    hipLaunchKernelGGL(convert_kernel<1>, grid, dim3(RS_THREADS), lds, s, a, a.tab);
  else
    hipLaunchKernelGGL(convert_kernel<0>, grid, dim3(RS_THREADS), lds, s, a, a.tab);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !a.norm) return e;
  const unsigned nb = (unsigned)std::min<size_t>(((size_t)a.m_max + 1023) / 1024, 256);
  hipLaunchKernelGGL(normalise_kernel, dim3(nb, (unsigned)B), dim3(256), 0, s, a.wav, a.n_out, a.m_max, a.peak,
                     a.quantize, target, a.gain);
  return hipGetLastError();
}

}  // namespace casr
