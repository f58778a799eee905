// The design of casr_convert_audio's resampler (include/casr.h): the rational ratio L / M of a rate,
// the taps of its polyphase Kaiser-windowed sinc, the table itself in double, and the output length.
// The kernels (convert.hip) and the C entry points (casr_capi.hip) read the plan and decide nothing
// themselves.  The operation is defined by these formulas, not by any other tool's output.
// Pure host C++ (no HIP runtime): tests/host_resample/resample_check.cpp builds from this header alone.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace casr {

constexpr int RS_RATE_OUT = 16000;
constexpr int RS_RATE_MIN = 4000, RS_RATE_MAX = 384000;
constexpr int RS_TABLE_MAX = 65536;   // floats of the largest table kept (L x taps)
constexpr int RS_CH_MAX = 8;
constexpr double RS_CUTOFF = 0.94;    // of the narrower Nyquist band
constexpr double RS_ZEROS = 32.0;     // sinc zero crossings on each side of the centre
constexpr double RS_BETA = 9.0;       // Kaiser window

struct ResamplePlan {
  int rate = 0;
  int L = 0, M = 0;  // 16000 / g and rate / g, g = gcd(16000, rate)
  int K = 0;         // taps j = -K + 1 .. K of every phase
  int taps = 0;      // 2 K
  double c = 0;      // cutoff in cycles per input sample x 2: 0.94 min(1, L / M)
  double hw = 0;     // half width of the window in input samples: 32 / c
  size_t table_floats() const { return (size_t)L * taps; }
};

enum { RS_OK = 0, RS_BAD_RATE = 1, RS_TABLE_TOO_LARGE = 2 };

inline int rs_gcd(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// RS_OK, RS_BAD_RATE (outside [4000, 384000]; the plan is untouched) or RS_TABLE_TOO_LARGE (more than
// 65,536 floats, e.g. 44,101 Hz: the plan is filled in, so the caller can report the numbers)
inline int resample_plan(int rate, ResamplePlan* p) {
  if (rate < RS_RATE_MIN || rate > RS_RATE_MAX) return RS_BAD_RATE;
  const int g = rs_gcd(RS_RATE_OUT, rate);
  p->rate = rate;
  p->L = RS_RATE_OUT / g;
  p->M = rate / g;
  const double r = (double)p->L / (double)p->M;
  p->c = RS_CUTOFF * (r < 1.0 ? r : 1.0);
  p->hw = RS_ZEROS / p->c;
  p->K = (int)ceil(p->hw);
  p->taps = 2 * p->K;
  return (size_t)p->L * p->taps > (size_t)RS_TABLE_MAX ? RS_TABLE_TOO_LARGE : RS_OK;
}

// n_out = ceil(n L / M)
inline int64_t resample_frames(int64_t n, const ResamplePlan& p) {
  return n <= 0 ? 0 : (n * p.L + p.M - 1) / p.M;
}

// modified Bessel function of the first kind, order 0, by its power series sum ((x / 2)^k / k!)^2:
// every term is positive, so the sum is good to double precision (23 terms at x = 9)
inline double bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-17 * sum) break;
  }
  return sum;
}

// h(u) = c sinc(c u) I0(9 sqrt(1 - (u / hw)^2)) / I0(9) for |u| < hw, else 0
inline double resample_h(const ResamplePlan& p, double u, double inv_i0_beta) {
  const double au = fabs(u);
  if (!(au < p.hw)) return 0.0;
  const double t = p.c * u;
  const double pi = 3.14159265358979323846;
  const double s = t == 0.0 ? 1.0 : sin(pi * t) / (pi * t);
  const double w = 1.0 - (u / p.hw) * (u / p.hw);
  return p.c * s * bessel_i0(RS_BETA * sqrt(w > 0.0 ? w : 0.0)) * inv_i0_beta;
}

// One phase's 2 K taps in double: row[j + K - 1] = h(p / L - j) / sum_j h, j = -K + 1 .. K
inline void resample_phase(const ResamplePlan& pl, int phase, double* row) {
  const double inv = 1.0 / bessel_i0(RS_BETA);
  double sum = 0.0;
  for (int i = 0; i < pl.taps; ++i) {
    const int j = i - pl.K + 1;
    row[i] = resample_h(pl, (double)phase / (double)pl.L - (double)j, inv);
    sum += row[i];
  }
  for (int i = 0; i < pl.taps; ++i) row[i] /= sum;
}

// The f32 table [L][taps]: computed in double, every phase scaled to unit DC gain, rounded once
inline void resample_filter(const ResamplePlan& pl, float* tab) {
  std::vector<double> row((size_t)pl.taps);
  for (int ph = 0; ph < pl.L; ++ph) {
    resample_phase(pl, ph, row.data());
    for (int i = 0; i < pl.taps; ++i) tab[(size_t)ph * pl.taps + i] = (float)row[(size_t)i];
  }
}

// ---------------------------------------------------------------- the kernel's tiling (convert.hip)
constexpr int RS_TILE = 512;        // consecutive outputs of one utterance per workgroup
constexpr int RS_THREADS = 256;     // RS_TILE / RS_THREADS outputs per lane
constexpr int RS_TAB_LDS_MAX = 2048;  // tables up to this many floats are copied into LDS (L = 4 at the usual rates)

// input samples a tile of RS_TILE outputs reads: first = floor(m0 M / L) - K + 1, last =
// floor((m0 + RS_TILE - 1) M / L) + K, so at most this many
inline int resample_span(const ResamplePlan& p) {
  return (int)(((int64_t)(RS_TILE - 1) * p.M) / p.L) + 2 + p.taps;
}
constexpr int RS_PEAK_STRIDE = 32;  // words between two utterances' peak words: one 128-byte line each
// L divides the RS_TILE / RS_THREADS = 2 adjacent outputs a lane then takes: every lane sees the same
// two phases, and the taps are wave-uniform loads (8, 24, 32, 48, 96 kHz)
inline bool resample_uniform_phases(const ResamplePlan& p) { return p.L <= RS_TILE / RS_THREADS; }
inline bool resample_tab_in_lds(const ResamplePlan& p) {
  return !resample_uniform_phases(p) && p.table_floats() <= (size_t)RS_TAB_LDS_MAX;
}
inline size_t resample_lds_bytes(const ResamplePlan& p) {
  return ((size_t)resample_span(p) + (resample_tab_in_lds(p) ? p.table_floats() : 0)) * sizeof(float);
}

}  // namespace casr
