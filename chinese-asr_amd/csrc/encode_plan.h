// How an encode chooses its kernels: plan_encode() takes one API call's shapes, the handle's options
// and arithmetic and the device's facts, and returns every path decision of that call as one
// EncodePlan.  The drivers (casr_capi.hip encode_impl, gemm16.hip, recurrence.hip, encoder.hip,
// features.hip) read the plan and decide nothing themselves; the launchers keep only the template
// dispatch.  Also here, because they must agree with the plan: the encode workspaces' sizes.
// Pure host C++ (no HIP runtime): tests/host_plan/encode_plan_check.cpp builds from this header alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "decode_plan.h"

namespace casr {

// ---------------------------------------------------------------- the device
// Read once per handle, on the handle's device (casr_capi.hip casr_create, by recurrence.hip
// read_device_facts: the only place that can name the kernels).
enum { REC_32x16 = 0, REC_16x32 = 1, REC_16x16 = 2, REC_LAYOUTS = 3 };  // rows x units of a workgroup
struct DeviceFacts {
  int cus;                      // compute units
  int rec_per_cu[REC_LAYOUTS];  // resident workgroups per CU of the persistent recurrence, the
                                // smaller of the two arithmetics' figures
};

// ---------------------------------------------------------------- shapes the plan reasons about
constexpr int s16_kpad(int K) { return (K + 63) / 64 * 64; }  // even number of 32-k tiles (gemm16.hip)
constexpr int G16_M = 256, G16_N = 256, G16_K = 32;  // gemm16.hip: tile rows, columns, k per stage
constexpr int GB_M = 128, GB_N = 128, GB_K = 32;     // encoder.hip gemm_nt_kernel's tile
constexpr int KR_G = 16;                             // encoder.hip keys16_kernel: A rows per item
constexpr int FS_MAX_T = 1024;                       // features.hip: frames the one-pass kernels hold
static_assert(s16_kpad(D) % (2 * G16_K) == 0 && C % (2 * G16_K) == 0 && (8 * H) % G16_N == 0 && (8 * H) % 128 == 0 &&
                  C % GB_K == 0,
              "the s16 input GEMM's and the keys GEMM's tiles divide the layer widths");

// XCD-aware tile order (encoder.hip TileOrder, gemm16.hip Order16): the smallest group count whose
// W share (NB / NG column blocks of tile_n rows x K words) fits 3/4 of an L2, and the grid
inline int xcd_groups(int NB, int tile_n, int K) {
  int NG = 1;
  while (NG < 8 && NB % (NG * 2) == 0 && (size_t)(NB / NG) * tile_n * K * 4 > (3u << 20)) NG *= 2;
  return NG;
}
inline int xcd_order_blocks(int NB, int NM, int NG) { return 8 * (NB / NG) * ((NM + 8 / NG - 1) / (8 / NG)); }

// ---------------------------------------------------------------- the plan
enum {
  ENC_OK = 0,
  ENC_BAD_SHAPE,    // B or Tp not positive, or B Tp rows past an int: an argument error
  ENC_KEYS_OFFSET,  // unsupported: the row-streaming keys form's 32-bit buffer offsets
  ENC_KM_FORM,      // a 16-k-major image with a form that reads row images (unreachable: encode_km)
};
enum { FEAT_GIVEN = 0, FEAT_IMAGE, FEAT_ROWS, FEAT_TWO_PASS };  // casr_encode, or casr_encode_fbank's three
enum { GEMM_F32 = 0, GEMM16_TILES, GEMM16_PERSIST, GEMM16_PP, GEMM16_PP_KM, GEMM16_PP_LEAN };
enum { TAIL_NONE = 0, TAIL_HALF, TAIL_BALANCED };
enum { KEYS_F32 = 0, KEYS16_TILES, KEYS16_ROWS };

// the persistent recurrence of one layer, and the per-step fallback's graphs
struct RecPlan {
  int32_t persistent;  // the persistent form is asked for and its grid is resident at once
  int32_t B, Tp, s16, km;
  int32_t layout, RG, UW;  // REC_*: rows and units per workgroup
  int32_t nrg, Bp;         // row groups; granule planes padded to 32 rows for every layout
  int32_t grid, block;
  int32_t sleep, gap, plain;  // CASR_OPT_REC_SLEEP resolved, _POLL_GAP, _STORE_PLAIN
  int32_t coop;               // CASR_OPT_REC_COOP: 0 plain launch, 1 cooperative, 2 chained by event
  int32_t refuse;             // CASR_OPT_REC_COOP_REFUSE (tests): this layer + 1's launch counts as refused
  // hand-off buffer: words reset_rec_layer fills with parity 0, with parity 1, and the placement table
  int32_t hx_zero, hx_tagged, hx_table;
  // per-step fallback: graphs per layer and their row ranges [row0, row1)
  int32_t nsplit, row0[2], row1[2];
  int waves() const { return RG * UW / 64; }  // per workgroup (trace layout)
  int producers() const { return H / UW; }    // workgroups per row group (trace layout)
  size_t hx_bytes() const { return ((size_t)hx_zero + hx_tagged + hx_table) * sizeof(uint32_t); }
};
// the input projection of one layer class (layer 0: K = 720, Kp = 768; layers 1..: K = Kp = 512)
struct InputGemmPlan {
  int32_t form;  // GEMM_*
  int32_t M, K, Kp, km;
  int32_t NB, NM, NG;  // column blocks, row tiles, XCD groups
  int32_t nk, nk16;    // 32-deep / 16-deep stages of the real width K
  int32_t NMm, total, grid, Mm;  // main launch: row tiles, tiles, workgroups, rows
  int32_t tail;                  // TAIL_*: rows [r0, M) after the main launch's
  int32_t r0, Mt;
  int32_t NMt, tail_grid;  // half tiles (TAIL_HALF), or the balanced tail's blocks
  int32_t RT;              // balanced: 32-row units per block
};
struct KeysPlan {
  int32_t form;  // KEYS_*
  int32_t B, Tp, Tq, km;
  int32_t NM, NG, grid;  // tiled forms: the tile order; grid of any form
  int32_t split;         // s16 after a per-step last layer: split_rows of the encoder output first
};
// Every field is an int32 (no padding), so the plan's bytes are its identity: plan_graph_key.
struct EncodePlan {
  int32_t status;  // ENC_*
  int32_t B, Tp, M, layers, residual, s16;
  int32_t km;    // the layer-input images are 16-k-block major (encode_km)
  int32_t feat;  // FEAT_*
  RecPlan rec;
  InputGemmPlan gemm[2];  // layer 0, layers 1..
  KeysPlan keys;
  const InputGemmPlan& layer_gemm(int l) const { return gemm[l == 0 ? 0 : 1]; }
};

// Whether one s16 encode keeps its layer-input images 16-k-block major [Kp / 16][R][16 hi | 16 lo]
// (CASR_OPT_X16_KM): only with the forms that read them, the ping-pong input GEMM, the balanced
// tail and the row-streaming keys; the other forms take row images [R][Kp / 32][32 hi | 32 lo]
inline bool encode_km(const Tuning& t) {
  return t[CASR_OPT_X16_KM] && t[CASR_OPT_GEMM16_PERSIST] == 2 && t[CASR_OPT_GEMM16_TAIL] != 1 &&
         t[CASR_OPT_KEYS_ROWS];
}

// casr_encode_fbank's (and casr_features') kernels for T frames: the layer-0 image straight from
// fbank (features_rows_kernel<true>) under s16, the one-pass f32 features, or past FS_MAX_T frames
// the two-pass kernels
inline int feature_path(int T, bool image) { return T > FS_MAX_T ? FEAT_TWO_PASS : image ? FEAT_IMAGE : FEAT_ROWS; }

// Layout per batch.  32x16 (512 threads: 32 rows x 16 units) while its grid of 16 x ceil(B/32) x 2
// workgroups needs all the CUs (B = 256: one per CU); 16x16 (256 threads) once 16 x ceil(B/16) x 2
// workgroups still fit one per CU (B <= 128): twice the workgroups, each with half the rows, so
// a step's MFMA and cell work per CU halves while the hand-off stays a 16-producer exchange.
// Measured (rec ms per batch, two interleaved rounds): beam B = 128 2.36-2.37 (32x16) -> 2.01-2.02
// (16x16); greedy B = 256 2.67-2.71 (32x16) vs 3.08-3.10 (16x16: two workgroups per CU).
// CASR_OPT_REC_LAYOUT forces one (1 = 32x16, 2 = 16x32, 3 = 16x16).
inline RecPlan plan_recurrence(int B, int Tp, const Tuning& t, bool s16, bool km, bool use_persistent,
                               const DeviceFacts& dev) {
  RecPlan r{};
  r.B = B;
  r.Tp = Tp;
  r.s16 = s16;
  r.km = km;
  switch (t[CASR_OPT_REC_LAYOUT]) {
    case 1: r.layout = REC_32x16; break;
    case 2: r.layout = REC_16x32; break;
    case 3: r.layout = REC_16x16; break;
    default: r.layout = (H / 16) * ((B + 15) / 16) * 2 <= dev.cus ? REC_16x16 : REC_32x16;
  }
  r.RG = r.layout == REC_32x16 ? 32 : 16;
  r.UW = r.layout == REC_16x32 ? 32 : 16;
  r.nrg = (B + r.RG - 1) / r.RG;
  r.Bp = (B + 31) / 32 * 32;
  r.grid = (H / r.UW) * r.nrg * 2;
  r.block = r.RG * r.UW;
  // the hand-off spins need every workgroup of the grid resident at once (one launch)
  r.persistent = use_persistent && r.grid <= dev.rec_per_cu[r.layout] * dev.cus;
  // (-1, the default: no sleep for grids of 64 workgroups or more, one unit below: B <= 16 in the
  // 16-row layout, 32 workgroups; measured round 6)
  r.sleep = t[CASR_OPT_REC_SLEEP] < 0 ? (r.grid >= 64 ? 0 : 1) : t[CASR_OPT_REC_SLEEP];
  r.gap = t[CASR_OPT_REC_POLL_GAP];
  r.plain = t[CASR_OPT_REC_STORE_PLAIN] != 0;
  r.coop = t[CASR_OPT_REC_COOP];
  r.refuse = t[CASR_OPT_REC_COOP_REFUSE];
  // three granule buffers [2][Bp][H] of tagged h words, then the placement table (one word per
  // workgroup).  Buffer j is first read at step j (j = 1, 2) or 3 (j = 0), expecting parity 1, 0, 1:
  // buffers 0 and 1 start with parity 0, buffer 2 with parity 1, the table at 0 (no id published)
  r.hx_tagged = 2 * r.Bp * H;
  r.hx_zero = 2 * r.hx_tagged;
  r.hx_table = r.grid;
  // per-step: rows are independent, so from B = 64 two row halves replay as two graphs on two
  // streams and one half's load latency hides behind the other's MFMAs
  r.nsplit = B >= 64 ? 2 : 1;
  const int half = ((B / 2) + 15) / 16 * 16;
  r.row0[0] = 0;
  r.row1[0] = r.nsplit == 1 ? B : half;
  r.row0[1] = r.nsplit == 1 ? 0 : half;
  r.row1[1] = r.nsplit == 1 ? 0 : B;
  return r;
}

// The s16 input projection of M rows on 256 x 256 tiles (gemm16.hip).  K: the real input width (the
// Kp-wide images are zero from K to Kp).
inline InputGemmPlan plan_input_gemm(int M, int K, const Tuning& t, bool s16, bool km, const DeviceFacts& dev) {
  InputGemmPlan g{};
  const int N = 8 * H, ncu = dev.cus;
  g.M = M;
  g.K = K;
  g.Kp = s16 ? s16_kpad(K) : K;
  g.km = km;
  if (!s16) return g;  // GEMM_F32: encoder.hip launch_input_proj
  const int persist = t[CASR_OPT_GEMM16_PERSIST], tail = t[CASR_OPT_GEMM16_TAIL];
  g.NB = N / G16_N;
  g.NM = g.NMm = (M + G16_M - 1) / G16_M;
  g.NG = xcd_groups(g.NB, G16_N, g.Kp);
  // the persistent forms run ceil(K / 32) (ping-pong: ceil(K / 16)) stages: layer 0 (K = 720,
  // Kp = 768) skips the all-zero last stage
  g.nk = (K + G16_K - 1) / G16_K;
  g.nk16 = (K + 15) / 16;
  if (!persist) {
    g.form = GEMM16_TILES;
    g.total = g.grid = xcd_order_blocks(g.NB, g.NM, g.NG);
    g.Mm = M;
    return g;
  }
  g.form = persist != 2 ? GEMM16_PERSIST : !km ? GEMM16_PP : t[CASR_OPT_GEMM16_LEAN] && g.nk16 >= 8 ? GEMM16_PP_LEAN : GEMM16_PP_KM;
  // Balanced last round.  NB x NM tiles over ncu workgroups leave a partial last round (B = 256:
  // 2128 tiles = 8 rounds + 80 tiles, so 80 CUs run a ninth tile while 176 idle; B = 128: 4
  // rounds + 40).  The persistent kernel takes the first F = floor(NB NM / ncu) rounds (whole row
  // tiles: F ncu / NB of them, every workgroup exactly F tiles) and the rows after them go to a
  // tail launch, while its 128 x 256 half tiles would fit one round.  Same per-element arithmetic
  // as the persistent kernel: bitwise equal.
  const int F = g.NB * g.NM / ncu;
  if (tail && F >= 1 && (F * ncu) % g.NB == 0 && F * ncu / g.NB < g.NM) {
    const int nm = F * ncu / g.NB;
    if (g.NB * ((M - nm * G16_M + 127) / 128) <= ncu) g.NMm = nm;
  }
  g.total = xcd_order_blocks(g.NB, g.NMm, g.NG);
  g.grid = g.total < ncu ? g.total : ncu;
  g.Mm = M < g.NMm * G16_M ? M : g.NMm * G16_M;
  if (g.NMm < g.NM) {
    g.r0 = g.NMm * G16_M;
    g.Mt = M - g.r0;
    if (tail == 2) {
      // gemm16_tail_kernel tiles of RT 32-row units x 128 columns: one round of ncu workgroups while
      // the rows allow RT <= 5 (past 5 x ncu units: more than one round)
      g.tail = TAIL_BALANCED;
      const int units = (g.Mt + 31) / 32 * (N / 128), rt = (units + ncu - 1) / ncu;
      g.RT = rt < 5 ? rt : 5;
      g.tail_grid = (g.Mt + 32 * g.RT - 1) / (32 * g.RT) * (N / 128);
    } else {
      // 128 x 256 half tiles (gemm16_bias_kernel<4, 1>, one per CU), which run at one wave per
      // SIMD; the same column slices per XCD as the main launch
      g.tail = TAIL_HALF;
      g.NMt = (g.Mt + 127) / 128;
      g.tail_grid = xcd_order_blocks(g.NB, g.NMt, g.NG);
    }
  }
  return g;
}

// cfg: enc_layers and residual are read.  T, fbank: casr_encode_fbank's frames (else T = 0).  s16: the
// s16 arithmetic is in effect (requested, and the blob's s16 images are valid).  use_persistent:
// casr_set_persistent.
inline EncodePlan plan_encode(int B, int Tp, int T, bool fbank, const casr_config& cfg, const Tuning& t, bool s16,
                              bool use_persistent, const DeviceFacts& dev) {
  EncodePlan p{};
  p.B = B;
  p.Tp = Tp;
  if (B <= 0 || Tp <= 0 || (int64_t)B * Tp > INT32_MAX) {
    p.status = ENC_BAD_SHAPE;
    return p;
  }
  const int M = p.M = B * Tp;
  p.layers = cfg.enc_layers;
  p.residual = cfg.residual != 0;
  p.s16 = s16;
  p.km = s16 && encode_km(t);
  p.feat = fbank ? feature_path(T, s16) : FEAT_GIVEN;
  p.rec = plan_recurrence(B, Tp, t, s16, p.km, use_persistent, dev);
  p.gemm[0] = plan_input_gemm(M, D, t, s16, p.km, dev);
  p.gemm[1] = plan_input_gemm(M, C, t, s16, p.km, dev);
  KeysPlan& k = p.keys;
  k.B = B;
  k.Tp = Tp;
  k.Tq = attn_tq(Tp);  // keysT row stride (16 B aligned rows for the attention)
  k.km = p.km;
  // s16x3 keys on every s16 path (the per-step fallback splits the encoder output first), so both
  // recurrences give the same keys bits
  k.split = s16;
  k.form = !s16 ? KEYS_F32 : t[CASR_OPT_KEYS_ROWS] ? KEYS16_ROWS : KEYS16_TILES;
  if (k.form == KEYS16_ROWS) {  // one workgroup per CU streams items of KR_G rows of one utterance
    const int NI = B * ((Tp + KR_G - 1) / KR_G);
    k.grid = NI < dev.cus ? NI : dev.cus;
    if ((size_t)2 * B * A * k.Tq * 4 >= 0xFFFFFFF0u) p.status = ENC_KEYS_OFFSET;  // its 32-bit buffer offsets
  } else {
    k.NM = (M + GB_M - 1) / GB_M;
    k.NG = xcd_groups(A / GB_N, GB_N, C);
    k.grid = xcd_order_blocks(A / GB_N, k.NM, k.NG);
  }
  // the forms that read row images never meet a 16-k-major one: encode_km allows it only with the
  // ping-pong GEMM, the balanced tail and the row-streaming keys
  for (const InputGemmPlan& g : p.gemm)
    if (p.km && ((g.form != GEMM16_PP_KM && g.form != GEMM16_PP_LEAN) || g.tail == TAIL_HALF)) p.status = ENC_KM_FORM;
  if (p.km && k.form != KEYS16_ROWS) p.status = ENC_KM_FORM;
  return p;
}

// ---------------------------------------------------------------- encode workspaces
struct EncodeSizes {
  size_t gin;    // [M][8 H] gate pre-activations of one layer
  size_t out;    // [M][C] a layer's output (two: out0, out1)
  size_t hbuf;   // [2][2][B][H] per-step recurrence: h, ping-pong
  size_t cst;    // [2][B][H] final c
  size_t hfin;   // [2][B][H] final h
  size_t keysT;  // [2][B][A][Tq]: keys | exp(2 keys) (KeysEpi)
  size_t lens;   // [B]
  size_t x16;    // s16: the current layer input's image, [M][s16_kpad(D)] words
  size_t hx;     // persistent recurrence: RecPlan::hx_bytes
  size_t feat;   // casr_encode_fbank outside the image path: the f32 features [M][D]
  size_t fstat;  // casr_encode_fbank: feature statistics scratch [B][2][D]
};
inline EncodeSizes encode_sizes(const EncodePlan& p) {
  const size_t M = (size_t)p.M, B = (size_t)p.B, f = sizeof(float);
  EncodeSizes z{};
  z.gin = M * 8 * H * f;
  z.out = M * C * f;
  z.hbuf = 2 * 2 * B * H * f;
  z.cst = z.hfin = 2 * B * H * f;
  z.keysT = 2 * B * A * p.keys.Tq * f;
  z.lens = B * sizeof(int32_t);
  z.x16 = p.s16 ? M * s16_kpad(D) * f : 0;
  z.hx = p.rec.persistent ? p.rec.hx_bytes() : 0;
  z.feat = p.feat == FEAT_ROWS || p.feat == FEAT_TWO_PASS ? M * D * f : 0;
  z.fstat = p.feat != FEAT_GIVEN ? B * 2 * D * f : 0;
  return z;
}

}  // namespace casr
