// Host side of the casr C ABI (include/casr.h): weight packing into kernel layouts,
// per-handle device workspaces, and the encode / decode drivers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "casr.h"
#include "align_plan.h"
#include "casr_internal.h"
#include "confusion_plan.h"
#include "edit_align_plan.h"
#include "edit_plan.h"

namespace casr {


// version word of the packed layout (bump whenever make_layout or a packer changes)
constexpr uint32_t LAYOUT_MAGIC = 0xCA5B0003u;

Layout make_layout(const casr_config& cfg) {
  Layout L{};
  size_t off = 0;
  auto take = [&](size_t n) {
    const size_t o = off;
    off += (n + 63) & ~size_t(63);  // 256 B alignment for every tensor
    return o;
  };
  L.layers = cfg.enc_layers;
  L.V = cfg.vocab;
  L.VP = (cfg.vocab + 63) / 64 * 64;
  for (int l = 0; l < cfg.enc_layers; ++l) {
    const int din = l == 0 ? D : C;
    L.enc_wih[l] = take((size_t)8 * H * din);
    L.enc_bias[l] = take((size_t)8 * H);
    L.enc_whh[l] = take((size_t)2 * 4 * H * H);
  }
  L.emb = take((size_t)cfg.vocab * E);
  L.dec_w = take((size_t)4 * HD * KDEC);
  L.dec_b = take((size_t)4 * HD);
  L.proj_w = take((size_t)L.VP * KPROJ);
  L.proj_b = take((size_t)L.VP);
  L.wencT = take((size_t)A * C);
  L.b_attn = take((size_t)A);
  L.w_hidden = take((size_t)HD * A);
  L.v = take((size_t)A);
  L.info = take(64);
  for (int l = 0; l < cfg.enc_layers; ++l) {
    const int din = l == 0 ? D : C;
    L.enc_wih16[l] = take((size_t)8 * H * s16_kpad(din));
    L.enc_whh16[l] = take((size_t)2 * 4 * H * H);
  }
  L.emb16 = take((size_t)cfg.vocab * E);
  L.dec_w16 = take((size_t)4 * HD * KDEC);
  L.proj_w16 = take((size_t)L.VP * KPROJ);
  L.wenc16 = take((size_t)A * C);
  L.total = off;
  return L;
}

// Write a [N][K] matrix (element accessor f(n, k), rows >= N zero) in MFMA-fragment-major
// order: 16-row x 64-k blocks, block (nt, kc) at (nt*NKC + kc)*FRAG, inside [q][lane][4]
// with lane row = lane&15, k = 16*(lane>>4) + 4q + e.
template <class Fn>
static void pack_frag(float* dst, int NT, int NKC, Fn f) {
  for (int nt = 0; nt < NT; ++nt)
    for (int kc = 0; kc < NKC; ++kc) {
      float* blk = dst + ((size_t)nt * NKC + kc) * FRAG;
      for (int q = 0; q < 4; ++q)
        for (int lane = 0; lane < 64; ++lane)
          for (int e = 0; e < 4; ++e) {
            const int n = nt * 16 + (lane & 15);
            const int k = kc * 64 + 16 * (lane >> 4) + 4 * q + e;
            blk[(q * 64 + lane) * 4 + e] = f(n, k);
          }
    }
}

// ---- s16x3 images (casr_common.h split16), host side: hi = f16_rn(x), lo = f16_rn((x - hi) 2^11)
static void split16_host(float x, uint16_t& hi, uint16_t& lo) {
  const _Float16 h = (_Float16)x;
  const float r = (x - (float)h) * 2048.0f;
  const _Float16 l = (r == r && std::fabs(r) < 65504.f) ? (_Float16)r : (_Float16)0.f;
  std::memcpy(&hi, &h, 2);
  std::memcpy(&lo, &l, 2);
}

// [N][K] (accessor f(n, k)) as s16 row images [N][Kp/32][32 hi | 32 lo], zeros past K
template <class Fn>
static void pack_rows16(float* dst, int N, int K, Fn f) {
  const int Kp = s16_kpad(K);
  uint16_t* o = reinterpret_cast<uint16_t*>(dst);
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < Kp; ++k) {
      uint16_t hi = 0, lo = 0;
      if (k < K) split16_host(f(n, k), hi, lo);
      uint16_t* t = o + (size_t)n * Kp * 2 + (k / 32) * 64 + (k % 32);
      t[0] = hi;
      t[32] = lo;
    }
}

// [N][K] in s16 fragment-major order: 16-row x 64-k blocks of FRAG floats, block (nt, kc) =
// [j = 0..1][hl = hi, lo][lane][8 halves] with lane row = lane & 15 and
// k = kc*64 + 16*(lane >> 4) + 8j + e: lane l's v_mfma_f32_16x16x32_f16 B operand for k-step j
// is one 16-B load, and its 16 k (both steps) are the 16 consecutive k of its f32 fragment row.
template <class Fn>
static void pack_frag16(float* dst, int NT, int NKC, Fn f) {
  uint16_t* o = reinterpret_cast<uint16_t*>(dst);
  for (int nt = 0; nt < NT; ++nt)
    for (int kc = 0; kc < NKC; ++kc) {
      uint16_t* blk = o + ((size_t)nt * NKC + kc) * FRAG * 2;
      for (int j = 0; j < 2; ++j)
        for (int lane = 0; lane < 64; ++lane)
          for (int e = 0; e < 8; ++e) {
            uint16_t hi, lo;
            split16_host(f(nt * 16 + (lane & 15), kc * 64 + 16 * (lane >> 4) + 8 * j + e), hi, lo);
            blk[((j * 2 + 0) * 64 + lane) * 8 + e] = hi;
            blk[((j * 2 + 1) * 64 + lane) * 8 + e] = lo;
          }
    }
}

}  // namespace casr

using namespace casr;

namespace {

thread_local std::string g_err;

struct DevBuf {
  void* p = nullptr;
  size_t n = 0;
  hipError_t ensure(size_t bytes) {
    if (bytes <= n) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) n = bytes;
    return e;
  }
  template <class T>
  T* as() const { return reinterpret_cast<T*>(p); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};

}  // namespace

struct casr_handle {
  casr_config cfg{};
  Layout L{};
  int device = 0;
  DeviceFacts dev{};  // of `device`, read at casr_create (plan_encode's input)
  const float* W = nullptr;
  std::string err;
  // encoder workspace
  DevBuf gin, out0, out1, hbuf, cst, hfin, keysT, lens;
  DevBuf feat;     // casr_encode_fbank outside the s16x3 image path: the f32 features
  DevBuf fstat;    // feature statistics scratch [B][2][D] (features.hip)
  DevBuf hx;       // persistent recurrence: tagged h words [3][2][Bp][H]
  // device guard bits, one word per source: [0] decode, [1] encoder + features, [2] front end.
  // Allocated and zeroed once; kernels OR bits in; casr_device_flags reads and clears them, so
  // they cover every call since the previous read (never reset inside a captured graph)
  DevBuf gflags;
  DevBuf fe_const; // FrontendConst (filterbank, window, twiddles), built on first casr_log_mel
  // casr_convert_audio: the f32 table of each rate seen, on host and device, built at the first call
  // at that rate (oldest first; RS_CACHE kept), and the per-utterance peak words
  struct ResampleTable {
    ResamplePlan plan;
    std::vector<float> host;  // the source of the stream-ordered upload: lives as long as the entry
    DevBuf dev;
  };
  static constexpr size_t RS_CACHE = 6;
  std::vector<ResampleTable*> rs_tables;
  DevBuf cvt_peak;
  DevBuf seg_q, seg_hist;  // casr_segment: the frames' levels [B][T] uint16 and the histograms [B][512]
  bool use_persistent = true;
  int precision = CASR_PREC_S16;  // requested (casr_set_precision)
  bool s16_valid = false;           // the bound blob's s16 images are usable (Layout::info)
  bool proj_small = false;          // every |W_p| < 16 (Layout::info + 4)
  bool dec_small = false;           // every decoder LSTM weight < 16 (Layout::info + 5)
  DevBuf x16;                       // s16 image of the current layer input [B*Tp][Kp] (or 16-k-block major)
  // the encoder layers' W_ih s16 images 16-k-block major (CASR_OPT_X16_KM), built at bind from an
  // s16-valid blob: layer l at wih16km_off[l]
  DevBuf wih16km;
  size_t wih16km_off[CASR_MAX_LAYERS] = {};
  // folded greedy decode (CASR_OPT_DEC_FOLD): fused projection | LSTM-gate fragment image and the
  // per-token gate table, built at bind from an s16-valid blob; the gates buffer [R][4 HD]
  DevBuf wfold, egates, fgates, wq16;
  bool fold_ready = false;
  // (round 4) the f32 fused image: the folded greedy step under the exact-f32 arithmetic
  DevBuf wfold32;
  DevBuf coldbuf;  // CASR_OPT_DIAG_COLD's flush source (measurement only)
  bool fold32_ready = false;
  bool s16() const { return precision == CASR_PREC_S16 && s16_valid; }
  int B = 0, Tp = 0;
  bool encoded = false;
  float* enc_out = nullptr;  // out0 or out1
  // decoder workspace
  DevBuf st, logits, small, bp, tk, rec;
  DevBuf ksbuf;  // the greedy folded GEMM's k-split sums and counters (R <= 32, CASR_OPT_DEC_KSPLIT)
  DevBuf asbuf;  // the split greedy attention's partials and counters (R <= 64, CASR_OPT_ATTN_SPLIT)
  DevBuf scorebuf;  // casr_score: state history, row partials, token feed (score_workspace_bytes)
  DecodeBufs d{};
  DevBuf gout;  // internal decode outputs written by captured graphs
  Profiler prof;
  // the last beam and the view of what it left in the decode workspaces (beam_state.h): set by the
  // beam entries (beam_ran), spent by casr_encode and by prepare_decode, read through beam_readable
  BeamState beam;
  BeamTree tree;
  DevBuf lmws;    // casr_beam_lm: term rows, LM sums, rec_lm (carve_beam_lm)
  DevBuf biasws;  // casr_beam_bias: gain rows, states, sums, rec_full (carve_beam_bias)
  DevBuf gramws;  // casr_beam_grammar: mask rows, states (carve_beam_gram)
  DevBuf mbrws;   // casr_beam_mbr: lists, weights and the byte distances (carve_mbr)
  DevBuf eaws;    // casr_edit_align: direction bits and the tile hand-offs (edit_align_plan)
  DevBuf estws;   // casr_lm_estimate: the counting tables (lm_estimate_plan.h est_carve)
  DevBuf prunews; // casr_lm_prune: the per-slot arrays and the dense result (lm_prune_plan.h lmp_carve)
  DevBuf cnws;    // casr_confusion, casr_beam_nbest, casr_beam_confusion: lists, units, votes (carve_confusion)
  // hipGraph replay of the launch-bound loops (per-layer recurrence, decode loop)
  // casr_set_graphs bits: 1 = the decode loop replays as a hipGraph, 2 = the per-step recurrence
  // fallback does.  Default 2: the decode loop launches eagerly (measured faster)
  int graph_mode = CASR_GRAPHS_RECURRENCE;
  hipStream_t cap = nullptr;      // capture stream
  hipStream_t xs[2] = {};         // replay streams, fenced to the caller's stream by events
  hipEvent_t ev_in = nullptr, ev_out[2] = {};
  GraphCache graphs;
  Tuning tune;  // casr_set_option
};

// An immutable backoff n-gram LM (ngram_table.h): the host tables, and for device >= 0 their copy on
// that device, which any number of handles there may read.
struct casr_lm {
  int device = -1;
  NgramTables host;
  NgramSuccTables succ;  // the successor lists (ngram_succ.h): casr_lm_terms, casr_beam_lm
  int64_t count[NGRAM_MAX_ORDER] = {};  // n-grams per order as given (casr_lm_prune's size plan)
  bool unk_given = false;               // the <unk> unigram was given, not defaulted
  void* dev[11] = {};    // uni, redirect, tab[0..2]; succ: list[0..2], dir, ctab[0..1]
  NgramView dview{};
  NgramSuccView dsucc{};
};

// An immutable phrase automaton (bias_plan.h): the host tables, and for device >= 0 their copy there.
struct casr_bias {
  int device = -1;
  BiasTables host;
  void* dev[5] = {};  // node, ctok, cnext, root_next, root_gain
  BiasView dview{};
};

struct casr_grammar {
  int device = -1;
  GrammarTables host;
  void* dev[6] = {};  // arc_off, arc_tok, arc_next, arc_dist, dist, is_final
  GrammarView dview{};
};

static int fail(casr_handle* h, int code, const char* fmt, ...);

// the handle's guard words (allocated and zeroed on first use; the caller has set the device)
static int32_t* guard_words(casr_handle* h) {
  if (!h->gflags.p) {
    if (h->gflags.ensure(64) != hipSuccess) return nullptr;
    if (hipMemset(h->gflags.p, 0, 64) != hipSuccess) {
      h->gflags.release();
      return nullptr;
    }
  }
  return h->gflags.as<int32_t>();
}
#define GUARD(h, i) (guard_words(h) + (i))

// Capture `body(stream)` once per key into a hipGraph on the handle's private capture stream,
// then replay it on the private replay stream, ordered after everything already enqueued on
// the caller's stream and before anything enqueued there afterwards (event fences both
// ways; the caller's stream may be the legacy null stream, which a graph is not launched on).
template <class Body>
static hipError_t get_graph(casr_handle* h, const std::vector<uint64_t>& key, Body&& body,
                            hipGraphExec_t* out) {
  hipError_t e;
  if (!h->cap) {
    e = hipStreamCreateWithFlags(&h->cap, hipStreamNonBlocking);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipStreamCreateWithFlags(&h->xs[i], hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&h->ev_out[i], hipEventDisableTiming);
    if (e != hipSuccess) return e;
  }
  hipGraphExec_t exec = h->graphs.find(key);
  if (!exec) {
    e = hipStreamBeginCapture(h->cap, hipStreamCaptureModeRelaxed);
    if (e != hipSuccess) return e;
    hipError_t eb = body(h->cap);
    hipGraph_t g = nullptr;
    e = hipStreamEndCapture(h->cap, &g);
    if (eb != hipSuccess) e = eb;
    if (e == hipSuccess) e = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
    if (g) (void)hipGraphDestroy(g);
    if (e != hipSuccess) return e;
    h->graphs.add(key, exec);
  }
  *out = exec;
  return hipSuccess;
}

// Replay n (<= 2) graphs concurrently, graph i on replay stream i, all after the work already
// on `s` and before anything enqueued on `s` afterwards.
static hipError_t launch_graphs(casr_handle* h, const hipGraphExec_t* ex, int n, hipStream_t s) {
  hipError_t e = hipEventRecord(h->ev_in, s);
  for (int i = 0; i < n && e == hipSuccess; ++i) {
    e = hipStreamWaitEvent(h->xs[i], h->ev_in, 0);
    if (e == hipSuccess) e = hipGraphLaunch(ex[i], h->xs[i]);
    if (e == hipSuccess) e = hipEventRecord(h->ev_out[i], h->xs[i]);
  }
  for (int i = 0; i < n && e == hipSuccess; ++i) e = hipStreamWaitEvent(s, h->ev_out[i], 0);
  return e;
}

template <class Body>
static hipError_t run_graph(casr_handle* h, const std::vector<uint64_t>& key, hipStream_t s, Body&& body) {
  hipGraphExec_t exec = nullptr;
  hipError_t e = get_graph(h, key, body, &exec);
  return e == hipSuccess ? launch_graphs(h, &exec, 1, s) : e;
}

static int fail(casr_handle* h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (h) h->err = buf;
  g_err = buf;
  return code;
}

#define HIP_OK(h, expr)                                                                \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail((h), CASR_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_),   \
                  __FILE__, __LINE__);                                                 \
  } while (0)

static int check_config(const casr_config* c) {
  if (!c) return fail(nullptr, CASR_ERR_ARG, "config is NULL");
  if (c->n_mels != F || c->feat_dim != D || c->enc_hidden != H || c->dec_hidden != HD ||
      c->embed_dim != E || c->attn_size != A)
    return fail(nullptr, CASR_ERR_UNSUPPORTED,
                "this build implements n_mels=80 feat_dim=720 enc_hidden=256 dec_hidden=512 "
                "embed_dim=256 attn_size=128 (got %d %d %d %d %d %d)",
                c->n_mels, c->feat_dim, c->enc_hidden, c->dec_hidden, c->embed_dim, c->attn_size);
  if (c->enc_layers < 1 || c->enc_layers > CASR_MAX_LAYERS || c->vocab < 4 || c->max_len < 1 ||
      c->sos < 0 || c->sos >= c->vocab || c->eos < 0 || c->eos >= c->vocab || !(c->temperature > 0.f))
    return fail(nullptr, CASR_ERR_ARG, "invalid config (layers=%d vocab=%d max_len=%d)",
                c->enc_layers, c->vocab, c->max_len);
  return CASR_OK;
}

extern "C" {

int casr_api_version(void) { return CASR_API_VERSION; }

size_t casr_packed_weights_floats(const casr_config* cfg) {
  if (check_config(cfg) != CASR_OK) return 0;
  return make_layout(*cfg).total;
}

int casr_pack_weights(const casr_config* cfg, const casr_weights_host* w, float* out) {
  int rc = check_config(cfg);
  if (rc) return rc;
  if (!w || !out) return fail(nullptr, CASR_ERR_ARG, "weights/out is NULL");
  const Layout L = make_layout(*cfg);
  // the s16x3 images need every MFMA weight inside the f16 range with room to spare; blob word
  // L.info records whether they are usable (casr_bind_weights reads it)
  // (the input projection's images need |w| < 16: gemm16.hip scales w_hi by 2^11 in f16)
  auto in_range = [](const float* p, size_t n, float lim = 16384.f) {
    for (size_t i = 0; i < n; ++i)
      if (!(std::fabs(p[i]) < lim)) return false;
    return true;
  };
  bool s16_ok = true;
  for (int l = 0; l < cfg->enc_layers; ++l)
    for (int d = 0; d < 2; ++d)
      if (w->enc_w_ih[l][d] && w->enc_w_hh[l][d] &&
          (!in_range(w->enc_w_ih[l][d], (size_t)4 * H * (l == 0 ? D : C), 16.f) ||
           !in_range(w->enc_w_hh[l][d], (size_t)4 * H * H)))
        s16_ok = false;
  if (w->embedding && w->dec_w_ih && w->dec_w_hh && w->proj_w &&
      (!in_range(w->embedding, (size_t)cfg->vocab * E) || !in_range(w->dec_w_ih, (size_t)4 * HD * (E + C)) ||
       !in_range(w->dec_w_hh, (size_t)4 * HD * HD) || !in_range(w->proj_w, (size_t)cfg->vocab * KPROJ)))
    s16_ok = false;
  // keys GEMM (encoder.hip gemm_nt_kernel<KeysEpi, true>): two accumulators, no 2^11 scaling of
  // w_hi, so the f16 range limit of the other s16 images applies
  if (w->attn_w_enc && !in_range(w->attn_w_enc, (size_t)C * A)) s16_ok = false;
  std::memset(out, 0, L.total * sizeof(float));
  out[L.info] = s16_ok ? 1.f : 0.f;
  // info word 4: every projection weight below 16 in magnitude, so w_hi 2^11 is an f16 and the
  // beam projection can run its one-accumulator s16x3 form (decoder.hip dgemm_kernel ONE)
  out[L.info + 4] = (w->proj_w && in_range(w->proj_w, (size_t)cfg->vocab * KPROJ, 16.f)) ? 1.f : 0.f;
  // info word 5: every decoder LSTM weight below 16 in magnitude: with word 4 the folded beam step's
  // fused GEMM (projection | LSTM gates) can run the one-accumulator form (decoder.hip FoldEpi)
  out[L.info + 5] = (w->dec_w_ih && w->dec_w_hh && in_range(w->dec_w_ih, (size_t)4 * HD * (E + C), 16.f) &&
                     in_range(w->dec_w_hh, (size_t)4 * HD * HD, 16.f))
                        ? 1.f
                        : 0.f;
  // layout stamp: casr_bind_weights refuses a blob packed by a build with another layout
  const uint32_t stamp[3] = {LAYOUT_MAGIC, (uint32_t)(L.total & 0xFFFFFFFFu), (uint32_t)(L.total >> 32)};
  std::memcpy(out + L.info + 1, stamp, sizeof stamp);
  const int V = cfg->vocab;
  for (int l = 0; l < cfg->enc_layers; ++l) {
    const int din = l == 0 ? D : C;
    for (int d = 0; d < 2; ++d)
      if (!w->enc_w_ih[l][d] || !w->enc_w_hh[l][d] || !w->enc_b_ih[l][d] || !w->enc_b_hh[l][d])
        return fail(nullptr, CASR_ERR_ARG, "encoder layer %d dir %d: NULL tensor", l, d);
    // input projection rows: d*4H + packed(g, u) <- W_ih_d[g*H + u]
    for (int d = 0; d < 2; ++d)
      for (int g = 0; g < 4; ++g)
        for (int u = 0; u < H; ++u) {
          const int pr = d * 4 * H + enc_gate_col(g, u);
          const int orow = g * H + u;
          std::memcpy(out + L.enc_wih[l] + (size_t)pr * din, w->enc_w_ih[l][d] + (size_t)orow * din,
                      sizeof(float) * din);
          out[L.enc_bias[l] + pr] = w->enc_b_ih[l][d][orow] + w->enc_b_hh[l][d][orow];
        }
    // recurrent matrices, fragment-major per direction: n-tile (jb*4 + g) = gate g of units
    // jb*16 .. jb*16+15
    for (int d = 0; d < 2; ++d) {
      const float* Whh = w->enc_w_hh[l][d];
      auto whh = [&](int n, int k) {
        const int jb = n / 64, g = (n / 16) % 4, u = jb * 16 + (n % 16);
        return Whh[(size_t)(g * H + u) * H + k];
      };
      pack_frag(out + L.enc_whh[l] + (size_t)d * 4 * H * H, 4 * H / 16, H / 64, whh);
      pack_frag16(out + L.enc_whh16[l] + (size_t)d * 4 * H * H, 4 * H / 16, H / 64, whh);
    }
    const float* wih = out + L.enc_wih[l];
    pack_rows16(out + L.enc_wih16[l], 8 * H, din, [&](int n, int k) { return wih[(size_t)n * din + k]; });
  }
  if (!w->embedding || !w->dec_w_ih || !w->dec_w_hh || !w->dec_b_ih || !w->dec_b_hh || !w->proj_w ||
      !w->proj_b || !w->attn_w_enc || !w->attn_b || !w->attn_w_hidden || !w->attn_v)
    return fail(nullptr, CASR_ERR_ARG, "decoder/attention: NULL tensor");
  std::memcpy(out + L.emb, w->embedding, sizeof(float) * (size_t)V * E);
  {
    uint16_t* e16 = reinterpret_cast<uint16_t*>(out + L.emb16);
    for (size_t i = 0; i < (size_t)V * E; ++i) split16_host(w->embedding[i], e16[2 * i], e16[2 * i + 1]);
  }
  // decoder LSTM: K order [emb | ctx | h] = [W_ih | W_hh]
  auto decw = [&](int n, int k) {
    const int jb = n / 64, g = (n / 16) % 4, u = jb * 16 + (n % 16);
    const int orow = g * HD + u;
    return k < E + C ? w->dec_w_ih[(size_t)orow * (E + C) + k] : w->dec_w_hh[(size_t)orow * HD + (k - E - C)];
  };
  pack_frag(out + L.dec_w, 4 * HD / 16, KDEC / 64, decw);
  pack_frag16(out + L.dec_w16, 4 * HD / 16, KDEC / 64, decw);
  for (int g = 0; g < 4; ++g)
    for (int u = 0; u < HD; ++u)
      out[L.dec_b + packed_gate_row(g, u)] = w->dec_b_ih[g * HD + u] + w->dec_b_hh[g * HD + u];
  // projection: reference input is cat([h, ctx]) (decoder.py:131); packed K order [ctx | h]
  auto projw = [&](int n, int k) {
    if (n >= V) return 0.f;
    return k < C ? w->proj_w[(size_t)n * KPROJ + HD + k] : w->proj_w[(size_t)n * KPROJ + (k - C)];
  };
  pack_frag(out + L.proj_w, L.VP / 16, KPROJ / 64, projw);
  pack_frag16(out + L.proj_w16, L.VP / 16, KPROJ / 64, projw);
  for (int n = 0; n < V; ++n) out[L.proj_b + n] = w->proj_b[n];
  for (int a = 0; a < A; ++a)
    for (int c = 0; c < C; ++c) out[L.wencT + (size_t)a * C + c] = w->attn_w_enc[(size_t)c * A + a];
  pack_rows16(out + L.wenc16, A, C, [&](int n, int k) { return out[L.wencT + (size_t)n * C + k]; });
  std::memcpy(out + L.b_attn, w->attn_b, sizeof(float) * A);
  std::memcpy(out + L.w_hidden, w->attn_w_hidden, sizeof(float) * HD * A);
  std::memcpy(out + L.v, w->attn_v, sizeof(float) * A);
  return CASR_OK;
}

int casr_create(const casr_config* cfg, int device, casr_handle** out) {
  if (!out) return fail(nullptr, CASR_ERR_ARG, "out is NULL");
  *out = nullptr;
  int rc = check_config(cfg);
  if (rc) return rc;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0)
    return fail(nullptr, CASR_ERR_HIP, "no HIP device available (%s)", hipGetErrorString(e));
  if (device < 0 || device >= n) return fail(nullptr, CASR_ERR_ARG, "device %d out of range", device);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, CASR_ERR_UNSUPPORTED, "device %d is %s; this library is built for gfx950",
                device, prop.gcnArchName);
  auto* h = new casr_handle();
  h->cfg = *cfg;
  h->L = make_layout(*cfg);
  h->device = device;
  // the device's facts, once per handle; the caller's current device is restored
  int cur = -1;
  e = hipGetDevice(&cur);
  if (e == hipSuccess) e = hipSetDevice(device);
  if (e == hipSuccess) {
    h->dev = read_device_facts();
    if (cur != device) e = hipSetDevice(cur);
  }
  if (e != hipSuccess) {
    delete h;
    return fail(nullptr, CASR_ERR_HIP, "casr_create: device %d: %s", device, hipGetErrorString(e));
  }
  *out = h;
  return CASR_OK;
}

int casr_bind_weights(casr_handle* h, const float* packed_device) {
  if (!h || !packed_device) return fail(h, CASR_ERR_ARG, "handle/weights NULL");
  HIP_OK(h, hipSetDevice(h->device));
  float info[6] = {};
  HIP_OK(h, hipMemcpy(info, packed_device + h->L.info, sizeof info, hipMemcpyDeviceToHost));
  uint32_t stamp[3];
  std::memcpy(stamp, info + 1, sizeof stamp);
  if (stamp[0] != LAYOUT_MAGIC || stamp[1] != (uint32_t)(h->L.total & 0xFFFFFFFFu) ||
      stamp[2] != (uint32_t)(h->L.total >> 32))
    return fail(h, CASR_ERR_ARG,
                "casr_bind_weights: the blob was not packed by this build's layout (stamp %08x, %u floats; "
                "expected %08x, %zu floats)", stamp[0], stamp[1], LAYOUT_MAGIC, h->L.total);
  h->s16_valid = info[0] == 1.f;
  h->proj_small = info[4] == 1.f;
  h->dec_small = info[5] == 1.f;
  h->W = packed_device;
  h->graphs.clear();  // captured graphs bake in the precision and weight pointers
  // the folded step's tables (decoder.hip build_fold): derived from this blob, so rebuilt at every
  // bind; the gate table always, the s16 fused image and the s16 query image only from a blob with
  // valid s16 images.  The f32 fused image (29 MB, read only by the greedy fold under the exact-f32
  // arithmetic) is built by the first such decode (ensure_fold32)
  h->fold_ready = h->fold32_ready = false;
  {
    const int V = h->cfg.vocab;
    HIP_OK(h, h->egates.ensure((size_t)V * 4 * HD * sizeof(float)));
    if (h->s16_valid) {
      HIP_OK(h, h->wfold.ensure(fold_image_bytes(V)));
      HIP_OK(h, h->wq16.ensure(FOLD_WQ16_FLOATS * sizeof(float)));
    }
    HIP_OK(h, build_fold(h->W, h->L, V, h->s16_valid ? h->wfold.as<float>() : nullptr, h->egates.as<float>(),
                         h->s16_valid ? h->wq16.as<float>() : nullptr, nullptr, nullptr));
    HIP_OK(h, hipStreamSynchronize(nullptr));
    h->fold_ready = h->s16_valid;
  }
  if (h->s16_valid) {  // 16-k-block-major copies of the input-projection weight images
    size_t tot = 0;
    for (int l = 0; l < h->cfg.enc_layers; ++l) {
      h->wih16km_off[l] = tot;
      tot += (size_t)8 * H * s16_kpad(l == 0 ? D : C);
    }
    HIP_OK(h, h->wih16km.ensure(tot * sizeof(float)));
    for (int l = 0; l < h->cfg.enc_layers; ++l)
      HIP_OK(h, launch_relayout_km16(h->W + h->L.enc_wih16[l], 8 * H, s16_kpad(l == 0 ? D : C),
                                     h->wih16km.as<float>() + h->wih16km_off[l], nullptr));
    HIP_OK(h, hipStreamSynchronize(nullptr));
  }
  return CASR_OK;
}

// the f32 fused image of the folded greedy step under the exact-f32 arithmetic, built once per bind
// by the first decode that needs it (on the null stream, synchronised: a decode's captured graph
// never contains the build)
static int ensure_fold32(casr_handle* h) {
  if (h->fold32_ready) return CASR_OK;
  const int V = h->cfg.vocab;
  HIP_OK(h, h->wfold32.ensure(fold_image_bytes(V)));
  HIP_OK(h, build_fold(h->W, h->L, V, nullptr, nullptr, nullptr, h->wfold32.as<float>(), nullptr));
  HIP_OK(h, hipStreamSynchronize(nullptr));
  h->fold32_ready = true;
  return CASR_OK;
}

int casr_set_precision(casr_handle* h, int precision) {
  if (!h) return fail(h, CASR_ERR_ARG, "handle NULL");
  if (precision != CASR_PREC_F32 && precision != CASR_PREC_S16X3 && precision != CASR_PREC_S16X1)
    return fail(h, CASR_ERR_ARG, "unknown precision %d", precision);
  if (precision != CASR_PREC_F32 && precision != CASR_PREC_S16)
    return fail(h, CASR_ERR_UNSUPPORTED, "this build computes %s; %s is the %s build", CASR_S16_ONE ? "s16x1" : "s16x3",
                CASR_S16_ONE ? "s16x3" : "s16x1", CASR_S16_ONE ? "libcasr_hip.so" : "libcasr_hip_s16x1.so");
  h->precision = precision;
  return CASR_OK;
}

int casr_get_precision(const casr_handle* h) {
  if (!h) return -1;
  return h->s16() ? CASR_PREC_S16 : CASR_PREC_F32;
}

void casr_destroy(casr_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  // work enqueued on any stream may still read the handle's buffers (a persistent recurrence
  // layer, a decode loop on the caller's stream, a graph replay on the private streams): drain
  // the device before graphs, streams and buffers go away
  (void)hipDeviceSynchronize();
  h->graphs.clear();
  if (h->cap) (void)hipStreamDestroy(h->cap);
  for (int i = 0; i < 2; ++i) {
    if (h->xs[i]) (void)hipStreamDestroy(h->xs[i]);
    if (h->ev_out[i]) (void)hipEventDestroy(h->ev_out[i]);
  }
  if (h->ev_in) (void)hipEventDestroy(h->ev_in);
  for (DevBuf* b : {&h->gin, &h->out0, &h->out1, &h->hbuf, &h->cst, &h->hfin, &h->keysT, &h->lens, &h->feat, &h->fstat, &h->hx, &h->x16, &h->gflags, &h->fe_const,
                    &h->st, &h->logits, &h->small, &h->bp, &h->tk, &h->rec, &h->gout, &h->wfold, &h->wfold32, &h->coldbuf,
                    &h->egates, &h->fgates, &h->wq16, &h->wih16km, &h->ksbuf, &h->asbuf, &h->scorebuf, &h->cvt_peak,
                    &h->seg_q, &h->seg_hist, &h->lmws, &h->mbrws, &h->eaws, &h->biasws, &h->cnws, &h->gramws, &h->estws, &h->prunews})
    b->release();
  for (casr_handle::ResampleTable* t : h->rs_tables) {
    t->dev.release();
    delete t;
  }
  delete h;
}

int casr_set_graphs(casr_handle* h, int enable) {
  if (!h) return fail(h, CASR_ERR_ARG, "handle NULL");
  if (enable < 0 || enable > 3) return fail(h, CASR_ERR_ARG, "casr_set_graphs: mode %d not in [0, 3]", enable);
  h->graph_mode = enable;
  return CASR_OK;
}

int casr_set_persistent(casr_handle* h, int enable) {
  if (!h) return fail(h, CASR_ERR_ARG, "handle NULL");
  h->use_persistent = enable != 0;
  return CASR_OK;
}

// (the persistent recurrence needs every workgroup of its grid resident at once: plan_recurrence)
int casr_recurrence_mode(const casr_handle* h, int B) {
  if (!h || B <= 0) return -1;
  return plan_recurrence(B, 1, h->tune, h->s16(), false, h->use_persistent, h->dev).persistent;
}

int casr_set_option(casr_handle* h, int option, int value) {
  if (!h) return fail(h, CASR_ERR_ARG, "handle NULL");
  if (option < 0 || option >= CASR_OPT_COUNT) return fail(h, CASR_ERR_ARG, "unknown option %d", option);
  if (!option_value_ok(option, value))
    return fail(h, CASR_ERR_ARG, "CASR_OPT_%s: value %d not in [%d, %d]%s", OPTIONS[option].name, value, OPTIONS[option].lo,
                OPTIONS[option].hi, option == CASR_OPT_ATTN_KPB ? ": 0 (auto), 4 or 8" : "");
  if (option == CASR_OPT_DIAG_COLD) {
    if (value) {
      HIP_OK(h, hipSetDevice(h->device));
      HIP_OK(h, h->coldbuf.ensure((size_t)1 << 30));
      HIP_OK(h, hipMemset(h->coldbuf.p, 0, (size_t)1 << 30));
    }
    h->prof.cold_buf = h->coldbuf.p;
    h->prof.cold_bytes = (size_t)1 << 30;
    h->prof.cold_mask = (uint32_t)value;
  }
  h->tune.v[option] = value;
  return CASR_OK;
}

int casr_get_option(const casr_handle* h, int option, int32_t* value) {
  if (!h || !value || option < 0 || option >= CASR_OPT_COUNT)
    return fail(nullptr, CASR_ERR_ARG, "casr_get_option: bad arguments");
  *value = h->tune[option];
  return CASR_OK;
}

const char* casr_last_error(const casr_handle* h) { return h ? h->err.c_str() : g_err.c_str(); }

int casr_features(casr_handle* h, const float* fbank, const int32_t* frames, int B, int T, float eps,
                  float* feat, int32_t* feat_len, void* stream) {
  if (!h || !fbank || !frames || !feat || !feat_len || B <= 0 || T < 3)
    return fail(h, CASR_ERR_ARG, "casr_features: bad arguments (B=%d T=%d)", B, T);
  HIP_OK(h, hipSetDevice(h->device));
  ProfScope ps(&h->prof, CASR_K_FEATURES, (hipStream_t)stream);
  HIP_OK(h, h->fstat.ensure((size_t)B * 2 * D * sizeof(float)));
  HIP_OK(h, launch_features(feature_path(T, false), fbank, frames, B, T, eps, feat, feat_len, h->fstat.as<float>(),
                            (hipStream_t)stream));
  return CASR_OK;
}

int casr_log_mel_frames(int n_samples) { return frontend_frames(n_samples); }

int casr_mel_filterbank(int n_stft, float f_min, float f_max, int n_mels, float* fb_host) {
  if (n_stft < 2 || n_mels < 1 || !fb_host || !(f_max > f_min))
    return fail(nullptr, CASR_ERR_ARG, "casr_mel_filterbank: bad arguments");
  mel_filterbank(n_stft, f_min, f_max, n_mels, fb_host);
  return CASR_OK;
}

int casr_log_mel(casr_handle* h, const float* wav, const int32_t* n_samples, int B, int n_max, int t_max,
                 float preemphasis, float* fbank, int32_t* frames, void* stream) {
  if (!h || !wav || !n_samples || !fbank || !frames || B <= 0 || n_max <= 0 || t_max <= 0)
    return fail(h, CASR_ERR_ARG, "casr_log_mel: bad arguments");
  // the reference skips the filter there and keeps all n samples (data.py:201-202): another
  // operation (no one-sample shift, another frame count) than y[m] = x[m+1] - pre x[m]
  if (!(preemphasis > 0.f))
    return fail(h, CASR_ERR_ARG,
                "casr_log_mel: preemphasis %g <= 0 is the reference's unfiltered form (data.py:201-202), "
                "which is not implemented",
                (double)preemphasis);
  if (t_max < frontend_frames(n_max))
    return fail(h, CASR_ERR_ARG, "casr_log_mel: t_max %d < %d frames of n_max %d samples", t_max,
                frontend_frames(n_max), n_max);
  if ((size_t)n_max * B > (size_t)1 << 40) return fail(h, CASR_ERR_ARG, "casr_log_mel: batch too large");
  HIP_OK(h, hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  if (!h->fe_const.p) {
    FrontendConst c;
    build_frontend_const(&c);
    HIP_OK(h, h->fe_const.ensure(sizeof(FrontendConst)));
    HIP_OK(h, hipMemcpy(h->fe_const.p, &c, sizeof c, hipMemcpyHostToDevice));
  }
  if (!guard_words(h)) return fail(h, CASR_ERR_HIP, "casr_log_mel: guard words not allocated");
  ProfScope ps(&h->prof, CASR_K_FEATURES, s);
  HIP_OK(h, launch_log_mel(wav, n_samples, B, n_max, t_max, preemphasis, h->fe_const.as<FrontendConst>(), fbank,
                           frames, GUARD(h, 2), s, h->tune[CASR_OPT_LOGMEL_Q16]));
  return CASR_OK;
}

// the plan of a rate, or the error casr_convert_audio and the host-only entry points report for it
static int resample_plan_checked(casr_handle* h, const char* who, int rate_in, ResamplePlan* p) {
  switch (resample_plan(rate_in, p)) {
    case RS_OK: return CASR_OK;
    case RS_BAD_RATE:
      return fail(h, CASR_ERR_UNSUPPORTED, "%s: rate %d Hz outside [%d, %d]", who, rate_in, RS_RATE_MIN, RS_RATE_MAX);
    default:
      return fail(h, CASR_ERR_UNSUPPORTED,
                  "%s: rate %d Hz needs L = %d phases x %d taps = %zu table floats > %d (M = %d)", who, rate_in, p->L,
                  p->taps, p->table_floats(), RS_TABLE_MAX, p->M);
  }
}

int casr_resample_plan(int rate_in, int32_t* L, int32_t* M, int32_t* taps) {
  if (!L || !M || !taps) return fail(nullptr, CASR_ERR_ARG, "casr_resample_plan: NULL output");
  ResamplePlan p;
  const int rc = resample_plan_checked(nullptr, "casr_resample_plan", rate_in, &p);
  if (rc != CASR_OK) return rc;
  *L = p.L;
  *M = p.M;
  *taps = p.taps;
  return CASR_OK;
}

int casr_resample_filter(int rate_in, float* table_host) {
  if (!table_host) return fail(nullptr, CASR_ERR_ARG, "casr_resample_filter: NULL output");
  ResamplePlan p;
  const int rc = resample_plan_checked(nullptr, "casr_resample_filter", rate_in, &p);
  if (rc != CASR_OK) return rc;
  resample_filter(p, table_host);
  return CASR_OK;
}

int casr_resample_frames(int n_in, int rate_in) {
  ResamplePlan p;
  if (resample_plan(rate_in, &p) != RS_OK) return -1;
  const int64_t n = resample_frames(n_in, p);
  return n > INT32_MAX ? -1 : (int)n;
}

// the handle's table of a rate: cached, or built now (host, double -> f32) and uploaded on `s`
static int resample_table(casr_handle* h, const ResamplePlan& p, hipStream_t s, const float** tab) {
  for (casr_handle::ResampleTable* t : h->rs_tables)
    if (t->plan.rate == p.rate) {
      *tab = t->dev.as<float>();
      return CASR_OK;
    }
  if (h->rs_tables.size() >= casr_handle::RS_CACHE) {
    // the oldest goes: hipFree waits for the device, so no enqueued kernel or upload still reads it
    casr_handle::ResampleTable* old = h->rs_tables.front();
    old->dev.release();
    delete old;
    h->rs_tables.erase(h->rs_tables.begin());
  }
  casr_handle::ResampleTable* t = new casr_handle::ResampleTable;
  t->plan = p;
  t->host.resize(p.table_floats());
  resample_filter(p, t->host.data());
  hipError_t e = t->dev.ensure(t->host.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpyAsync(t->dev.p, t->host.data(), t->host.size() * sizeof(float), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) {
    t->dev.release();
    delete t;
    return fail(h, CASR_ERR_HIP, "casr_convert_audio: table of %d Hz: %s", p.rate, hipGetErrorString(e));
  }
  h->rs_tables.push_back(t);
  *tab = t->dev.as<float>();
  return CASR_OK;
}

int casr_convert_audio(casr_handle* h, const float* pcm, const int32_t* n_in, int B, int n_max_in, int channels,
                       int rate_in, int m_max, int quantize, float norm_db, float* wav, int32_t* n_out, float* gain,
                       void* stream) {
  if (!h || !pcm || !n_in || !wav || !n_out)
    return fail(h, CASR_ERR_ARG, "casr_convert_audio: NULL handle, pcm, n_in, wav or n_out");
  if (B <= 0 || B > 65535 || n_max_in <= 0 || m_max <= 0 || m_max > INT32_MAX - RS_TILE)
    return fail(h, CASR_ERR_ARG, "casr_convert_audio: bad shape (B=%d n_max_in=%d m_max=%d)", B, n_max_in, m_max);
  if (channels < 1 || channels > RS_CH_MAX)
    return fail(h, CASR_ERR_ARG, "casr_convert_audio: %d channels not in [1, %d]", channels, RS_CH_MAX);
  ResamplePlan p;
  const int rc = resample_plan_checked(h, "casr_convert_audio", rate_in, &p);
  if (rc != CASR_OK) return rc;
  if ((int64_t)m_max < resample_frames(n_max_in, p))
    return fail(h, CASR_ERR_ARG, "casr_convert_audio: m_max %d < %lld outputs of n_max_in %d frames at %d Hz", m_max,
                (long long)resample_frames(n_max_in, p), n_max_in, rate_in);
  if (resample_lds_bytes(p) > 64 * 1024 - 256)  // (the kernel's few static words on top)
    return fail(h, CASR_ERR_UNSUPPORTED, "casr_convert_audio: rate %d Hz needs %zu B of LDS per tile > 64 KiB", rate_in,
                resample_lds_bytes(p));
  HIP_OK(h, hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  if (!guard_words(h)) return fail(h, CASR_ERR_HIP, "casr_convert_audio: guard words not allocated");
  const bool norm = norm_db < 0.f;  // >= 0 (or NaN) switches stage (d) off
  ConvertArgs a{};
  a.tab = nullptr;
  if (p.L != p.M) {
    const int rt = resample_table(h, p, s, &a.tab);
    if (rt != CASR_OK) return rt;
  }
  if (norm) HIP_OK(h, h->cvt_peak.ensure((size_t)B * RS_PEAK_STRIDE * sizeof(uint32_t)));
  a.pcm = pcm;
  a.n_in = n_in;
  a.n_max_in = n_max_in;
  a.ch = channels;
  a.m_max = m_max;
  a.inv_ch = 1.0f / (float)channels;
  a.L = p.L;
  a.M = p.M;
  a.K = p.K;
  a.taps = p.taps;
  a.quantize = quantize != 0;
  a.norm = norm;
  a.wav = wav;
  a.n_out = n_out;
  a.gain = gain;
  a.peak = h->cvt_peak.as<uint32_t>();
  a.err = GUARD(h, 2);
  const double lin = std::pow(10.0, (double)norm_db / 20.0);
  const float target = norm ? (float)(a.quantize ? 32768.0 * lin : lin) : 1.f;
  HIP_OK(h, launch_convert(a, B, p, target, s));
  return CASR_OK;
}

int casr_segment_default_params(casr_segment_params* p) {
  if (!p) return fail(nullptr, CASR_ERR_ARG, "casr_segment_default_params: NULL");
  *p = segment_default_params();
  return CASR_OK;
}

int casr_segment_bound(int T, const casr_segment_params* p) { return p ? (int)segment_bound(T, *p) : -1; }

static int segment_params_checked(casr_handle* h, const char* who, const casr_segment_params* p) {
  if (!p) return fail(h, CASR_ERR_ARG, "%s: NULL parameters", who);
  if (!segment_params_valid(*p))
    return fail(h, CASR_ERR_ARG,
                "%s: invalid parameters (max_frames %d min_frames %d min_pause %d min_speech %d pad %d max_gap %d "
                "pct_lo %d pct_hi %d rel_q8 %d rise_min %d)",
                who, p->max_frames, p->min_frames, p->min_pause, p->min_speech, p->pad, p->max_gap, p->pct_lo,
                p->pct_hi, p->rel_q8, p->rise_min);
  return CASR_OK;
}

int casr_segment_host(const float* fbank, const int32_t* frames, int B, int T, int n_mels,
                      const casr_segment_params* p, int s_max, int32_t* seg_start, int32_t* seg_len, int32_t* n_seg,
                      int32_t* thr) {
  const int rc = segment_params_checked(nullptr, "casr_segment_host", p);
  if (rc != CASR_OK) return rc;
  if (B < 0 || T < 0 || s_max < 0 || (B > 0 && (!frames || !n_seg)) || (B > 0 && T > 0 && !fbank) ||
      (B > 0 && s_max > 0 && (!seg_start || !seg_len)))
    return fail(nullptr, CASR_ERR_ARG, "casr_segment_host: NULL pointer or bad shape (B=%d T=%d s_max=%d)", B, T, s_max);
  if (n_mels <= 0 || n_mels % SEG_LANES)
    return fail(nullptr, CASR_ERR_UNSUPPORTED, "casr_segment_host: n_mels %d is not a positive multiple of %d", n_mels,
                SEG_LANES);
  for (int b = 0; b < B; ++b)
    if (frames[b] < 0 || frames[b] > T)
      return fail(nullptr, CASR_ERR_ARG, "casr_segment_host: frames[%d] = %d not in [0, %d]", b, frames[b], T);
  for (int b = 0; b < B; ++b)
    segment_row_host(fbank + (size_t)b * T * n_mels, frames[b], n_mels, *p, s_max,
                     seg_start + (size_t)b * s_max, seg_len + (size_t)b * s_max, n_seg + b, thr ? thr + b : nullptr);
  return CASR_OK;
}

int casr_segment(casr_handle* h, const float* fbank, const int32_t* frames, int B, int T,
                 const casr_segment_params* p, int s_max, int32_t* seg_start, int32_t* seg_len, int32_t* n_seg,
                 int32_t* thr, void* stream) {
  if (!h || !fbank || !frames || !n_seg || (s_max > 0 && (!seg_start || !seg_len)))
    return fail(h, CASR_ERR_ARG, "casr_segment: NULL handle, fbank, frames, n_seg, seg_start or seg_len");
  if (B <= 0 || B > 65535 || T <= 0 || T > INT32_MAX - 65536 || s_max < 0)
    return fail(h, CASR_ERR_ARG, "casr_segment: bad shape (B=%d T=%d s_max=%d)", B, T, s_max);
  const int rc = segment_params_checked(h, "casr_segment", p);
  if (rc != CASR_OK) return rc;
  if (h->cfg.n_mels % SEG_LANES)
    return fail(h, CASR_ERR_UNSUPPORTED, "casr_segment: n_mels %d is not a multiple of %d", h->cfg.n_mels, SEG_LANES);
  HIP_OK(h, hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  if (!guard_words(h)) return fail(h, CASR_ERR_HIP, "casr_segment: guard words not allocated");
  HIP_OK(h, h->seg_q.ensure((size_t)B * T * sizeof(uint16_t)));
  HIP_OK(h, h->seg_hist.ensure((size_t)B * SEG_BINS * sizeof(uint32_t)));
  SegmentArgs a{};
  a.fbank = fbank;
  a.frames = frames;
  a.B = B;
  a.T = T;
  a.n_mels = h->cfg.n_mels;
  a.s_max = s_max;
  a.p = *p;
  a.seg_start = seg_start;
  a.seg_len = seg_len;
  a.n_seg = n_seg;
  a.thr = thr;
  a.q = h->seg_q.as<uint16_t>();
  a.hist = h->seg_hist.as<uint32_t>();
  a.err = GUARD(h, 2);
  HIP_OK(h, launch_segment(a, s));
  return CASR_OK;
}

int casr_gather_segments(casr_handle* h, const float* fbank, int B, int T, const int32_t* seg_src,
                         const int32_t* seg_start, const int32_t* seg_len, int S, int t_seg, float* out,
                         int32_t* frames_out, void* stream) {
  if (!h || !fbank || !seg_src || !seg_start || !seg_len || !out || !frames_out)
    return fail(h, CASR_ERR_ARG, "casr_gather_segments: NULL argument");
  if (B <= 0 || T <= 0 || S <= 0 || t_seg <= 0)
    return fail(h, CASR_ERR_ARG, "casr_gather_segments: bad shape (B=%d T=%d S=%d t_seg=%d)", B, T, S, t_seg);
  if (((uintptr_t)fbank | (uintptr_t)out) & 15)
    return fail(h, CASR_ERR_ARG, "casr_gather_segments: fbank and out must be 16-byte aligned");
  if (h->cfg.n_mels % 4)
    return fail(h, CASR_ERR_UNSUPPORTED, "casr_gather_segments: n_mels %d is not a multiple of 4", h->cfg.n_mels);
  HIP_OK(h, hipSetDevice(h->device));
  if (!guard_words(h)) return fail(h, CASR_ERR_HIP, "casr_gather_segments: guard words not allocated");
  HIP_OK(h, launch_gather_segments(fbank, B, T, h->cfg.n_mels, seg_src, seg_start, seg_len, S, t_seg, out, frames_out,
                                   GUARD(h, 2), (hipStream_t)stream));
  return CASR_OK;
}

int casr_gather_utterances(casr_handle* h, const float* const* utt_ptrs, const int32_t* lens, int B,
                           int Tp, float* feat, void* stream) {
  if (!h || !utt_ptrs || !lens || !feat || B <= 0 || Tp <= 0)
    return fail(h, CASR_ERR_ARG, "casr_gather_utterances: bad arguments");
  HIP_OK(h, hipSetDevice(h->device));
  HIP_OK(h, launch_gather_utts(utt_ptrs, lens, B, Tp, feat, (hipStream_t)stream));
  return CASR_OK;
}

// The encoder.  fb != nullptr (casr_encode_fbank): the inputs are fbank [B][T][n_mels] + frames
// and the features are computed here (s16x3: straight into the layer-0 image); otherwise
// feat [B][Tp][feat_dim] + lens.  Every path decision is the plan's (encode_plan.h plan_encode); the
// one runtime event is a refused cooperative launch, after which `persistent` is off.
static int encode_impl(casr_handle* h, const float* feat, const int32_t* lens, int B, int Tp, hipStream_t s,
                       const float* fb = nullptr, const int32_t* frames = nullptr, int T = 0, float eps = 0.f) {
  const EncodePlan plan = plan_encode(B, Tp, T, fb != nullptr, h->cfg, h->tune, h->s16(), h->use_persistent, h->dev);
  switch (plan.status) {
    case ENC_BAD_SHAPE: return fail(h, CASR_ERR_ARG, "encode: bad shape (B=%d Tp=%d)", B, Tp);
    case ENC_KEYS_OFFSET:
      return fail(h, CASR_ERR_UNSUPPORTED, "encode: keys of B=%d Tp=%d are past the row-streaming form's 32-bit offsets", B, Tp);
    case ENC_KM_FORM: return fail(h, CASR_ERR_UNSUPPORTED, "encode: a 16-k-major image with a row-image kernel form");
    default: break;
  }
  const RecPlan& rec = plan.rec;
  const EncodeSizes size = encode_sizes(plan);
  HIP_OK(h, h->gin.ensure(size.gin));
  HIP_OK(h, h->out0.ensure(size.out));
  HIP_OK(h, h->out1.ensure(size.out));
  HIP_OK(h, h->hbuf.ensure(size.hbuf));
  HIP_OK(h, h->cst.ensure(size.cst));
  HIP_OK(h, h->hfin.ensure(size.hfin));
  HIP_OK(h, h->keysT.ensure(size.keysT));
  HIP_OK(h, h->lens.ensure(size.lens));
  // (the guard words, allocated at their first use, keep their place in the allocation order: the
  // hand-off buffer's address after them is the one the recurrence was tuned and measured at)
  if (!guard_words(h)) return fail(h, CASR_ERR_HIP, "casr_encode: guard words not allocated");
  int32_t* eflag = GUARD(h, 1);
  HIP_OK(h, h->x16.ensure(size.x16));
  HIP_OK(h, h->hx.ensure(size.hx));
  HIP_OK(h, h->fstat.ensure(size.fstat));
  HIP_OK(h, h->feat.ensure(size.feat));
  if (!fb) HIP_OK(h, hipMemcpyAsync(h->lens.p, lens, size.lens, hipMemcpyDeviceToDevice, s));
  bool persistent = rec.persistent;
  if (!persistent) {  // the persistent recurrence writes the padded frames itself
    HIP_OK(h, hipMemsetAsync(h->out0.p, 0, size.out, s));
    HIP_OK(h, hipMemsetAsync(h->out1.p, 0, size.out, s));
  }
  {  // final h
    FillList fl;
    fl.add32(h->hfin.p, 0u, size.hfin / sizeof(float));
    HIP_OK(h, fill_multi(fl, s));
  }
  const bool s16 = plan.s16;
  const int32_t* dl = h->lens.as<int32_t>();
  float* outs[2] = {h->out0.as<float>(), h->out1.as<float>()};
  if (fb) {
    ProfScope ps(&h->prof, CASR_K_FEATURES, s);
    if (plan.feat == FEAT_IMAGE) {  // feat stays NULL: layer 0 reads only the image (no residual input)
      HIP_OK(h, launch_features_x16(plan, fb, frames, T, eps, h->lens.as<int32_t>(), h->fstat.as<float>(),
                                    h->x16.as<uint16_t>(), eflag, s));
    } else {
      HIP_OK(h, launch_features(plan.feat, fb, frames, B, T, eps, h->feat.as<float>(), h->lens.as<int32_t>(),
                                h->fstat.as<float>(), s));
      feat = h->feat.as<float>();
    }
  }
  const float* x = feat;
  float* hb = h->hbuf.as<float>();
  for (int l = 0; l < plan.layers; ++l) {
    const InputGemmPlan& g = plan.layer_gemm(l);
    float* out = outs[l & 1];
    {
    ProfScope ps(&h->prof, CASR_K_INPUT_PROJ, s);
    if (s16) {
      // the layer input's image: layer 0's from the features kernel, a later layer's from the
      // persistent layer before it (no split pass)
      const bool have_image = l == 0 ? plan.feat == FEAT_IMAGE : persistent;
      if (!have_image)
        HIP_OK(h, launch_split_rows(x, g.K, plan.M, g.K, g.Kp, h->x16.as<uint16_t>(), eflag, s, plan.km));
      HIP_OK(h, launch_input_proj_s16_big(g, h->x16.as<float>(),
                                          plan.km ? h->wih16km.as<float>() + h->wih16km_off[l] : h->W + h->L.enc_wih16[l],
                                          h->W + h->L.enc_bias[l], h->gin.as<float>(), s));
    } else {
      HIP_OK(h, launch_input_proj(x, plan.M, g.K, h->W + h->L.enc_wih[l], h->W + h->L.enc_bias[l],
                                  h->gin.as<float>(), s));
    }
    }
    const int residual = plan.residual && l > 0;
    // layer 0 has no residual input: pass an internal pointer so a graph never bakes in the
    // caller's feature buffer
    const float* xin = residual ? x : out;
    const float* whh = h->W + (s16 ? h->L.enc_whh16[l] : h->L.enc_whh[l]);
    x = out;
    if (persistent) {
      // one launch runs all Tp steps; h and c start at zero inside (util.py:1236-1247)
      HIP_OK(h, reset_rec_layer(rec, h->hx.as<uint32_t>(), s));
      // diagnostics only: CASR_REC_TRACE=<file> dumps per-wave phase timestamps of layer 0
      const char* trace_path = l == 0 ? std::getenv("CASR_REC_TRACE") : nullptr;
      DevBuf tbuf;
      const size_t tbytes = (size_t)rec.grid * rec.waves() * Tp * 5 * sizeof(uint32_t);
      if (trace_path) {
        HIP_OK(h, tbuf.ensure(tbytes));
        HIP_OK(h, hipMemsetAsync(tbuf.p, 0, tbytes, s));
      }
      hipError_t er;
      if (rec.refuse == l + 1) {
        er = hipErrorCooperativeLaunchTooLarge;  // tests only: this layer's launch "refused"
      } else {
        ProfScope ps(&h->prof, CASR_K_REC_STEP, s);
        // (s16: the image of the layer's output, the last layer's feeds the keys GEMM)
        er = launch_rec_layer(rec, whh, h->gin.as<float>(), xin, out, s16 ? h->x16.as<uint16_t>() : nullptr, h->hx.as<uint32_t>(),
                              h->hfin.as<float>(), h->cst.as<float>(), dl, residual, eflag, tbuf.as<uint32_t>(), s);
      }
      if (er == hipErrorCooperativeLaunchTooLarge) {
        // the device cannot hold the whole grid at once (e.g. CUs taken by other work): this layer
        // and the next ones run the per-step recurrence (same bits) instead of spinning
        (void)hipGetLastError();
        persistent = false;
      } else {
        HIP_OK(h, er);
      }
      if (persistent && trace_path) {
        std::vector<uint32_t> hostv(tbytes / 4);
        HIP_OK(h, hipMemcpyAsync(hostv.data(), tbuf.p, tbytes, hipMemcpyDeviceToHost, s));
        HIP_OK(h, hipStreamSynchronize(s));
        tbuf.release();
        if (FILE* f = std::fopen(trace_path, "wb")) {
          const int32_t hdr[5] = {rec.grid, rec.waves(), Tp, 5, rec.producers()};
          std::fwrite(hdr, sizeof hdr, 1, f);
          std::fwrite(hostv.data(), 4, hostv.size(), f);
          std::fclose(f);
        }
      }
      if (persistent) continue;
    }
    // the persistent layers write their padded frames themselves; the per-step ones need zeros
    if (rec.persistent) HIP_OK(h, hipMemsetAsync(out, 0, size.out, s));
    // h (both ping-pong buffers) and c start at zero (RNN_RES state None, util.py:1236-1247)
    HIP_OK(h, fill_u32(hb, 0, size.hbuf / sizeof(float), s));
    HIP_OK(h, fill_u32(h->cst.p, 0, size.cst / sizeof(float), s));
    // every buffer the step loop is handed: the launch arguments and the pointer part of its graphs' key
    const void* const buf[] = {whh, h->gin.p, xin, out, hb, h->cst.p, h->hfin.p, dl};
    auto rec_loop = [&](hipStream_t st, Profiler* prof, int r0, int r1) -> hipError_t {
      hipError_t e = hipSuccess;
      for (int step = 0; step < Tp && e == hipSuccess; ++step) {
        const float* hprev = hb + (size_t)(step & 1) * 2 * B * H;
        float* hnext = hb + (size_t)((step + 1) & 1) * 2 * B * H;
        ProfScope ps(prof, CASR_K_REC_STEP, st);
        e = launch_rec_step(whh, h->gin.as<float>(), xin, out, hprev, hnext,
                            h->cst.as<float>(), h->hfin.as<float>(), dl, B, Tp, step, residual, r0, r1, s16, st);
      }
      return e;
    };
    if (h->graph_mode & CASR_GRAPHS_RECURRENCE) {
      hipGraphExec_t ex[2] = {};
      for (int p = 0; p < rec.nsplit; ++p) {
        const int r0 = rec.row0[p], r1 = rec.row1[p];
        const int32_t scalars[] = {l, r0, r1};
        const std::vector<uint64_t> key = plan_graph_key(1, &plan, sizeof plan, scalars, 3, buf, sizeof buf / sizeof buf[0]);
        HIP_OK(h, get_graph(h, key, [&](hipStream_t cs) { return rec_loop(cs, nullptr, r0, r1); }, &ex[p]));
      }
      ProfScope ps(&h->prof, CASR_K_REC_STEP, s, Tp);  // one pair per replay of Tp steps
      HIP_OK(h, launch_graphs(h, ex, rec.nsplit, s));
    } else {
      HIP_OK(h, rec_loop(s, &h->prof, 0, B));
    }
  }
  h->enc_out = const_cast<float*>(x);
  {
  ProfScope ps(&h->prof, CASR_K_KEYS, s);
  if (s16) {  // from the image the last persistent layer wrote, or of a split pass after a per-step one
    if (!persistent && plan.keys.split)
      HIP_OK(h, launch_split_rows(h->enc_out, C, plan.M, C, C, h->x16.as<uint16_t>(), eflag, s, plan.km));
    HIP_OK(h, launch_keys_s16(plan.keys, h->x16.as<float>(), h->W + h->L.wenc16, h->W + h->L.b_attn,
                              h->keysT.as<float>(), s));
  } else {
    HIP_OK(h, launch_keys(plan.keys, h->enc_out, h->W + h->L.wencT, h->W + h->L.b_attn, h->keysT.as<float>(), s));
  }
  }
  h->B = B;
  h->Tp = Tp;
  h->encoded = true;
  h->beam = BeamState{};
  return CASR_OK;
}

int casr_encode(casr_handle* h, const float* feat, const int32_t* lens, int B, int Tp, void* stream) {
  if (!h) return fail(h, CASR_ERR_ARG, "handle NULL");
  if (!h->W) return fail(h, CASR_ERR_STATE, "casr_encode: no weights bound");
  if (!feat || !lens || B <= 0 || Tp <= 0) return fail(h, CASR_ERR_ARG, "casr_encode: bad arguments");
  HIP_OK(h, hipSetDevice(h->device));
  return encode_impl(h, feat, lens, B, Tp, (hipStream_t)stream);
}

int casr_encode_fbank(casr_handle* h, const float* fbank, const int32_t* frames, int B, int T, float eps,
                      int32_t* feat_len, void* stream) {
  if (!h) return fail(h, CASR_ERR_ARG, "handle NULL");
  if (!h->W) return fail(h, CASR_ERR_STATE, "casr_encode_fbank: no weights bound");
  if (!fbank || !frames || B <= 0 || T < 3)
    return fail(h, CASR_ERR_ARG, "casr_encode_fbank: bad arguments (B=%d T=%d)", B, T);
  HIP_OK(h, hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const int rc = encode_impl(h, nullptr, nullptr, B, T / 3, s, fbank, frames, T, eps);
  if (rc == CASR_OK && feat_len)
    HIP_OK(h, hipMemcpyAsync(feat_len, h->lens.p, sizeof(int32_t) * B, hipMemcpyDeviceToDevice, s));
  return rc;
}

int casr_encoder_results(casr_handle* h, float* enc, float* h_final, float* c_final, float* keys,
                         void* stream) {
  if (!h || !h->encoded) return fail(h, CASR_ERR_STATE, "casr_encoder_results: nothing encoded");
  HIP_OK(h, hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const int B = h->B, Tp = h->Tp;
  if (enc)
    HIP_OK(h, hipMemcpyAsync(enc, h->enc_out, (size_t)B * Tp * C * sizeof(float), hipMemcpyDeviceToDevice, s));
  // [2][B][H] -> [B][fw | bw]
  if (h_final)
    HIP_OK(h, hipMemcpy2DAsync(h_final, C * sizeof(float), h->hfin.p, H * sizeof(float), H * sizeof(float), B,
                               hipMemcpyDeviceToDevice, s));
  if (h_final)
    HIP_OK(h, hipMemcpy2DAsync(h_final + H, C * sizeof(float), h->hfin.as<float>() + (size_t)B * H,
                               H * sizeof(float), H * sizeof(float), B, hipMemcpyDeviceToDevice, s));
  if (c_final)
    HIP_OK(h, hipMemcpy2DAsync(c_final, C * sizeof(float), h->cst.p, H * sizeof(float), H * sizeof(float), B,
                               hipMemcpyDeviceToDevice, s));
  if (c_final)
    HIP_OK(h, hipMemcpy2DAsync(c_final + H, C * sizeof(float), h->cst.as<float>() + (size_t)B * H,
                               H * sizeof(float), H * sizeof(float), B, hipMemcpyDeviceToDevice, s));
  if (keys)
    HIP_OK(h, hipMemcpy2DAsync(keys, Tp * sizeof(float), h->keysT.p, attn_tq(Tp) * sizeof(float),
                               Tp * sizeof(float), (size_t)B * A, hipMemcpyDeviceToDevice, s));
  return CASR_OK;
}

// the decode loop replays as a graph unless a decode kernel class is being timed per launch
static bool decode_graph_ok(const casr_handle* h) {
  const uint32_t dec = (1u << CASR_K_DEC_LSTM) | (1u << CASR_K_ATTENTION) | (1u << CASR_K_PROJ) |
                       (1u << CASR_K_SELECT);
  return (h->graph_mode & CASR_GRAPHS_DECODE) && !(h->prof.mask & dec);
}

// Every device buffer a decode's launchers read or write.  prepare_decode fills this one list from
// the handle; DecodeArgs, DecodeBufs and FoldBufs are filled from the list alone, and the list is
// the pointer part of the decode's hipGraph key (decode_graph_key), so a buffer added here is keyed.
enum {
  DP_W, DP_ENC, DP_KEYS, DP_HFIN, DP_CFIN, DP_LENS, DP_ERR,            // weights, the encode, guard words
  DP_STATE, DP_LOGITS, DP_SMALL, DP_BP, DP_TK, DP_RECORDS,             // decode workspaces
  DP_KSPLIT, DP_ATTN_SPLIT,                                            // plan.ksplit / plan.split only
  DP_WFOLD, DP_EMB_GATES, DP_WQ16, DP_GATES,                           // plan.fold only
  DP_OUT,                                                              // graph replay: the handle-owned outputs
  DP_COUNT
};
struct DecodeCall {
  DecodeArgs a{};
  void* buf[DP_COUNT] = {};
  std::vector<uint64_t> key(int kind, std::initializer_list<float> scalars) const {
    return decode_graph_key(kind, a.plan, scalars.begin(), (int)scalars.size(), buf, DP_COUNT);
  }
};

// One API call's decode: the plan (decode_plan.h), the workspaces it needs, and the launchers' arguments
static int prepare_decode(casr_handle* h, int caller, int k, bool want_align, DecodeCall& c, int score_len = 0) {
  if (!h->encoded) return fail(h, CASR_ERR_STATE, "decode before casr_encode");
  const int B = h->B, Tp = h->Tp, L = h->cfg.max_len, V = h->cfg.vocab;
  const BlobFacts blob{h->s16(), h->fold_ready, h->proj_small, h->dec_small};
  const DecodePlan plan = plan_decode(caller, B, Tp, k, want_align, h->cfg, h->L.VP, h->tune, blob, attention_static_lds(),
                                      score_len);
  switch (plan.status) {
    case PLAN_BAD_K: return fail(h, CASR_ERR_ARG, "beam width %d not in [1, %d]", k, KMAX_BEAM);
    case PLAN_K_VOCAB:
      return fail(h, CASR_ERR_ARG, "beam width %d keeps 2k = %d candidates, more than the vocabulary's %d tokens", k, 2 * k, V);
    case PLAN_LDS:
      return fail(h, CASR_ERR_UNSUPPORTED, "attention needs %d B of LDS (k=%d, Tp=%d) > 160 KiB", plan.lds_bytes, k, Tp);
    case PLAN_VOCAB:
      return fail(h, CASR_ERR_UNSUPPORTED, "casr_score: the vocabulary's projection column blocks > %d row partials", GP_NB);
    default: break;
  }
  if (plan.build_fold32) {
    const int rc = ensure_fold32(h);
    if (rc) return rc;
  }
  const int R = plan.R;
  // from here the decode workspaces are this call's: they are carved anew (another R moves newdone)
  // and its kernels clear newdone and overwrite the scores, so the last beam is spent.  A call
  // refused above leaves it readable; a beam entry sets its own state after this (beam_ran)
  h->beam = BeamState{};
  DecodeBufs& d = h->d;
  d = DecodeBufs{};
  HIP_OK(h, h->st.ensure(carve_state(nullptr, plan, d)));
  HIP_OK(h, h->logits.ensure(carve_logits(nullptr, R, V, d)));
  HIP_OK(h, h->small.ensure(carve_small(nullptr, B, R, L, d)));
  HIP_OK(h, h->bp.ensure((size_t)L * R * sizeof(int32_t)));
  HIP_OK(h, h->tk.ensure((size_t)L * R * sizeof(int32_t)));
  HIP_OK(h, h->rec.ensure(carve_records(nullptr, B, L, plan.k, d)));
  if (plan.ksplit || plan.ksplit_last) HIP_OK(h, h->ksbuf.ensure(carve_ksplit(nullptr, d)));
  if (plan.split) HIP_OK(h, h->asbuf.ensure(carve_attn_split(nullptr, R, d)));
  if (plan.fold) HIP_OK(h, h->fgates.ensure((size_t)R * 4 * HD * sizeof(float)));
  if (!guard_words(h)) return fail(h, CASR_ERR_HIP, "decode: guard words not allocated");

  void** buf = c.buf;
  buf[DP_W] = const_cast<float*>(h->W);
  buf[DP_ENC] = h->enc_out;
  buf[DP_KEYS] = h->keysT.p;
  buf[DP_HFIN] = h->hfin.p;
  buf[DP_CFIN] = h->cst.p;
  buf[DP_LENS] = h->lens.p;
  buf[DP_ERR] = GUARD(h, 0);
  buf[DP_STATE] = h->st.p;
  buf[DP_LOGITS] = h->logits.p;
  buf[DP_SMALL] = h->small.p;
  buf[DP_BP] = h->bp.p;
  buf[DP_TK] = h->tk.p;
  buf[DP_RECORDS] = h->rec.p;
  if (plan.ksplit || plan.ksplit_last) buf[DP_KSPLIT] = h->ksbuf.p;
  if (plan.split) buf[DP_ATTN_SPLIT] = h->asbuf.p;
  if (plan.fold) {
    buf[DP_WFOLD] = plan.s16 ? h->wfold.p : h->wfold32.p;
    buf[DP_EMB_GATES] = h->egates.p;
    buf[DP_WQ16] = h->wq16.p;
    buf[DP_GATES] = h->fgates.p;
  }

  carve_state(buf[DP_STATE], plan, d);
  carve_logits(buf[DP_LOGITS], R, V, d);
  carve_small(buf[DP_SMALL], B, R, L, d);
  carve_records(buf[DP_RECORDS], B, L, plan.k, d);
  if (buf[DP_KSPLIT]) carve_ksplit(buf[DP_KSPLIT], d);
  if (buf[DP_ATTN_SPLIT]) carve_attn_split(buf[DP_ATTN_SPLIT], R, d);
  d.err = static_cast<int32_t*>(buf[DP_ERR]);
  d.bp = static_cast<int32_t*>(buf[DP_BP]);
  d.tk = static_cast<int32_t*>(buf[DP_TK]);
  DecodeArgs& a = c.a;
  a.W = static_cast<const float*>(buf[DP_W]);
  a.L = h->L;
  a.enc = static_cast<const float*>(buf[DP_ENC]);
  a.keysT = static_cast<const float*>(buf[DP_KEYS]);
  a.hfin = static_cast<const float*>(buf[DP_HFIN]);
  a.cfin = static_cast<const float*>(buf[DP_CFIN]);
  a.lens = static_cast<const int32_t*>(buf[DP_LENS]);
  a.B = B;
  a.Tp = Tp;
  a.k = plan.k;
  a.V = V;
  a.max_len = L;
  a.sos = h->cfg.sos;
  a.eos = h->cfg.eos;
  a.temperature = h->cfg.temperature;
  a.prof = &h->prof;
  a.plan = plan;
  a.fb = FoldBufs{static_cast<const float*>(buf[DP_WFOLD]), static_cast<const float*>(buf[DP_EMB_GATES]),
                  static_cast<const float*>(buf[DP_WQ16]), static_cast<float*>(buf[DP_GATES])};
  return CASR_OK;
}

// a beam entry's decode is prepared: the handle's beam state, and the readers' view of the tree and
// the records it is about to write (casr_internal.h beam_tree_of)
static void beam_ran(casr_handle* h, int kind, const DecodeArgs& a, float lm_weight, float length_weight) {
  h->beam = BeamState{kind, a.k, lm_weight, length_weight};
  h->tree = beam_tree_of(a, h->d);
}

// the gate of the beam's readers (beam_state.h beam_gate) as the API's refusal; why: what the reader
// assumes of a casr_beam (the readers with a GATE_AFTER_FUSED refusal)
static int beam_readable(casr_handle* h, int reader, const char* why = "") {
  switch (h ? beam_gate(h->beam, reader) : GATE_BEFORE) {
    case GATE_OK: return CASR_OK;
    case GATE_AFTER_FUSED:
      if (h->beam.grammar)
        return fail(h, CASR_ERR_STATE, "%s after casr_beam_grammar: %s", BEAM_READER_NAME[reader], why);
      return fail(h, CASR_ERR_STATE, "%s after casr_beam_lm or casr_beam_bias: %s", BEAM_READER_NAME[reader], why);
    default: return fail(h, CASR_ERR_STATE, "%s before %s", BEAM_READER_NAME[reader], BEAM_READER_FOLLOWS[reader]);
  }
}

int casr_greedy(casr_handle* h, int32_t* tokens, int32_t* out_len, uint8_t* finished, float* accum,
                float* align, void* stream) {
  if (!h || !tokens || !out_len || !finished || !accum) return fail(h, CASR_ERR_ARG, "casr_greedy: NULL output");
  HIP_OK(h, hipSetDevice(h->device));
  DecodeCall c;
  int rc = prepare_decode(h, PLAN_GREEDY, 1, align != nullptr, c);
  if (rc) return rc;
  DecodeArgs& a = c.a;
  hipStream_t s = (hipStream_t)stream;
  if (!decode_graph_ok(h)) {
    dg_trace_init();  // CASR_DG_TRACE diagnostics only
    HIP_OK(h, run_greedy(a, h->d, tokens, out_len, finished, accum, align, s));
    dg_trace_dump();
    return CASR_OK;
  }
  // graph replay into handle-owned outputs, then copies to the caller's buffers
  const int B = h->B, L = h->cfg.max_len;
  const size_t nal = align ? (size_t)L * h->Tp * B : 0;
  GreedyOut o{};
  HIP_OK(h, h->gout.ensure(carve_greedy_out(nullptr, B, L, nal, o)));
  carve_greedy_out(c.buf[DP_OUT] = h->gout.p, B, L, nal, o);
  a.prof = nullptr;
  dg_trace_init();  // CASR_DG_TRACE diagnostics only (outside any capture)
  HIP_OK(h, run_graph(h, c.key(2, {}), s, [&](hipStream_t cs) {
    return run_greedy(a, h->d, o.tokens, o.len, o.fin, o.accum, o.align, cs);
  }));
  dg_trace_dump();  // CASR_DG_TRACE diagnostics only (no-op otherwise)
  CopyList cl;  // the graph's outputs to the caller's buffers in one launch
  cl.add(tokens, o.tokens, sizeof(int32_t) * B * L);
  cl.add(out_len, o.len, sizeof(int32_t) * B);
  cl.add(finished, o.fin, B);
  cl.add(accum, o.accum, sizeof(float) * B);
  if (align) cl.add(align, o.align, sizeof(float) * nal);
  HIP_OK(h, copy_multi(cl, s));
  return CASR_OK;
}

int casr_beam(casr_handle* h, int k, float lm_weight, float length_weight, int32_t* best_tokens,
              int32_t* best_len, float* best_score, int32_t* steps, void* stream) {
  if (!h || !best_tokens || !best_len || !best_score || !steps)
    return fail(h, CASR_ERR_ARG, "casr_beam: NULL output");
  HIP_OK(h, hipSetDevice(h->device));
  DecodeCall c;
  int rc = prepare_decode(h, PLAN_BEAM, k, false, c);
  if (rc) return rc;
  DecodeArgs& a = c.a;
  hipStream_t s = (hipStream_t)stream;
  beam_ran(h, BEAM_PLAIN, a, lm_weight, length_weight);
  if (!decode_graph_ok(h)) {
    dg_trace_init();  // CASR_DG_TRACE diagnostics only
    HIP_OK(h, run_beam(a, h->d, lm_weight, length_weight, best_tokens, best_len, best_score, steps, s));
    dg_trace_dump();
    return CASR_OK;
  }
  const int B = h->B, L = h->cfg.max_len;
  BeamOut o{};
  HIP_OK(h, h->gout.ensure(carve_beam_out(nullptr, B, L, o)));
  carve_beam_out(c.buf[DP_OUT] = h->gout.p, B, L, o);
  a.prof = nullptr;
  dg_trace_init();  // CASR_DG_TRACE diagnostics only (outside any capture)
  HIP_OK(h, run_graph(h, c.key(3, {lm_weight, length_weight}), s, [&](hipStream_t cs) {
    return run_beam(a, h->d, lm_weight, length_weight, o.tokens, o.len, o.score, o.steps, cs);
  }));
  dg_trace_dump();
  CopyList cl;  // the graph's outputs to the caller's buffers in one launch
  cl.add(best_tokens, o.tokens, sizeof(int32_t) * B * L);
  cl.add(best_len, o.len, sizeof(int32_t) * B);
  cl.add(best_score, o.score, sizeof(float) * B);
  cl.add(steps, o.steps, sizeof(int32_t));
  HIP_OK(h, copy_multi(cl, s));
  return CASR_OK;
}

int casr_beam_records(casr_handle* h, int32_t* rec_tokens, float* rec_score, uint8_t* rec_valid,
                      void* stream) {
  const int rc = beam_readable(h, READ_RECORDS);
  if (rc) return rc;
  if (!rec_tokens || !rec_score || !rec_valid) return fail(h, CASR_ERR_ARG, "casr_beam_records: NULL output");
  HIP_OK(h, hipSetDevice(h->device));
  HIP_OK(h, run_beam_records(h->tree, rec_tokens, rec_score, rec_valid, (hipStream_t)stream));
  return CASR_OK;
}

int casr_score(casr_handle* h, const int32_t* targets, const int32_t* tgt_len, int L, float* token_logp,
               float* total_logp, int32_t* best_token, float* best_logp, float* mean_logp, float* align,
               void* stream) {
  if (!h || !targets || !tgt_len || !token_logp || !total_logp)
    return fail(h, CASR_ERR_ARG, "casr_score: NULL handle, targets, tgt_len, token_logp or total_logp");
  if (!h->W) return fail(h, CASR_ERR_STATE, "casr_score before casr_bind_weights");
  if (!h->encoded) return fail(h, CASR_ERR_STATE, "casr_score before casr_encode");
  if (L < 1 || L > h->cfg.max_len) return fail(h, CASR_ERR_ARG, "casr_score: L = %d not in [1, %d]", L, h->cfg.max_len);
  HIP_OK(h, hipSetDevice(h->device));
  DecodeCall c;
  int rc = prepare_decode(h, PLAN_SCORE, 1, false, c, L);
  if (rc) return rc;
  HIP_OK(h, h->scorebuf.ensure(score_workspace_bytes(h->B, L)));
  const ScoreBufs sb = score_carve(h->scorebuf.p, h->B, L);
  HIP_OK(h, run_score(c.a, h->d, sb, targets, tgt_len, L, token_logp, total_logp, best_token, best_logp, mean_logp, align,
                      (hipStream_t)stream));
  return CASR_OK;
}

// casr_lm_create, casr_bias_create: the n host tables copied to `device`, dev[i] of bytes[i] (an empty
// table keeps a 16-byte allocation).  On an error the caller destroys its object, which frees dev
static hipError_t upload_tables(int device, int n, const void* const* src, const size_t* bytes, void** dev) {
  hipError_t e = hipSetDevice(device);
  for (int i = 0; i < n && e == hipSuccess; ++i) {
    e = hipMalloc(&dev[i], bytes[i] ? bytes[i] : 16);
    if (e == hipSuccess && bytes[i]) e = hipMemcpy(dev[i], src[i], bytes[i], hipMemcpyHostToDevice);
  }
  return e;
}

int casr_lm_create(int device, int order, int vocab, const int64_t* count, const int32_t* const* ids,
                   const float* const* prob, const float* const* backoff, casr_lm** out) {
  if (!out) return fail(nullptr, CASR_ERR_ARG, "casr_lm_create: out is NULL");
  *out = nullptr;
  if (device < -1) return fail(nullptr, CASR_ERR_ARG, "casr_lm_create: device %d", device);
  casr_lm* lm = new casr_lm();
  std::string why;
  const int rc = ngram_build(order, vocab, count, ids, prob, backoff, &lm->host, &why);
  if (rc != NGRAM_OK) {
    delete lm;
    return fail(nullptr, rc, "casr_lm_create: %s", why.c_str());
  }
  ngram_succ_build(lm->host, count, ids, prob, &lm->succ);
  for (int n = 0; n < order; ++n) lm->count[n] = count[n];
  for (int64_t i = 0; i < count[0]; ++i) lm->unk_given = lm->unk_given || ids[0][i] == vocab + 2;
  lm->device = device;
  if (device >= 0) {
    const NgramTables& t = lm->host;
    const NgramSuccTables& u = lm->succ;
    const void* src[11] = {t.uni.data(), t.redirect.data(), t.tab[0].data(), t.tab[1].data(), t.tab[2].data(),
                           u.list[0].data(), u.list[1].data(), u.list[2].data(), u.dir.data(), u.ctab[0].data(),
                           u.ctab[1].data()};
    const size_t bytes[11] = {t.uni.size() * sizeof(NgramUni), t.redirect.size() * sizeof(int32_t),
                              t.tab[0].size() * sizeof(NgramEntry), t.tab[1].size() * sizeof(NgramEntry),
                              t.tab[2].size() * sizeof(NgramEntry), u.list[0].size() * sizeof(NgramSucc),
                              u.list[1].size() * sizeof(NgramSucc), u.list[2].size() * sizeof(NgramSucc),
                              u.dir.size() * sizeof(NgramSuccRange), u.ctab[0].size() * sizeof(NgramCtxEntry),
                              u.ctab[1].size() * sizeof(NgramCtxEntry)};
    const hipError_t e = upload_tables(device, 11, src, bytes, lm->dev);  // (an order without reachable n-grams: an empty list)
    if (e != hipSuccess) {
      casr_lm_destroy(lm);
      return fail(nullptr, CASR_ERR_HIP, "casr_lm_create: %s", hipGetErrorString(e));
    }
    lm->dview = t.view();
    lm->dview.uni = static_cast<const NgramUni*>(lm->dev[0]);
    lm->dview.redirect = static_cast<const int32_t*>(lm->dev[1]);
    for (int i = 0; i < NGRAM_MAX_ORDER - 1; ++i) lm->dview.tab[i] = static_cast<const NgramEntry*>(lm->dev[2 + i]);
    lm->dsucc = u.view();
    for (int i = 0; i < NGRAM_MAX_ORDER - 1; ++i) lm->dsucc.list[i] = static_cast<const NgramSucc*>(lm->dev[5 + i]);
    lm->dsucc.dir = static_cast<const NgramSuccRange*>(lm->dev[8]);
    for (int i = 0; i < NGRAM_MAX_ORDER - 2; ++i) lm->dsucc.ctab[i] = static_cast<const NgramCtxEntry*>(lm->dev[9 + i]);
  }
  *out = lm;
  return CASR_OK;
}

void casr_lm_destroy(casr_lm* lm) {
  if (!lm) return;
  if (lm->device >= 0 && hipSetDevice(lm->device) == hipSuccess)
    for (void* p : lm->dev)
      if (p) (void)hipFree(p);
  delete lm;
}

int casr_lm_score_host(const casr_lm* lm, const int32_t* tokens, const int32_t* lens, int n, int L, int bos,
                       float* q) {
  if (!lm || !lens || !q || (!tokens && L > 0) || n < 0 || L < 0)
    return fail(nullptr, CASR_ERR_ARG, "casr_lm_score_host: NULL argument, n < 0 or L < 0");
  for (int i = 0; i < n; ++i)
    if (lens[i] < 0 || lens[i] > L)
      return fail(nullptr, CASR_ERR_ARG, "casr_lm_score_host: lens[%d] = %d not in [0, %d]", i, lens[i], L);
  const NgramView m = lm->host.view();
  for (int i = 0; i < n; ++i) q[i] = ngram_sentence(m, tokens + (size_t)i * L, lens[i], bos != 0);
  return CASR_OK;
}

// the LM's device copy serves this handle: the same device, the same vocabulary
static int lm_matches_handle(casr_handle* h, const casr_lm* lm, const char* who) {
  if (lm->device != h->device)
    return fail(h, CASR_ERR_ARG, "%s: the LM is %s, the handle on device %d", who,
                lm->device < 0 ? "host-only" : "on another device", h->device);
  if (lm->host.V != h->cfg.vocab)
    return fail(h, CASR_ERR_ARG, "%s: the LM's vocab %d is not the handle's %d", who, lm->host.V, h->cfg.vocab);
  return CASR_OK;
}

int casr_lm_score(casr_handle* h, const casr_lm* lm, const int32_t* tokens, const int32_t* lens, int n, int L,
                  int bos, float* q, void* stream) {
  if (!h || !lm || !tokens || !lens || !q || n < 0 || L < 1)
    return fail(h, CASR_ERR_ARG, "casr_lm_score: NULL argument, n < 0 or L < 1");
  const int rc = lm_matches_handle(h, lm, "casr_lm_score");
  if (rc) return rc;
  HIP_OK(h, hipSetDevice(h->device));
  if (!guard_words(h)) return fail(h, CASR_ERR_HIP, "casr_lm_score: no guard words");
  int32_t* err = GUARD(h, 0);
  HIP_OK(h, launch_lm_score(lm->dview, tokens, lens, n, L, bos != 0, q, err, (hipStream_t)stream));
  return CASR_OK;
}

// ---- Kneser-Ney estimation (lm_estimate_plan.h; the kernels in lm_estimate.hip)
struct casr_lm_est {
  casr::EstResult r;
};
static int g_est_combine = 1;

int casr_lm_estimate_host(int order, int vocab, const int32_t* tokens, const int64_t* offsets, int64_t n,
                          casr_lm_est** est) {
  if (!est) return fail(nullptr, CASR_ERR_ARG, "casr_lm_estimate_host: est is NULL");
  *est = nullptr;
  casr_lm_est* o = new casr_lm_est();
  std::string why;
  const int rc = est_estimate_host(order, vocab, tokens, offsets, n, &o->r, &why);
  if (rc != NGRAM_OK) {
    delete o;
    return fail(nullptr, rc, "casr_lm_estimate_host: %s", why.c_str());
  }
  *est = o;
  return CASR_OK;
}

int casr_lm_estimate(casr_handle* h, int order, const int32_t* tokens, const int64_t* offsets, int64_t n,
                     void* stream, casr_lm_est** est) {
  if (est) *est = nullptr;
  if (!h || !tokens || !offsets || !est) return fail(h, CASR_ERR_ARG, "casr_lm_estimate: NULL argument");
  if (order < 1 || order > NGRAM_MAX_ORDER) return fail(h, CASR_ERR_ARG, "casr_lm_estimate: order %d outside 1..4", order);
  if (n < 1) return fail(h, CASR_ERR_ARG, "casr_lm_estimate: n < 1");
  const int V = h->cfg.vocab;
  if ((int64_t)V + 3 > NGRAM_MAX_IDS) return fail(h, CASR_ERR_UNSUPPORTED, "casr_lm_estimate: vocab + 3 = %d > 65535", V + 3);
  if (n > EST_MAX_POSITIONS) return fail(h, CASR_ERR_UNSUPPORTED, "casr_lm_estimate: more than 2^28 positions");
  HIP_OK(h, hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  int64_t total = 0;
  HIP_OK(h, hipMemcpyAsync(&total, offsets + n, sizeof total, hipMemcpyDeviceToHost, s));
  HIP_OK(h, hipStreamSynchronize(s));
  if (total < 0) return fail(h, CASR_ERR_ARG, "casr_lm_estimate: offsets[n] = %lld < 0", (long long)total);
  if (total + n > EST_MAX_POSITIONS)
    return fail(h, CASR_ERR_UNSUPPORTED, "casr_lm_estimate: %lld positions > 2^28", (long long)(total + n));
  if (!guard_words(h)) return fail(h, CASR_ERR_HIP, "casr_lm_estimate: no guard words");
  HIP_OK(h, h->estws.ensure((size_t)est_workspace_bytes(order, total + n)));
  casr_lm_est* o = new casr_lm_est();
  uint32_t flags = 0;
  const hipError_t e = run_lm_estimate(order, V, tokens, offsets, n, total, h->estws.p, g_est_combine, GUARD(h, 0), s,
                                       &o->r, &flags);
  if (e != hipSuccess || (flags & EST_FLAG_FULL)) {
    delete o;
    if (e != hipSuccess) return fail(h, CASR_ERR_HIP, "casr_lm_estimate: %s", hipGetErrorString(e));
    return fail(h, CASR_ERR_ARG, "casr_lm_estimate: the offsets overlap: a counting table proved full");
  }
  *est = o;
  return CASR_OK;
}

int casr_lm_estimate_combine(int on) {
  const int was = g_est_combine;
  g_est_combine = on != 0;
  return was;
}

int casr_lm_estimate_info(const casr_lm_est* est, int64_t* count, double* discount, int32_t* fallback,
                          int64_t* n_types, int64_t* positions) {
  if (!est) return fail(nullptr, CASR_ERR_ARG, "casr_lm_estimate_info: NULL object");
  const EstResult& r = est->r;
  for (int m = 0; m < NGRAM_MAX_ORDER; ++m) {
    if (count) count[m] = (int64_t)r.key[m].size();
    if (fallback) fallback[m] = r.fallback[m];
    for (int k = 0; k < 3 && discount; ++k) discount[3 * m + k] = r.D[m][k];
  }
  if (n_types) *n_types = r.n_types;
  if (positions) *positions = r.positions;
  return CASR_OK;
}

int casr_lm_estimate_arrays(const casr_lm_est* est, int n, int32_t* ids, float* prob, float* backoff,
                            int64_t* adjusted, double* p_f64, double* gamma_f64) {
  if (!est || n < 1 || n > est->r.order)
    return fail(nullptr, CASR_ERR_ARG, "casr_lm_estimate_arrays: NULL object or n outside 1..order");
  const EstResult& r = est->r;
  const size_t c = r.key[n - 1].size();
  for (size_t i = 0; i < c; ++i) {
    if (ids) est_key_ids(r.key[n - 1][i], n, ids + i * n);
    if (prob) prob[i] = est_stored_prob(r, n, i);
    if (backoff) backoff[i] = est_stored_backoff(r, n, i);
    if (adjusted) adjusted[i] = r.adjusted[n - 1][i];
    if (p_f64) p_f64[i] = r.p[n - 1][i];
    if (gamma_f64) gamma_f64[i] = r.gamma[n - 1][i];
  }
  return CASR_OK;
}

int casr_lm_estimate_counts(const casr_lm_est* est, int n, int64_t* raw) {
  if (!est || !raw || n < 1 || n > est->r.order)
    return fail(nullptr, CASR_ERR_ARG, "casr_lm_estimate_counts: NULL argument or n outside 1..order");
  const std::vector<uint32_t>& c = est->r.count[n - 1];
  for (size_t i = 0; i < c.size(); ++i) raw[i] = c[i];
  return CASR_OK;
}

int casr_lm_estimate_timing(const casr_lm_est* est, double* ms) {
  if (!est || !ms) return fail(nullptr, CASR_ERR_ARG, "casr_lm_estimate_timing: NULL argument");
  for (int i = 0; i < 8; ++i) ms[i] = est->r.stage_ms[i];
  return CASR_OK;
}

void casr_lm_estimate_destroy(casr_lm_est* est) { delete est; }

int64_t casr_lm_estimate_workspace_bytes(int order, int64_t positions) { return est_workspace_bytes(order, positions); }

// ---- relative-entropy pruning (lm_prune_plan.h; the kernels in lm_prune.hip)
struct casr_lm_pruned {
  casr::LmpResult r;
};

static LmpDims lm_prune_dims(const casr_lm* lm) { return lmp_dims(lm->host, lm->succ, lm->count, lm->unk_given); }

int casr_lm_prune_host(const casr_lm* lm, double theta, casr_lm_pruned** out) {
  if (out) *out = nullptr;
  if (!lm || !out) return fail(nullptr, CASR_ERR_ARG, "casr_lm_prune_host: NULL argument");
  if (!(theta >= 0.0) || !isfinite(theta)) return fail(nullptr, CASR_ERR_ARG, "casr_lm_prune_host: theta %g", theta);
  casr_lm_pruned* o = new casr_lm_pruned();
  if (!lmp_prune_host(lm->host, lm->succ, lm_prune_dims(lm), theta, &o->r)) {
    delete o;
    return fail(nullptr, CASR_ERR_ARG, "casr_lm_prune_host: the LM object is inconsistent");
  }
  *out = o;
  return CASR_OK;
}

int casr_lm_prune(casr_handle* h, const casr_lm* lm, double theta, void* stream, casr_lm_pruned** out) {
  if (out) *out = nullptr;
  if (!h || !lm || !out) return fail(h, CASR_ERR_ARG, "casr_lm_prune: NULL argument");
  if (!(theta >= 0.0) || !isfinite(theta)) return fail(h, CASR_ERR_ARG, "casr_lm_prune: theta %g", theta);
  const int rc = lm_matches_handle(h, lm, "casr_lm_prune");
  if (rc) return rc;
  HIP_OK(h, hipSetDevice(h->device));
  const LmpDims d = lm_prune_dims(lm);
  HIP_OK(h, h->prunews.ensure((size_t)lmp_carve(nullptr, d, nullptr, nullptr, nullptr)));
  casr_lm_pruned* o = new casr_lm_pruned();
  uint32_t flags = 0;
  const hipError_t e = run_lm_prune(lm->host, lm->dview, lm->dsucc, d, theta, h->prunews.p, (hipStream_t)stream, &o->r, &flags);
  if (e != hipSuccess || flags) {
    delete o;
    if (e != hipSuccess) return fail(h, CASR_ERR_HIP, "casr_lm_prune: %s", hipGetErrorString(e));
    return fail(h, CASR_ERR_ARG, "casr_lm_prune: the LM object is inconsistent");
  }
  *out = o;
  return CASR_OK;
}

int casr_lm_prune_info(const casr_lm_pruned* p, int64_t* count_in, int64_t* count_out, int64_t* n_protected,
                       int64_t* n_degenerate, double* tau) {
  if (!p) return fail(nullptr, CASR_ERR_ARG, "casr_lm_prune_info: NULL object");
  const LmpResult& r = p->r;
  for (int m = 0; m < NGRAM_MAX_ORDER; ++m) {
    if (count_in) count_in[m] = (int64_t)r.key[m].size();
    if (count_out) count_out[m] = r.count_out[m];
    if (n_protected) n_protected[m] = r.n_protected[m];
  }
  if (n_degenerate) *n_degenerate = r.n_degenerate;
  if (tau) *tau = r.tau;
  return CASR_OK;
}

int casr_lm_prune_arrays(const casr_lm_pruned* p, int n, int32_t* ids, float* prob, float* backoff,
                         double* backoff_f64) {
  if (!p || n < 1 || n > p->r.order)
    return fail(nullptr, CASR_ERR_ARG, "casr_lm_prune_arrays: NULL object or n outside 1..order");
  const LmpResult& r = p->r;
  size_t at = 0;
  for (size_t i = 0; i < r.key[n - 1].size(); ++i) {
    if (!r.kept[n - 1][i]) continue;
    if (ids) lmp_key_ids(r.key[n - 1][i], n, ids + at * n);
    if (prob) prob[at] = r.prob[n - 1][i];
    if (backoff) backoff[at] = r.out_backoff[n - 1][i];
    if (backoff_f64) backoff_f64[at] = r.out_b64[n - 1][i];
    ++at;
  }
  return CASR_OK;
}

int casr_lm_prune_decisions(const casr_lm_pruned* p, int n, int32_t* ids, double* delta, uint8_t* kept) {
  if (!p || n < 1 || n > p->r.order)
    return fail(nullptr, CASR_ERR_ARG, "casr_lm_prune_decisions: NULL object or n outside 1..order");
  const LmpResult& r = p->r;
  for (size_t i = 0; i < r.key[n - 1].size(); ++i) {
    if (ids) lmp_key_ids(r.key[n - 1][i], n, ids + i * n);
    if (delta) delta[i] = r.delta[n - 1][i];
    if (kept) kept[i] = r.kept[n - 1][i];
  }
  return CASR_OK;
}

int casr_lm_prune_timing(const casr_lm_pruned* p, double* ms) {
  if (!p || !ms) return fail(nullptr, CASR_ERR_ARG, "casr_lm_prune_timing: NULL argument");
  for (int i = 0; i < 8; ++i) ms[i] = p->r.stage_ms[i];
  return CASR_OK;
}

void casr_lm_prune_destroy(casr_lm_pruned* p) { delete p; }

int64_t casr_lm_prune_workspace_bytes(const casr_lm* lm) {
  if (!lm) return -1;
  return lmp_carve(nullptr, lm_prune_dims(lm), nullptr, nullptr, nullptr);
}

int casr_beam_rescore(casr_handle* h, const casr_lm* lm, double lm_weight, double length_weight,
                      int32_t* best_tokens, int32_t* best_len, float* best_score, float* best_lm, float* rec_lm,
                      void* stream) {
  if (!h || !lm || !best_tokens || !best_len || !best_score)
    return fail(h, CASR_ERR_ARG, "casr_beam_rescore: NULL handle, LM or output");
  int rc = beam_readable(h, READ_RESCORE, "the second pass rescores a casr_beam");
  if (!rc) rc = lm_matches_handle(h, lm, "casr_beam_rescore");
  if (rc) return rc;
  if (!rescore_supported(h->cfg.max_len, h->beam.k))
    return fail(h, CASR_ERR_UNSUPPORTED, "casr_beam_rescore: max_len %d x k %d past the LDS", h->cfg.max_len, h->beam.k);
  HIP_OK(h, hipSetDevice(h->device));
  HIP_OK(h, run_beam_rescore(h->tree, lm->dview, lm_weight, length_weight, h->beam.lm_weight, h->beam.length_weight,
                             best_tokens, best_len, best_score, best_lm, rec_lm, (hipStream_t)stream));
  return CASR_OK;
}

int casr_edit_distance_host(const int32_t* a, const int32_t* a_len, int La, const int32_t* b, const int32_t* b_len,
                            int Lb, int n, int32_t* dist, int32_t* ops) {
  if (n < 0 || La < 0 || Lb < 0 || (n > 0 && (!a_len || !b_len || !dist || (!a && La > 0) || (!b && Lb > 0))))
    return fail(nullptr, CASR_ERR_ARG, "casr_edit_distance_host: NULL argument, or n, La or Lb < 0");
  for (int i = 0; i < n; ++i)
    if (a_len[i] < 0 || a_len[i] > La || b_len[i] < 0 || b_len[i] > Lb)
      return fail(nullptr, CASR_ERR_ARG, "casr_edit_distance_host: pair %d has lengths %d, %d outside [0, %d], [0, %d]", i,
                  a_len[i], b_len[i], La, Lb);
  for (int i = 0; i < n; ++i)
    dist[i] = edit_distance_rows(a + (size_t)i * La, a_len[i], b + (size_t)i * Lb, b_len[i],
                                 ops ? ops + (size_t)i * 3 : nullptr);
  return CASR_OK;
}

int casr_edit_distance(casr_handle* h, const int32_t* a, const int32_t* a_len, int La, const int32_t* b,
                       const int32_t* b_len, int Lb, int n, int32_t* dist, int32_t* ops, void* stream) {
  if (!h || n < 0 || (n > 0 && (!a || !a_len || !b || !b_len || !dist)))
    return fail(h, CASR_ERR_ARG, "casr_edit_distance: NULL argument or n < 0");
  if (edit_plan_pairs(La, Lb, n, ops != nullptr).form == EDIT_FORM_NONE)
    return fail(h, CASR_ERR_UNSUPPORTED, "casr_edit_distance: La = %d, Lb = %d not in [1, %d]", La, Lb, EDIT_MAX_LEN);
  HIP_OK(h, hipSetDevice(h->device));
  if (!guard_words(h)) return fail(h, CASR_ERR_HIP, "casr_edit_distance: no guard words");
  HIP_OK(h, launch_edit_pairs(a, a_len, La, b, b_len, Lb, n, dist, ops, GUARD(h, 0), (hipStream_t)stream));
  return CASR_OK;
}

static int edit_align_host_entry(const char* who, bool tiles, const int32_t* a, const int32_t* a_len, int La,
                                 const int32_t* b, const int32_t* b_len, int Lb, int n, int32_t* dist, int32_t* ops,
                                 int32_t* b_of_a, int32_t* a_of_b) {
  if (n < 0 || La < 0 || Lb < 0 || (n > 0 && (!a_len || !b_len || !dist || (!a && La > 0) || (!b && Lb > 0))))
    return fail(nullptr, CASR_ERR_ARG, "%s: NULL argument, or n, La or Lb < 0", who);
  for (int i = 0; i < n; ++i)
    if (a_len[i] < 0 || a_len[i] > La || b_len[i] < 0 || b_len[i] > Lb)
      return fail(nullptr, CASR_ERR_ARG, "%s: pair %d has lengths %d, %d outside [0, %d], [0, %d]", who, i, a_len[i],
                  b_len[i], La, Lb);
  if (b_of_a) std::fill(b_of_a, b_of_a + (size_t)n * La, -1);
  if (a_of_b) std::fill(a_of_b, a_of_b + (size_t)n * Lb, -1);
  for (int i = 0; i < n; ++i)
    dist[i] = (tiles ? ea_pair_tiles : ea_pair_rows)(a + (size_t)i * La, a_len[i], b + (size_t)i * Lb, b_len[i],
                                                     ops ? ops + (size_t)i * 3 : nullptr,
                                                     b_of_a ? b_of_a + (size_t)i * La : nullptr,
                                                     a_of_b ? a_of_b + (size_t)i * Lb : nullptr);
  return CASR_OK;
}

int casr_edit_align_host(const int32_t* a, const int32_t* a_len, int La, const int32_t* b, const int32_t* b_len, int Lb,
                         int n, int32_t* dist, int32_t* ops, int32_t* b_of_a, int32_t* a_of_b) {
  return edit_align_host_entry("casr_edit_align_host", false, a, a_len, La, b, b_len, Lb, n, dist, ops, b_of_a, a_of_b);
}

int casr_edit_align_tiles_host(const int32_t* a, const int32_t* a_len, int La, const int32_t* b, const int32_t* b_len,
                               int Lb, int n, int32_t* dist, int32_t* ops, int32_t* b_of_a, int32_t* a_of_b) {
  return edit_align_host_entry("casr_edit_align_tiles_host", true, a, a_len, La, b, b_len, Lb, n, dist, ops, b_of_a,
                               a_of_b);
}

int casr_edit_align_plan(int La, int Lb, int n, int with_bits, int64_t* out, int64_t* grid) {
  if (!out) return fail(nullptr, CASR_ERR_ARG, "casr_edit_align_plan: NULL out");
  const EaPlan pl = edit_align_plan(La, Lb, n, with_bits != 0);
  out[0] = pl.ok;
  out[1] = pl.tiles_r;
  out[2] = pl.tiles_c;
  out[3] = pl.launches;
  out[4] = (int64_t)pl.bits_bytes;
  out[5] = (int64_t)pl.bytes;
  if (grid)
    for (int d = 0; d < pl.launches; ++d) grid[d] = (int64_t)ea_diag_tiles(d, pl.tiles_r, pl.tiles_c) * n;
  return CASR_OK;
}

int64_t casr_edit_align_workspace_bytes(const casr_handle* h) { return h ? (int64_t)h->eaws.n : -1; }

int casr_edit_align(casr_handle* h, const int32_t* a, const int32_t* a_len, int La, const int32_t* b,
                    const int32_t* b_len, int Lb, int n, int32_t* dist, int32_t* ops, int32_t* b_of_a, int32_t* a_of_b,
                    void* stream) {
  if (!h || n < 0 || (n > 0 && (!a || !a_len || !b || !b_len || !dist)))
    return fail(h, CASR_ERR_ARG, "casr_edit_align: NULL argument or n < 0");
  if (La < 1 || Lb < 1 || La > EA_MAX_LEN || Lb > EA_MAX_LEN)
    return fail(h, CASR_ERR_UNSUPPORTED, "casr_edit_align: La = %d, Lb = %d not in [1, %d]", La, Lb, EA_MAX_LEN);
  const EaPlan pl = edit_align_plan(La, Lb, n, ops || b_of_a || a_of_b);
  if (!pl.ok)
    return fail(h, CASR_ERR_UNSUPPORTED, "casr_edit_align: the direction bits of %d pairs of %d x %d pass %zu bytes", n,
                La, Lb, EA_BITS_LIMIT);
  if (n == 0) return CASR_OK;
  HIP_OK(h, hipSetDevice(h->device));
  if (!guard_words(h)) return fail(h, CASR_ERR_HIP, "casr_edit_align: no guard words");
  HIP_OK(h, h->eaws.ensure(pl.bytes));
  HIP_OK(h, run_edit_align(a, a_len, La, b, b_len, Lb, n, dist, ops, b_of_a, a_of_b, h->eaws.p, GUARD(h, 0),
                           (hipStream_t)stream));
  return CASR_OK;
}

int casr_align_path_host(const float* align, const int32_t* enc_len, const int32_t* tgt_len, int B, int Tp, int L,
                         int32_t* first, int32_t* last, int32_t* peak, int32_t* path_score) {
  if (!align || !enc_len || !tgt_len || !first || !last || !peak || B < 1 || Tp < 1 || L < 1 || L > ALIGN_MAX_L)
    return fail(nullptr, CASR_ERR_ARG, "casr_align_path_host: NULL argument, B or Tp < 1, or L outside [1, %d]",
                ALIGN_MAX_L);
  for (int b = 0; b < B; ++b) {
    int T = enc_len[b], n = tgt_len[b];
    align_clamp(T, Tp);
    align_clamp(n, L);
    const int32_t s = align_path_utterance(align + b, (size_t)Tp * B, (size_t)B, T, n, L, first + (size_t)b * L,
                                           last + (size_t)b * L, peak + (size_t)b * L);
    if (path_score) path_score[b] = s;
  }
  return CASR_OK;
}

int casr_align_path(casr_handle* h, const float* align, const int32_t* enc_len, const int32_t* tgt_len, int B, int Tp,
                    int L, int32_t* first, int32_t* last, int32_t* peak, int32_t* path_score, void* stream) {
  if (!h || !align || !enc_len || !tgt_len || !first || !last || !peak || B < 1 || Tp < 1 || L < 1 || L > ALIGN_MAX_L)
    return fail(h, CASR_ERR_ARG, "casr_align_path: NULL argument, B or Tp < 1, or L outside [1, %d]", ALIGN_MAX_L);
  if (Tp > ALIGN_MAX_TP)
    return fail(h, CASR_ERR_UNSUPPORTED, "casr_align_path: Tp = %d > %d (the move bits stay in LDS)", Tp, ALIGN_MAX_TP);
  HIP_OK(h, hipSetDevice(h->device));
  if (!guard_words(h)) return fail(h, CASR_ERR_HIP, "casr_align_path: no guard words");
  HIP_OK(h, launch_align_path(align, enc_len, tgt_len, B, Tp, L, h->tune[CASR_OPT_ALIGN_GROUP], first, last, peak,
                              path_score, GUARD(h, 0), (hipStream_t)stream));
  return CASR_OK;
}

// the posterior scale of casr_mbr_host, casr_beam_mbr, casr_posterior_units_host and casr_beam_confusion
static int scale_checked(casr_handle* h, const char* who, double scale) {
  if (!(scale >= 0.0) || !std::isfinite(scale))
    return fail(h, CASR_ERR_ARG, "%s: scale %g is negative or not finite", who, scale);
  return CASR_OK;
}

int casr_mbr_host(const int32_t* rec_tokens, const float* rec_score, const uint8_t* rec_valid, const float* rec_lm,
                  int B, int max_len, int k, double scale, double lm_weight, double length_weight, int32_t* best_index,
                  double* rec_risk) {
  if (B < 0 || max_len < 1 || k < 1 || (B > 0 && (!rec_tokens || !rec_score || !rec_valid || !best_index)))
    return fail(nullptr, CASR_ERR_ARG, "casr_mbr_host: NULL argument, B < 0, or max_len or k < 1");
  if (int rs = scale_checked(nullptr, "casr_mbr_host", scale)) return rs;
  const size_t LK = (size_t)max_len * k;
  for (int b = 0; b < B; ++b)
    best_index[b] = mbr_utterance_host(rec_tokens + b * LK * max_len, rec_score + b * LK, rec_valid + b * LK,
                                       rec_lm ? rec_lm + b * LK : nullptr, max_len, k, scale, lm_weight, length_weight,
                                       rec_risk ? rec_risk + b * LK : nullptr);
  return CASR_OK;
}

int casr_beam_mbr(casr_handle* h, double scale, const float* rec_lm, double lm_weight, double length_weight,
                  int32_t* best_tokens, int32_t* best_len, float* best_score, int32_t* best_index, double* best_risk,
                  double* rec_risk, void* stream) {
  if (!h || !best_tokens || !best_len || !best_score)
    return fail(h, CASR_ERR_ARG, "casr_beam_mbr: NULL handle, best_tokens, best_len or best_score");
  if (int rs = scale_checked(h, "casr_beam_mbr", scale)) return rs;
  const int rc = beam_readable(h, READ_MBR, "the fallback assumes the scores of a casr_beam");
  if (rc) return rc;
  const BeamTree& t = h->tree;
  if (!mbr_supported(t.L, t.k))
    return fail(h, CASR_ERR_UNSUPPORTED, "casr_beam_mbr: max_len %d x k %d: distances are bytes (max_len <= %d) and the tree must fit 64 KB of LDS",
                t.L, t.k, EDIT_MBR_MAX_LEN);
  HIP_OK(h, hipSetDevice(h->device));
  MbrBufs w{};
  HIP_OK(h, h->mbrws.ensure(carve_mbr(nullptr, t.B, t.L, t.k, w)));
  carve_mbr(h->mbrws.p, t.B, t.L, t.k, w);
  h->beam.mbr = true;
  HIP_OK(h, run_beam_mbr(t, w, h->tune[CASR_OPT_MBR_MAP], scale, rec_lm, lm_weight, length_weight, h->beam.lm_weight,
                         h->beam.length_weight, best_tokens, best_len, best_score, best_index, best_risk, rec_risk,
                         (hipStream_t)stream));
  return CASR_OK;
}

int casr_beam_mbr_distances(casr_handle* h, uint8_t* dist, int32_t* n_rec, void* stream) {
  if (!h || !dist) return fail(h, CASR_ERR_ARG, "casr_beam_mbr_distances: NULL handle or output");
  const int rc = beam_readable(h, READ_MBR_DISTANCES);
  if (rc) return rc;
  const BeamTree& t = h->tree;
  HIP_OK(h, hipSetDevice(h->device));
  MbrBufs w{};
  carve_mbr(h->mbrws.p, t.B, t.L, t.k, w);
  HIP_OK(h, run_mbr_distances(t, w, dist, n_rec, (hipStream_t)stream));
  return CASR_OK;
}

int casr_posterior_units_host(const float* rec_score, const uint8_t* rec_valid, const float* rec_lm, int B,
                              int max_len, int k, double scale, double lm_weight, double length_weight,
                              int64_t* rec_unit, int64_t* total) {
  if (B < 0 || max_len < 1 || k < 1 || (B > 0 && (!rec_score || !rec_valid || !rec_unit)))
    return fail(nullptr, CASR_ERR_ARG, "casr_posterior_units_host: NULL argument, B < 0, or max_len or k < 1");
  if (int rs = scale_checked(nullptr, "casr_posterior_units_host", scale)) return rs;
  const size_t LK = (size_t)max_len * k;
  for (int b = 0; b < B; ++b) {
    const int64_t U = cn_units_utterance_host(rec_score + b * LK, rec_valid + b * LK, rec_lm ? rec_lm + b * LK : nullptr,
                                              max_len, k, scale, lm_weight, length_weight, rec_unit + b * LK);
    if (total) total[b] = U;
  }
  return CASR_OK;
}

int casr_nbest_host(const int32_t* rec_tokens, const float* rec_score, const uint8_t* rec_valid,
                    const float* rec_lm, int B, int max_len, int k, int N, double lm_weight, double length_weight,
                    int32_t* nbest_index, int32_t* nbest_tokens, int32_t* nbest_len, double* nbest_comb) {
  if (B < 0 || max_len < 1 || k < 1 ||
      (B > 0 && (!rec_tokens || !rec_score || !rec_valid || !nbest_index || !nbest_tokens || !nbest_len || !nbest_comb)))
    return fail(nullptr, CASR_ERR_ARG, "casr_nbest_host: NULL argument, B < 0, or max_len or k < 1");
  if (N < 1 || N > CN_MAX_N) return fail(nullptr, CASR_ERR_ARG, "casr_nbest_host: N = %d not in [1, %d]", N, CN_MAX_N);
  const size_t LK = (size_t)max_len * k;
  for (int b = 0; b < B; ++b)
    cn_nbest_utterance_host(rec_tokens + b * LK * max_len, rec_score + b * LK, rec_valid + b * LK,
                            rec_lm ? rec_lm + b * LK : nullptr, max_len, k, N, lm_weight, length_weight,
                            nbest_index + (size_t)b * N, nbest_tokens + (size_t)b * N * max_len,
                            nbest_len + (size_t)b * N, nbest_comb + (size_t)b * N);
  return CASR_OK;
}

int casr_confusion_host(const int32_t* rec_tokens, const uint8_t* rec_valid, const int64_t* rec_unit,
                        const int32_t* pivot, int B, int max_len, int k, int vocab, int M, int32_t* n_slots,
                        int32_t* slot_token, int64_t* slot_mass, int64_t* pivot_mass, int64_t* total) {
  if (B < 0 || max_len < 1 || k < 1 || vocab < 1 ||
      (B > 0 && (!rec_tokens || !rec_valid || !rec_unit || !pivot || !n_slots || !slot_token || !slot_mass ||
                 !pivot_mass || !total)))
    return fail(nullptr, CASR_ERR_ARG, "casr_confusion_host: NULL argument, B < 0, or max_len, k or vocab < 1");
  if (M < 1 || M > CN_MAX_M) return fail(nullptr, CASR_ERR_ARG, "casr_confusion_host: M = %d not in [1, %d]", M, CN_MAX_M);
  const size_t LK = (size_t)max_len * k, SM = (size_t)cn_slots(max_len);
  for (int b = 0; b < B; ++b)
    n_slots[b] = cn_confusion_utterance_host(rec_tokens + b * LK * max_len, rec_valid + b * LK, rec_unit + b * LK,
                                             pivot[b], max_len, k, vocab, M, slot_token + b * SM * M,
                                             slot_mass + b * SM * M, pivot_mass + (size_t)b * max_len, total + b);
  return CASR_OK;
}

int casr_confusion(casr_handle* h, const int32_t* rec_tokens, const uint8_t* rec_valid, const int64_t* rec_unit,
                   const int32_t* pivot, int B, int max_len, int k, int vocab, int M, int32_t* n_slots,
                   int32_t* slot_token, int64_t* slot_mass, int64_t* pivot_mass, int64_t* total, void* stream) {
  if (!h || !rec_tokens || !rec_valid || !rec_unit || !pivot || !n_slots || !slot_token || !slot_mass || !pivot_mass ||
      !total || B < 1 || B > 65535 || max_len < 1 || k < 1 || vocab < 1)
    return fail(h, CASR_ERR_ARG, "casr_confusion: NULL argument, B outside [1, 65535], or max_len, k or vocab < 1");
  if (M < 1 || M > CN_MAX_M) return fail(h, CASR_ERR_ARG, "casr_confusion: M = %d not in [1, %d]", M, CN_MAX_M);
  if (!confusion_supported(B, max_len, k, vocab, false))
    return fail(h, CASR_ERR_UNSUPPORTED, "casr_confusion: max_len %d (<= %d), k %d (<= %d), vocab %d (<= %d) and the masses must fit the LDS",
                max_len, CN_MAX_LEN, k, CN_MAX_K, vocab, CN_MAX_VOCAB);
  HIP_OK(h, hipSetDevice(h->device));
  if (!guard_words(h)) return fail(h, CASR_ERR_HIP, "casr_confusion: no guard words");
  CnBufs w{};
  HIP_OK(h, h->cnws.ensure(carve_confusion(nullptr, B, max_len, k, true, w)));
  carve_confusion(h->cnws.p, B, max_len, k, true, w);
  HIP_OK(h, run_confusion(w, rec_tokens, rec_valid, rec_unit, pivot, B, max_len, k, vocab, M, n_slots, slot_token,
                          slot_mass, pivot_mass, total, GUARD(h, 0), (hipStream_t)stream));
  return CASR_OK;
}

// the refusals casr_beam_nbest and casr_beam_confusion share: the gate, and the lists' length limit
static int beam_comb_readable(casr_handle* h, int reader) {
  const int rc = beam_readable(h, reader, "c is the comb of a casr_beam's records");
  if (rc) return rc;
  if (h->tree.L > CN_MAX_LEN)
    return fail(h, CASR_ERR_UNSUPPORTED, "%s: max_len %d (<= %d)", BEAM_READER_NAME[reader], h->tree.L, CN_MAX_LEN);
  return CASR_OK;
}

int casr_beam_nbest(casr_handle* h, int N, const float* rec_lm, double lm_weight, double length_weight,
                    int32_t* nbest_index, int32_t* nbest_tokens, int32_t* nbest_len, double* nbest_comb,
                    void* stream) {
  if (!h || !nbest_index || !nbest_tokens || !nbest_len || !nbest_comb)
    return fail(h, CASR_ERR_ARG, "casr_beam_nbest: NULL handle or output");
  if (N < 1 || N > CN_MAX_N) return fail(h, CASR_ERR_ARG, "casr_beam_nbest: N = %d not in [1, %d]", N, CN_MAX_N);
  const int rc = beam_comb_readable(h, READ_NBEST);
  if (rc) return rc;
  const BeamTree& t = h->tree;
  HIP_OK(h, hipSetDevice(h->device));
  CnBufs w{};
  HIP_OK(h, h->cnws.ensure(carve_confusion(nullptr, t.B, t.L, t.k, false, w)));
  carve_confusion(h->cnws.p, t.B, t.L, t.k, false, w);
  HIP_OK(h, run_beam_nbest(t, w, N, rec_lm, lm_weight, length_weight, nbest_index, nbest_tokens, nbest_len, nbest_comb,
                           (hipStream_t)stream));
  return CASR_OK;
}

int casr_beam_confusion(casr_handle* h, int M, double scale, const float* rec_lm, double lm_weight,
                        double length_weight, const int32_t* pivot, int32_t* n_slots, int32_t* slot_token,
                        int64_t* slot_mass, int64_t* pivot_mass, int64_t* total, int64_t* rec_unit, void* stream) {
  if (!h || !n_slots || !slot_token || !slot_mass || !pivot_mass || !total)
    return fail(h, CASR_ERR_ARG, "casr_beam_confusion: NULL handle or output");
  if (M < 1 || M > CN_MAX_M) return fail(h, CASR_ERR_ARG, "casr_beam_confusion: M = %d not in [1, %d]", M, CN_MAX_M);
  if (int rs = scale_checked(h, "casr_beam_confusion", scale)) return rs;
  const int rc = beam_comb_readable(h, READ_CONFUSION);
  if (rc) return rc;
  const BeamTree& t = h->tree;
  // the network's own limits (casr_beam_nbest has none of them)
  if (!confusion_supported(t.B, t.L, t.k, t.V, true))
    return fail(h, CASR_ERR_UNSUPPORTED, "casr_beam_confusion: k %d, vocab %d (<= %d): votes are int16 and the masses must fit the LDS",
                t.k, t.V, CN_MAX_VOCAB);
  HIP_OK(h, hipSetDevice(h->device));
  CnBufs w{};
  HIP_OK(h, h->cnws.ensure(carve_confusion(nullptr, t.B, t.L, t.k, true, w)));
  carve_confusion(h->cnws.p, t.B, t.L, t.k, true, w);
  HIP_OK(h, run_beam_confusion(t, w, M, scale, rec_lm, lm_weight, length_weight, pivot, n_slots, slot_token, slot_mass,
                               pivot_mass, total, rec_unit, (hipStream_t)stream));
  return CASR_OK;
}

// casr_lm_terms, casr_beam_lm, casr_beam_bias: lm_matches_handle, and a term row fits its LDS
static int lm_on_handle(casr_handle* h, const casr_lm* lm, const char* who) {
  const int rc = lm_matches_handle(h, lm, who);
  if (rc) return rc;
  if (!lm_terms_supported(lm->host.V))
    return fail(h, CASR_ERR_UNSUPPORTED, "%s: a term row of %d words is past the %d KB of LDS it is assembled in", who,
                lm->host.V, (int)(LM_TERMS_LDS_BYTES / 1024));
  return CASR_OK;
}

int casr_lm_terms_host(const casr_lm* lm, const int32_t* ctx, const int32_t* nc, int n, int eos_token, float* terms) {
  if (!lm || n < 0 || (n > 0 && (!ctx || !nc || !terms)))
    return fail(nullptr, CASR_ERR_ARG, "casr_lm_terms_host: NULL argument or n < 0");
  const NgramView m = lm->host.view();
  const NgramSuccView sv = lm->succ.view();
  bool bad = false;
  for (int i = 0; i < n; ++i)
    ngram_terms_row(m, sv, ctx + (size_t)i * (NGRAM_MAX_ORDER - 1), nc[i], eos_token, terms + (size_t)i * m.V, &bad);
  return CASR_OK;
}

int casr_lm_terms(casr_handle* h, const casr_lm* lm, const int32_t* ctx, const int32_t* nc, int n, int eos_token,
                  float* terms, void* stream) {
  if (!h || !lm || n < 0 || (n > 0 && (!ctx || !nc || !terms)))
    return fail(h, CASR_ERR_ARG, "casr_lm_terms: NULL argument or n < 0");
  int rc = lm_on_handle(h, lm, "casr_lm_terms");
  if (rc) return rc;
  HIP_OK(h, hipSetDevice(h->device));
  if (!guard_words(h)) return fail(h, CASR_ERR_HIP, "casr_lm_terms: no guard words");
  const LmTermsSrc src{0, ctx, nc, nullptr, nullptr, nullptr, 0, 1, 0, 0};
  HIP_OK(h, launch_lm_terms(lm->dview, lm->dsucc, src, n, eos_token, terms, GUARD(h, 0), (hipStream_t)stream));
  return CASR_OK;
}

int casr_beam_lm(casr_handle* h, const casr_lm* lm, int k, float lm_weight, float length_weight,
                 int32_t* best_tokens, int32_t* best_len, float* best_score, float* best_lm, int32_t* steps,
                 void* stream) {
  if (!h || !lm || !best_tokens || !best_len || !best_score || !best_lm || !steps)
    return fail(h, CASR_ERR_ARG, "casr_beam_lm: NULL handle, LM or output");
  if (!h->W) return fail(h, CASR_ERR_STATE, "casr_beam_lm before casr_bind_weights");
  if (!h->encoded) return fail(h, CASR_ERR_STATE, "casr_beam_lm before casr_encode");
  int rc = lm_on_handle(h, lm, "casr_beam_lm");
  if (rc) return rc;
  HIP_OK(h, hipSetDevice(h->device));
  DecodeCall c;
  rc = prepare_decode(h, PLAN_BEAM_LM, k, false, c);
  if (rc) return rc;
  const DecodeArgs& a = c.a;
  BeamLmBufs w{};
  HIP_OK(h, h->lmws.ensure(carve_beam_lm(nullptr, a.B, a.plan.R, a.max_len, a.k, a.V, w)));
  carve_beam_lm(h->lmws.p, a.B, a.plan.R, a.max_len, a.k, a.V, w);
  beam_ran(h, BEAM_LM, a, lm_weight, length_weight);
  // (never a hipGraph: launched eagerly whatever casr_set_graphs says)
  dg_trace_init();  // CASR_DG_TRACE diagnostics only
  HIP_OK(h, run_beam_lm(a, h->d, w, lm->dview, lm->dsucc, lm_weight, length_weight, best_tokens, best_len, best_score,
                        best_lm, steps, (hipStream_t)stream));
  dg_trace_dump();
  return CASR_OK;
}

int casr_beam_record_lm(casr_handle* h, float* rec_lm, void* stream) {
  const int rc = beam_readable(h, READ_RECORD_LM);
  if (rc) return rc;
  if (!rec_lm) return fail(h, CASR_ERR_ARG, "casr_beam_record_lm: NULL output");
  const BeamTree& t = h->tree;
  HIP_OK(h, hipSetDevice(h->device));
  BeamLmBufs w{};
  carve_beam_lm(h->lmws.p, t.B, t.B * t.k, t.L, t.k, t.V, w);
  HIP_OK(h, run_beam_record_lm(t, w, rec_lm, (hipStream_t)stream));
  return CASR_OK;
}

int casr_bias_create(int device, int vocab, int n_phrases, const int32_t* tokens, const int32_t* lens,
                     const int32_t* boost, casr_bias** out) {
  if (!out) return fail(nullptr, CASR_ERR_ARG, "casr_bias_create: out is NULL");
  *out = nullptr;
  if (device < -1) return fail(nullptr, CASR_ERR_ARG, "casr_bias_create: device %d", device);
  casr_bias* bo = new casr_bias();
  std::string why;
  const int rc = bias_build(vocab, n_phrases, tokens, lens, boost, &bo->host, &why);
  if (rc != BIAS_OK) {
    delete bo;
    return fail(nullptr, rc, "casr_bias_create: %s", why.c_str());
  }
  bo->device = device;
  if (device >= 0) {
    const BiasTables& t = bo->host;
    const void* src[5] = {t.node.data(), t.ctok.data(), t.cnext.data(), t.root_next.data(), t.root_gain.data()};
    const size_t bytes[5] = {t.node.size() * sizeof(BiasNode), t.ctok.size() * sizeof(int32_t),
                             t.cnext.size() * sizeof(int32_t), t.root_next.size() * sizeof(int32_t),
                             t.root_gain.size() * sizeof(int32_t)};
    const hipError_t e = upload_tables(device, 5, src, bytes, bo->dev);  // (no phrases: the root has no children)
    if (e != hipSuccess) {
      casr_bias_destroy(bo);
      return fail(nullptr, CASR_ERR_HIP, "casr_bias_create: %s", hipGetErrorString(e));
    }
    bo->dview = BiasView{t.V, (int)t.node.size(), static_cast<const BiasNode*>(bo->dev[0]),
                         static_cast<const int32_t*>(bo->dev[1]), static_cast<const int32_t*>(bo->dev[2]),
                         static_cast<const int32_t*>(bo->dev[3]), static_cast<const int32_t*>(bo->dev[4])};
  }
  *out = bo;
  return CASR_OK;
}

void casr_bias_destroy(casr_bias* bias) {
  if (!bias) return;
  if (bias->device >= 0 && hipSetDevice(bias->device) == hipSuccess)
    for (void* p : bias->dev)
      if (p) (void)hipFree(p);
  delete bias;
}

int casr_bias_score_host(const casr_bias* bias, const int32_t* tokens, const int32_t* lens, int n, int L,
                         int32_t* full, int32_t* tail, int32_t* state) {
  if (!bias || n < 0 || L < 0 || (n > 0 && (!lens || (!tokens && L > 0))))
    return fail(nullptr, CASR_ERR_ARG, "casr_bias_score_host: NULL argument, n < 0 or L < 0");
  for (int i = 0; i < n; ++i)
    if (lens[i] < 0 || lens[i] > L)
      return fail(nullptr, CASR_ERR_ARG, "casr_bias_score_host: lens[%d] = %d not in [0, %d]", i, lens[i], L);
  const BiasView m = bias->host.view();
  for (int i = 0; i < n; ++i) {
    int32_t f, t, s;
    bias_sentence(m, tokens + (size_t)i * L, lens[i], &f, &t, &s);
    if (full) full[i] = f;
    if (tail) tail[i] = t;
    if (state) state[i] = s;
  }
  return CASR_OK;
}

// the refusals casr_bias_score, casr_bias_rows and casr_beam_bias share
static int bias_on_handle(casr_handle* h, const casr_bias* bias, const char* who) {
  if (bias->device != h->device)
    return fail(h, CASR_ERR_ARG, "%s: the bias object is %s, the handle on device %d", who,
                bias->device < 0 ? "host-only" : "on another device", h->device);
  if (bias->host.V != h->cfg.vocab)
    return fail(h, CASR_ERR_ARG, "%s: the bias object's vocab %d is not the handle's %d", who, bias->host.V,
                h->cfg.vocab);
  return CASR_OK;
}

int casr_bias_score(casr_handle* h, const casr_bias* bias, const int32_t* tokens, const int32_t* lens, int n,
                    int L, int32_t* full, int32_t* tail, int32_t* state, void* stream) {
  if (!h || !bias || n < 0 || (n > 0 && (!tokens || !lens)))
    return fail(h, CASR_ERR_ARG, "casr_bias_score: NULL argument or n < 0");
  int rc = bias_on_handle(h, bias, "casr_bias_score");
  if (rc) return rc;
  if (L < 1 || L > BIAS_MAX_SENT)
    return fail(h, CASR_ERR_UNSUPPORTED, "casr_bias_score: L = %d not in [1, %d]", L, BIAS_MAX_SENT);
  HIP_OK(h, hipSetDevice(h->device));
  if (!guard_words(h)) return fail(h, CASR_ERR_HIP, "casr_bias_score: no guard words");
  HIP_OK(h, launch_bias_score(bias->dview, tokens, lens, n, L, full, tail, state, GUARD(h, 0), (hipStream_t)stream));
  return CASR_OK;
}

int casr_bias_rows_host(const casr_bias* bias, const int32_t* state, int n, int32_t* gain, int32_t* next) {
  if (!bias || n < 0 || (n > 0 && (!state || !gain)))
    return fail(nullptr, CASR_ERR_ARG, "casr_bias_rows_host: NULL argument or n < 0");
  const BiasView m = bias->host.view();
  for (int i = 0; i < n; ++i)
    if (state[i] < 0 || state[i] >= m.n_nodes)
      return fail(nullptr, CASR_ERR_ARG, "casr_bias_rows_host: state[%d] = %d not in [0, %d)", i, state[i], m.n_nodes);
  for (int i = 0; i < n; ++i)
    bias_row_host(m, state[i], gain + (size_t)i * m.V, next ? next + (size_t)i * m.V : nullptr);
  return CASR_OK;
}

int casr_bias_rows(casr_handle* h, const casr_bias* bias, const int32_t* state, int n, int32_t* gain,
                   int32_t* next, void* stream) {
  if (!h || !bias || n < 0 || (n > 0 && (!state || !gain)))
    return fail(h, CASR_ERR_ARG, "casr_bias_rows: NULL argument or n < 0");
  int rc = bias_on_handle(h, bias, "casr_bias_rows");
  if (rc) return rc;
  if (!bias_rows_supported(bias->host.V))
    return fail(h, CASR_ERR_UNSUPPORTED, "casr_bias_rows: a row of %d words is past the %d KB of LDS it is assembled in",
                bias->host.V, (int)(BIAS_ROWS_LDS_BYTES / 1024));
  HIP_OK(h, hipSetDevice(h->device));
  if (!guard_words(h)) return fail(h, CASR_ERR_HIP, "casr_bias_rows: no guard words");
  const BiasRowsSrc src{0, state, nullptr, 0, 1, 0};
  HIP_OK(h, launch_bias_rows(bias->dview, src, n, gain, next, GUARD(h, 0), (hipStream_t)stream));
  return CASR_OK;
}

int casr_beam_bias(casr_handle* h, const casr_bias* bias, const casr_lm* lm, int k, float bias_weight,
                   float lm_weight, float length_weight, int32_t* best_tokens, int32_t* best_len,
                   float* best_score, float* best_lm, float* best_bias, int32_t* steps, void* stream) {
  if (!h || !bias || !best_tokens || !best_len || !best_score || !best_bias || !steps)
    return fail(h, CASR_ERR_ARG, "casr_beam_bias: NULL handle, bias object or output");
  if (!h->W) return fail(h, CASR_ERR_STATE, "casr_beam_bias before casr_bind_weights");
  if (!h->encoded) return fail(h, CASR_ERR_STATE, "casr_beam_bias before casr_encode");
  int rc = bias_on_handle(h, bias, "casr_beam_bias");
  if (rc) return rc;
  if (!bias_rows_supported(bias->host.V))
    return fail(h, CASR_ERR_UNSUPPORTED, "casr_beam_bias: a row of %d words is past the %d KB of LDS it is assembled in",
                bias->host.V, (int)(BIAS_ROWS_LDS_BYTES / 1024));
  if (lm) {
    rc = lm_on_handle(h, lm, "casr_beam_bias");
    if (rc) return rc;
  }
  HIP_OK(h, hipSetDevice(h->device));
  DecodeCall c;
  rc = prepare_decode(h, PLAN_BEAM_LM, k, false, c);
  if (rc) return rc;
  const DecodeArgs& a = c.a;
  BeamLmBufs lw{};
  if (lm) {
    HIP_OK(h, h->lmws.ensure(carve_beam_lm(nullptr, a.B, a.plan.R, a.max_len, a.k, a.V, lw)));
    carve_beam_lm(h->lmws.p, a.B, a.plan.R, a.max_len, a.k, a.V, lw);
  }
  BeamBiasBufs w{};
  HIP_OK(h, h->biasws.ensure(carve_beam_bias(nullptr, a.B, a.plan.R, a.max_len, a.k, a.V, w)));
  carve_beam_bias(h->biasws.p, a.B, a.plan.R, a.max_len, a.k, a.V, w);
  beam_ran(h, lm ? BEAM_BIAS_LM : BEAM_BIAS, a, lm_weight, length_weight);  // (with an LM casr_beam_record_lm reads lmws)
  // (never a hipGraph: launched eagerly whatever casr_set_graphs says)
  dg_trace_init();  // CASR_DG_TRACE diagnostics only
  HIP_OK(h, run_beam_bias(a, h->d, lm ? &lw : nullptr, w, bias->dview, lm ? &lm->dview : nullptr,
                          lm ? &lm->dsucc : nullptr, bias_weight, lm_weight, length_weight, best_tokens, best_len,
                          best_score, lm ? best_lm : nullptr, best_bias, steps, (hipStream_t)stream));
  dg_trace_dump();
  return CASR_OK;
}

int casr_beam_record_bias(casr_handle* h, float* rec_bias, void* stream) {
  const int rc = beam_readable(h, READ_RECORD_BIAS);
  if (rc) return rc;
  if (!rec_bias) return fail(h, CASR_ERR_ARG, "casr_beam_record_bias: NULL output");
  const BeamTree& t = h->tree;
  HIP_OK(h, hipSetDevice(h->device));
  BeamBiasBufs w{};
  carve_beam_bias(h->biasws.p, t.B, t.B * t.k, t.L, t.k, t.V, w);
  HIP_OK(h, run_beam_record_bias(t, w, rec_bias, (hipStream_t)stream));
  return CASR_OK;
}

int casr_grammar_create(int device, int vocab, int eos_token, int n_states, const int64_t* arc_off,
                        const int32_t* arc_tok, const int32_t* arc_next, const uint8_t* is_final, casr_grammar** out) {
  if (!out) return fail(nullptr, CASR_ERR_ARG, "casr_grammar_create: out is NULL");
  *out = nullptr;
  if (device < -1) return fail(nullptr, CASR_ERR_ARG, "casr_grammar_create: device %d", device);
  casr_grammar* go = new casr_grammar();
  std::string why;
  const int rc = gram_build(vocab, eos_token, n_states, arc_off, arc_tok, arc_next, is_final, &go->host, &why);
  if (rc != GRAM_OK) {
    delete go;
    return fail(nullptr, rc, "casr_grammar_create: %s", why.c_str());
  }
  go->device = device;
  if (device >= 0) {
    const GrammarTables& t = go->host;
    const void* src[6] = {t.arc_off.data(), t.arc_tok.data(),  t.arc_next.data(),
                          t.arc_dist.data(), t.dist.data(), t.is_final.data()};
    const size_t bytes[6] = {t.arc_off.size() * sizeof(int32_t), t.arc_tok.size() * sizeof(int32_t),
                             t.arc_next.size() * sizeof(int32_t), t.arc_dist.size() * sizeof(int32_t),
                             t.dist.size() * sizeof(int32_t), t.is_final.size()};
    const hipError_t e = upload_tables(device, 6, src, bytes, go->dev);  // (no arcs: empty arrays)
    if (e != hipSuccess) {
      casr_grammar_destroy(go);
      return fail(nullptr, CASR_ERR_HIP, "casr_grammar_create: %s", hipGetErrorString(e));
    }
    go->dview = GrammarView{t.V, t.eos, t.n_states(), static_cast<const int32_t*>(go->dev[0]),
                            static_cast<const int32_t*>(go->dev[1]), static_cast<const int32_t*>(go->dev[2]),
                            static_cast<const int32_t*>(go->dev[3]), static_cast<const int32_t*>(go->dev[4]),
                            static_cast<const uint8_t*>(go->dev[5])};
  }
  *out = go;
  return CASR_OK;
}

void casr_grammar_destroy(casr_grammar* g) {
  if (!g) return;
  if (g->device >= 0 && hipSetDevice(g->device) == hipSuccess)
    for (void* p : g->dev)
      if (p) (void)hipFree(p);
  delete g;
}

int casr_grammar_info(const casr_grammar* g, int32_t* n_states, int64_t* n_arcs, int32_t* dist) {
  if (!g) return fail(nullptr, CASR_ERR_ARG, "casr_grammar_info: the grammar is NULL");
  if (n_states) *n_states = g->host.n_states();
  if (n_arcs) *n_arcs = (int64_t)g->host.arc_tok.size();
  if (dist) std::memcpy(dist, g->host.dist.data(), g->host.dist.size() * sizeof(int32_t));
  return CASR_OK;
}

int casr_grammar_mask_words(int vocab) { return vocab < 1 ? 0 : gram_mask_words(vocab); }

int casr_grammar_accept_host(const casr_grammar* g, const int32_t* tokens, const int32_t* lens, int n, int L,
                             int32_t* consumed, int32_t* state, uint8_t* accepted) {
  if (!g || n < 0 || L < 0 || (n > 0 && (!lens || (!tokens && L > 0))))
    return fail(nullptr, CASR_ERR_ARG, "casr_grammar_accept_host: NULL argument, n < 0 or L < 0");
  for (int i = 0; i < n; ++i)
    if (lens[i] < 0 || lens[i] > L)
      return fail(nullptr, CASR_ERR_ARG, "casr_grammar_accept_host: lens[%d] = %d not in [0, %d]", i, lens[i], L);
  const GrammarView m = g->host.view();
  for (int i = 0; i < n; ++i) {
    int32_t c, s;
    uint8_t ok;
    gram_sentence(m, tokens + (size_t)i * L, lens[i], &c, &s, &ok);
    if (consumed) consumed[i] = c;
    if (state) state[i] = s;
    if (accepted) accepted[i] = ok;
  }
  return CASR_OK;
}

// the refusals casr_grammar_accept, casr_grammar_rows and casr_beam_grammar share
static int grammar_on_handle(casr_handle* h, const casr_grammar* g, const char* who) {
  if (g->device != h->device)
    return fail(h, CASR_ERR_ARG, "%s: the grammar is %s, the handle on device %d", who,
                g->device < 0 ? "host-only" : "on another device", h->device);
  if (g->host.V != h->cfg.vocab)
    return fail(h, CASR_ERR_ARG, "%s: the grammar's vocab %d is not the handle's %d", who, g->host.V, h->cfg.vocab);
  if (g->host.eos != h->cfg.eos)
    return fail(h, CASR_ERR_ARG, "%s: the grammar's eos %d is not the handle's %d", who, g->host.eos, h->cfg.eos);
  if (!gram_rows_supported(g->host.V))
    return fail(h, CASR_ERR_UNSUPPORTED, "%s: four mask rows of vocab %d are past the %d KB of LDS they are assembled in",
                who, g->host.V, (int)(GRAM_ROWS_LDS_BYTES / 1024));
  return CASR_OK;
}

int casr_grammar_accept(casr_handle* h, const casr_grammar* g, const int32_t* tokens, const int32_t* lens, int n,
                        int L, int32_t* consumed, int32_t* state, uint8_t* accepted, void* stream) {
  if (!h || !g || n < 0 || (n > 0 && (!tokens || !lens)))
    return fail(h, CASR_ERR_ARG, "casr_grammar_accept: NULL argument or n < 0");
  int rc = grammar_on_handle(h, g, "casr_grammar_accept");
  if (rc) return rc;
  if (L < 1 || L > GRAM_MAX_SENT)
    return fail(h, CASR_ERR_UNSUPPORTED, "casr_grammar_accept: L = %d not in [1, %d]", L, GRAM_MAX_SENT);
  HIP_OK(h, hipSetDevice(h->device));
  if (!guard_words(h)) return fail(h, CASR_ERR_HIP, "casr_grammar_accept: no guard words");
  HIP_OK(h, launch_gram_accept(g->dview, tokens, lens, n, L, consumed, state, accepted, GUARD(h, 0),
                               (hipStream_t)stream));
  return CASR_OK;
}

int casr_grammar_rows_host(const casr_grammar* g, const int32_t* state, const int32_t* budget, int n,
                           uint32_t* mask) {
  if (!g || n < 0 || (n > 0 && (!state || !budget || !mask)))
    return fail(nullptr, CASR_ERR_ARG, "casr_grammar_rows_host: NULL argument or n < 0");
  const GrammarView m = g->host.view();
  for (int i = 0; i < n; ++i)
    if (state[i] != GRAM_DEAD && (state[i] < 0 || state[i] >= m.n_states))
      return fail(nullptr, CASR_ERR_ARG, "casr_grammar_rows_host: state[%d] = %d not -1 or in [0, %d)", i, state[i],
                  m.n_states);
  const int GW = gram_mask_words(m.V);
  bool bad = false;
  for (int i = 0; i < n; ++i) gram_row_host(m, state[i], budget[i], mask + (size_t)i * GW, &bad);
  return CASR_OK;
}

int casr_grammar_rows(casr_handle* h, const casr_grammar* g, const int32_t* state, const int32_t* budget, int n,
                      uint32_t* mask, void* stream) {
  if (!h || !g || n < 0 || (n > 0 && (!state || !budget || !mask)))
    return fail(h, CASR_ERR_ARG, "casr_grammar_rows: NULL argument or n < 0");
  int rc = grammar_on_handle(h, g, "casr_grammar_rows");
  if (rc) return rc;
  HIP_OK(h, hipSetDevice(h->device));
  if (!guard_words(h)) return fail(h, CASR_ERR_HIP, "casr_grammar_rows: no guard words");
  const GramRowsSrc src{0, state, budget, nullptr, 0, 1, 0, 0};
  HIP_OK(h, launch_gram_rows(g->dview, src, n, mask, GUARD(h, 0), (hipStream_t)stream));
  return CASR_OK;
}

int casr_beam_grammar(casr_handle* h, const casr_grammar* g, const casr_lm* lm, const int32_t* start, int k,
                      float lm_weight, float length_weight, int32_t* best_tokens, int32_t* best_len,
                      float* best_score, float* best_lm, uint8_t* complete, int32_t* steps, void* stream) {
  if (!h || !g || !best_tokens || !best_len || !best_score || !complete || !steps)
    return fail(h, CASR_ERR_ARG, "casr_beam_grammar: NULL handle, grammar or output");
  if (!h->W) return fail(h, CASR_ERR_STATE, "casr_beam_grammar before casr_bind_weights");
  if (!h->encoded) return fail(h, CASR_ERR_STATE, "casr_beam_grammar before casr_encode");
  int rc = grammar_on_handle(h, g, "casr_beam_grammar");
  if (rc) return rc;
  if (lm) {
    rc = lm_on_handle(h, lm, "casr_beam_grammar");
    if (rc) return rc;
  }
  HIP_OK(h, hipSetDevice(h->device));
  DecodeCall c;
  rc = prepare_decode(h, PLAN_BEAM_LM, k, false, c);
  if (rc) return rc;
  const DecodeArgs& a = c.a;
  BeamLmBufs lw{};
  if (lm) {
    HIP_OK(h, h->lmws.ensure(carve_beam_lm(nullptr, a.B, a.plan.R, a.max_len, a.k, a.V, lw)));
    carve_beam_lm(h->lmws.p, a.B, a.plan.R, a.max_len, a.k, a.V, lw);
  }
  BeamGramBufs w{};
  HIP_OK(h, h->gramws.ensure(carve_beam_gram(nullptr, a.plan.R, a.V, w)));
  carve_beam_gram(h->gramws.p, a.plan.R, a.V, w);
  beam_ran(h, lm ? BEAM_LM : BEAM_PLAIN, a, lm_weight, length_weight);  // (with an LM casr_beam_record_lm reads lmws)
  h->beam.grammar = true;
  // (never a hipGraph: launched eagerly whatever casr_set_graphs says)
  dg_trace_init();  // CASR_DG_TRACE diagnostics only
  HIP_OK(h, run_beam_grammar(a, h->d, lm ? &lw : nullptr, w, g->dview, lm ? &lm->dview : nullptr,
                             lm ? &lm->dsucc : nullptr, start, lm_weight, length_weight, best_tokens, best_len,
                             best_score, lm ? best_lm : nullptr, complete, steps, (hipStream_t)stream));
  dg_trace_dump();
  return CASR_OK;
}

int casr_device_flags(casr_handle* h, int32_t* flags, void* stream) {
  if (!h || !flags) return fail(h, CASR_ERR_ARG, "casr_device_flags: bad arguments");
  *flags = 0;
  HIP_OK(h, hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  int32_t w[3] = {0, 0, 0};
  if (h->gflags.p) {
    HIP_OK(h, hipMemcpyAsync(w, h->gflags.p, sizeof w, hipMemcpyDeviceToHost, s));
    HIP_OK(h, hipStreamSynchronize(s));
    if (w[0] | w[1] | w[2]) HIP_OK(h, hipMemsetAsync(h->gflags.p, 0, sizeof w, s));  // read and clear
  }
  *flags = w[0] | w[1] | w[2];
  return CASR_OK;
}

int casr_profile_enable(casr_handle* h, uint32_t class_mask) {
  if (!h) return fail(h, CASR_ERR_ARG, "handle NULL");
  h->prof.mask = class_mask;
  h->prof.reset();
  return CASR_OK;
}

int casr_profile_read(casr_handle* h, int cls, int32_t* launches, double* total_ms) {
  if (!h || cls < 0 || cls >= CASR_K_COUNT || !launches || !total_ms)
    return fail(h, CASR_ERR_ARG, "casr_profile_read: bad arguments");
  Profiler& p = h->prof;
  const size_t n = p.used[cls] / 2;
  double ms = 0.0;
  int32_t nl = 0;
  if (n) HIP_OK(h, hipEventSynchronize(p.ev[cls][2 * n - 1]));
  for (size_t i = 0; i < n; ++i) {
    float t = 0.f;
    HIP_OK(h, hipEventElapsedTime(&t, p.ev[cls][2 * i], p.ev[cls][2 * i + 1]));
    ms += t;
    nl += p.weight[cls][i];
  }
  *launches = nl;
  *total_ms = ms;
  return CASR_OK;
}

}  // extern "C"
