// Internal contracts between the casr host code (casr_capi.hip) and the kernel TUs.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "beam_state.h"
#include "bias_plan.h"
#include "casr.h"
#include "encode_plan.h"
#include "grammar_plan.h"
#include "lm_estimate_plan.h"
#include "lm_prune_plan.h"
#include "ngram_succ.h"
#include "ngram_table.h"
#include "resample_design.h"
#include "segment_plan.h"

// the s16 arithmetic of this build (casr_common.h CASR_S16_ONE: the s16x1 build)
#ifndef CASR_S16_ONE
#define CASR_S16_ONE 0
#endif
constexpr int CASR_PREC_S16 = CASR_S16_ONE ? CASR_PREC_S16X1 : CASR_PREC_S16X3;

namespace casr {

// (the dimensions of the deployed configuration: casr_dims.h)

// Device guard bits: a data-dependent index (token id, predecessor row, back-pointer) out of
// range is clamped to a valid one and reported here instead of faulting the GPU.
constexpr int CASR_DEV_BAD_TOKEN = 1;    // decoder input token not in [0, V)
constexpr int CASR_DEV_BAD_SRC = 2;      // predecessor row not in [0, R)
constexpr int CASR_DEV_NAN_LOGITS = 4;   // no finite maximum in a logit row (greedy)
constexpr int CASR_DEV_BAD_CAND = 8;     // beam candidate index not in [0, k*V)
constexpr int CASR_DEV_BAD_BACKPTR = 16; // back-pointer walk left [0, k)
constexpr int CASR_DEV_REC_TIMEOUT = 32; // persistent recurrence: a bounded hand-off wait expired
constexpr int CASR_DEV_BAD_AUDIO = 64;   // front-end: n_samples < 513 (torch.stft raises) or > n_max; convert: n_in outside [0, n_max_in]; segment / gather_segments: frames or a segment out of range
constexpr int CASR_DEV_F16_RANGE = 128;  // s16x3 path: a finite operand beyond the f16 range (>= 65520)

// MFMA-fragment-major weight block: a 16-row x 64-k tile stored as [q=0..3][lane][4] so
// lane l reads row (l&15), k = 16*(l>>4) + 4q + e with one coalesced 16 B load per q.
constexpr int FRAG = 16 * 64;

// Offsets (in floats) of every tensor inside the packed weight blob.
struct Layout {
  size_t enc_wih[CASR_MAX_LAYERS];   // [2*4H][Din]  row-major, gate-interleaved rows
  size_t enc_bias[CASR_MAX_LAYERS];  // [2*4H]       b_ih + b_hh, same row order
  size_t enc_whh[CASR_MAX_LAYERS];   // frag-major [2][H/16][4][H/64]
  size_t emb;                        // [V][E]
  size_t dec_w;                      // frag-major [HD/16][4][KDEC/64]
  size_t dec_b;                      // [4HD] gate-interleaved
  size_t proj_w;                     // frag-major [VP/64 * 4][KPROJ/64], k order [ctx | h]
  size_t proj_b;                     // [VP]
  size_t wencT;                      // [A][C]
  size_t wenc16;                     // [A][C/32][32 hi | 32 lo]: s16 row image of wencT (keys GEMM)
  size_t b_attn;                     // [A]
  size_t w_hidden;                   // [HD][A]
  size_t v;                          // [A]
  size_t info;                       // [64]: info[0] = 1 when the s16x3 images are valid
  // s16x3 images (casr_common.h split16) of the MFMA operands, same float count as the f32 ones
  size_t enc_wih16[CASR_MAX_LAYERS]; // [2*4H][Kp/32][32 hi | 32 lo], Kp = Din rounded up to 64
  size_t enc_whh16[CASR_MAX_LAYERS]; // s16 frag-major [2][H/16][4][H/64] (recurrence.hip)
  size_t emb16;                      // [V][E] split words (split16_word)
  size_t dec_w16;                    // s16 frag-major, same tiling / k order as dec_w
  size_t proj_w16;                   // s16 frag-major, same tiling / k order as proj_w
  size_t total;
  int layers, V, VP;
};

Layout make_layout(const casr_config& cfg);

// Packed row index of (gate g, unit u) for a gate-interleaved LSTM matrix with hidden
// size n_hidden: blocks of 16 units, each block = 4 gates x 16 units.
inline int packed_gate_row(int g, int u) { return (u / 16) * 64 + g * 16 + (u % 16); }
// Encoder input-projection column (Gin) of gate g of unit u within one direction: the four gates
// of a unit are adjacent (16-unit blocks of [unit][gate]), so a recurrence cell reads its gate
// pre-activations with one 16-B load instead of four 4-B loads (recurrence.hip, encoder.hip)
inline int enc_gate_col(int g, int u) { return (u / 16) * 64 + (u % 16) * 4 + g; }

// ---------------------------------------------------------------- launch timing
// Event pairs around launches of enabled kernel classes (casr_profile_enable).
// flush kernel of CASR_OPT_DIAG_COLD (fill.hip): reads n float4 of buf
hipError_t flush_caches(const void* buf, size_t bytes, hipStream_t s);

struct Profiler {
  uint32_t mask = 0;
  uint32_t cold_mask = 0;         // CASR_OPT_DIAG_COLD: classes launched after a cache flush
  const void* cold_buf = nullptr;  // the flush kernel's 1 GiB source
  size_t cold_bytes = 0;
  void cold(int cls, hipStream_t s) const {
    if (((cold_mask >> cls) & 1u) && cold_buf) (void)flush_caches(cold_buf, cold_bytes, s);
  }
  std::vector<hipEvent_t> ev[CASR_K_COUNT];
  std::vector<int> weight[CASR_K_COUNT];  // launches covered by each event pair
  size_t used[CASR_K_COUNT] = {};
  bool on(int cls) const { return (mask >> cls) & 1u; }
  // n > 1: the pair brackets a graph replay of n launches of this class (boundaries included)
  void mark(int cls, hipStream_t s, int n = 1) {
    if (!on(cls)) return;
    if (used[cls] == ev[cls].size()) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return;
      ev[cls].push_back(e);
    }
    if ((used[cls] & 1) == 0) {
      if (weight[cls].size() <= used[cls] / 2) weight[cls].resize(used[cls] / 2 + 1);
      weight[cls][used[cls] / 2] = n;
    }
    (void)hipEventRecord(ev[cls][used[cls]++], s);
  }
  void reset() {
    for (int c = 0; c < CASR_K_COUNT; ++c) used[c] = 0;
  }
  ~Profiler() {
    for (auto& v : ev)
      for (hipEvent_t e : v) (void)hipEventDestroy(e);
  }
};

// RAII begin/end marker
struct ProfScope {
  Profiler* p;
  int cls;
  hipStream_t s;
  ProfScope(Profiler* p_, int c, hipStream_t s_, int n = 1) : p(p_), cls(c), s(s_) {
    if (p) {
      p->cold(cls, s);  // CASR_OPT_DIAG_COLD (measurement only): before the class's first event
      p->mark(cls, s, n);
    }
  }
  ~ProfScope() {
    if (p) p->mark(cls, s);
  }
};

// Instantiated hipGraphs keyed by everything a captured sequence bakes in (shapes, weight
// and workspace pointers, scalar arguments).  A key miss re-captures; a small LRU bound
// keeps stale entries (e.g. after a workspace grew) from piling up.
struct GraphCache {
  struct Entry {
    std::vector<uint64_t> key;
    hipGraphExec_t exec;
  };
  std::vector<Entry> entries;
  hipGraphExec_t find(const std::vector<uint64_t>& key) {
    for (size_t i = 0; i < entries.size(); ++i)
      if (entries[i].key == key) {
        if (i + 1 != entries.size()) std::swap(entries[i], entries.back());
        return entries.back().exec;
      }
    return nullptr;
  }
  void add(std::vector<uint64_t> key, hipGraphExec_t exec) {
    if (entries.size() >= 24) {
      (void)hipGraphExecDestroy(entries.front().exec);
      entries.erase(entries.begin());
    }
    entries.push_back(Entry{std::move(key), exec});
  }
  void clear() {
    for (auto& e : entries) (void)hipGraphExecDestroy(e.exec);
    entries.clear();
  }
  ~GraphCache() { clear(); }
};

// ---------------------------------------------------------------- kernel launchers
// fill.hip (graph-safe replacements for hipMemsetAsync)
hipError_t fill_u32(void* p, uint32_t v, size_t n_words, hipStream_t s);
hipError_t fill_u8(void* p, uint8_t v, size_t n_bytes, hipStream_t s);
// up to FILL_MAX_SEG fills (4-byte words or bytes) / device-to-device copies in one launch
constexpr int FILL_MAX_SEG = 8;
struct FillSeg {
  void* p;
  size_t count;    // elements
  uint32_t v;
  uint32_t bytes;  // element size: 4 or 1
};
struct FillList {
  FillSeg seg[FILL_MAX_SEG];
  int n = 0;
  void add32(void* p, uint32_t v, size_t n_words) { seg[n++] = FillSeg{p, n_words, v, 4}; }
  void add8(void* p, uint8_t v, size_t n_bytes) { seg[n++] = FillSeg{p, n_bytes, v, 1}; }
};
hipError_t fill_multi(const FillList& fl, hipStream_t s);
struct CopySeg {
  void* dst;
  const void* src;
  size_t bytes;
};
struct CopyList {
  CopySeg seg[FILL_MAX_SEG];
  int n = 0;
  void add(void* dst, const void* src, size_t bytes) { seg[n++] = CopySeg{dst, src, bytes}; }
};
hipError_t copy_multi(const CopyList& cl, hipStream_t s);

// frontend.hip: wav -> log-mel.  Constant tables live in one device struct per handle.
constexpr int FE_FBW = 20;  // widest mel filter kept (nonzero bins; the widest has 17)
struct FrontendConst {
  float fb[F][FE_FBW];          // filter m's nonzero weights, bins lo[m] .. hi[m] - 1
  int32_t lo[F], hi[F];         // nonzero bin range of each mel filter
  float win[400];               // periodic hann(400)
  float tw256r[256], tw256i[256];  // exp(-2 pi i k / 256), rounded once from double
  float tw512r[257], tw512i[257];  // exp(-2 pi i q / 512)
};
void mel_filterbank(int n_stft, float f_min, float f_max, int n_mels, float* fb);
void build_frontend_const(FrontendConst* c);
int frontend_frames(int n_samples);
// form: 1 = the 16-lane kernel (default), 0 = one wave per frame (round 4); the same bits
hipError_t launch_log_mel(const float* wav, const int32_t* nsamp, int B, int Nmax, int Tmax, float pre,
                          const FrontendConst* k, float* out, int32_t* frames, int32_t* err, hipStream_t s,
                          int form = 1);

// convert.hip: casr_convert_audio's stages (a) to (d) for one batch of one format; the plan, the
// tiling and the LDS need are resample_design.h's
struct ConvertArgs {
  const float* pcm;      // [B][n_max_in][ch]
  const int32_t* n_in;   // [B]
  int n_max_in, ch, m_max;
  float inv_ch;          // 1 / ch rounded to f32
  int L, M, K, taps;     // the plan (L == M: pass-through of the downmix)
  const float* tab;      // device table [L][taps]
  int quantize, norm;    // norm: stage (d) follows, so the peaks are reduced
  float* wav;            // [B][m_max]
  int32_t* n_out;        // [B]
  float* gain;           // [B] or null
  uint32_t* peak;        // [B] scratch (norm only): max |q|, or the bits of max |y|
  int32_t* err;          // guard word
};
// target: 32768 10^(norm_db / 20) (quantize) or 10^(norm_db / 20), rounded to f32
hipError_t launch_convert(const ConvertArgs& a, int B, const ResamplePlan& p, float target, hipStream_t s);

// segment.hip: casr_segment's two launches (the histogram words are cleared first) and
// casr_gather_segments; the decision text is segment_plan.h's
struct SegmentArgs {
  const float* fbank;      // [B][T][n_mels]
  const int32_t* frames;   // [B]
  int B, T, n_mels, s_max;
  casr_segment_params p;   // valid (segment_params_valid)
  int32_t* seg_start;      // [B][s_max]
  int32_t* seg_len;        // [B][s_max]
  int32_t* n_seg;          // [B]
  int32_t* thr;            // [B] or null
  uint16_t* q;             // [B][T] workspace: the frames' levels
  uint32_t* hist;          // [B][512] workspace
  int32_t* err;            // guard word
};
hipError_t launch_segment(const SegmentArgs& a, hipStream_t s);
hipError_t launch_gather_segments(const float* fbank, int B, int T, int n_mels, const int32_t* seg_src,
                                  const int32_t* seg_start, const int32_t* seg_len, int S, int t_seg, float* out,
                                  int32_t* frames_out, int32_t* err, hipStream_t s);

// features.hip
// the layer-0 s16 image straight from fbank (features_rows_kernel<true>): the plan's FEAT_IMAGE
// stats: [B][2][D] floats of scratch (per-utterance mean and std + eps of the 720 dimensions)
hipError_t launch_features_x16(const EncodePlan& p, const float* fbank, const int32_t* frames, int T, float eps,
                               int32_t* feat_len, float* stats, uint16_t* x16, int32_t* err, hipStream_t s);
// path: feature_path's FEAT_ROWS (T <= FS_MAX_T) or FEAT_TWO_PASS
hipError_t launch_features(int path, const float* fbank, const int32_t* frames, int B, int T, float eps,
                           float* feat, int32_t* feat_len, float* stats, hipStream_t s);
hipError_t launch_gather_utts(const float* const* ptrs, const int32_t* lens, int B, int Tp,
                              float* feat, hipStream_t s);

// encoder.hip
hipError_t launch_input_proj(const float* X, int M, int Din, const float* W, const float* bias,
                             float* Gin, hipStream_t s);
// s16 images of an activation or weight matrix with rows R and Kp (multiple of 64) k per row, in one
// of two layouts (the same words): the row image [R][Kp / 32][32 hi | 32 lo] halves, or (km, round
// 5, CASR_OPT_X16_KM) 16-k-block major [Kp / 16][R][16 hi | 16 lo], in which 16 consecutive rows of
// one 16-k block are 1 KB contiguous (whole 128-B lines for the input GEMM's 16-deep stages).
// (which layout one encode uses: encode_plan.h encode_km)
// gemm16.hip: the s16x3 input projection on 256 x 256 tiles in the form g plans; X16 / W16 are s16
// images with g.Kp k per row (g.km: both 16-k-block major, X16 with g.M rows)
hipError_t launch_input_proj_s16_big(const InputGemmPlan& g, const float* X16, const float* W16, const float* bias,
                                     float* Gin, hipStream_t s);
// a row-image weight matrix [R][Kp] -> its 16-k-block-major image (bind time)
hipError_t launch_relayout_km16(const float* rowimg, int R, int Kp, float* km, hipStream_t s);
hipError_t launch_split_rows(const float* X, int ldx, int M, int K, int Kp, uint16_t* out, int32_t* err,
                             hipStream_t s, int km = 0);
hipError_t launch_rec_step(const float* Whh_f, const float* Gin, const float* xin, float* out,
                           const float* hprev, float* hnext, float* cst, float* hfin,
                           const int32_t* lens, int B, int Tp, int step, int residual, int row0,
                           int row1, int s16, hipStream_t s);
// recurrence.hip: persistent per-layer recurrence (all Tp steps in one launch) in the shape r plans
DeviceFacts read_device_facts();  // of the current device (once per handle)
hipError_t reset_rec_layer(const RecPlan& r, uint32_t* hx, hipStream_t s);  // before EVERY launch_rec_layer
// x16 (s16 only, may be null): also write out's s16 image (the next layer's input-GEMM operand,
// zeros past each length), replacing a split_rows pass.
// With r.coop == 1 the launch is cooperative: a grid that cannot be co-resident returns
// an error (hipErrorCooperativeLaunchTooLarge) instead of spinning into the hand-off timeout.
hipError_t launch_rec_layer(const RecPlan& r, const float* Whh_f, const float* Gin, const float* xin, float* out,
                            uint16_t* x16, uint32_t* hx, float* hfin, float* cst, const int32_t* lens, int residual,
                            int32_t* err, uint32_t* trace, hipStream_t s);
// enc16: the encoder output's s16 image (k.km: 16-k-block major); k.form KEYS16_ROWS or KEYS16_TILES
hipError_t launch_keys_s16(const KeysPlan& k, const float* enc16, const float* wenc16, const float* b_attn,
                           float* keysT, hipStream_t s);
hipError_t launch_keys(const KeysPlan& k, const float* enc, const float* wencT, const float* b_attn, float* keysT,
                       hipStream_t s);

// decoder.hip
// (GreedyPart, GP_NB, GP_NT and the fused image's tiling, FOLD_*: decode_plan.h)

// a beam select's operands and outputs (beam_select.h; beam_select_kernel's argument, and the
// folded beam attention's prologue select, AttnCell::bs)
struct BeamSelArgs {
  const float* logits;
  int V, B, k, l, L, eos;
  float temperature;
  const float* score_cur;
  float* score_next;
  int32_t* tok_next;
  int32_t* src_next;
  uint8_t* topfin;
  int32_t* bp;
  int32_t* tk;
  float* rec_score;
  int32_t* rec_src;
  uint8_t* rec_valid;
  int32_t* newdone;
  int32_t* err;
  GreedyPart gp;
  int nbp;
};

// Greedy select of step lsel fused into a later kernel of step lsel + 1 (the LSTMCell GEMM's
// prologue, decoder.hip DecLstmA; or the folded step's attention kernel, attention.hip): the
// projection's per-block row partials of step lsel are reduced by the consumer itself and the
// bookkeeping of greedy_select_part_kernel (model.py:540-590) is done by one writer per row.
struct GreedySel {
  GreedyPart gp;
  int nbp, lsel, L, eos;
  uint8_t* fin;
  int32_t* out_len;
  float* accum;
  int32_t* tokens;
  int32_t* newdone;
};

#ifdef __HIPCC__
// the writer's bookkeeping of row r once its token t and log-probability lp are known (lane 0
// only): tokens, finished, lengths, score and the newly-finished counter, as model.py:554-578
__device__ __forceinline__ void greedy_book(const GreedySel& gs, int r, int t, float lp, uint8_t fin0, float acc0,
                                            int len0) {
  gs.tokens[(size_t)r * gs.L + gs.lsel] = t;
  const bool was = fin0 != 0;
  const bool cur = t == gs.eos;
  float acc = acc0;
  if (!was && cur) acc = acc + lp;  // model.py:567
  const bool now = was || cur;
  if (!now) {
    gs.out_len[r] = len0 + 1;  // model.py:573
    acc = acc + lp;            // model.py:576
  }
  gs.accum[r] = acc;
  if (now && !was) {
    gs.fin[r] = 1;
    atomicAdd(&gs.newdone[gs.lsel], 1);
  }
}
#endif

// Folded greedy decode (CASR_OPT_DEC_FOLD): per step l >= 1 two launches instead of three.
//   KA (attention.hip, attention_kernel<1, true>): select of step l-1 from the projection
//      partials, gates = gates_prev[r] + emb_gates[tok] (the per-token table: emb . W_emb^T +
//      b_ih + b_hh), the LSTM cell, q = h . W_hidden by f32 fma chains, then the attention.
//   KB (decoder.hip, dgemm_kernel<.., FoldEpi>): [ctx | h] . [W_p ; W_ch]^T on one fused
//      fragment image: the vocabulary tiles (greedy partials) and the LSTM gate tiles of the next
//      step (K = 1024: the ctx | h part of the LSTM contraction, decoder.py:104-114), one GEMM
//      over the same A rows.
// bytes of one fused image (s16 or f32: the same tiling)
inline size_t fold_image_bytes(int V) { return (size_t)(fold_gtile0(V) + FOLD_GT) * (KPROJ / 64) * FRAG * sizeof(float); }
constexpr size_t FOLD_WQ16_FLOATS = (size_t)A * HD;  // the W_hidden fragment image (beam query)
struct FoldBufs {
  const float* wfold;      // fragment image (s16, or f32 under the exact-f32 arithmetic):
                           // [fold_gtile0(V) + FOLD_GT tiles][KPROJ / 64] FRAG blocks
  const float* emb_gates;  // [V][4 HD] packed gate-row order (packed_gate_row), biases included
  const float* wq16;       // s16 fragment image of W_hidden^T: [A / 16 tiles][HD / 64] FRAG blocks
  float* gates;            // [R][4 HD] the next step's [ctx | h] . W_ch^T, packed gate-row order
};
// build the fused images and the per-token gate table from a bound blob: wfold and wq16 from the s16
// images, wfold32 from the f32 fragment images (the folded greedy step under the exact-f32
// arithmetic), emb_gates from the embedding and the decoder LSTM weights; each nullptr is skipped
hipError_t build_fold(const float* W, const Layout& L, int V, float* wfold, float* emb_gates, float* wq16,
                      float* wfold32, hipStream_t s);

// (DecodeBufs and the workspaces' layouts: decode_plan.h)

struct DecodeArgs {
  const float* W;        // packed blob base
  Layout L;
  const float* enc;      // [B][Tp][C]
  const float* keysT;    // [B][A][Tp]
  const float* hfin;     // [2][B][H]
  const float* cfin;     // [2][B][H]
  const int32_t* lens;   // [B]
  int B, Tp, k, V, max_len, sos, eos;
  float temperature;
  Profiler* prof;        // may be null
  DecodePlan plan;       // every path decision of this call (decode_plan.h plan_decode)
  FoldBufs fb;           // fold tables and the gates buffer (plan.fold only)
};

// the view of the tree and the records a beam entry's decode writes (the one place BeamTree is filled):
// run_beam* finalize through it, casr_capi.hip keeps it in the handle for the readers
inline BeamTree beam_tree_of(const DecodeArgs& a, const DecodeBufs& d) {
  return BeamTree{a.B, a.k, a.max_len, a.V, d.bp, d.tk, d.newdone, d.rec_score, d.rec_src, d.rec_valid,
                  {d.score[0], d.score[1]}, d.err};
}

// attention.hip: one decode step's additive attention for all R rows (writes ctx into st)
hipError_t launch_attention_step(const DecodeArgs& a, float* st, const float* qpart, float* align,
                                 int32_t* newdone, int l, int total, hipStream_t s);
// the folded step's attention (KA above): st_old supplies c, st receives h, c and ctx.  Greedy
// (k = 1): sel = the fused select of step gs.lsel (else tokens from tok).  Beam (k > 1, 4 or 8 rows
// per block): tokens and predecessor rows from the beam select (tok, src)
struct AttnCell {
  const float* st_old;
  const float* gates;
  const float* emb_gates;
  const float* w_hidden;  // [HD][A]
  const float* wq16;      // beam: FoldBufs::wq16
  const int32_t* tok;     // sel == 0 (beam: the select's tokens of the block's rows)
  const int32_t* src;     // beam: the predecessor row of each row (gates_prev and c are read there)
  int32_t* err;
  int sel;
  GreedySel gs;
  int bsel;        // beam, one block per utterance: the select of step l - 1 runs in the prologue (bs)
  BeamSelArgs bs;
  // greedy, CASR_OPT_ATTN_SPLIT (round 6): split > 1 blocks of tc steps per utterance, their
  // (max, sum, context) partials [B][AT_SPLIT_MAX][C + 4] and per-utterance arrival counters
  int split, tc;
  float* spart;
  int32_t* scnt;
};
hipError_t launch_attention_cell_step(const DecodeArgs& a, float* st, const AttnCell& cell, float* align,
                                      int32_t* newdone, int l, int total, hipStream_t s);
// the static LDS of the attention kernel forms, read once from the code object (plan_decode's input)
AttnStaticLds attention_static_lds();
void attn_trace_bind(uint32_t* buf);  // CASR_DG_TRACE diagnostics (attention.hip)

void dg_trace_init();  // decoder.hip, CASR_DG_TRACE diagnostics
void dg_trace_dump();
hipError_t run_greedy(const DecodeArgs& a, DecodeBufs& d, int32_t* tokens, int32_t* out_len,
                      uint8_t* finished, float* accum, float* align, hipStream_t s);
hipError_t run_beam(const DecodeArgs& a, DecodeBufs& d, float lm_weight, float length_weight,
                    int32_t* best_tokens, int32_t* best_len, float* best_score, int32_t* steps,
                    hipStream_t s);
// The readers of a finished beam take its BeamTree (beam_state.h): casr_capi.hip keeps the beam_tree_of
// the beam entry that ran in the handle; their kernels read it by beam_tree.h's rules
hipError_t run_beam_records(const BeamTree& t, int32_t* rec_tokens, float* rec_score, uint8_t* rec_valid,
                            hipStream_t s);

// Teacher-forced scoring (casr_score, score.hip).  L steps of the three-launch step without its
// projection (decoder.hip score_steps), every step's state slab kept in a history, then ONE
// projection GEMM over the R = L B rows [ctx | h] of slabs 1..L (score_project) whose epilogue
// writes per row and 80-column block the greedy partials, the block's sum of logits and the
// target's logit; score_rows_kernel combines them.  Row i = l B + b everywhere.
struct ScoreBufs {
  float* hist;      // [L + 1][B][ST] state slabs: slab 0 the initial state, slab l + 1 step l's
  GreedyPart part;  // [L B][GP_NB] (tmx unused)
  float* xsum;      // [L B][GP_NB] sum of the block's logits over columns n < V
  float* tl;        // [L B] the target's logit (rows with a scored target only)
  int32_t* feed;    // [L][B] decoder input of step l: sos, then targets[b][l - 1] (eos past tgt_len)
  int32_t* tgt;     // [L][B] targets[b][l] clamped to [0, V), or -1 at l >= tgt_len[b]
};
size_t score_workspace_bytes(int B, int L);
ScoreBufs score_carve(void* base, int B, int L);
// decoder.hip: the step loop (a.plan: the PLAN_SCORE caller's) and the batched projection
hipError_t score_steps(const DecodeArgs& a, DecodeBufs& d, const ScoreBufs& sb, int L, float* align, hipStream_t s);
hipError_t score_project(const DecodeArgs& a, const DecodeBufs& d, const ScoreBufs& sb, int L, hipStream_t s);
// score.hip
hipError_t run_score(const DecodeArgs& a, DecodeBufs& d, const ScoreBufs& sb, const int32_t* targets,
                     const int32_t* tgt_len, int L, float* token_logp, float* total_logp, int32_t* best_token,
                     float* best_logp, float* mean_logp, float* align, hipStream_t s);

// ngram.hip: the backoff n-gram LM on the device (ngram_table.h's query).  m holds device pointers.
// Sentence scores q [n] of tokens [n][L] (LM ids) with lens [n]
hipError_t launch_lm_score(const NgramView& m, const int32_t* tokens, const int32_t* lens, int n, int L, int bos,
                           float* q, int32_t* err, hipStream_t s);
// lm_estimate.hip: the Kneser-Ney estimate of a corpus of `total` tokens in n sentences (device pointers)
// over the zeroed-by-it workspace ws of est_workspace_bytes(order, total + n); synchronises the stream.
// *flags: EST_FLAG_FULL where the result is refused (*out is then untouched); combine = 0 counts
// without the LDS combining (the same result)
hipError_t run_lm_estimate(int order, int V, const int32_t* tokens, const int64_t* offsets, int64_t n, int64_t total,
                           void* ws, int combine, int32_t* err, hipStream_t s, EstResult* out, uint32_t* flags);
// lm_prune.hip: relative-entropy pruning of the LM whose device views are dm and ds (host: its host tables,
// for the unigrams of the result) over the workspace ws of lmp_carve(d); synchronises the stream.  *flags:
// LMP_FLAG_INCONSISTENT where the result is refused (*out is then untouched)
hipError_t run_lm_prune(const NgramTables& host, const NgramView& dm, const NgramSuccView& ds, const LmpDims& d,
                        double theta, void* ws, hipStream_t s, LmpResult* out, uint32_t* flags);
// the second pass over the beam tree run_beam left (one workgroup per utterance); the beam
// weights are casr_beam's own, for its unfinished fallback.  rescore_supported: its LDS fits
bool rescore_supported(int max_len, int k);
hipError_t run_beam_rescore(const BeamTree& t, const NgramView& m, double lm_weight, double length_weight,
                            float beam_lm_weight, float beam_length_weight, int32_t* best_tokens, int32_t* best_len,
                            float* best_score, float* best_lm, float* rec_lm, hipStream_t s);

// beam_lm.hip: the LM fused into the beam's first pass (casr_lm_terms, casr_beam_lm).
// Where a term row's context comes from: tree == 0 the arrays ctx [n][3] / nc [n]; tree == 1 the beam
// tree at decode step l (row i = b k + j: its tokens before, <s> before step 0), skipping the rows the
// select of step l does not read
struct LmTermsSrc {
  int tree;
  const int32_t* ctx;
  const int32_t* nc;
  const int32_t* bp;
  const int32_t* tk;
  const int32_t* newdone;
  int l, k, B, R;
};
constexpr size_t LM_TERMS_LDS_BYTES = 64 * 1024;  // a term row (4 V bytes) is assembled in LDS
bool lm_terms_supported(int V);
// terms [n][V] of n rows; m and sv hold device pointers
hipError_t launch_lm_terms(const NgramView& m, const NgramSuccView& sv, const LmTermsSrc& src, int n, int eos_token,
                           float* terms, int32_t* err, hipStream_t s);
// the fused beam's own buffers (handle-owned, beside DecodeBufs)
struct BeamLmBufs {
  float* terms;   // [R][V] the step's term rows
  float* g[2];    // [R] the LM sums (ping-pong, as DecodeBufs::score)
  float* rec_lm;  // [B][L][k] LM sum of each finished record
};
inline size_t carve_beam_lm(void* base, int B, int R, int L, int k, int V, BeamLmBufs& w) {
  Carver c(base);
  w.terms = c.rows((size_t)R * V);
  for (int i = 0; i < 2; ++i) w.g[i] = c.take<float>(R);
  w.rec_lm = c.take<float>((size_t)B * L * k);
  return c.bytes(256);
}
// what the fused select has beyond a beam select's operands (BeamSelArgs)
struct BeamLmArgs {
  const float* terms;
  const float* g_cur;
  float* g_next;
  float* rec_lm;
  float lm_weight, len_l;  // len_l = (float)((double)length_weight (l + 1))
};
hipError_t launch_beam_lm_select(const BeamSelArgs& a, const BeamLmArgs& g, int K2, hipStream_t s);
hipError_t run_beam_record_lm(const BeamTree& t, const BeamLmBufs& w, float* rec_lm, hipStream_t s);
// decoder.hip: run_beam's steps (a.plan: the PLAN_BEAM_LM caller's) with the term rows and the fused
// select after each
hipError_t run_beam_lm(const DecodeArgs& a, DecodeBufs& d, const BeamLmBufs& w, const NgramView& m,
                       const NgramSuccView& sv, float lm_weight, float length_weight, int32_t* best_tokens,
                       int32_t* best_len, float* best_score, float* best_lm, int32_t* steps, hipStream_t s);

// bias.hip: hotword biasing (bias_plan.h's automaton; casr_bias_score, casr_bias_rows, casr_beam_bias).
// Where a gain row's state comes from: tree == 0 the array state [n]; tree == 1 the row's state at decode
// step l (row i = b k + j), skipping the rows the select of step l does not read, as LmTermsSrc
struct BiasRowsSrc {
  int tree;
  const int32_t* state;
  const int32_t* newdone;
  int l, k, B;
};
constexpr size_t BIAS_ROWS_LDS_BYTES = 64 * 1024;  // a gain row and its states (8 V bytes) are assembled in LDS
bool bias_rows_supported(int V);
// gain [n][V] and next [n][V] (or null) of n rows; m holds device pointers
hipError_t launch_bias_rows(const BiasView& m, const BiasRowsSrc& src, int n, int32_t* gain, int32_t* next,
                            int32_t* err, hipStream_t s);
hipError_t launch_bias_score(const BiasView& m, const int32_t* tokens, const int32_t* lens, int n, int L,
                             int32_t* full, int32_t* tail, int32_t* state, int32_t* err, hipStream_t s);
// the biased beam's own buffers (handle-owned, beside DecodeBufs and BeamLmBufs)
struct BeamBiasBufs {
  int32_t* gain;      // [R][V] the step's gain rows
  int32_t* st[2];     // [R] the rows' automaton states (ping-pong, as DecodeBufs::score)
  int32_t* full[2];   // [R] ... and C_r = full(y_r)
  int32_t* rec_full;  // [B][L][k] full of each finished record
};
inline size_t carve_beam_bias(void* base, int B, int R, int L, int k, int V, BeamBiasBufs& w) {
  Carver c(base);
  w.gain = c.take<int32_t>((size_t)R * V, 16);  // rows read 16 B at a time
  for (int i = 0; i < 2; ++i) w.st[i] = c.take<int32_t>(R);
  for (int i = 0; i < 2; ++i) w.full[i] = c.take<int32_t>(R);
  w.rec_full = c.take<int32_t>((size_t)B * L * k);
  return c.bytes(256);
}
// what the biased select has beyond a fused select's operands; m holds device pointers
struct BeamBiasArgs {
  BiasView m;
  const int32_t* gain;
  const int32_t* st_cur;
  const int32_t* full_cur;
  int32_t* st_next;
  int32_t* full_next;
  int32_t* rec_full;
  float bias_weight;
};
// beam_lm.hip: the fused select with the bias row read beside the logits and, with g.terms, the term rows
hipError_t launch_beam_bias_select(const BeamSelArgs& a, const BeamLmArgs& g, const BeamBiasArgs& q, int K2,
                                   hipStream_t s);
// the final choice of casr_beam_lm and casr_beam_bias over the tree t.  lw null: no LM took part; w and m
// null: no bias did (one of the two is there)
hipError_t launch_beam_fused_finalize(const BeamTree& t, const BeamLmBufs* lw, const BeamBiasBufs* w,
                                      const BiasView* m, float bias_weight, float lm_weight, float length_weight,
                                      int32_t* best_tokens, int32_t* best_len, float* best_score, float* best_lm,
                                      float* best_bias, int32_t* steps, hipStream_t s);
hipError_t run_beam_record_bias(const BeamTree& t, const BeamBiasBufs& w, float* rec_bias, hipStream_t s);
// decoder.hip: run_beam_lm's steps with the gain rows (and, with lw, the term rows) before the select
hipError_t run_beam_bias(const DecodeArgs& a, DecodeBufs& d, const BeamLmBufs* lw, const BeamBiasBufs& w,
                         const BiasView& bm, const NgramView* m, const NgramSuccView* sv, float bias_weight,
                         float lm_weight, float length_weight, int32_t* best_tokens, int32_t* best_len,
                         float* best_score, float* best_lm, float* best_bias, int32_t* steps, hipStream_t s);

// grammar.hip: grammar-constrained decoding (grammar_plan.h's acceptor; casr_grammar_accept,
// casr_grammar_rows, casr_beam_grammar).  Where a mask row's state and budget come from: tree == 0 the
// arrays state [n] / budget [n]; tree == 1 the row's state at decode step l (row i = b k + j) under the one
// budget budget_l, skipping the rows the select of step l does not read, as BiasRowsSrc
struct GramRowsSrc {
  int tree;
  const int32_t* state;
  const int32_t* budget;  // tree == 0
  const int32_t* newdone;
  int l, k, B, budget_l;
};
constexpr size_t GRAM_ROWS_LDS_BYTES = 64 * 1024;  // four mask rows (V / 2 bytes) are assembled in LDS
bool gram_rows_supported(int V);
// mask [n][gram_mask_words(V)] of n rows; m holds device pointers
hipError_t launch_gram_rows(const GrammarView& m, const GramRowsSrc& src, int n, uint32_t* mask, int32_t* err,
                            hipStream_t s);
hipError_t launch_gram_accept(const GrammarView& m, const int32_t* tokens, const int32_t* lens, int n, int L,
                              int32_t* consumed, int32_t* state, uint8_t* accepted, int32_t* err, hipStream_t s);
// the rows' states before step 0: start[b] (null: 0) in every row of utterance b
hipError_t launch_gram_start(const int32_t* start, int B, int k, int32_t* state, hipStream_t s);
// the constrained beam's own buffers (handle-owned, beside DecodeBufs and BeamLmBufs)
struct BeamGramBufs {
  uint32_t* mask;  // [R][GW] the step's mask rows
  int32_t* st[2];  // [R] the rows' grammar states (ping-pong, as DecodeBufs::score); -1: a dead row
};
inline size_t carve_beam_gram(void* base, int R, int V, BeamGramBufs& w) {
  Carver c(base);
  w.mask = c.take<uint32_t>((size_t)R * gram_mask_words(V), 16);  // rows read 16 B at a time
  for (int i = 0; i < 2; ++i) w.st[i] = c.take<int32_t>(R);
  return c.bytes(256);
}
// what the constrained select has beyond a fused select's operands; m holds device pointers
struct BeamGramArgs {
  GrammarView m;
  const uint32_t* mask;
  const int32_t* st_cur;
  int32_t* st_next;
};
// beam_lm.hip: the fused select with its GRAM switch (g.terms null: no LM), and the final choice of
// casr_beam_grammar (casr_beam_lm's; its live-row fallback skips the dead rows of st)
hipError_t launch_beam_gram_select(const BeamSelArgs& a, const BeamLmArgs& g, const BeamGramArgs& q, int K2,
                                   hipStream_t s);
hipError_t launch_beam_gram_finalize(const BeamTree& t, const BeamLmBufs* lw, const BeamGramBufs& w, float lm_weight,
                                     float length_weight, int32_t* best_tokens, int32_t* best_len, float* best_score,
                                     float* best_lm, uint8_t* complete, int32_t* steps, hipStream_t s);
// decoder.hip: run_beam_lm's steps with the mask rows (and, with lw, the term rows) before the select
hipError_t run_beam_grammar(const DecodeArgs& a, DecodeBufs& d, const BeamLmBufs* lw, const BeamGramBufs& w,
                            const GrammarView& gm, const NgramView* m, const NgramSuccView* sv, const int32_t* start,
                            float lm_weight, float length_weight, int32_t* best_tokens, int32_t* best_len,
                            float* best_score, float* best_lm, uint8_t* complete, int32_t* steps, hipStream_t s);

// edit.hip: edit distance on the device (edit_plan.h's rule, backtrace, total order and plan).
// n pairs a [n][La] / b [n][Lb] with their lengths; ops null or [n][3]
hipError_t launch_edit_pairs(const int32_t* a, const int32_t* a_len, int La, const int32_t* b, const int32_t* b_len,
                             int Lb, int n, int32_t* dist, int32_t* ops, int32_t* err, hipStream_t s);
// casr_beam_mbr's buffers (handle-owned, beside DecodeBufs); positions are those in an utterance's list
struct MbrBufs {
  double* w;       // [B][L k] exp(scale (c - c_max)) of the utterance's valid records, in list order
  int32_t* list;   // [B][L k] their flat indices step k + rank, ascending
  int32_t* count;  // [B]
  uint8_t* dist;   // [B][L k][L k] d(p, q) at [p][q] for q < p only
};
size_t carve_mbr(void* base, int B, int L, int k, MbrBufs& w);
bool mbr_supported(int max_len, int k);
// the MBR choice over the beam tree run_beam left; map: CASR_OPT_MBR_MAP
hipError_t run_beam_mbr(const BeamTree& t, const MbrBufs& w, int map, double scale, const float* rec_lm,
                        double lm_weight, double length_weight, float beam_lm_weight, float beam_length_weight,
                        int32_t* best_tokens, int32_t* best_len, float* best_score, int32_t* best_index,
                        double* best_risk, double* rec_risk, hipStream_t s);
hipError_t run_mbr_distances(const BeamTree& t, const MbrBufs& w, uint8_t* dist, int32_t* n_rec, hipStream_t s);

// edit_align.hip: the edit script of long pairs (edit_align_plan.h's tiles, bit layout, backtrace and
// plan).  ws: edit_align_plan(..).bytes of workspace; ops, b_of_a [n][La] and a_of_b [n][Lb] may be null
hipError_t run_edit_align(const int32_t* a, const int32_t* a_len, int La, const int32_t* b, const int32_t* b_len,
                          int Lb, int n, int32_t* dist, int32_t* ops, int32_t* b_of_a, int32_t* a_of_b, void* ws,
                          int32_t* err, hipStream_t s);

// confusion.hip: N-best lists and confusion networks over a beam's records (confusion_plan.h).
// The handle-owned workspace; positions are those in an utterance's list
struct CnBufs {
  double* c;       // [B][L k] comb of the utterance's valid records, in list order
  int64_t* unit;   // [B][L k] their posterior units
  int32_t* list;   // [B][L k] their flat indices step k + rank, ascending
  int32_t* count;  // [B]
  int32_t* ppos;   // [B] the pivot's position in the list, -1 without one
  int32_t* ptok;   // [B][L] the pivot's tokens
  int16_t* votes;  // [B][2 L + 1][L k] slot-major (null: an N-best call)
};
size_t carve_confusion(void* base, int B, int L, int k, bool votes, CnBufs& w);
bool confusion_supported(int B, int max_len, int k, int V, bool tree);
hipError_t run_beam_nbest(const BeamTree& t, const CnBufs& w, int N, const float* rec_lm, double lm_weight,
                          double length_weight, int32_t* nbest_index, int32_t* nbest_tokens, int32_t* nbest_len,
                          double* nbest_comb, hipStream_t s);
hipError_t run_beam_confusion(const BeamTree& t, const CnBufs& w, int M, double scale, const float* rec_lm,
                              double lm_weight, double length_weight, const int32_t* pivot, int32_t* n_slots,
                              int32_t* slot_token, int64_t* slot_mass, int64_t* pivot_mass, int64_t* total,
                              int64_t* rec_unit, hipStream_t s);
hipError_t run_confusion(const CnBufs& w, const int32_t* rec_tokens, const uint8_t* rec_valid, const int64_t* rec_unit,
                         const int32_t* pivot, int B, int L, int k, int V, int M, int32_t* n_slots,
                         int32_t* slot_token, int64_t* slot_mass, int64_t* pivot_mass, int64_t* total, int32_t* err,
                         hipStream_t s);

// ---- align.hip: the monotone path through align [L][Tp][B] (align_plan.h); group: CASR_OPT_ALIGN_GROUP
hipError_t launch_align_path(const float* align, const int32_t* enc_len, const int32_t* tgt_len, int B, int Tp, int L,
                             int group, int32_t* first, int32_t* last, int32_t* peak, int32_t* path_score,
                             int32_t* err, hipStream_t s);

}  // namespace casr
