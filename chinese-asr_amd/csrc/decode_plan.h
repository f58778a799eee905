// How a decode chooses its kernels: plan_decode() takes one API call's shapes, the handle's options
// and the bound blob's facts, and returns every path decision of that call as one DecodePlan.  The
// drivers (casr_capi.hip, decoder.hip, attention.hip, score.hip) read the plan and decide nothing
// themselves: that includes the block shape, grid and arguments of every decode GEMM launch (a
// DgemmPlan each, of the shape table in decode_gemm_shapes.h), from which the counts that other
// kernels must agree with (row partials per row, query partials per row) are derived.  Also here,
// because they must agree with the plan: the option table, the decode workspaces' layouts, and the
// hipGraph key of a captured decode.
// Pure host C++ (no HIP runtime): tests/host_plan/plan_check.cpp builds from this header alone.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "attention_lds.h"
#include "casr.h"
#include "casr_dims.h"
#include "decode_gemm_shapes.h"

namespace casr {

// ---------------------------------------------------------------- options
constexpr int AT_SPLIT_MAX = 8;  // CASR_OPT_ATTN_SPLIT: time-step ranges per utterance at most

// one row per CASR_OPT_* (include/casr.h), in enum order: default and accepted range
struct OptionRow {
  int id;
  const char* name;
  int def, lo, hi;
};
constexpr OptionRow OPTIONS[] = {
    {CASR_OPT_FUSE_SELECT, "FUSE_SELECT", 1, 0, 1},
    {CASR_OPT_REC_LAYOUT, "REC_LAYOUT", 0, 0, 3},
    {CASR_OPT_REC_STORE_PLAIN, "REC_STORE_PLAIN", 1, 0, 1},
    {CASR_OPT_REC_SLEEP, "REC_SLEEP", -1, -1, 16},
    {CASR_OPT_REC_POLL_GAP, "REC_POLL_GAP", 2, 1, 8},
    {CASR_OPT_REC_COOP, "REC_COOP", 2, 0, 2},
    {CASR_OPT_GEMM16_PERSIST, "GEMM16_PERSIST", 2, 0, 2},
    {CASR_OPT_GEMM16_TAIL, "GEMM16_TAIL", 2, 0, 2},
    {CASR_OPT_ATTN_KPB, "ATTN_KPB", 0, 0, 8},  // (0, 4 or 8: option_value_ok)
    {CASR_OPT_ATTN_DIRECT, "ATTN_DIRECT", 0, 0, 1},
    {CASR_OPT_DEC_FOLD, "DEC_FOLD", 1, 0, 1},
    {CASR_OPT_REC_COOP_REFUSE, "REC_COOP_REFUSE", 0, 0, CASR_MAX_LAYERS},
    {CASR_OPT_DIAG_COLD, "DIAG_COLD", 0, 0, (1 << CASR_K_COUNT) - 1},
    {CASR_OPT_LOGMEL_Q16, "LOGMEL_Q16", 1, 0, 1},
    {CASR_OPT_KEYS_ROWS, "KEYS_ROWS", 1, 0, 1},
    {CASR_OPT_X16_KM, "X16_KM", 1, 0, 1},
    {CASR_OPT_DEC_KSPLIT, "DEC_KSPLIT", 1, 0, 1},
    {CASR_OPT_GEMM16_LEAN, "GEMM16_LEAN", 0, 0, 1},
    {CASR_OPT_ATTN_SPLIT, "ATTN_SPLIT", 0, 0, AT_SPLIT_MAX},
    {CASR_OPT_MBR_MAP, "MBR_MAP", 0, 0, 2},
    {CASR_OPT_ALIGN_GROUP, "ALIGN_GROUP", 0, 0, 16},  // (0 or a power of two: option_value_ok)
};
constexpr bool options_in_enum_order() {
  for (int i = 0; i < CASR_OPT_COUNT; ++i)
    if (OPTIONS[i].id != i) return false;
  return true;
}
static_assert(sizeof(OPTIONS) / sizeof(OPTIONS[0]) == CASR_OPT_COUNT && options_in_enum_order(),
              "one OPTIONS row per CASR_OPT_*, in enum order");

inline bool option_value_ok(int option, int value) {
  if (option < 0 || option >= CASR_OPT_COUNT) return false;
  if (option == CASR_OPT_ATTN_KPB && value != 0 && value != 4 && value != 8) return false;
  if (option == CASR_OPT_ALIGN_GROUP && (value & (value - 1))) return false;
  return value >= OPTIONS[option].lo && value <= OPTIONS[option].hi;
}

// Tuning options of a handle (include/casr.h CASR_OPT_*): speed only, every value gives the same
// bits (CASR_OPT_ATTN_DIRECT: a numerics variant within the attention tolerance).
struct Tuning {
  int v[CASR_OPT_COUNT];
  Tuning() {
    for (int i = 0; i < CASR_OPT_COUNT; ++i) v[i] = OPTIONS[i].def;
  }
  int operator[](int i) const { return v[i]; }
};

// ---------------------------------------------------------------- shapes the plan reasons about
// projection column blocks (5 x 16 columns each) whose per-row partials the selects combine: V <= 5120
constexpr int GP_NB = 64;
constexpr int GP_NT = 320;  // 16-column tiles per row (V <= 5120)
struct GreedyPart {
  float* mx;    // [R][GP_NB] block maximum of the row's logits
  float* se;    // [R][GP_NB] sum exp(x - block maximum)
  int32_t* ix;  // [R][GP_NB] first column of the block maximum
  float* tmx;   // [R][GP_NT] maximum of each 16-column tile (beam at temperature 1), or nullptr
};

// the fused image of the folded step (casr_internal.h FoldBufs): vocabulary tiles, then LSTM gate tiles
constexpr int FOLD_GT = 4 * HD / 16;  // LSTM gate tiles (16 gate rows each) in the fused image
constexpr int FOLD_NT = 7;            // 16-column tiles per fused GEMM block (112 columns)
inline int fold_vtiles(int V) { return (V + 15) / 16; }
// (round 4) the gate tiles of the fused image start at the vocabulary tiles rounded up to a whole
// 7-tile wave column (zero tiles between): no wave column holds both vocabulary and gate tiles, so
// the fused GEMM's epilogue has no mixed column, the one that ended last
inline int fold_gtile0(int V) { return (fold_vtiles(V) + FOLD_NT - 1) / FOLD_NT * FOLD_NT; }

// the greedy folded GEMM's k split at R <= 32 (decoder.hip dgemm_kernel KS): DG_KS blocks per
// output block, at most DG_KS_GROUPS output blocks of 2 epilogue waves
constexpr int DG_KS_GROUPS = 64, DG_KS_COUNTERS = 2 * DG_KS_GROUPS;
constexpr size_t DG_KS_PART_BYTES = (size_t)DG_KS_COUNTERS * DG_KS * FOLD_NT * 64 * 16;  // f32x4 per lane
static_assert((KPROJ / 64) % DG_KS == 0, "the fused GEMM's 64-deep k tiles split evenly over DG_KS blocks");

// Within a class every shape has the same tiles per wave column, so the row partials a select reads
// (one per wave column: DecodePlan::nbp) do not depend on R: 5 in the projection (GreedyPart), a
// whole FOLD_NT wave column of the fused image in the folded GEMM
constexpr int PROJ_WAVE_TILES = 5;
static_assert(dg_shapes_ok(DG_LSTM_32x64, DG_LSTM_128x128, 0) &&
                  dg_shapes_ok(DG_PROJ_32x80, DG_PROJ_256x160_ONE, PROJ_WAVE_TILES) &&
                  dg_shapes_ok(DG_FOLD_32x112_KS, DG_FOLD_128x224_ONE, FOLD_NT),
              "decode GEMM shapes: 8 waves, the ring within the LDS, one partial block width per class");

// Which shape runs (the measurements behind each rule: decoder.hip, above launch_dec_lstm).
// decode rows at which the LSTMCell (128 x 128), projection (256 x 160) and beam fold (256 x 224)
// blocks fill the CUs in one round; below it the narrower blocks do
inline bool dec_wide(int R) { return R >= 2048; }
inline int dec_lstm_shape(int R) {
  return R <= 256 ? DG_LSTM_32x64 : R <= 512 ? DG_LSTM_64x64 : !dec_wide(R) ? DG_LSTM_128x64 : DG_LSTM_128x128;
}
// one: the one-accumulator shapes (s16 in effect and every |W_p| < 16)
inline int proj_shape(int R, bool one) {
  if (R <= 512) return R <= 32 ? DG_PROJ_32x80 : R <= 256 ? DG_PROJ_64x80 : DG_PROJ_128x80;
  return !one ? DG_PROJ_128x160 : !dec_wide(R) ? DG_PROJ_128x160_ONE : DG_PROJ_256x160_ONE;
}
// (the beam fold runs under s16 with small weights only: plan_decode's fold rule)
inline int fold_gemm_shape(bool beam, int R, bool ksplit) {
  if (beam) return dec_wide(R) ? DG_FOLD_256x224_ONE : DG_FOLD_128x224_ONE;
  return ksplit ? DG_FOLD_32x112_KS : R <= 32 ? DG_FOLD_32x112 : DG_FOLD_64x112;
}

// ---------------------------------------------------------------- the plan
// the API call that decodes.  PLAN_BEAM_LM (casr_beam_lm, casr_beam_bias): casr_beam's steps at that
// shape; the select, which ranks with the LM term and / or the phrase bias, is always a launch of its own
// (it reads the whole logits row)
enum { PLAN_GREEDY = 0, PLAN_BEAM = 1, PLAN_SCORE = 2, PLAN_BEAM_LM = 3 };
enum {
  PLAN_OK = 0,
  PLAN_BAD_K,     // beam width outside [1, KMAX_BEAM]: an argument error
  PLAN_LDS,       // unsupported: the three-launch attention's LDS (lds_bytes) is over the limit
  PLAN_VOCAB,     // unsupported (score): more projection column blocks than row partials
  PLAN_K_VOCAB,   // beam: 2k candidates per utterance from a vocabulary of fewer than 2k tokens: an argument error
};

// facts of the bound blob and the handle's arithmetic
struct BlobFacts {
  int s16;         // the s16 arithmetic is in effect (requested, and the blob's s16 images are valid)
  int s16_images;  // the folded step's s16 tables were built from valid s16 images
  int proj_small;  // every |W_p| < 16 (blob info word 4)
  int dec_small;   // every decoder LSTM weight < 16 (blob info word 5)
};
// static LDS of the attention kernel forms (its __shared__ words), read from the code object
struct AttnStaticLds {
  int kpb1, kpb1_cell, kpb2, kpb4, kpb8;  // attention_kernel<1>, <1, 1>, <2>, <4>, <8>
};

// Every field is an int32 (no padding), so the plan's bytes are its identity: decode_graph_key.
struct DecodePlan {
  int32_t status;  // PLAN_*
  int32_t lds_bytes;  // LDS of one three-launch attention block without the value prefetch
  // the inputs a captured sequence bakes in
  int32_t caller, B, Tp, k, R, align, s16, proj_small, attn_direct;
  int32_t score_len;      // casr_score: the target length (the batched projection has score_len x B rows), else 0
  int32_t kpb;            // beam rows per attention block
  int32_t fold;           // the folded step (CASR_OPT_DEC_FOLD in effect)
  int32_t build_fold32;   // the f32 fused image must exist before this decode (greedy fold under f32)
  int32_t fuse_select;    // the select of step l runs inside a kernel of step l + 1: the LSTMCell
                          // (greedy three-launch step) or the attention (greedy fold, beam fold)
  int32_t partials, nbp;  // the projection writes per-block row partials; their blocks per row (else 0)
  int32_t tile_max;       // ... and the 16-column tile maxima (beam)
  int32_t store_logits;   // ... and the logits themselves
  int32_t ksplit;         // the fused GEMM's k split, at the steps that also compute the next gates
  int32_t ksplit_last;    // ... and at the last step (vocabulary tiles only: fewer column blocks)
  int32_t asplit, tc, split;  // the split greedy attention: ranges asked for, steps per range, ranges; 0 = unsplit
  int32_t K2;             // beam select width (candidates kept per utterance): 4, 8, 16 or 32
  int32_t fin_lds;        // beam finalize: LDS of the wave form, or 0 = the thread-per-utterance form
  int32_t q_slots;        // attention query partials per decoder row: one per LSTMCell column block
  // the decode GEMM launches (all zero where the call has no such launch)
  DgemmPlan lstm;         // the LSTMCell (the folded step: step 0 only)
  DgemmPlan proj;         // the three-launch step's projection; casr_score: the batched one, score_len x B rows
  DgemmPlan fold_gates;   // the folded GEMM at the steps that also compute the next gates
  DgemmPlan fold_last;    // ... and at the last step (vocabulary tiles only)
};

// beam rows per block at k > 2 (CASR_OPT_ATTN_KPB, 0 = auto).  4 rows per block at B < 256: 8 rows
// per block (one block per utterance, half the grid at B = 128) measured 3.68 ms vs 2.87 ms per
// B = 128, k = 8 batch, and 2 or 1 rows per block 2.81 / 3.57 ms against 2.80 (round 2).  At B >= 256
// one block per utterance already covers the CUs and streams each utterance's keys and values once
// per step instead of k / 4 times (auto: 8 rows per block there).
inline int attention_kpb(int B, int k, int opt) {
  if (k == 1) return 1;
  if (k == 2) return 2;
  if (opt == 4 || opt == 8) return opt;
  return B >= 256 && k >= 8 ? 8 : 4;
}

// LDS of one attention block without the value prefetch (which takes what is left): the dynamic
// area plus the kernel's static words.  cell: the folded greedy step's attention_kernel<1, 1>
inline size_t attention_lds_bytes(int kpb, int Tp, const AttnStaticLds& st, bool cell = false) {
  switch (kpb) {
    case 1:
      return cell ? attn_smem_floats<1, 1>(Tp) * sizeof(float) + st.kpb1_cell
                  : attn_smem_floats<1>(Tp) * sizeof(float) + st.kpb1;
    case 2: return attn_smem_floats<2>(Tp) * sizeof(float) + st.kpb2;
    case 8: return attn_smem_floats<8>(Tp) * sizeof(float) + st.kpb8;
    default: return attn_smem_floats<4>(Tp) * sizeof(float) + st.kpb4;
  }
}

// cfg: vocab, max_len and temperature are read.  VP: the vocabulary padded to the blob's projection
// tiles (Layout::VP).  want_align: greedy with an alignment output.  score_len: the target length of
// casr_score (validated by the caller), 0 for the other callers.
inline DecodePlan plan_decode(int caller, int B, int Tp, int k, bool want_align, const casr_config& cfg, int VP,
                              const Tuning& t, const BlobFacts& blob, const AttnStaticLds& lds, int score_len = 0) {
  DecodePlan p{};
  const int V = cfg.vocab, L = cfg.max_len;
  const bool greedy = caller == PLAN_GREEDY, beam = caller == PLAN_BEAM || caller == PLAN_BEAM_LM;
  if (!beam) k = 1;
  p.caller = caller;
  p.B = B;
  p.Tp = Tp;
  p.k = k;
  p.score_len = caller == PLAN_SCORE ? score_len : 0;
  if (k < 1 || k > KMAX_BEAM) {
    p.status = PLAN_BAD_K;
    return p;
  }
  // every beam step keeps 2k candidates per utterance (the reference's topk over the vocabulary, which
  // raises there): with fewer tokens the step-0 list would carry its sentinels into the bookkeeping
  if (beam && 2 * k > V) {
    p.status = PLAN_K_VOCAB;
    return p;
  }
  const int R = p.R = B * k;
  p.align = greedy && want_align;
  p.s16 = blob.s16 != 0;
  p.proj_small = blob.proj_small != 0;
  p.attn_direct = t[CASR_OPT_ATTN_DIRECT];
  p.kpb = attention_kpb(B, k, t[CASR_OPT_ATTN_KPB]);
  p.lds_bytes = (int32_t)attention_lds_bytes(p.kpb, Tp, lds);
  if ((size_t)p.lds_bytes > LDS_LIMIT_BYTES) {
    p.status = PLAN_LDS;
    return p;
  }
  // the folded step: greedy (casr_greedy), or beam at R >= 1024 rows with 4 or 8 beam rows per
  // attention block and every projection / LSTM weight < 16 (the fused GEMM's one-accumulator
  // beam shapes, decoder.hip launch_fold_gemm).  casr_beam at k = 1 is a beam caller: it takes
  // the beam guards, never the greedy clause (its fused GEMM would pick the one-accumulator shapes)
  const bool fold_beam = beam && R >= 1024 && blob.proj_small && blob.dec_small && p.kpb >= 4;
  // (a vocabulary beyond the 64 seven-tile partial blocks of the fused GEMM keeps the three-launch step)
  const int VT = fold_vtiles(V), VG = fold_gtile0(V), fold_blocks = VG / FOLD_NT;
  const bool fold_vocab = fold_blocks <= GP_NB;
  // the folded greedy attention (attention_kernel<1, 1>) holds its cell-phase area on top of the
  // three-launch step's LDS: at Tp where only the latter fits, greedy keeps the three-launch step
  const bool fold_lds = !greedy || attention_lds_bytes(p.kpb, Tp, lds, true) <= LDS_LIMIT_BYTES;
  // the folded greedy attention reads the early-exit counters of steps 0..max_len-1 one per lane
  const bool fold_len = !greedy || L <= 64;
  const bool fold_shape = (greedy || fold_beam) && fold_vocab && fold_lds && fold_len && t[CASR_OPT_DEC_FOLD];
  // greedy folds in either arithmetic (round 4: the exact-f32 MFMAs on the f32 fused image, which the
  // caller builds first); the beam fold's one-accumulator shapes and its s16 query need the s16 images
  p.build_fold32 = fold_shape && greedy && !p.s16;
  p.fold = fold_shape && (p.s16 ? blob.s16_images != 0 : greedy);
  // the decode GEMM launches.  The LSTMCell: 4 gate tiles per 16 units, and one query partial per row
  // from each of its column blocks; the projection over R rows (casr_score: score_len x B at once)
  p.lstm = plan_dgemm(dec_lstm_shape(R), R, FOLD_GT, FOLD_GT, KDEC);
  p.q_slots = HD / (4 * DG_SHAPES[p.lstm.shape].NT);
  const int RP = caller == PLAN_SCORE ? p.score_len * B : R;
  if (!p.fold) p.proj = plan_dgemm(proj_shape(RP, p.s16 && p.proj_small), RP, VP / 16, VP / 16, KPROJ);
  // greedy fold at R <= 32 (CASR_OPT_DEC_KSPLIT): DG_KS blocks per 32 x 112 output block while the
  // launch's column blocks fit the arrival counters
  const bool ks = greedy && R <= 32 && t[CASR_OPT_DEC_KSPLIT];
  auto fold_gemm = [&](int cover) {
    const DgemmPlan g = plan_dgemm(fold_gemm_shape(beam, R, false), R, VG + FOLD_GT, cover, KPROJ);
    return ks && g.NB <= DG_KS_GROUPS ? plan_dgemm(fold_gemm_shape(beam, R, true), R, VG + FOLD_GT, cover, KPROJ) : g;
  };
  if (p.fold) {
    p.fold_gates = fold_gemm(VG + FOLD_GT);
    p.fold_last = fold_gemm(VT);
    p.ksplit = p.fold_gates.shape == DG_FOLD_32x112_KS;
    p.ksplit_last = p.fold_last.shape == DG_FOLD_32x112_KS;
  }
  // per-block row partials from the projection epilogue: the vocabulary must fit the 64 partial
  // blocks; beam search uses them at temperature 1 only (they are of x, not x / T).  One per wave
  // column of the planned shape over the vocabulary's tiles (the same in every shape of a class, so
  // the select's partial sums do not depend on R)
  const DgShape& psh = DG_SHAPES[p.fold ? p.fold_gates.shape : p.proj.shape];
  const int blocks = ((p.fold ? VT : VP / 16) + dg_wave_tiles(psh) - 1) / dg_wave_tiles(psh);
  p.partials = blocks <= GP_NB && (!beam || cfg.temperature == 1.0f);
  p.nbp = p.partials ? blocks : 0;
  if (caller == PLAN_SCORE && !p.partials) {
    p.status = PLAN_VOCAB;
    return p;
  }
  p.tile_max = p.partials && beam && V <= 16 * GP_NT;
  p.store_logits = beam || !p.partials;
  if (greedy)  // CASR_OPT_FUSE_SELECT = 0 keeps every select a launch (the same bits either way)
    p.fuse_select = t[CASR_OPT_FUSE_SELECT] && p.partials;
  // beam: the folded step with one attention block per utterance (k = 4 or 8 rows per block), or
  // k = 8 at 4 rows per attention block (both blocks of an utterance run the select, CELL 4)
  if (caller == PLAN_BEAM)
    p.fuse_select = p.fold && t[CASR_OPT_FUSE_SELECT] && (k == 4 || k == 8) && (p.kpb == k || (k == 8 && p.kpb == 4));
  // greedy fold at R <= 64 (CASR_OPT_ATTN_SPLIT; 1: ranges by R, 2..AT_SPLIT_MAX: that many): ranges
  // of a multiple of 4 steps; not with an alignment output, and a short input stays unsplit
  if (greedy && p.fold && R <= 64 && t[CASR_OPT_ATTN_SPLIT] && !p.align) {
    const int o = t[CASR_OPT_ATTN_SPLIT], asplit = o == 1 ? (R <= 32 ? 8 : 4) : o, tq = attn_tq(Tp);
    const int tc = ((tq + asplit - 1) / asplit + 3) & ~3, split = (tq + tc - 1) / tc;
    if (split >= 2) {
      p.asplit = asplit;
      p.tc = tc;
      p.split = split;
    }
  }
  if (beam) {
    p.K2 = k <= 2 ? 4 : k <= 4 ? 8 : k <= 8 ? 16 : 32;
    // (a max_len x k past the LDS: the thread-per-utterance form)
    const size_t fin_lds = (size_t)((L * k + 7) & ~7) * (3 * sizeof(int32_t) + 1) + 16;
    p.fin_lds = fin_lds <= 64 * 1024 ? (int32_t)fin_lds : 0;
  }
  return p;
}

// ---------------------------------------------------------------- decode workspaces
struct DecodeBufs {
  float* st[2];          // [R][ST]
  float* logits;         // [R][V]
  GreedyPart part;       // per-block row partials of the projection (after the logits)
  float* qpart;          // [plan.q_slots][R][A] attention query partials, one per LSTMCell column block
  int32_t* tok[2];       // [R]
  int32_t* src[2];       // [R]
  float* score[2];       // [R]
  int32_t* newdone;      // [max_len] rows/utterances newly finished at each step
  int32_t* err;          // [1] CASR_DEV_* guard bits set by kernels (casr_debug_flags)
  // greedy
  uint8_t* fin;          // [R]
  // beam
  uint8_t* topfin;       // [B]
  int32_t* bp;           // [L][R]
  int32_t* tk;           // [L][R]
  float* rec_score;      // [B][L][k]
  int32_t* rec_src;      // [B][L][k]
  uint8_t* rec_valid;    // [B][L][k]
  // DecodePlan::ksplit: the k-range sums and arrival counters (else nullptr)
  float* kspart;         // [groups][2 waves][DG_KS][FOLD_NT tiles][64 lanes] x 4 floats
  int32_t* kscnt;
  // DecodePlan::split: the split attention's partials and counters (else nullptr)
  float* aspart;         // [R][AT_SPLIT_MAX][C + 4]
  int32_t* ascnt;        // [R]
};
// handle-owned outputs of a decode replayed as a hipGraph (copied to the caller's buffers afterwards)
struct GreedyOut {
  int32_t* tokens;  // [B][L]
  int32_t* len;     // [B]
  float* accum;     // [B]
  float* align;     // [L][Tp][B], or nullptr
  uint8_t* fin;     // [B]
};
struct BeamOut {
  int32_t* tokens;  // [B][L]
  int32_t* len;     // [B]
  int32_t* steps;   // [1]
  float* score;     // [B]
};

// Walks one workspace's description: take() hands out the next region (nullptr while base is null,
// a sizing pass) and bytes() is what the description needs, so size and pointers cannot disagree.
class Carver {
 public:
  explicit Carver(void* base) : base_(static_cast<char*>(base)) {}
  template <class T>
  T* take(size_t n, size_t align = alignof(T)) {
    off_ = (off_ + align - 1) & ~(align - 1);
    T* p = base_ ? reinterpret_cast<T*>(base_ + off_) : nullptr;
    off_ += n * sizeof(T);
    return p;
  }
  float* rows(size_t n) { return take<float>(n, 16); }  // float rows read 16 B at a time
  size_t bytes(size_t tail = 0) const { return off_ + tail; }

 private:
  char* base_;
  size_t off_ = 0;
};

// Each carve_*(base, ...) fills its pointers from base (nullptr: sizes only) and returns the bytes.
// st [2][R][ST] | qpart
inline size_t carve_state(void* base, const DecodePlan& p, DecodeBufs& d) {
  Carver c(base);
  const size_t R = (size_t)p.R;
  d.st[0] = c.rows(R * ST);
  d.st[1] = c.rows(R * ST);
  d.qpart = c.rows((size_t)p.q_slots * R * A);
  return c.bytes();
}
// logits | row partials | tile maxima
inline size_t carve_logits(void* base, int R, int V, DecodeBufs& d) {
  Carver c(base);
  d.logits = c.rows((size_t)R * V);
  d.part.mx = c.rows((size_t)R * GP_NB);
  d.part.se = c.rows((size_t)R * GP_NB);
  d.part.ix = c.take<int32_t>((size_t)R * GP_NB, 16);
  d.part.tmx = c.rows((size_t)R * GP_NT);
  return c.bytes();
}
// per-row tokens, predecessors and scores (ping-pong), the early-exit counters and the finished flags
// (the flags keep a word's room each and the tail its 256 B: this workspace has never been smaller)
inline size_t carve_small(void* base, int B, int R, int L, DecodeBufs& d) {
  Carver c(base);
  for (int i = 0; i < 2; ++i) d.tok[i] = c.take<int32_t>(R);
  for (int i = 0; i < 2; ++i) d.src[i] = c.take<int32_t>(R);
  for (int i = 0; i < 2; ++i) d.score[i] = c.take<float>(R);
  d.newdone = c.take<int32_t>(L);
  d.topfin = c.take<uint8_t>(sizeof(int32_t) * B);
  d.fin = c.take<uint8_t>(sizeof(int32_t) * (R + 1));
  return c.bytes(256);
}
// finished-hypothesis records of the beam search, n = B L k each
inline size_t carve_records(void* base, int B, int L, int k, DecodeBufs& d) {
  Carver c(base);
  const size_t n = (size_t)B * L * k;
  d.rec_score = c.take<float>(n);
  d.rec_src = c.take<int32_t>(n);
  d.rec_valid = c.take<uint8_t>(n);
  return c.bytes(256);
}
inline size_t carve_ksplit(void* base, DecodeBufs& d) {
  Carver c(base);
  d.kspart = c.rows(DG_KS_PART_BYTES / sizeof(float));
  d.kscnt = c.take<int32_t>(DG_KS_COUNTERS);
  return c.bytes();
}
inline size_t carve_attn_split(void* base, int R, DecodeBufs& d) {
  Carver c(base);
  d.aspart = c.rows((size_t)R * AT_SPLIT_MAX * (C + 4));
  d.ascnt = c.take<int32_t>(R);
  return c.bytes();
}
// nal: floats of the alignment output (0: none)
inline size_t carve_greedy_out(void* base, int B, int L, size_t nal, GreedyOut& o) {
  Carver c(base);
  o.tokens = c.take<int32_t>((size_t)B * L);
  o.len = c.take<int32_t>(B);
  o.accum = c.take<float>(B);
  o.align = c.take<float>(nal);
  if (!nal) o.align = nullptr;
  o.fin = c.take<uint8_t>(B);
  return c.bytes(64);
}
inline size_t carve_beam_out(void* base, int B, int L, BeamOut& o) {
  Carver c(base);
  o.tokens = c.take<int32_t>((size_t)B * L);
  o.len = c.take<int32_t>(B);
  o.steps = c.take<int32_t>(1);
  o.score = c.take<float>(B);
  return c.bytes(64);
}

// ---------------------------------------------------------------- hipGraph key of a captured sequence
// Everything a captured sequence bakes in: the kind of capture, the plan's bytes (a DecodePlan or an
// EncodePlan: int32 fields only), the scalar arguments (4-byte words: their bit patterns) and the
// base pointer of every buffer handed to the launchers.
inline std::vector<uint64_t> plan_graph_key(int kind, const void* plan, size_t plan_bytes, const void* scalars,
                                            int n_scalars, const void* const* bufs, int n_bufs) {
  std::vector<uint64_t> key;
  key.reserve(1 + plan_bytes / 4 + n_scalars + n_bufs);
  key.push_back((uint64_t)kind);
  uint32_t w;
  for (size_t i = 0; i < plan_bytes / 4; ++i) {
    memcpy(&w, static_cast<const char*>(plan) + 4 * i, 4);
    key.push_back(w);
  }
  for (int i = 0; i < n_scalars; ++i) {
    memcpy(&w, static_cast<const char*>(scalars) + 4 * i, 4);
    key.push_back(w);
  }
  for (int i = 0; i < n_bufs; ++i) key.push_back((uint64_t)(uintptr_t)bufs[i]);
  return key;
}
inline std::vector<uint64_t> decode_graph_key(int kind, const DecodePlan& plan, const float* scalars, int n_scalars,
                                              const void* const* bufs, int n_bufs) {
  static_assert(sizeof(DecodePlan) % sizeof(uint32_t) == 0, "DecodePlan: int32 fields only");
  return plan_graph_key(kind, &plan, sizeof plan, scalars, n_scalars, bufs, n_bufs);
}

}  // namespace casr
