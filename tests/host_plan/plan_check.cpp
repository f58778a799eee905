// Host check of the decode plan (chinese-asr_amd/csrc/decode_plan.h): built from that header alone
// with clang AddressSanitizer + UndefinedBehaviorSanitizer and run as a program by
// tests/test_decode_plan_host.py; no GPU, no HIP runtime.
//
// The expected values are the decisions the drivers made before the plan existed (prepare_decode,
// decoder.hip's row_partials / proj_col_blocks / fsel, attention.hip's attention_kpb), read from that
// code and worked out by hand here; the sizes in check_carving are that code's allocation formulas.
// The decode GEMM shapes, grids and arguments (check_shape_table, check_gemm_plans) are those of the
// block-shape ladders decoder.hip's launchers held before the plan named them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "decode_plan.h"

using namespace casr;

#define EXPECT(c)                                                                  \
  do {                                                                             \
    if (!(c)) {                                                                    \
      std::fprintf(stderr, "plan_check: %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      std::exit(3);                                                                \
    }                                                                              \
  } while (0)

// the table's inputs "unless a row says otherwise"
struct In {
  int caller = PLAN_GREEDY, B = 256, Tp = 266, k = 1;
  bool align = false;
  int V = 5004, L = 40, score_len = 0;
  float T = 1.f;
  Tuning t;
  BlobFacts blob{1, 1, 1, 1};
  In& opt(int o, int v) {
    t.v[o] = v;
    return *this;
  }
};
static In greedy(int B = 256) {
  In in;
  in.B = B;
  return in;
}
static In beam(int B, int k) {
  In in;
  in.caller = PLAN_BEAM;
  in.B = B;
  in.k = k;
  return in;
}
static const AttnStaticLds kLds{336, 336, 336, 336, 336};
static DecodePlan plan(const In& in) {
  casr_config cfg{};
  cfg.vocab = in.V;
  cfg.max_len = in.L;
  cfg.temperature = in.T;
  return plan_decode(in.caller, in.B, in.Tp, in.k, in.align, cfg, (in.V + 63) / 64 * 64, in.t, in.blob, kLds,
                     in.score_len);
}
static In score(int B, int L) {
  In in;
  in.caller = PLAN_SCORE;
  in.B = B;
  in.score_len = L;
  return in;
}
static In with_blob(In in, BlobFacts b) {
  in.blob = b;
  return in;
}
static In with_vocab(In in, int V) {
  in.V = V;
  return in;
}

static void check_greedy() {
  DecodePlan p = plan(greedy());
  EXPECT(p.status == PLAN_OK && p.R == 256 && p.fold && p.fuse_select && p.partials && p.nbp == 45);
  EXPECT(!p.ksplit && !p.ksplit_last && !p.split && p.kpb == 1 && !p.store_logits && !p.tile_max && !p.build_fold32);
  p = plan(greedy().opt(CASR_OPT_DEC_FOLD, 0));
  EXPECT(!p.fold && p.partials && p.nbp == 64 && p.fuse_select && !p.store_logits);
  {  // V = 5204 (VP = 5248): 66 five-tile blocks > 64
    In in = greedy().opt(CASR_OPT_DEC_FOLD, 0);
    in.V = 5204;
    p = plan(in);
    EXPECT(p.status == PLAN_OK && !p.fold && !p.partials && p.nbp == 0 && !p.fuse_select && p.store_logits);
    in = greedy();
    in.V = 5204;
    p = plan(in);
    EXPECT(p.fold && p.partials && p.nbp == 47 && p.fuse_select);
  }
  for (int L : {64, 65}) {
    In in = greedy();
    in.L = L;
    EXPECT(plan(in).status == PLAN_OK && plan(in).fold == (L <= 64));
  }
  // the folded attention's LDS: 560 + 9 Tq floats + 2560 cell floats + 336 static bytes
  EXPECT(attention_lds_bytes(1, 4180, kLds, true) == 163296 && attention_lds_bytes(1, 4200, kLds, true) == 164016);
  EXPECT(LDS_LIMIT_BYTES == 163840);
  for (int Tp : {4180, 4200, 4300, 4600}) {
    In in = greedy();
    in.Tp = Tp;
    p = plan(in);
    if (Tp == 4600) {
      EXPECT(p.status == PLAN_LDS && (size_t)p.lds_bytes > LDS_LIMIT_BYTES);
    } else {
      EXPECT(p.status == PLAN_OK && p.fold == (Tp == 4180) && p.partials && p.fuse_select);
    }
  }
  {  // f32 in effect, and s16 requested on a blob without valid s16 images: the same plan
    In f32 = greedy(), inval = greedy();
    f32.blob = BlobFacts{0, 1, 1, 1};
    inval.blob = BlobFacts{0, 0, 1, 1};
    p = plan(f32);
    EXPECT(p.fold && p.build_fold32 && !p.s16 && p.nbp == 45);
    const DecodePlan q = plan(inval);
    EXPECT(std::memcmp(&p, &q, sizeof p) == 0);
    // (s16 in effect but the tables not built: no fold)
    In odd = greedy();
    odd.blob = BlobFacts{1, 0, 1, 1};
    EXPECT(!plan(odd).fold && !plan(odd).build_fold32);
  }
  // the k split: R <= 32, and the launch's column blocks within the 64 arrival-counter groups
  p = plan(greedy(32));
  EXPECT(p.fold && p.ksplit && p.ksplit_last);  // 443 tiles / 7 = 64 blocks; last step 45
  EXPECT(!plan(greedy(33)).ksplit && !plan(greedy(33)).ksplit_last);
  EXPECT(!plan(greedy(32).opt(CASR_OPT_DEC_KSPLIT, 0)).ksplit && !plan(greedy(32).opt(CASR_OPT_DEC_KSPLIT, 0)).ksplit_last);
  EXPECT(!plan(greedy(32).opt(CASR_OPT_DEC_FOLD, 0)).ksplit);
  {
    In in = greedy(32);
    in.V = 5204;  // 457 tiles / 7 = 66 blocks > 64; the last step's 47 vocabulary blocks fit (as before the plan)
    p = plan(in);
    EXPECT(p.fold && !p.ksplit && p.ksplit_last);
  }
  // the split attention
  p = plan(greedy(32).opt(CASR_OPT_ATTN_SPLIT, 1));
  EXPECT(p.asplit == 8 && p.tc == 36 && p.split == 8);
  p = plan(greedy(64).opt(CASR_OPT_ATTN_SPLIT, 1));
  EXPECT(p.asplit == 4 && p.tc == 68 && p.split == 4);
  p = plan(greedy(65).opt(CASR_OPT_ATTN_SPLIT, 1));
  EXPECT(!p.asplit && !p.tc && !p.split);
  {
    In in = greedy(32).opt(CASR_OPT_ATTN_SPLIT, 1);
    in.Tp = 4;
    EXPECT(!plan(in).split && plan(in).fold);
    in = greedy(32).opt(CASR_OPT_ATTN_SPLIT, 1);
    in.align = true;
    EXPECT(!plan(in).split && plan(in).align && plan(in).fold);
  }
  p = plan(greedy(48).opt(CASR_OPT_ATTN_SPLIT, 3));
  EXPECT(p.asplit == 3 && p.tc == 92 && p.split == 3);
}

static void check_beam() {
  DecodePlan p = plan(beam(256, 8));
  EXPECT(p.status == PLAN_OK && p.R == 2048 && p.kpb == 8 && p.fold && p.fuse_select && p.K2 == 16);
  EXPECT(p.partials && p.nbp == 45 && p.tile_max && p.store_logits && !p.ksplit && !p.split && !p.build_fold32);
  p = plan(beam(128, 8));
  EXPECT(p.kpb == 4 && p.fold && p.fuse_select);
  p = plan(beam(128, 8).opt(CASR_OPT_ATTN_KPB, 8));
  EXPECT(p.kpb == 8 && p.fold && p.fuse_select);
  p = plan(beam(256, 4));
  EXPECT(p.kpb == 4 && p.fold && p.fuse_select && p.K2 == 8);
  p = plan(beam(64, 16));
  EXPECT(p.kpb == 4 && p.fold && !p.fuse_select && p.K2 == 32);
  p = plan(beam(127, 8));
  EXPECT(p.R == 1016 && !p.fold && p.nbp == 64 && !p.fuse_select);
  p = plan(beam(512, 2));
  EXPECT(p.kpb == 2 && !p.fold && p.K2 == 4);
  p = plan(beam(1024, 1));
  EXPECT(p.status == PLAN_OK && p.kpb == 1 && !p.fold && p.K2 == 4 && p.store_logits);
  {
    In in = beam(256, 8);
    in.blob.proj_small = 0;
    EXPECT(!plan(in).fold);
    in = beam(256, 8);
    in.blob.dec_small = 0;
    EXPECT(!plan(in).fold);
    in = beam(256, 8);
    in.blob = BlobFacts{0, 1, 1, 1};
    EXPECT(!plan(in).fold && !plan(in).build_fold32);
  }
  p = plan(beam(256, 8).opt(CASR_OPT_FUSE_SELECT, 0));
  EXPECT(p.fold && !p.fuse_select);
  {
    In in = beam(256, 8);
    in.T = 0.7f;
    p = plan(in);
    EXPECT(p.fold && p.fuse_select && !p.partials && p.nbp == 0 && !p.tile_max && p.store_logits);
    in = beam(256, 8);
    in.V = 5204;
    p = plan(in);
    EXPECT(p.fold && p.partials && p.nbp == 47 && !p.tile_max);
  }
  EXPECT(plan(beam(256, 0)).status == PLAN_BAD_K && plan(beam(256, 17)).status == PLAN_BAD_K);
  EXPECT(plan(beam(256, 1)).status == PLAN_OK && plan(beam(256, 16)).status == PLAN_OK);
  p = plan(beam(256, 16));
  EXPECT(p.fin_lds == 8336);
  {
    In in = beam(256, 16);
    in.L = 320;  // 66,576 B > 64 KiB: the thread-per-utterance finalize
    EXPECT(plan(in).status == PLAN_OK && plan(in).fin_lds == 0);
  }
}

static void check_score() {
  for (int s16 = 0; s16 < 2; ++s16) {
    In in;
    in.caller = PLAN_SCORE;
    in.blob = BlobFacts{s16, s16, 1, 1};
    const DecodePlan p = plan(in);
    EXPECT(p.status == PLAN_OK && p.k == 1 && p.R == 256 && !p.fold && !p.build_fold32 && !p.fuse_select);
    EXPECT(p.partials && p.nbp == 64 && !p.ksplit && !p.split && p.s16 == s16);
  }
  In in;
  in.caller = PLAN_SCORE;
  in.V = 5204;
  EXPECT(plan(in).status == PLAN_VOCAB);
}

// ---------------------------------------------------------------- the decode GEMM shapes
// Expected values: the block-shape ladders the launchers of decoder.hip held before the plan named
// the shapes (launch_dec_lstm, launch_proj, launch_fold_gemm, launch_dg), worked out by hand.
// At V = 5004: 316 projection tiles (VP = 5056), 313 vocabulary tiles, the gate tiles from tile 315,
// 443 tiles of the fused image; 128 LSTM gate tiles; 20 / 16 64-deep k tiles (K = 1280 / 1024).
static bool same(const DgemmPlan& g, int shape, int NB, int NR, int grid, int ntiles, int nkt) {
  return g.shape == shape && g.NB == NB && g.NR == NR && g.grid == grid && g.ntiles == ntiles && g.nkt == nkt;
}
static bool unused(const DgemmPlan& g) { return same(g, 0, 0, 0, 0, 0, 0); }

static void check_shape_table() {
  // dgemm_kernel's template arguments of each rung: WR NT S RS WC IL BKW ONE SA KS
  const int want[DG_SHAPE_COUNT][10] = {
      {2, 4, 4, 1, 1, 0, 64, 0, 4, 1},    // LSTMCell R <= 256          <2,4,4>
      {4, 4, 4, 1, 1, 0, 64, 0, 4, 1},    //          R <= 512          <4,4,4>
      {8, 4, 3, 1, 1, 1, 64, 0, 3, 1},    //          R < 2048          <8,4,3,1,1,IL>
      {8, 8, 2, 1, 1, 1, 64, 0, 2, 1},    //          R >= 2048         <8,8,2,1,1,IL>
      {2, 5, 4, 1, 1, 0, 64, 0, 4, 1},    // projection R <= 32         <2,5,4>
      {4, 5, 4, 1, 1, 0, 64, 0, 4, 1},    //          R <= 256          <4,5,4>
      {8, 5, 3, 1, 1, 0, 64, 0, 3, 1},    //          R <= 512          <8,5,3>
      {4, 10, 2, 2, 2, 1, 64, 0, 2, 1},   //          R > 512           <4,10,2,2,2,IL>
      {4, 10, 2, 2, 2, 1, 64, 1, 2, 1},   //          ... s16, small    <4,10,2,2,2,IL,64,ONE>
      {4, 10, 3, 4, 2, 1, 32, 1, 3, 1},   //          ... R >= 2048     <4,10,3,4,2,IL,32,ONE>
      {2, 7, 3, 1, 1, 0, 64, 0, 3, 4},    // fold greedy, k split       <2,7,3,1,1,-,64,-,3,4>
      {2, 7, 3, 1, 1, 0, 64, 0, 3, 1},    //          R <= 32           <2,7,3>
      {4, 7, 3, 1, 1, 0, 64, 0, 3, 1},    //          otherwise         <4,7,3>
      {4, 14, 2, 4, 2, 1, 32, 1, 3, 1},   // fold beam R >= 2048        <4,14,2,4,2,IL,32,ONE,3>
      {4, 14, 3, 2, 2, 1, 32, 1, 3, 1},   //          otherwise         <4,14,3,2,2,IL,32,ONE>
  };
  const int ids[DG_SHAPE_COUNT] = {DG_LSTM_32x64,   DG_LSTM_64x64,       DG_LSTM_128x64,      DG_LSTM_128x128,
                                   DG_PROJ_32x80,   DG_PROJ_64x80,       DG_PROJ_128x80,      DG_PROJ_128x160,
                                   DG_PROJ_128x160_ONE, DG_PROJ_256x160_ONE, DG_FOLD_32x112_KS, DG_FOLD_32x112,
                                   DG_FOLD_64x112,  DG_FOLD_256x224_ONE, DG_FOLD_128x224_ONE};
  for (int i = 0; i < DG_SHAPE_COUNT; ++i) {
    EXPECT(ids[i] == i);
    const DgShape& s = DG_SHAPES[i];
    const int got[10] = {s.WR, s.NT, s.S, s.RS, s.WC, s.IL, s.BKW, s.ONE, s.SA, s.KS};
    EXPECT(std::memcmp(got, want[i], sizeof got) == 0 && s.name && s.name[0]);
    // rows, columns, tiles per wave column, k slices
    const int BM = 16 * want[i][0] * want[i][3];
    EXPECT(dg_block_rows(s) == BM && dg_block_cols(s) == 16 * want[i][1]);
    EXPECT(dg_wave_tiles(s) == want[i][1] / want[i][4] && dg_k_slices(s) * want[i][0] * want[i][4] == 8);
    // the ring as the kernel's static_assert sized it: S stages of [A | W], SA - S more A tiles
    const int BKW = want[i][6], atile = BM * BKW, wtile = want[i][1] * (BKW == 32 ? 512 : 1024);
    const int ring = (want[i][2] * (atile + wtile) + (want[i][8] - want[i][2]) * atile) * 4;
    EXPECT(dg_ring_bytes(s) == ring && ring <= 160 * 1024 && dg_shape_ok(s));
    EXPECT(dg_s16_only(s) == (want[i][6] == 32 || want[i][7] == 1));
    // one partial block width per class
    if (i >= DG_PROJ_32x80 && i <= DG_PROJ_256x160_ONE) EXPECT(dg_wave_tiles(s) == 5);
    if (i >= DG_FOLD_32x112_KS) EXPECT(dg_wave_tiles(s) == 7 && dg_wave_tiles(s) == FOLD_NT);
  }
  EXPECT(dg_ring_bytes(DG_SHAPES[DG_PROJ_256x160_ONE]) == 159744);  // 3 x (256 x 32 + 10 x 512) floats
  EXPECT(dg_ring_bytes(DG_SHAPES[DG_FOLD_256x224_ONE]) == 152 * 1024);  // 2 x (8192 + 7168) + 8192 floats
  EXPECT(dg_ring_bytes(DG_SHAPES[DG_PROJ_128x80]) == 159744 && dg_ring_bytes(DG_SHAPES[DG_LSTM_32x64]) == 98304);
  EXPECT(xcd_grid(64, 1) == 64 && xcd_grid(45, 4) == 192 && xcd_grid(1, 1) == 8 && xcd_grid(16, 16) == 256);
}

static void check_gemm_plans() {
  const BlobFacts f32{0, 1, 1, 1}, big_w{1, 1, 0, 1};
  auto nofold = [](In in) { return in.opt(CASR_OPT_DEC_FOLD, 0); };
  // LSTMCell by R (greedy: R = B), either arithmetic; the query slots follow its column blocks
  const struct { int R, shape, NB, NR, grid, q; } lstm[] = {
      {32, DG_LSTM_32x64, 32, 1, 32, 32},    {256, DG_LSTM_32x64, 32, 8, 256, 32},
      {257, DG_LSTM_64x64, 32, 5, 160, 32},  {512, DG_LSTM_64x64, 32, 8, 256, 32},
      {513, DG_LSTM_128x64, 32, 5, 160, 32}, {2047, DG_LSTM_128x64, 32, 16, 512, 32},
      {2048, DG_LSTM_128x128, 16, 16, 256, 16}, {4096, DG_LSTM_128x128, 16, 32, 512, 16}};
  for (const auto& c : lstm)
    for (const BlobFacts& b : {BlobFacts{1, 1, 1, 1}, f32})
      for (int fold = 0; fold < 2; ++fold) {
        const DecodePlan p = plan(with_blob(greedy(c.R).opt(CASR_OPT_DEC_FOLD, fold), b));
        EXPECT(p.status == PLAN_OK && p.fold == fold && same(p.lstm, c.shape, c.NB, c.NR, c.grid, 128, 20));
        EXPECT(p.q_slots == c.q && p.q_slots == HD / (4 * DG_SHAPES[p.lstm.shape].NT));
      }
  EXPECT(same(plan(beam(256, 8)).lstm, DG_LSTM_128x128, 16, 16, 256, 128, 20) && plan(beam(256, 8)).q_slots == 16);
  EXPECT(same(plan(beam(40, 8)).lstm, DG_LSTM_64x64, 32, 5, 160, 128, 20) && plan(beam(40, 8)).q_slots == 32);

  // the step projection by R: s16 with every |W_p| < 16, s16 with a large weight, f32
  // (shape2 ...: what a large weight or f32 plans instead, the two-accumulator 128 x 160 at R > 512)
  const struct { int R, shape, NB, NR, grid, nkt, shape2, NR2, grid2; } proj[] = {
      {32, DG_PROJ_32x80, 64, 1, 64, 16, DG_PROJ_32x80, 1, 64},
      {33, DG_PROJ_64x80, 64, 1, 64, 16, DG_PROJ_64x80, 1, 64},
      {256, DG_PROJ_64x80, 64, 4, 256, 16, DG_PROJ_64x80, 4, 256},
      {257, DG_PROJ_128x80, 64, 3, 192, 16, DG_PROJ_128x80, 3, 192},
      {512, DG_PROJ_128x80, 64, 4, 256, 16, DG_PROJ_128x80, 4, 256},
      {513, DG_PROJ_128x160_ONE, 32, 5, 160, 16, DG_PROJ_128x160, 5, 160},
      {2047, DG_PROJ_128x160_ONE, 32, 16, 512, 16, DG_PROJ_128x160, 16, 512},
      {2048, DG_PROJ_256x160_ONE, 32, 8, 256, 32, DG_PROJ_128x160, 16, 512}};
  for (const auto& c : proj) {
    DecodePlan p = plan(nofold(greedy(c.R)));
    EXPECT(!p.fold && same(p.proj, c.shape, c.NB, c.NR, c.grid, 316, c.nkt) && p.nbp == 64);
    EXPECT(unused(p.fold_gates) && unused(p.fold_last) && !p.ksplit && !p.ksplit_last);
    p = plan(with_blob(nofold(greedy(c.R)), big_w));
    EXPECT(p.s16 && !p.fold && same(p.proj, c.shape2, c.NB, c.NR2, c.grid2, 316, 16) && p.nbp == 64);
    p = plan(with_blob(nofold(greedy(c.R)), f32));
    EXPECT(!p.s16 && !p.fold && same(p.proj, c.shape2, c.NB, c.NR2, c.grid2, 316, 16) && p.nbp == 64);
  }
  // beam callers take the same projection rules (R = B k)
  EXPECT(same(plan(beam(40, 8)).proj, DG_PROJ_128x80, 64, 3, 192, 316, 16));                // R = 320
  EXPECT(same(plan(beam(72, 8)).proj, DG_PROJ_128x160_ONE, 32, 5, 160, 316, 16));           // R = 576
  EXPECT(same(plan(with_blob(beam(72, 8), big_w)).proj, DG_PROJ_128x160, 32, 5, 160, 316, 16));
  EXPECT(same(plan(with_blob(beam(256, 8), big_w)).proj, DG_PROJ_128x160, 32, 16, 512, 316, 16) &&
         !plan(with_blob(beam(256, 8), big_w)).fold);

  // the folded GEMM: greedy by R and the k split, at a gate-computing step and at the last step
  DecodePlan p = plan(greedy(32));
  EXPECT(p.fold && unused(p.proj) && p.nbp == 45);
  EXPECT(same(p.fold_gates, DG_FOLD_32x112_KS, 64, 1, 256, 443, 16) && p.ksplit);
  EXPECT(same(p.fold_last, DG_FOLD_32x112_KS, 45, 1, 192, 443, 16) && p.ksplit_last);
  p = plan(greedy(32).opt(CASR_OPT_DEC_KSPLIT, 0));
  EXPECT(same(p.fold_gates, DG_FOLD_32x112, 64, 1, 64, 443, 16) && same(p.fold_last, DG_FOLD_32x112, 45, 1, 48, 443, 16));
  EXPECT(!p.ksplit && !p.ksplit_last);
  p = plan(greedy(33));
  EXPECT(same(p.fold_gates, DG_FOLD_64x112, 64, 1, 64, 443, 16) && same(p.fold_last, DG_FOLD_64x112, 45, 1, 48, 443, 16));
  p = plan(with_blob(greedy(256), f32));
  EXPECT(same(p.fold_gates, DG_FOLD_64x112, 64, 4, 256, 443, 16) && same(p.fold_last, DG_FOLD_64x112, 45, 4, 192, 443, 16));
  EXPECT(p.nbp == 45 && !p.ksplit);
  // V = 5204: 326 vocabulary tiles, gates from tile 329, 457 tiles = 66 blocks > 64 counters: the
  // gate steps keep the unsplit 32 x 112 shape, the last step's 47 blocks split
  p = plan(with_vocab(greedy(32), 5204));
  EXPECT(same(p.fold_gates, DG_FOLD_32x112, 66, 1, 72, 457, 16) && !p.ksplit);
  EXPECT(same(p.fold_last, DG_FOLD_32x112_KS, 47, 1, 192, 457, 16) && p.ksplit_last && p.nbp == 47);
  // beam: 224-column blocks, 32-deep stages (R = 2047 is no B k of a folding beam: 2040 stands in)
  p = plan(beam(128, 8));
  EXPECT(same(p.fold_gates, DG_FOLD_128x224_ONE, 32, 8, 256, 443, 32) && same(p.fold_last, DG_FOLD_128x224_ONE, 23, 8, 192, 443, 32));
  p = plan(beam(255, 8));
  EXPECT(p.fold && same(p.fold_gates, DG_FOLD_128x224_ONE, 32, 16, 512, 443, 32) && p.nbp == 45 && p.q_slots == 32);
  p = plan(beam(256, 8));
  EXPECT(same(p.fold_gates, DG_FOLD_256x224_ONE, 32, 8, 256, 443, 32) && same(p.fold_last, DG_FOLD_256x224_ONE, 23, 8, 192, 443, 32));
  EXPECT(unused(p.proj) && !p.ksplit && !p.ksplit_last);

  // casr_score: the LSTMCell at R = B, the batched projection at R = L B on either side of 512 and 2048
  p = plan(score(16, 32));
  EXPECT(p.status == PLAN_OK && p.score_len == 32 && same(p.lstm, DG_LSTM_32x64, 32, 1, 32, 128, 20) && p.q_slots == 32);
  EXPECT(same(p.proj, DG_PROJ_128x80, 64, 4, 256, 316, 16) && p.nbp == 64);
  EXPECT(same(plan(score(16, 33)).proj, DG_PROJ_128x160_ONE, 32, 5, 160, 316, 16) && plan(score(16, 33)).nbp == 64);
  EXPECT(same(plan(with_blob(score(16, 33), f32)).proj, DG_PROJ_128x160, 32, 5, 160, 316, 16));
  EXPECT(same(plan(with_blob(score(16, 33), big_w)).proj, DG_PROJ_128x160, 32, 5, 160, 316, 16));
  EXPECT(same(plan(score(64, 31)).proj, DG_PROJ_128x160_ONE, 32, 16, 512, 316, 16));  // R = 1984
  EXPECT(same(plan(score(64, 32)).proj, DG_PROJ_256x160_ONE, 32, 8, 256, 316, 32));   // R = 2048
  EXPECT(same(plan(with_blob(score(64, 32), f32)).proj, DG_PROJ_128x160, 32, 16, 512, 316, 16));
  EXPECT(plan(score(64, 32)).q_slots == 32 && plan(greedy(16)).score_len == 0);
  {  // the scored length is an input of the score caller only
    In in = greedy(16);
    in.score_len = 7;
    const DecodePlan a = plan(in), b = plan(greedy(16));
    EXPECT(std::memcmp(&a, &b, sizeof a) == 0);
  }

  // over every caller, R, arithmetic and option: an s16-only shape is never planned under f32, the
  // k split only within the arrival counters, nbp from the planned shape's tiles per wave column
  for (int R : {1, 32, 33, 256, 257, 512, 513, 1024, 2040, 2048, 4096})
    for (int V : {16, 1000, 5004, 5120, 5204})
      for (const BlobFacts& b : {BlobFacts{1, 1, 1, 1}, f32, big_w, BlobFacts{1, 1, 1, 0}})
        for (int fold = 0; fold < 2; ++fold)
          for (int caller : {PLAN_GREEDY, PLAN_BEAM, PLAN_SCORE}) {
            In in = caller == PLAN_BEAM ? beam((R + 7) / 8, 8) : caller == PLAN_SCORE ? score((R + 39) / 40, 40) : greedy(R);
            in.V = V;
            in.blob = b;
            in.opt(CASR_OPT_DEC_FOLD, fold);
            const DecodePlan q = plan(in);
            if (q.status != PLAN_OK) continue;
            const int vtiles = (V + 15) / 16, ptiles = (V + 63) / 64 * 4;
            for (const DgemmPlan* g : {&q.lstm, &q.proj, &q.fold_gates, &q.fold_last}) {
              if (unused(*g)) continue;
              EXPECT(g->shape >= 0 && g->shape < DG_SHAPE_COUNT && g->grid > 0);
              EXPECT(q.s16 || !dg_s16_only(DG_SHAPES[g->shape]));
              EXPECT(g->shape != DG_FOLD_32x112_KS || (g->NB <= DG_KS_GROUPS && q.R <= 32));
              EXPECT(g->NB * DG_SHAPES[g->shape].NT >= (g == &q.fold_last ? vtiles : g->ntiles));
            }
            EXPECT(unused(q.proj) == (q.fold != 0) && unused(q.fold_gates) == !q.fold && unused(q.fold_last) == !q.fold);
            EXPECT(q.ksplit == (q.fold && q.fold_gates.shape == DG_FOLD_32x112_KS));
            EXPECT(q.ksplit_last == (q.fold && q.fold_last.shape == DG_FOLD_32x112_KS));
            if (q.partials)
              EXPECT(q.nbp == (q.fold ? (vtiles + 6) / 7 : (ptiles + 4) / 5) && q.nbp <= GP_NB);
          }
}

// ---------------------------------------------------------------- the accepted vocabularies
// check_config accepts any vocab >= 4.  Over the small vocabularies, both sides of the partial-block
// limit of the projection (V = 5120 | 5121) and of the fused GEMM (V = 7168 | 7169), every R of the
// sweep above and the three callers: each launch's column blocks cover the tiles it must write, and
// every table a kernel indexes by a column block or a tile (GreedyPart's GP_NB and GP_NT, the k
// split's DG_KS_GROUPS arrival counters) is only planned within its size.
static void check_vocab_sweep() {
  std::vector<int> vs;
  for (int V = 4; V <= 100; ++V) vs.push_back(V);
  for (int V = 5000; V <= 5130; ++V) vs.push_back(V);
  for (int V = 7160; V <= 7175; ++V) vs.push_back(V);
  for (int V : vs)
    for (int R : {1, 32, 33, 256, 257, 512, 513, 1024, 2040, 2048, 4096})
      for (int fold = 0; fold < 2; ++fold)
        for (int caller : {PLAN_GREEDY, PLAN_BEAM, PLAN_SCORE}) {
          In in = caller == PLAN_BEAM ? beam((R + 7) / 8, 8) : caller == PLAN_SCORE ? score((R + 39) / 40, 40) : greedy(R);
          in.V = V;
          in.opt(CASR_OPT_DEC_FOLD, fold);
          const DecodePlan q = plan(in);
          const int vtiles = (V + 15) / 16, ptiles = (V + 63) / 64 * 4, gt0 = (vtiles + 6) / 7 * 7;
          if (caller == PLAN_BEAM && 16 > V) {  // 2k candidates from fewer than 2k tokens
            EXPECT(q.status == PLAN_K_VOCAB);
            continue;
          }
          if (caller == PLAN_SCORE && (ptiles + 4) / 5 > GP_NB) {
            EXPECT(q.status == PLAN_VOCAB);
            continue;
          }
          EXPECT(q.status == PLAN_OK);
          EXPECT(fold_vtiles(V) == vtiles && fold_gtile0(V) == gt0 && gt0 >= vtiles && gt0 - vtiles < FOLD_NT);
          // the launches: column blocks x tiles per block over the tiles each must cover
          EXPECT(q.lstm.NB * DG_SHAPES[q.lstm.shape].NT >= FOLD_GT && q.lstm.ntiles == FOLD_GT);
          if (!q.fold) {
            EXPECT(q.proj.ntiles == ptiles && q.proj.NB * DG_SHAPES[q.proj.shape].NT >= ptiles && ptiles >= vtiles);
            EXPECT(unused(q.fold_gates) && unused(q.fold_last));
          } else {
            EXPECT(unused(q.proj) && q.fold_gates.ntiles == gt0 + FOLD_GT && q.fold_last.ntiles == gt0 + FOLD_GT);
            EXPECT(q.fold_gates.NB * DG_SHAPES[q.fold_gates.shape].NT >= gt0 + FOLD_GT);
            EXPECT(q.fold_last.NB * DG_SHAPES[q.fold_last.shape].NT >= vtiles);
            // the fold only while its vocabulary blocks fit the partial blocks, and never for score
            EXPECT(gt0 / FOLD_NT <= GP_NB && caller != PLAN_SCORE && fold);
          }
          if (caller == PLAN_GREEDY) EXPECT(q.fold == (fold && gt0 / FOLD_NT <= GP_NB));
          // row partials: one per wave column of the planned shape, within GreedyPart's GP_NB
          const int blocks = q.fold ? (vtiles + 6) / 7 : (ptiles + 4) / 5;
          EXPECT(q.partials == (blocks <= GP_NB) && q.nbp == (q.partials ? blocks : 0) && q.nbp <= GP_NB);
          EXPECT(q.tile_max == (caller == PLAN_BEAM && q.partials && V <= 16 * GP_NT));
          EXPECT(!q.tile_max || vtiles <= GP_NT);
          EXPECT(q.store_logits == (caller == PLAN_BEAM || !q.partials));
          if (caller == PLAN_GREEDY) EXPECT(q.fuse_select == q.partials);
          // the k split only within its arrival counters
          for (const DgemmPlan* g : {&q.fold_gates, &q.fold_last}) {
            if (unused(*g)) continue;
            const bool ks = g->shape == DG_FOLD_32x112_KS;
            EXPECT(!ks || (g->NB <= DG_KS_GROUPS && q.R <= 32 && caller == PLAN_GREEDY));
            if (caller == PLAN_GREEDY && q.R <= 32) EXPECT(ks == (g->NB <= DG_KS_GROUPS));
          }
          EXPECT(q.ksplit == (q.fold && q.fold_gates.shape == DG_FOLD_32x112_KS));
          EXPECT(q.ksplit_last == (q.fold && q.fold_last.shape == DG_FOLD_32x112_KS));
        }
  // the four boundaries by value.  V = 5120 fills all 64 partial blocks and the whole tile table
  auto nofold = [](In in) { return in.opt(CASR_OPT_DEC_FOLD, 0); };
  DecodePlan p = plan(with_vocab(beam(40, 8), 5120));
  EXPECT(!p.fold && p.partials && p.nbp == GP_NB && p.tile_max && p.proj.ntiles == GP_NT && p.proj.NB == 64);
  p = plan(with_vocab(nofold(greedy(19)), 5120));
  EXPECT(!p.fold && p.partials && p.nbp == 64 && p.fuse_select && !p.store_logits);
  EXPECT(plan(with_vocab(score(5, 40), 5120)).status == PLAN_OK && plan(with_vocab(score(5, 40), 5120)).nbp == 64);
  p = plan(with_vocab(beam(128, 8), 5120));
  EXPECT(p.fold && p.partials && p.nbp == 46 && p.tile_max && p.fuse_select);
  // V = 5121: 324 projection tiles, 65 blocks: the three-launch step without partials and tile maxima
  p = plan(with_vocab(beam(40, 8), 5121));
  EXPECT(p.status == PLAN_OK && !p.fold && !p.partials && p.nbp == 0 && !p.tile_max && p.store_logits && p.proj.NB == 65);
  p = plan(with_vocab(nofold(greedy(19)), 5121));
  EXPECT(!p.fold && !p.partials && p.nbp == 0 && !p.fuse_select && p.store_logits);
  EXPECT(plan(with_vocab(score(5, 40), 5121)).status == PLAN_VOCAB);
  p = plan(with_vocab(greedy(19), 5121));  // (the fused GEMM's seven-tile blocks: 321 tiles, 46 blocks)
  EXPECT(p.fold && p.partials && p.nbp == 46 && p.fuse_select);
  p = plan(with_vocab(beam(128, 8), 5121));  // ... the folded beam keeps its partials, not the tile maxima
  EXPECT(p.fold && p.partials && p.nbp == 46 && !p.tile_max && p.fuse_select);
  // V = 7168: 448 vocabulary tiles, no pad tile, fold_blocks == 64: the last vocabulary that folds.  The
  // gate steps' 83 column blocks are past the arrival counters, the last step's 64 fit them
  p = plan(with_vocab(greedy(19), 7168));
  EXPECT(fold_vtiles(7168) == 448 && fold_gtile0(7168) == 448);
  EXPECT(p.fold && p.partials && p.nbp == 64 && p.fuse_select && !p.store_logits);
  EXPECT(same(p.fold_gates, DG_FOLD_32x112, 83, 1, 88, 576, 16) && !p.ksplit);
  EXPECT(same(p.fold_last, DG_FOLD_32x112_KS, 64, 1, 256, 576, 16) && p.ksplit_last);
  EXPECT(plan(with_vocab(beam(128, 8), 7168)).fold && !plan(with_vocab(beam(128, 8), 7168)).tile_max);
  // V = 7169: 449 tiles, 65 blocks: even greedy keeps the three-launch step, with a full-row select
  p = plan(with_vocab(greedy(19), 7169));
  EXPECT(fold_vtiles(7169) == 449 && fold_gtile0(7169) == 455);
  EXPECT(p.status == PLAN_OK && !p.fold && !p.build_fold32 && !p.partials && !p.fuse_select && p.store_logits);
  EXPECT(!p.ksplit && !p.ksplit_last && p.proj.ntiles == 452 && p.proj.NB == 91);
  EXPECT(!plan(with_vocab(beam(128, 8), 7169)).fold && !plan(with_vocab(beam(128, 8), 7169)).partials);
  EXPECT(plan(with_vocab(score(5, 40), 7169)).status == PLAN_VOCAB);
}

// A beam step keeps 2k candidates per utterance (model.py:863, torch.topk over the vocabulary, raises
// there): refused for every beam caller, before anything else is planned
static void check_width_against_vocab() {
  for (int caller : {PLAN_BEAM, PLAN_BEAM_LM})
    for (int V : {4, 5, 31, 32, 33, 83})
      for (int k = 1; k <= KMAX_BEAM; ++k) {
        In in = with_vocab(beam(3, k), V);
        in.caller = caller;
        const DecodePlan p = plan(in);
        EXPECT(p.status == (2 * k > V ? PLAN_K_VOCAB : PLAN_OK));
        if (p.status != PLAN_OK) EXPECT(p.R == 0 && p.K2 == 0 && unused(p.lstm) && unused(p.proj));
      }
  EXPECT(plan(with_vocab(beam(3, 4), 4)).status == PLAN_K_VOCAB);   // the pair that must never launch
  EXPECT(plan(with_vocab(beam(3, 2), 4)).status == PLAN_OK && plan(with_vocab(beam(3, 2), 4)).K2 == 4);
  EXPECT(plan(with_vocab(beam(3, 17), 4)).status == PLAN_BAD_K);    // (the width's own range comes first)
  // greedy and score have no width
  EXPECT(plan(with_vocab(greedy(3), 4)).status == PLAN_OK && plan(with_vocab(score(3, 1), 4)).status == PLAN_OK);
}

static void check_keys() {
  const DecodePlan p = plan(beam(256, 8));
  const float sc[2] = {0.25f, 0.5f};
  int x = 0, y = 0;
  const void* bufs[2] = {&x, &y};
  const std::vector<uint64_t> base = decode_graph_key(3, p, sc, 2, bufs, 2);
  EXPECT(base == decode_graph_key(3, p, sc, 2, bufs, 2));
  for (size_t i = 0; i < sizeof(DecodePlan) / sizeof(int32_t); ++i) {  // any one field
    DecodePlan q = p;
    int32_t w;
    std::memcpy(&w, reinterpret_cast<char*>(&q) + 4 * i, 4);
    w ^= 1;
    std::memcpy(reinterpret_cast<char*>(&q) + 4 * i, &w, 4);
    EXPECT(decode_graph_key(3, q, sc, 2, bufs, 2) != base);
  }
  const DecodePlan nofuse = plan(beam(256, 8).opt(CASR_OPT_FUSE_SELECT, 0));
  EXPECT(nofuse.fuse_select != p.fuse_select && decode_graph_key(3, nofuse, sc, 2, bufs, 2) != base);
  EXPECT(decode_graph_key(2, p, sc, 2, bufs, 2) != base);
  const float sc2[2] = {0.25f, 0.75f};
  EXPECT(decode_graph_key(3, p, sc2, 2, bufs, 2) != base);
  const void* bufs2[2] = {&x, &x};
  EXPECT(decode_graph_key(3, p, sc, 2, bufs2, 2) != base);
}

// one carved workspace: its regions (pointer, bytes, required alignment) inside [base, base + size)
struct Region {
  const void* p;
  size_t bytes, align;
};
static void check_regions(char* base, size_t size, size_t at_least, const std::vector<Region>& rs) {
  EXPECT(size >= at_least);
  for (size_t i = 0; i < rs.size(); ++i) {
    const char* p = static_cast<const char*>(rs[i].p);
    EXPECT(p >= base && p + rs[i].bytes <= base + size);
    EXPECT((size_t)(p - base) % rs[i].align == 0 && (uintptr_t)p % rs[i].align == 0);
    std::memset(const_cast<char*>(p), (int)i + 1, rs[i].bytes);  // (under ASan: inside the allocation)
    for (size_t j = 0; j < i; ++j) {
      const char* q = static_cast<const char*>(rs[j].p);
      EXPECT(p + rs[i].bytes <= q || q + rs[j].bytes <= p);
    }
  }
}
// sizing pass, then the carve of an exact-size 16 B-aligned allocation
template <class Carve>
static char* carved(Carve carve, size_t* size) {
  *size = carve(nullptr);
  char* base = static_cast<char*>(std::aligned_alloc(256, (*size + 255) / 256 * 256));
  EXPECT(base && carve(base) == *size);
  return base;
}

static void check_carving() {
  const int cases[4][4] = {{1, 1, 1, 4}, {3, 16, 40, 5004}, {256, 8, 40, 5004}, {5, 2, 64, 5204}};
  const int Tp = 266;
  for (const auto& cs : cases) {
    const int B = cs[0], k = cs[1], L = cs[2], V = cs[3];
    const size_t R = (size_t)B * k, f = sizeof(float);
    DecodeBufs d{};
    size_t size;
    const DecodePlan pl = plan(beam(B, k));
    EXPECT(pl.status == PLAN_OK && pl.R == (int)R);
    char* base = carved([&](void* p) { return carve_state(p, pl, d); }, &size);
    const size_t slots = R >= 2048 ? HD / 32 : HD / 16;
    EXPECT((size_t)pl.q_slots == slots);
    check_regions(base, size, (2 * R * ST + slots * R * A) * f,
                  {{d.st[0], R * ST * f, 16}, {d.st[1], R * ST * f, 16}, {d.qpart, slots * R * A * f, 16}});
    std::free(base);

    base = carved([&](void* p) { return carve_logits(p, (int)R, V, d); }, &size);
    check_regions(base, size, (R * V + 3 * R * 64 + R * 320) * f,
                  {{d.logits, R * V * f, 16}, {d.part.mx, R * 64 * f, 16}, {d.part.se, R * 64 * f, 16},
                   {d.part.ix, R * 64 * 4, 16}, {d.part.tmx, R * 320 * f, 16}});
    std::free(base);

    base = carved([&](void* p) { return carve_small(p, B, (int)R, L, d); }, &size);
    check_regions(base, size, (6 * R + L + B + R + 1) * 4 + 256,
                  {{d.tok[0], R * 4, 4}, {d.tok[1], R * 4, 4}, {d.src[0], R * 4, 4}, {d.src[1], R * 4, 4},
                   {d.score[0], R * f, 4}, {d.score[1], R * f, 4}, {d.newdone, (size_t)L * 4, 4},
                   {d.topfin, (size_t)B, 1}, {d.fin, R, 1}});
    std::free(base);

    const size_t n = (size_t)B * L * k;
    base = carved([&](void* p) { return carve_records(p, B, L, k, d); }, &size);
    check_regions(base, size, n * (f + 4 + 1) + 256, {{d.rec_score, n * f, 4}, {d.rec_src, n * 4, 4}, {d.rec_valid, n, 1}});
    std::free(base);

    base = carved([&](void* p) { return carve_ksplit(p, d); }, &size);
    check_regions(base, size, DG_KS_PART_BYTES + DG_KS_COUNTERS * 4,
                  {{d.kspart, (size_t)128 * 4 * 7 * 64 * 16, 16}, {d.kscnt, 128 * 4, 4}});
    std::free(base);

    base = carved([&](void* p) { return carve_attn_split(p, (int)R, d); }, &size);
    check_regions(base, size, R * 8 * (C + 4) * f + R * 4, {{d.aspart, R * 8 * (C + 4) * f, 16}, {d.ascnt, R * 4, 4}});
    std::free(base);

    for (size_t nal : {(size_t)0, (size_t)L * Tp * B}) {
      GreedyOut o{};
      base = carved([&](void* p) { return carve_greedy_out(p, B, L, nal, o); }, &size);
      std::vector<Region> rs = {{o.tokens, (size_t)B * L * 4, 4}, {o.len, (size_t)B * 4, 4}, {o.accum, B * f, 4},
                                {o.fin, (size_t)B, 1}};
      EXPECT((o.align != nullptr) == (nal != 0));
      if (nal) rs.push_back({o.align, nal * f, 4});
      check_regions(base, size, 4 * ((size_t)B * L + B) + f * (B + nal) + B + 64, rs);
      std::free(base);
    }
    BeamOut o{};
    base = carved([&](void* p) { return carve_beam_out(p, B, L, o); }, &size);
    check_regions(base, size, 4 * ((size_t)B * L + B + 1) + f * B + 64,
                  {{o.tokens, (size_t)B * L * 4, 4}, {o.len, (size_t)B * 4, 4}, {o.steps, 4, 4}, {o.score, B * f, 4}});
    std::free(base);
  }
}

static void check_options() {
  const int defaults[CASR_OPT_COUNT] = {1, 0, 1, -1, 2, 2, 2, 2, 0, 0, 1, 0, 0, 1, 1, 1, 1, 0, 0};
  const Tuning t;
  for (int o = 0; o < CASR_OPT_COUNT; ++o) {
    EXPECT(OPTIONS[o].id == o && t[o] == defaults[o] && OPTIONS[o].def == defaults[o]);
    EXPECT(OPTIONS[o].lo <= OPTIONS[o].def && OPTIONS[o].def <= OPTIONS[o].hi);
    EXPECT(option_value_ok(o, OPTIONS[o].lo) && option_value_ok(o, OPTIONS[o].hi) && option_value_ok(o, OPTIONS[o].def));
    EXPECT(!option_value_ok(o, OPTIONS[o].lo - 1) && !option_value_ok(o, OPTIONS[o].hi + 1));
  }
  for (int v : {1, 2, 3, 5, 6, 7}) EXPECT(!option_value_ok(CASR_OPT_ATTN_KPB, v));
  EXPECT(option_value_ok(CASR_OPT_ATTN_KPB, 4));
  EXPECT(!option_value_ok(-1, 0) && !option_value_ok(CASR_OPT_COUNT, 0));
  EXPECT(OPTIONS[CASR_OPT_ATTN_SPLIT].hi == AT_SPLIT_MAX && OPTIONS[CASR_OPT_REC_SLEEP].hi == 16);
}

int main() {
  check_greedy();
  check_beam();
  check_score();
  check_shape_table();
  check_gemm_plans();
  check_vocab_sweep();
  check_width_against_vocab();
  check_keys();
  check_carving();
  check_options();
  std::puts("plan_check ok");
  return 0;
}
