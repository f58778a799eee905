// Host check of the encode plan (chinese-asr_amd/csrc/encode_plan.h): built from that header alone
// with clang AddressSanitizer + UndefinedBehaviorSanitizer and run as a program by
// tests/test_encode_plan_host.py; no GPU, no HIP runtime.
//
// The expected values are the decisions the launchers made before the plan existed (encode_impl,
// launch_input_proj_s16_big, rec_layout / launch_rec_layer / reset_rec_layer, launch_keys_s16,
// features_x16_supported), read from that code and worked out by hand here; the sizes in
// check_workspaces are that code's ensure() formulas.  The device: 256 CUs, 2 resident workgroups
// per CU in every layout.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "encode_plan.h"

using namespace casr;

#define EXPECT(c)                                                                       \
  do {                                                                                  \
    if (!(c)) {                                                                         \
      std::fprintf(stderr, "encode_plan_check: %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      std::exit(3);                                                                     \
    }                                                                                   \
  } while (0)

static const DeviceFacts kDev{256, {2, 2, 2}};

// the tables' inputs "unless a row says otherwise": the bench shape under s16, casr_encode
struct In {
  int B = 256, Tp = 266, T = 0;
  bool fbank = false, s16 = true, persistent = true;
  Tuning t;
  DeviceFacts dev = kDev;
  In& opt(int o, int v) {
    t.v[o] = v;
    return *this;
  }
};
static In batch(int B, int Tp = 266) {
  In in;
  in.B = B;
  in.Tp = Tp;
  return in;
}
static In fbank(int T, bool s16 = true) {
  In in;
  in.T = T;
  in.Tp = T / 3;
  in.fbank = true;
  in.s16 = s16;
  return in;
}
static EncodePlan plan(const In& in) {
  casr_config cfg{};
  cfg.enc_layers = 4;
  cfg.residual = 1;
  return plan_encode(in.B, in.Tp, in.T, in.fbank, cfg, in.t, in.s16, in.persistent, in.dev);
}

static void check_recurrence() {
  // automatic layout: 16x16 while 16 x ceil(B / 16) x 2 workgroups fit one per CU, else 32x16
  RecPlan r = plan(batch(256)).rec;
  EXPECT(r.persistent && r.layout == REC_32x16 && r.RG == 32 && r.UW == 16 && r.nrg == 8 && r.Bp == 256);
  EXPECT(r.grid == 256 && r.block == 512 && r.sleep == 0 && r.gap == 2 && r.plain == 1 && r.coop == 2 && r.refuse == 0);
  EXPECT(r.waves() == 8 && r.producers() == 16 && r.B == 256 && r.Tp == 266 && r.s16 == 1 && r.km == 1);
  r = plan(batch(128)).rec;
  EXPECT(r.persistent && r.layout == REC_16x16 && r.RG == 16 && r.UW == 16 && r.nrg == 8 && r.Bp == 128);
  EXPECT(r.grid == 256 && r.block == 256 && r.waves() == 4 && r.sleep == 0);
  r = plan(batch(37)).rec;
  EXPECT(r.persistent && r.layout == REC_16x16 && r.nrg == 3 && r.Bp == 64 && r.grid == 96 && r.sleep == 0);
  r = plan(batch(16)).rec;
  EXPECT(r.persistent && r.layout == REC_16x16 && r.nrg == 1 && r.Bp == 32 && r.grid == 32 && r.sleep == 1);
  // 64 workgroups is the first grid without the sleep (B = 17..32 in the 16-row layout)
  EXPECT(plan(batch(17)).rec.grid == 64 && plan(batch(17)).rec.sleep == 0);
  // both sides of the automatic rule: B = 128 is the last 16x16 batch
  EXPECT(plan(batch(129)).rec.layout == REC_32x16 && plan(batch(129)).rec.grid == 160);
  // the options
  EXPECT(plan(batch(16).opt(CASR_OPT_REC_SLEEP, 0)).rec.sleep == 0);
  EXPECT(plan(batch(256).opt(CASR_OPT_REC_SLEEP, 16)).rec.sleep == 16);
  EXPECT(plan(batch(256).opt(CASR_OPT_REC_POLL_GAP, 8)).rec.gap == 8);
  EXPECT(plan(batch(256).opt(CASR_OPT_REC_STORE_PLAIN, 0)).rec.plain == 0);
  for (int c = 0; c <= 2; ++c) EXPECT(plan(batch(256).opt(CASR_OPT_REC_COOP, c)).rec.coop == c);
  EXPECT(plan(batch(256).opt(CASR_OPT_REC_COOP_REFUSE, 3)).rec.refuse == 3);
  r = plan(batch(128).opt(CASR_OPT_REC_LAYOUT, 1)).rec;
  EXPECT(r.layout == REC_32x16 && r.grid == 128 && r.block == 512 && r.nrg == 4);
  r = plan(batch(256).opt(CASR_OPT_REC_LAYOUT, 2)).rec;
  EXPECT(r.layout == REC_16x32 && r.RG == 16 && r.UW == 32 && r.nrg == 16 && r.grid == 256 && r.block == 512);
  EXPECT(r.waves() == 8 && r.producers() == 8 && r.persistent);
  r = plan(batch(256).opt(CASR_OPT_REC_LAYOUT, 3)).rec;
  EXPECT(r.layout == REC_16x16 && r.grid == 512 && r.block == 256 && r.persistent);  // 512 = 256 CUs x 2
  // fits: the grid within cus x per_cu of its layout, and the persistent form asked for
  EXPECT(!plan(batch(257).opt(CASR_OPT_REC_LAYOUT, 3)).rec.persistent);  // 544 workgroups
  In one = batch(256);
  one.dev.rec_per_cu[REC_32x16] = 1;
  EXPECT(plan(one).rec.persistent);  // 256 <= 256 x 1
  one.B = 257;
  EXPECT(plan(one).rec.grid == 288 && !plan(one).rec.persistent);
  one.dev.rec_per_cu[REC_32x16] = 0;  // the occupancy query failed
  one.B = 1;
  one.opt(CASR_OPT_REC_LAYOUT, 1);
  EXPECT(!plan(one).rec.persistent);
  In off = batch(256);
  off.persistent = false;
  EXPECT(!plan(off).rec.persistent && plan(off).rec.grid == 256);  // the shape is planned either way
  // the per-step fallback's graphs
  r = plan(batch(63)).rec;
  EXPECT(r.nsplit == 1 && r.row0[0] == 0 && r.row1[0] == 63);
  r = plan(batch(64)).rec;
  EXPECT(r.nsplit == 2 && r.row0[0] == 0 && r.row1[0] == 32 && r.row0[1] == 32 && r.row1[1] == 64);
  r = plan(batch(100)).rec;
  EXPECT(r.nsplit == 2 && r.row0[0] == 0 && r.row1[0] == 64 && r.row0[1] == 64 && r.row1[1] == 100);
  // f32: the same shapes, no image
  In f = batch(256);
  f.s16 = false;
  EXPECT(plan(f).rec.s16 == 0 && plan(f).rec.km == 0 && plan(f).rec.grid == 256);
}

struct TailRow {
  int B, M, NM, NMm, tail_rows, RT, blocks;
};
static void check_input_gemm() {
  // defaults (ping-pong, balanced tail, 16-k-major images), Tp = 266
  const TailRow rows[] = {{256, 68096, 266, 256, 2560, 5, 256},
                          {128, 34048, 133, 128, 1280, 3, 224},
                          {37, 9842, 39, 32, 1650, 4, 208},
                          {31, 8246, 33, 32, 54, 1, 32}};
  for (const TailRow& w : rows) {
    const EncodePlan p = plan(batch(w.B));
    EXPECT(p.status == ENC_OK && p.M == w.M && p.km == 1);
    for (int l = 0; l < 2; ++l) {
      const InputGemmPlan& g = p.gemm[l];
      EXPECT(&p.layer_gemm(l) == &g && &p.layer_gemm(3) == &p.gemm[1]);
      EXPECT(g.form == GEMM16_PP_KM && g.M == w.M && g.km == 1 && g.NB == 8 && g.NM == w.NM && g.NG == 2);
      EXPECT(g.K == (l ? 512 : 720) && g.Kp == (l ? 512 : 768) && g.nk16 == (l ? 32 : 45) && g.nk == (l ? 16 : 23));
      EXPECT(g.NMm == w.NMm && g.Mm == w.NMm * 256 && g.total == 8 * w.NMm && g.grid == 256);
      EXPECT(g.tail == TAIL_BALANCED && g.r0 == w.NMm * 256 && g.Mt == w.tail_rows && g.r0 + g.Mt == w.M);
      EXPECT(g.RT == w.RT && g.tail_grid == w.blocks && g.NMt == 0);
    }
  }
  // B = 30: F ncu / NB = NM = 32 whole row tiles, nothing after them; B <= 29: F = 0
  InputGemmPlan g = plan(batch(30)).gemm[0];
  EXPECT(g.M == 7980 && g.NM == 32 && g.NMm == 32 && g.tail == TAIL_NONE && g.Mm == 7980 && g.total == 256 && g.grid == 256);
  EXPECT(g.r0 == 0 && g.Mt == 0 && g.RT == 0 && g.tail_grid == 0);
  g = plan(batch(29)).gemm[1];
  EXPECT(g.M == 7714 && g.NM == 31 && g.NMm == 31 && g.tail == TAIL_NONE && g.Mm == 7714 && g.total == 256 && g.grid == 256);
  g = plan(batch(1, 3)).gemm[0];  // one partial tile: 8 column blocks, a grid of 32 (4 row slots per XCD pair)
  EXPECT(g.M == 3 && g.NM == 1 && g.total == 32 && g.grid == 32 && g.Mm == 3 && g.tail == TAIL_NONE);
  // CASR_OPT_GEMM16_TAIL: 1 = the half tiles (row images), 0 = no tail
  EncodePlan p = plan(batch(256).opt(CASR_OPT_GEMM16_TAIL, 1));
  g = p.gemm[0];
  EXPECT(p.km == 0 && g.form == GEMM16_PP && g.NMm == 256 && g.tail == TAIL_HALF && g.Mt == 2560 && g.NMt == 20);
  EXPECT(g.tail_grid == 160 && g.RT == 0);
  g = plan(batch(37).opt(CASR_OPT_GEMM16_TAIL, 1)).gemm[1];
  EXPECT(g.tail == TAIL_HALF && g.NMt == 13 && g.tail_grid == 128 && g.r0 == 8192);
  p = plan(batch(256).opt(CASR_OPT_GEMM16_TAIL, 0));
  g = p.gemm[0];
  EXPECT(p.km == 1 && g.form == GEMM16_PP_KM && g.NMm == 266 && g.tail == TAIL_NONE && g.Mm == 68096 && g.total == 2144);
  EXPECT(g.grid == 256);
  // CASR_OPT_GEMM16_PERSIST: 1 = the 32-deep persistent kernel (row images), 0 = the per-tile grid
  p = plan(batch(256).opt(CASR_OPT_GEMM16_PERSIST, 1));
  EXPECT(p.km == 0 && p.gemm[0].form == GEMM16_PERSIST && p.gemm[0].nk == 23 && p.gemm[1].nk == 16);
  EXPECT(p.gemm[0].tail == TAIL_BALANCED && p.gemm[0].RT == 5 && p.gemm[0].km == 0 && p.gemm[0].NMm == 256);
  p = plan(batch(256).opt(CASR_OPT_GEMM16_PERSIST, 0));
  g = p.gemm[0];
  EXPECT(p.km == 0 && g.form == GEMM16_TILES && g.grid == 2144 && g.NMm == 266 && g.Mm == 68096 && g.tail == TAIL_NONE);
  // lean needs the 16-k-major images (and nk16 >= 8: 45 and 32 here)
  p = plan(batch(256).opt(CASR_OPT_GEMM16_LEAN, 1));
  EXPECT(p.gemm[0].form == GEMM16_PP_LEAN && p.gemm[1].form == GEMM16_PP_LEAN && p.gemm[0].tail == TAIL_BALANCED);
  p = plan(batch(256).opt(CASR_OPT_GEMM16_LEAN, 1).opt(CASR_OPT_X16_KM, 0));
  EXPECT(p.km == 0 && p.gemm[0].form == GEMM16_PP && p.gemm[1].form == GEMM16_PP);
  {
    Tuning t;
    t.v[CASR_OPT_GEMM16_LEAN] = 1;
    EXPECT(plan_input_gemm(1000, 127, t, true, true, kDev).form == GEMM16_PP_LEAN);  // nk16 = 8
    EXPECT(plan_input_gemm(1000, 112, t, true, true, kDev).form == GEMM16_PP_KM);    // nk16 = 7
  }
  // f32: encoder.hip's GEMM, nothing of the s16 forms
  In f = batch(256);
  f.s16 = false;
  p = plan(f);
  EXPECT(p.s16 == 0 && p.km == 0 && p.gemm[0].form == GEMM_F32 && p.gemm[0].K == 720 && p.gemm[0].Kp == 720);
  EXPECT(p.gemm[1].form == GEMM_F32 && p.gemm[1].K == 512 && p.gemm[1].M == 68096);
}

// km = 1 only for X16_KM with PERSIST = 2, TAIL != 1 and KEYS_ROWS under s16, and no combination
// reaches a form that cannot read its image
static void check_km() {
  for (int s16 = 0; s16 < 2; ++s16)
    for (int x = 0; x < 2; ++x)
      for (int ps = 0; ps <= 2; ++ps)
        for (int tl = 0; tl <= 2; ++tl)
          for (int kr = 0; kr < 2; ++kr)
            for (int lean = 0; lean < 2; ++lean)
              for (int B : {256, 37, 30, 1}) {
                In in = batch(B);
                in.s16 = s16 != 0;
                in.opt(CASR_OPT_X16_KM, x).opt(CASR_OPT_GEMM16_PERSIST, ps).opt(CASR_OPT_GEMM16_TAIL, tl);
                in.opt(CASR_OPT_KEYS_ROWS, kr).opt(CASR_OPT_GEMM16_LEAN, lean);
                const EncodePlan p = plan(in);
                EXPECT(p.status == ENC_OK);
                EXPECT(p.km == (s16 && x && ps == 2 && tl != 1 && kr));
                EXPECT(p.rec.km == p.km && p.keys.km == p.km && p.gemm[0].km == p.km && p.gemm[1].km == p.km);
                for (const InputGemmPlan& g : p.gemm) {
                  const bool reads_km = g.form == GEMM16_PP_KM || g.form == GEMM16_PP_LEAN;
                  EXPECT(reads_km == (p.km != 0));
                  if (p.km) EXPECT(g.tail != TAIL_HALF);
                  if (g.form == GEMM16_PP_LEAN) EXPECT(lean && p.km);
                }
                if (p.km) EXPECT(p.keys.form == KEYS16_ROWS);
              }
}

static void check_features() {
  EXPECT(plan(batch(256)).feat == FEAT_GIVEN);
  EXPECT(plan(fbank(1024)).feat == FEAT_IMAGE && plan(fbank(1024)).Tp == 341);
  EXPECT(plan(fbank(3)).feat == FEAT_IMAGE);
  EXPECT(plan(fbank(1025)).feat == FEAT_TWO_PASS);
  EXPECT(plan(fbank(1024, false)).feat == FEAT_ROWS && plan(fbank(800, false)).feat == FEAT_ROWS);
  EXPECT(plan(fbank(1025, false)).feat == FEAT_TWO_PASS);
  EXPECT(feature_path(1024, false) == FEAT_ROWS && feature_path(1025, false) == FEAT_TWO_PASS);  // casr_features
}

static void check_keys() {
  KeysPlan k = plan(batch(256)).keys;  // min(B ceil(Tp / 16), cus) = min(256 x 17, 256)
  EXPECT(k.form == KEYS16_ROWS && k.grid == 256 && k.B == 256 && k.Tp == 266 && k.Tq == 268 && k.km == 1 && k.split == 1);
  k = plan(batch(1, 3)).keys;
  EXPECT(k.form == KEYS16_ROWS && k.grid == 1 && k.Tq == 4);
  k = plan(batch(3, 40)).keys;
  EXPECT(k.grid == 9);
  // the tiled forms: 532 row tiles of 128, one column block, 8 x ceil(532 / 8) workgroups
  EncodePlan p = plan(batch(256).opt(CASR_OPT_KEYS_ROWS, 0));
  EXPECT(p.km == 0 && p.keys.form == KEYS16_TILES && p.keys.NM == 532 && p.keys.NG == 1 && p.keys.grid == 536);
  In f = batch(256);
  f.s16 = false;
  k = plan(f).keys;
  EXPECT(k.form == KEYS_F32 && k.NM == 532 && k.NG == 1 && k.grid == 536 && k.split == 0 && k.km == 0 && k.Tq == 268);
  f.opt(CASR_OPT_KEYS_ROWS, 0);
  EXPECT(plan(f).keys.form == KEYS_F32);
  // 32-bit buffer offsets of the row-streaming form: 2 B A Tq 4 bytes below 0xFFFFFFF0
  EXPECT(plan(batch(4096, 1020)).status == ENC_OK);
  EXPECT(plan(batch(4096, 1021)).status == ENC_KEYS_OFFSET);  // Tq = 1024: 2^32 bytes
  EXPECT(plan(batch(4096, 1024).opt(CASR_OPT_KEYS_ROWS, 0)).status == ENC_OK);
  // bad shapes
  EXPECT(plan(batch(0)).status == ENC_BAD_SHAPE && plan(batch(4, 0)).status == ENC_BAD_SHAPE);
  EXPECT(plan(batch(-1)).status == ENC_BAD_SHAPE && plan(batch(65536, 32768)).status == ENC_BAD_SHAPE);
}

static void check_workspaces() {
  In in = fbank(800);
  EncodePlan p = plan(in);
  EncodeSizes z = encode_sizes(p);
  const size_t rows = 256 * 266;
  EXPECT(p.M == (int)rows);
  EXPECT(z.gin == rows * 8 * 256 * 4 && z.out == rows * 512 * 4 && z.hbuf == (size_t)2 * 2 * 256 * 256 * 4);
  EXPECT(z.cst == (size_t)2 * 256 * 256 * 4 && z.hfin == z.cst && z.keysT == (size_t)2 * 256 * 128 * 268 * 4);
  EXPECT(z.lens == 256 * 4 && z.x16 == rows * 768 * 4 && z.feat == 0 && z.fstat == (size_t)256 * 2 * 720 * 4);
  // the hand-off buffer: three granule buffers [2][Bp][H] and one table word per workgroup; the fill
  // segments tile it exactly (two buffers of parity 0, one of parity 1, the table)
  EXPECT(z.hx == ((size_t)3 * 2 * 256 * 256 + 256) * 4);
  for (int B : {256, 128, 37, 16, 1}) {
    const RecPlan r = plan(batch(B)).rec;
    const size_t Bp = (size_t)(B + 31) / 32 * 32;
    EXPECT(r.hx_zero == (int)(2 * 2 * Bp * 256) && r.hx_tagged == (int)(2 * Bp * 256) && r.hx_table == r.grid);
    EXPECT(r.hx_bytes() == (3 * 2 * Bp * 256 + (size_t)r.grid) * 4);
    EXPECT(encode_sizes(plan(batch(B))).hx == r.hx_bytes());
  }
  // outside the image path: the f32 features; casr_encode: neither features nor statistics
  in.T = 3075;
  in.Tp = 1025;
  z = encode_sizes(plan(in));
  EXPECT(z.feat == (size_t)256 * 1025 * 720 * 4 && z.fstat == (size_t)256 * 2 * 720 * 4);
  EXPECT(encode_sizes(plan(fbank(800, false))).feat == rows * 720 * 4);
  z = encode_sizes(plan(batch(256)));
  EXPECT(z.feat == 0 && z.fstat == 0 && z.x16 == rows * 768 * 4);
  // f32: no image; per-step: no hand-off buffer
  In f = batch(37);
  f.s16 = false;
  f.persistent = false;
  z = encode_sizes(plan(f));
  EXPECT(z.x16 == 0 && z.hx == 0 && z.gin == (size_t)37 * 266 * 2048 * 4 && z.keysT == (size_t)2 * 37 * 128 * 268 * 4);
}

static std::vector<uint64_t> key_of(const EncodePlan& p, int l, int r0, int r1, const void* const* bufs) {
  const int32_t sc[3] = {l, r0, r1};
  return plan_graph_key(1, &p, sizeof p, sc, 3, bufs, 2);
}
static void check_key() {
  static_assert(sizeof(EncodePlan) % sizeof(int32_t) == 0, "EncodePlan: int32 fields only");
  static_assert(sizeof(EncodePlan) == sizeof(int32_t) * 9 + sizeof(RecPlan) + 2 * sizeof(InputGemmPlan) + sizeof(KeysPlan),
                "no padding");
  int a, b, c;
  const void* bufs[2] = {&a, &b};
  const void* bufs2[2] = {&a, &c};
  const EncodePlan p = plan(batch(256));
  const std::vector<uint64_t> base = key_of(p, 1, 0, 128, bufs);
  EXPECT(base.size() == 1 + sizeof(EncodePlan) / 4 + 3 + 2);
  EXPECT(base == key_of(plan(batch(256)), 1, 0, 128, bufs));
  // every option that changes a launch changes the plan's bytes, and so the key
  const int changed[][2] = {{CASR_OPT_REC_LAYOUT, 3},  {CASR_OPT_REC_STORE_PLAIN, 0}, {CASR_OPT_REC_SLEEP, 3},
                            {CASR_OPT_REC_POLL_GAP, 4}, {CASR_OPT_REC_COOP, 1},       {CASR_OPT_REC_COOP_REFUSE, 2},
                            {CASR_OPT_GEMM16_PERSIST, 1}, {CASR_OPT_GEMM16_PERSIST, 0}, {CASR_OPT_GEMM16_TAIL, 1},
                            {CASR_OPT_GEMM16_TAIL, 0},  {CASR_OPT_KEYS_ROWS, 0},      {CASR_OPT_X16_KM, 0},
                            {CASR_OPT_GEMM16_LEAN, 1}};
  for (const auto& o : changed) {
    const EncodePlan q = plan(batch(256).opt(o[0], o[1]));
    EXPECT(std::memcmp(&p, &q, sizeof p) != 0);
    EXPECT(key_of(q, 1, 0, 128, bufs) != base);
  }
  // ... and so do the arithmetic, the persistent switch, the shape and the feature path
  In v = batch(256);
  v.s16 = false;
  EXPECT(key_of(plan(v), 1, 0, 128, bufs) != base);
  v = batch(256);
  v.persistent = false;
  EXPECT(key_of(plan(v), 1, 0, 128, bufs) != base);
  EXPECT(key_of(plan(batch(255)), 1, 0, 128, bufs) != base && key_of(plan(batch(256, 265)), 1, 0, 128, bufs) != base);
  // the layer, the row range, the buffers and the kind
  EXPECT(key_of(p, 2, 0, 128, bufs) != base && key_of(p, 1, 128, 256, bufs) != base && key_of(p, 1, 0, 127, bufs) != base);
  EXPECT(key_of(p, 1, 0, 128, bufs2) != base);
  const int32_t sc[3] = {1, 0, 128};
  EXPECT(plan_graph_key(2, &p, sizeof p, sc, 3, bufs, 2) != base);
  // options the encode never reads leave the plan alone
  EXPECT(key_of(plan(batch(256).opt(CASR_OPT_ATTN_KPB, 8).opt(CASR_OPT_DEC_FOLD, 0)), 1, 0, 128, bufs) == base);
}

int main() {
  check_recurrence();
  check_input_gemm();
  check_km();
  check_features();
  check_keys();
  check_workspaces();
  check_key();
  std::printf("encode_plan_check ok\n");
  return 0;
}
