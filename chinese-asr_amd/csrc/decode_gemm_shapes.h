// The block shapes of the decode GEMM (decoder.hip dgemm_kernel), shared with the host-only decode
// plan (decode_plan.h): one row per instantiated shape, and the arithmetic that follows from a row
// (rows and columns per block, tiles per wave column, k slices, the ring's LDS).  The kernel's own
// constants and static_asserts call the same functions, so the kernel and the plan cannot disagree.
// Plain constexpr C++ (hipcc treats constexpr functions as host and device functions).
#pragma once
#include <stdint.h>

#include "attention_lds.h"  // LDS_LIMIT_BYTES

namespace casr {

// one id per shape: the three-launch step's LSTMCell and projection, then the folded step's GEMM
// (names: rows x columns of a block)
enum {
  DG_LSTM_32x64 = 0,     // R <= 256
  DG_LSTM_64x64,         // R <= 512
  DG_LSTM_128x64,        // 512 < R < 2048
  DG_LSTM_128x128,       // R >= 2048
  DG_PROJ_32x80,         // R <= 32
  DG_PROJ_64x80,         // R <= 256
  DG_PROJ_128x80,        // R <= 512
  DG_PROJ_128x160,       // R > 512; f32, or some |W_p| >= 16
  DG_PROJ_128x160_ONE,   // 512 < R < 2048, s16 and every |W_p| < 16
  DG_PROJ_256x160_ONE,   // R >= 2048, s16 and every |W_p| < 16
  DG_FOLD_32x112_KS,     // greedy, R <= 32, the k split
  DG_FOLD_32x112,        // greedy, R <= 32
  DG_FOLD_64x112,        // greedy, R > 32
  DG_FOLD_256x224_ONE,   // beam, R >= 2048
  DG_FOLD_128x224_ONE,   // beam, R < 2048
  DG_SHAPE_COUNT
};

// dgemm_kernel's template arguments (its comment in decoder.hip says what each does).  IL, BKW = 32
// and ONE take effect under s16 only: the f32 kernel of a shape is <WR, NT, S, ..., RS, WC> alone.
struct DgShape {
  const char* name;
  int WR, NT, S, RS, WC, IL, BKW, ONE, SA, KS;
};
constexpr int DG_KS = 4;  // the greedy folded GEMM's k split: blocks per output block
constexpr DgShape DG_SHAPES[] = {
    //                       WR  NT  S RS WC IL BKW ONE SA KS
    {"lstm 32x64",            2,  4, 4, 1, 1, 0, 64, 0, 4, 1},
    {"lstm 64x64",            4,  4, 4, 1, 1, 0, 64, 0, 4, 1},
    {"lstm 128x64",           8,  4, 3, 1, 1, 1, 64, 0, 3, 1},
    {"lstm 128x128",          8,  8, 2, 1, 1, 1, 64, 0, 2, 1},
    {"proj 32x80",            2,  5, 4, 1, 1, 0, 64, 0, 4, 1},
    {"proj 64x80",            4,  5, 4, 1, 1, 0, 64, 0, 4, 1},
    {"proj 128x80",           8,  5, 3, 1, 1, 0, 64, 0, 3, 1},
    {"proj 128x160",          4, 10, 2, 2, 2, 1, 64, 0, 2, 1},
    {"proj 128x160 one",      4, 10, 2, 2, 2, 1, 64, 1, 2, 1},
    {"proj 256x160 one",      4, 10, 3, 4, 2, 1, 32, 1, 3, 1},
    {"fold 32x112 k split",   2,  7, 3, 1, 1, 0, 64, 0, 3, DG_KS},
    {"fold 32x112",           2,  7, 3, 1, 1, 0, 64, 0, 3, 1},
    {"fold 64x112",           4,  7, 3, 1, 1, 0, 64, 0, 3, 1},
    {"fold 256x224 one",      4, 14, 2, 4, 2, 1, 32, 1, 3, 1},
    {"fold 128x224 one",      4, 14, 3, 2, 2, 1, 32, 1, 3, 1},
};
static_assert(sizeof(DG_SHAPES) / sizeof(DG_SHAPES[0]) == DG_SHAPE_COUNT, "one DG_SHAPES row per shape id");

constexpr int DG_FRAG = 16 * 64;  // floats of one W fragment block: 16 rows x 64 k

constexpr int dg_block_rows(const DgShape& s) { return 16 * s.WR * s.RS; }
constexpr int dg_block_cols(const DgShape& s) { return 16 * s.NT; }
constexpr int dg_wave_tiles(const DgShape& s) { return s.NT / s.WC; }  // 16-column tiles per wave column
constexpr int dg_k_slices(const DgShape& s) { return 8 / (s.WR * s.WC); }
// floats of one ring stage: the A tile (block rows x BKW k) and the W tile (NT fragment blocks, half
// of each in a 32-deep stage)
constexpr int dg_a_tile(const DgShape& s) { return dg_block_rows(s) * s.BKW; }
constexpr int dg_w_tile(const DgShape& s) { return s.NT * (DG_FRAG * s.BKW / 64); }
// the ring: S stages of [A | W], and SA - S more A tiles where the A ring is the deeper one
constexpr int dg_ring_bytes(const DgShape& s) {
  return (s.S * (dg_a_tile(s) + dg_w_tile(s)) + (s.SA - s.S) * dg_a_tile(s)) * 4;
}
// 32-deep stages and the one-accumulator form exist for the s16 images only
constexpr bool dg_s16_only(const DgShape& s) { return s.BKW == 32 || s.ONE; }
// the 8 waves of a block are row groups x column groups x k slices, and the ring fits the LDS
constexpr bool dg_shape_ok(const DgShape& s) {
  return s.WR * s.WC * dg_k_slices(s) == 8 && s.NT % s.WC == 0 && dg_k_slices(s) <= 4 &&
         (s.BKW == 64 || s.BKW == 32) && s.SA >= s.S && (size_t)dg_ring_bytes(s) <= LDS_LIMIT_BYTES;
}
constexpr bool dg_shapes_ok(int first, int last, int wave_tiles) {
  for (int i = first; i <= last; ++i)
    if (!dg_shape_ok(DG_SHAPES[i]) || (wave_tiles && dg_wave_tiles(DG_SHAPES[i]) != wave_tiles)) return false;
  return true;
}

// grid of NB column blocks x NR row blocks dealt over the 8 XCDs (decoder.hip xcd_tile): column
// blocks padded to a multiple of 8, so all row blocks of one column block share an XCD
constexpr int xcd_grid(int NB, int NR) { return 8 * ((NB + 7) / 8) * NR; }

// One launch of dgemm_kernel: the shape and the arguments that follow from it.  int32 fields only
// (part of DecodePlan, whose bytes are the graph key).
struct DgemmPlan {
  int32_t shape;   // DG_*
  int32_t NB, NR;  // column blocks, row blocks
  int32_t grid;    // xcd_grid(NB, NR) x the shape's KS
  int32_t ntiles;  // 16-row W fragment blocks that exist
  int32_t nkt;     // ring stages per block column: 64-deep k tiles, twice as many 32-deep ones
};
// cover: the column tiles the blocks must cover (ntiles, or the folded GEMM's vocabulary tiles at the
// last step); K: the contraction length
constexpr DgemmPlan plan_dgemm(int shape, int R, int ntiles, int cover, int K) {
  const DgShape& s = DG_SHAPES[shape];
  const int NB = (cover + s.NT - 1) / s.NT, NR = (R + dg_block_rows(s) - 1) / dg_block_rows(s);
  return DgemmPlan{shape, NB, NR, xcd_grid(NB, NR) * s.KS, ntiles, K / s.BKW};
}

}  // namespace casr
