// LDS layout arithmetic of the attention kernel (attention.hip), shared with the host-only decode
// plan (decode_plan.h): the plan's LDS guards and the kernel's carve read the same formulas.
// Plain constexpr C++ (hipcc treats constexpr functions as host and device functions).
#pragma once
#include <stddef.h>

#include "casr_dims.h"

namespace casr {

constexpr int AT_THREADS = 512;
constexpr int AT_MAXG = 8;      // a-groups of the score phase
constexpr int AT_CH = 20;       // keys rows in flight per score batch (apg = 19 at Tp = 266)
constexpr int AT_APAD = A + AT_CH;  // q / v rows in LDS, zero-padded so a batch never branches

// keysT row stride: Tp rounded up to 4 (16 B aligned rows)
constexpr int attn_tq(int Tp) { return (Tp + 3) & ~3; }

template <int KPB, int MAXG = AT_MAXG>
constexpr int attn_scratch_floats(int Tq) {
  // score partials [MAXG][KPB][Tq] | context partials [4][KPB][C]
  return MAXG * KPB * Tq > 4 * KPB * C ? MAXG * KPB * Tq : 4 * KPB * C;
}
// (round 6) the split folded greedy attention (attention_kernel<1, 1, true>): a block takes Tq / S
// steps, so its score phase can use up to 32 a-groups of 4 keys rows (the unsplit form's 8 groups of
// 16 rows would leave most of the block's threads idle on a short range)
constexpr int AT_MAXG_SPLIT = 32;

// the folded step's cell phase (CELL): h [HD] | query slices [AT_QS][A]
constexpr int AT_QS = AT_THREADS / (A / 4);  // 16 unit slices of HD / AT_QS = 32 units
constexpr int AT_CELL_FLOATS = HD + AT_QS * A;
static_assert(AT_QS * A >= 4 * HD, "the token's gate-table row fits the query slice area (CELL 1)");

// LDS: qs, eqs [AT_APAD][KPB] | vs, v2s [A] | (AT_MAXG unused) | scratch | es [Tq][KPB] | (CELL: h,
// query slices) | value rows
// (CELL 2, the beam cell phase, keeps its h rows and query slices in the score scratch instead)
template <int KPB, int CELL = 0, bool TSPLIT = false>
constexpr size_t attn_smem_floats(int Tp) {
  return (size_t)2 * KPB * AT_APAD + 2 * A + AT_MAXG +
         attn_scratch_floats<KPB, TSPLIT ? AT_MAXG_SPLIT : AT_MAXG>(attn_tq(Tp)) + KPB * attn_tq(Tp) +
         (CELL == 1 ? AT_CELL_FLOATS : 0);
}

// what a workgroup may hold on gfx950
constexpr size_t LDS_LIMIT_BYTES = 160 * 1024;

}  // namespace casr
