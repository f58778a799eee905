// The edit script of long pairs on the device (include/casr.h casr_edit_align): distance, operation
// counts and the two maps of rows of up to CASR_EDIT_ALIGN_MAX_LEN symbols.  The cell rule and the
// direction code are edit_plan.h's; the tiles, the hand-offs, the bit layout, the backtrace and the
// plan are edit_align_plan.h's, the text the host compiles too.
//
// Three kinds of launch, all ordinary and in stream order; no workgroup waits for another:
//   fill       the maps to -1, dist of pairs with an empty row, the guard bit of a clamped length
//   sweep      one launch per anti-diagonal of tiles, one wave per tile, the pairs side by side
//   backtrace  one wave per pair over the bits the sweeps left
// Every workgroup of the sweep and the backtrace is ONE wave: its barriers order that wave's LDS traffic.
#include "casr_internal.h"
#include "edit_align_plan.h"

namespace casr {

struct EaArgs {
  const int32_t* a;
  const int32_t* a_len;
  const int32_t* b;
  const int32_t* b_len;
  int La, Lb, n;
  int tiles_r, tiles_c;  // of La x Lb: the layout of every pair's bits
  int32_t* dist;
  int32_t* ops;     // or null
  int32_t* b_of_a;  // or null
  int32_t* a_of_b;  // or null
  uint32_t* bits;   // [n][tiles_r][tiles_c][EA_TILE_WORDS], or null: no bits are kept
  int32_t* colc;    // [n][La + 1]
  int32_t* rowc;    // [n][tiles_c][65]
  int32_t* err;
};

// ------------------------------------------------------------------ fill
__global__ __launch_bounds__(256) void ea_fill_kernel(EaArgs p) {
  const size_t step = (size_t)gridDim.x * blockDim.x, at = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p.b_of_a)
    for (size_t i = at; i < (size_t)p.n * p.La; i += step) p.b_of_a[i] = -1;
  if (p.a_of_b)
    for (size_t i = at; i < (size_t)p.n * p.Lb; i += step) p.a_of_b[i] = -1;
  for (size_t i = at; i < (size_t)p.n; i += step) {
    int m = p.a_len[i], n = p.b_len[i];
    const bool bad = ea_clamp(m, p.La) | ea_clamp(n, p.Lb);
    if (m == 0 || n == 0) p.dist[i] = m > n ? m : n;
    if (bad) atomicOr(p.err, CASR_DEV_BAD_TOKEN);
  }
}

// ------------------------------------------------------------------ sweep
// Tile (ti, tj) of pair `pair`: lane = column, one anti-diagonal of the tile per step as in edit.hip's
// wave form: at step t lane c fills row il = t - c; up is its own previous value, left its left
// neighbour's value of the step before (one cross-lane move), diag the left it fetched a step ago.
// Lane 0 takes left from the column it was handed.  Everything a step reads from memory sits in LDS,
// fetched a step ahead, so the chain from one step to the next is registers and the cross-lane move:
//   sa    [63 + EA_TR + 64]  a[i0 + il] at 63 + il; the pads are read by lanes outside the tile, unused
//   sleft [EA_TR + 64]       D[i0 + 1 + il][j0] at il
//   sright[EA_TR]            the tile's last column, then stored to colc in one piece
//   sbits [EA_TILE_WORDS]    a lane's finished words, then stored to the workspace as uint4 rows
template <bool BITS>
__global__ __launch_bounds__(EA_TC) void ea_sweep_kernel(EaArgs p, int d, int lo, int cnt) {
  __shared__ int32_t sa[63 + EA_TR + 64];
  __shared__ int32_t sleft[EA_TR + 64];
  __shared__ int32_t sright[EA_TR];
  __shared__ __attribute__((aligned(16))) uint32_t sbits[BITS ? EA_TILE_WORDS : 4];
  const int ln = threadIdx.x;
  const size_t pair = blockIdx.x / cnt;
  const int ti = lo + (int)(blockIdx.x - pair * cnt), tj = d - ti;
  int m = p.a_len[pair], n = p.b_len[pair];
  ea_clamp(m, p.La);
  ea_clamp(n, p.Lb);
  if (m == 0 || n == 0 || ti >= ea_tiles_r(m) || tj >= ea_tiles_c(n)) return;  // (uniform)
  const int i0 = ti * EA_TR, j0 = tj * EA_TC, rows = ea_tile_rows(m, ti), cols = ea_tile_cols(n, tj);
  const int32_t* a = p.a + pair * p.La + i0;
  int32_t* colc = p.colc + pair * ea_colc_words(p.La);
  int32_t* rowc = p.rowc + pair * ea_rowc_words(p.Lb);
  const bool on = ln < cols;

  for (int x = ln; x < 63 + EA_TR + 64; x += EA_TC) {
    const int il = x - 63;
    sa[x] = il >= 0 && il < rows ? a[il] : 0;
  }
  for (int x = ln; x < EA_TR + 64; x += EA_TC) sleft[x] = x < rows ? ea_left(ti, tj, x, colc) : 0;
  if (BITS)
    for (int x = ln; x < EA_TILE_WORDS; x += EA_TC) sbits[x] = 0u;
  const int32_t bj = on ? p.b[pair * p.Lb + j0 + ln] : 0;
  int v = on ? ea_top(ti, tj, ln, rowc) : 0;        // D[i0][j0 + ln + 1]
  int diag = ln == 0 ? ea_corner(ti, tj, rowc) : 0;  // lane 0's first diagonal; the others get theirs below
  __syncthreads();
  const int next_corner = sleft[rows - 1];  // D[i0 + rows][j0]: the corner of the tile below

  uint32_t acc = 0;
  const int T = rows + cols - 1;
  int32_t ai = sa[63 - ln], lf = sleft[0];
  for (int t = 0; t < T; ++t) {
    const int il = t - ln;
    const int32_t ai_next = sa[64 + il], lf_next = sleft[t + 1];
    const bool act = on && il >= 0 && il < rows;
    int left = __shfl_up(v, 1);
    if (ln == 0) left = lf;
    if (act) {
      const bool match = ai == bj;
      const int dd = edit_cell(match, diag, v, left);
      if (BITS) {
        acc |= (uint32_t)edit_dir(match, dd, diag, v) << ea_tile_shift(il);
        if ((il & 15) == 15 || il == rows - 1) {
          sbits[ea_tile_word(il, ln)] = acc;
          acc = 0;
        }
      }
      v = dd;
      if (ln == cols - 1) sright[il] = dd;
    }
    diag = left;
    ai = ai_next;
    lf = lf_next;
  }
  __syncthreads();

  if (BITS) {
    uint4* out = reinterpret_cast<uint4*>(p.bits + pair * ((size_t)p.tiles_r * p.tiles_c * EA_TILE_WORDS) +
                                          ea_tile_base(ti, tj, p.tiles_c));
    const uint4* in = reinterpret_cast<const uint4*>(sbits);
    for (int x = ln; x < EA_TILE_WORDS / 4; x += EA_TC) out[x] = in[x];
  }
  for (int x = ln; x < rows; x += EA_TC) colc[i0 + 1 + x] = sright[x];
  if (on) rowc[ea_rowc_index(tj, 1 + ln)] = v;
  if (ln == 0) rowc[ea_rowc_index(tj, 0)] = next_corner;
  if (ti == ea_tiles_r(m) - 1 && tj == ea_tiles_c(n) - 1 && ln == cols - 1) p.dist[pair] = v;
}

// ------------------------------------------------------------------ backtrace
// One wave per pair.  The walk takes m + n dependent steps at most; each tile it enters is staged in
// LDS first (a coalesced 2 KB read), so a step costs an LDS read, not a trip to memory.  Lane 0 walks.
__global__ __launch_bounds__(EA_BT_THREADS) void ea_backtrace_kernel(EaArgs p) {
  __shared__ __attribute__((aligned(16))) uint32_t stile[EA_TILE_WORDS];
  const size_t pair = blockIdx.x;
  const int ln = threadIdx.x;
  int m = p.a_len[pair], n = p.b_len[pair];
  ea_clamp(m, p.La);
  ea_clamp(n, p.Lb);
  const uint32_t* bits = p.bits + pair * ((size_t)p.tiles_r * p.tiles_c * EA_TILE_WORDS);
  int32_t* b_of_a = p.b_of_a ? p.b_of_a + pair * p.La : nullptr;
  int32_t* a_of_b = p.a_of_b ? p.a_of_b + pair * p.Lb : nullptr;
  EaWalk w{m, n, 0, 0, 0};
  while (w.i > 0 && w.j > 0) {  // (uniform: every lane follows lane 0's position)
    const int ti = ea_walk_ti(w), tj = ea_walk_tj(w);
    const uint4* in = reinterpret_cast<const uint4*>(bits + ea_tile_base(ti, tj, p.tiles_c));
    uint4* st = reinterpret_cast<uint4*>(stile);
    for (int x = ln; x < EA_TILE_WORDS / 4; x += EA_BT_THREADS) st[x] = in[x];
    __syncthreads();
    if (ln == 0) ea_walk_tile(stile, ti, tj, w, b_of_a, a_of_b);
    w.i = __shfl(w.i, 0);
    w.j = __shfl(w.j, 0);
    __syncthreads();
  }
  if (ln == 0) ea_walk_finish(w, p.ops ? p.ops + pair * 3 : nullptr);
}

// ------------------------------------------------------------------ the call
hipError_t run_edit_align(const int32_t* a, const int32_t* a_len, int La, const int32_t* b, const int32_t* b_len,
                          int Lb, int n, int32_t* dist, int32_t* ops, int32_t* b_of_a, int32_t* a_of_b, void* ws,
                          int32_t* err, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const bool want = ops || b_of_a || a_of_b;
  const EaPlan pl = edit_align_plan(La, Lb, n, want);
  if (!pl.ok) return hipErrorInvalidValue;
  char* base = static_cast<char*>(ws);
  EaArgs p{a, a_len, b, b_len, La, Lb, n, pl.tiles_r, pl.tiles_c, dist, ops, b_of_a, a_of_b,
           want ? reinterpret_cast<uint32_t*>(base) : nullptr,
           reinterpret_cast<int32_t*>(base + ea_round256(pl.bits_bytes)),
           reinterpret_cast<int32_t*>(base + ea_round256(pl.bits_bytes) + ea_round256(pl.colc_bytes)), err};
  const size_t cells = (size_t)n * (La > Lb ? La : Lb);
  const unsigned fill_blocks = (unsigned)std::min<size_t>((cells + 255) / 256, 2048);
  hipLaunchKernelGGL(ea_fill_kernel, dim3(fill_blocks), dim3(256), 0, s, p);
  for (int d = 0; d < pl.launches; ++d) {
    const int lo = ea_diag_lo(d, pl.tiles_c), cnt = ea_diag_tiles(d, pl.tiles_r, pl.tiles_c);
    const dim3 grid((unsigned)((size_t)cnt * n));
    if (want)
      hipLaunchKernelGGL(ea_sweep_kernel<true>, grid, dim3(EA_TC), 0, s, p, d, lo, cnt);
    else
      hipLaunchKernelGGL(ea_sweep_kernel<false>, grid, dim3(EA_TC), 0, s, p, d, lo, cnt);
  }
  if (want) hipLaunchKernelGGL(ea_backtrace_kernel, dim3(n), dim3(EA_BT_THREADS), 0, s, p);
  return hipGetLastError();
}

}  // namespace casr
