// The edit script of long pairs (include/casr.h casr_edit_align*): the tile shape, the launches of a
// call and their grids, the workspace, the tile-major layout of the direction bits with its index
// functions, the hand-off index math and the backtrace that fills the two maps, once, as plain C++
// that the kernels (edit_align.hip), the host entry points and the sanitizer program
// (tests/host_asan/edit_align_check.cpp) all compile.  The cell rule, the rule a cell's backtrace
// takes and the 2-bit code are edit_plan.h's (edit_cell, edit_dir, EDIT_*); nothing restates them.
//
// Tiles.  The table of a pair is cut into tiles of EA_TC = 64 columns (one per lane of a wave) by
// EA_TR rows; tile (ti, tj) holds the cells (i, j), 0-based, with ti EA_TR <= i < (ti + 1) EA_TR and
// tj 64 <= j < (tj + 1) 64.  A tile needs the column left of it, the row above it and the corner
// between them:
//   colc [La + 1]           colc[r] = D[r][j0] for the rows r = i0 + 1 .. i0 + rows of the tile about
//                           to run at column j0; the tile overwrites them with its own last column
//                           D[r][j0 + cols].  Tiles of one launch have different ti: disjoint rows.
//   rowc [tiles_c][65]      slot tj: entry 0 = D[i0][j0], entries 1 + c = D[i0][j0 + 1 + c]: the bottom
//                           row of tile (ti - 1, tj) WITH the corner at its left, which that tile knows
//                           (the last entry of the column it was handed).  The corner cannot be read
//                           from colc or from a plain row: both have been overwritten by the time
//                           (ti, tj) runs.  Tiles of one launch have different tj: disjoint slots.
// Launch d runs the tiles with ti + tj = d: what a tile reads was written one launch earlier.
//
// Bits.  Two bits per cell, 16 rows to a 32-bit word as in edit_plan.h, but TILE-MAJOR: the words of a
// tile are contiguous (EA_TILE_WORDS = 64 EA_TR / 16), row group major and lane minor, and tile
// (ti, tj) starts at (ti tiles_c + tj) EA_TILE_WORDS.  A wave collects a tile's words in LDS and
// stores them as 16-byte vectors, lane after lane: whole cache lines, no scattered word stores.
#pragma once
#include <stdint.h>

#include <vector>

#include "casr.h"
#include "edit_plan.h"

namespace casr {

constexpr int EA_MAX_LEN = CASR_EDIT_ALIGN_MAX_LEN;  // longest row of the device entry
constexpr int EA_TC = EDIT_WAVE;                     // columns of a tile
constexpr int EA_TR = 128;                           // rows of a tile
constexpr int EA_TILE_WORDS = EA_TC * (EA_TR / 16);  // 512 words = 2 KB
constexpr int EA_ROW_SLOT = EA_TC + 1;               // corner + 64 values
constexpr size_t EA_BITS_LIMIT = (size_t)1 << 30;    // direction bits of one call
constexpr int EA_BT_THREADS = 64;                    // the backtrace: one wave per pair

static_assert(EA_TR % 16 == 0 && EA_TILE_WORDS % (4 * EA_TC) == 0, "a tile's words leave as whole uint4 rows");

// ---------------------------------------------------------------- tiles and the bit layout
CASR_EDIT_HD inline int ea_tiles_r(int m) { return (m + EA_TR - 1) / EA_TR; }
CASR_EDIT_HD inline int ea_tiles_c(int n) { return (n + EA_TC - 1) / EA_TC; }
CASR_EDIT_HD inline int ea_tile_rows(int m, int ti) { return m - ti * EA_TR < EA_TR ? m - ti * EA_TR : EA_TR; }
CASR_EDIT_HD inline int ea_tile_cols(int n, int tj) { return n - tj * EA_TC < EA_TC ? n - tj * EA_TC : EA_TC; }
// words of a table of m x n cells (tiles are stored whole)
CASR_EDIT_HD inline size_t ea_bits_words(int m, int n) {
  return (size_t)ea_tiles_r(m) * ea_tiles_c(n) * EA_TILE_WORDS;
}
CASR_EDIT_HD inline size_t ea_tile_base(int ti, int tj, int tiles_c) {
  return ((size_t)ti * tiles_c + tj) * EA_TILE_WORDS;
}
// inside a tile: row il, column c
CASR_EDIT_HD inline int ea_tile_word(int il, int c) { return (il >> 4) * EA_TC + c; }
CASR_EDIT_HD inline int ea_tile_shift(int il) { return edit_bits_shift(il); }

// ---------------------------------------------------------------- the hand-offs
CASR_EDIT_HD inline size_t ea_colc_words(int La) { return (size_t)La + 1; }
CASR_EDIT_HD inline size_t ea_rowc_words(int Lb) { return (size_t)ea_tiles_c(Lb) * EA_ROW_SLOT; }
CASR_EDIT_HD inline size_t ea_rowc_index(int tj, int e) { return (size_t)tj * EA_ROW_SLOT + e; }
// D[i0][j0] of tile (ti, tj): on the table's edges a formula, else what the tile above left
CASR_EDIT_HD inline int ea_corner(int ti, int tj, const int32_t* rowc) {
  return tj == 0 ? ti * EA_TR : ti == 0 ? tj * EA_TC : rowc[ea_rowc_index(tj, 0)];
}
// D[i0][j0 + 1 + c]
CASR_EDIT_HD inline int ea_top(int ti, int tj, int c, const int32_t* rowc) {
  return ti == 0 ? tj * EA_TC + c + 1 : rowc[ea_rowc_index(tj, 1 + c)];
}
// D[i0 + 1 + il][j0]
CASR_EDIT_HD inline int ea_left(int ti, int tj, int il, const int32_t* colc) {
  return tj == 0 ? ti * EA_TR + il + 1 : colc[ti * EA_TR + 1 + il];
}

// a length as the kernels take it: clamped into [0, L]; true when it was outside
CASR_EDIT_HD inline bool ea_clamp(int& len, int L) {
  if (len >= 0 && len <= L) return false;
  len = len < 0 ? 0 : L;
  return true;
}

// ---------------------------------------------------------------- the backtrace
struct EaWalk {
  int i, j;           // the cell the walk stands on, as (i, j) of D
  int ins, del, rep;  // so far
};

// The part of the backtrace that lies in tile (ti, tj), whose words start at `tile`: edit_backtrace's
// rules, and at a diagonal step through cell (i, j) b_of_a[i] = j and a_of_b[j] = i (either may be null).
// Returns with the walk on the tile's upper or left edge.
CASR_EDIT_HD inline void ea_walk_tile(const uint32_t* tile, int ti, int tj, EaWalk& w, int32_t* b_of_a,
                                      int32_t* a_of_b) {
  const int i0 = ti * EA_TR, j0 = tj * EA_TC;
  while (w.i > i0 && w.j > j0) {
    const int il = w.i - 1 - i0, c = w.j - 1 - j0;
    const int dir = (tile[ea_tile_word(il, c)] >> ea_tile_shift(il)) & 3;
    if (dir == EDIT_DIAG || dir == EDIT_REPLACE) {
      w.rep += dir == EDIT_REPLACE;
      --w.i;
      --w.j;
      if (b_of_a) b_of_a[w.i] = w.j;
      if (a_of_b) a_of_b[w.j] = w.i;
    } else if (dir == EDIT_DELETE) {
      ++w.del;
      --w.i;
    } else {
      ++w.ins;
      --w.j;
    }
  }
}

// the tile the walk enters next (w.i, w.j > 0)
CASR_EDIT_HD inline int ea_walk_ti(const EaWalk& w) { return (w.i - 1) / EA_TR; }
CASR_EDIT_HD inline int ea_walk_tj(const EaWalk& w) { return (w.j - 1) / EA_TC; }

// the first row or column: only deletes or only inserts are left
CASR_EDIT_HD inline void ea_walk_finish(EaWalk& w, int32_t* ops) {
  w.del += w.i;
  w.ins += w.j;
  w.i = w.j = 0;
  if (ops) {
    ops[0] = w.ins;
    ops[1] = w.del;
    ops[2] = w.rep;
  }
}

// the whole backtrace over bits of tiles_c tile columns; the maps must hold -1 already
inline void ea_backtrace(const uint32_t* bits, int tiles_c, int m, int n, int32_t* ops, int32_t* b_of_a,
                         int32_t* a_of_b) {
  EaWalk w{m, n, 0, 0, 0};
  while (w.i > 0 && w.j > 0) {
    const int ti = ea_walk_ti(w), tj = ea_walk_tj(w);
    ea_walk_tile(bits + ea_tile_base(ti, tj, tiles_c), ti, tj, w, b_of_a, a_of_b);
  }
  ea_walk_finish(w, ops);
}

// ---------------------------------------------------------------- one pair on the host
// The rolling-row form: a row of D rolls over i, the bits go to their tile-major words.  Reads
// a[0 .. m) and b[0 .. n) and nothing past them; b_of_a [m] and a_of_b [n] (or null) are written whole.
inline int32_t ea_pair_rows(const int32_t* a, int m, const int32_t* b, int n, int32_t* ops, int32_t* b_of_a,
                            int32_t* a_of_b) {
  std::vector<int32_t> row((size_t)n + 1);
  for (int j = 0; j <= n; ++j) row[j] = j;
  const bool want = ops || b_of_a || a_of_b;
  const int tiles_c = ea_tiles_c(n);
  std::vector<uint32_t> bits;
  if (want) bits.assign(ea_bits_words(m, n), 0u);
  for (int i = 0; i < m; ++i) {
    int diag = row[0], left = i + 1;
    row[0] = left;
    const int32_t ai = a[i];
    const int ti = i / EA_TR, il = i - ti * EA_TR;
    for (int j = 0; j < n; ++j) {
      const int up = row[j + 1];
      const bool match = ai == b[j];
      const int d = edit_cell(match, diag, up, left);
      if (want) {
        const int tj = j / EA_TC;
        bits[ea_tile_base(ti, tj, tiles_c) + ea_tile_word(il, j - tj * EA_TC)] |=
            (uint32_t)edit_dir(match, d, diag, up) << ea_tile_shift(il);
      }
      row[j + 1] = d;
      diag = up;
      left = d;
    }
  }
  if (b_of_a) for (int i = 0; i < m; ++i) b_of_a[i] = -1;
  if (a_of_b) for (int j = 0; j < n; ++j) a_of_b[j] = -1;
  if (want) ea_backtrace(bits.data(), tiles_c, m, n, ops, b_of_a, a_of_b);
  return row[n];
}

// One tile in the order the device takes it, on the hand-off arrays of the pair: reads its left column,
// top row and corner through the index math above, fills its cells, leaves its last column in colc and
// its bottom row with the next corner in rowc.  Returns D at the tile's last cell.
inline int32_t ea_tile_host(const int32_t* a, int m, const int32_t* b, int n, int ti, int tj, int32_t* colc,
                            int32_t* rowc, uint32_t* tile) {
  const int i0 = ti * EA_TR, j0 = tj * EA_TC, rows = ea_tile_rows(m, ti), cols = ea_tile_cols(n, tj);
  int32_t row[EA_TC + 1];  // D[i0 + il][j0 .. j0 + cols]
  row[0] = ea_corner(ti, tj, rowc);
  for (int c = 0; c < cols; ++c) row[1 + c] = ea_top(ti, tj, c, rowc);
  const int32_t next_corner = ea_left(ti, tj, rows - 1, colc);
  for (int il = 0; il < rows; ++il) {
    int diag = row[0], left = ea_left(ti, tj, il, colc);
    row[0] = left;
    const int32_t ai = a[i0 + il];
    for (int c = 0; c < cols; ++c) {
      const int up = row[c + 1];
      const bool match = ai == b[j0 + c];
      const int d = edit_cell(match, diag, up, left);
      if (tile) tile[ea_tile_word(il, c)] |= (uint32_t)edit_dir(match, d, diag, up) << ea_tile_shift(il);
      row[c + 1] = d;
      diag = up;
      left = d;
    }
    colc[i0 + 1 + il] = row[cols];
  }
  rowc[ea_rowc_index(tj, 0)] = next_corner;
  for (int c = 0; c < cols; ++c) rowc[ea_rowc_index(tj, 1 + c)] = row[1 + c];
  return row[cols];
}

// ---------------------------------------------------------------- the plan
struct EaPlan {
  bool ok;             // the device entry takes the call
  int tiles_r, tiles_c;
  int launches;        // sweep launches: tiles_r + tiles_c - 1, one anti-diagonal of tiles each
  size_t bits_bytes;   // n pairs' direction bits
  size_t colc_bytes, rowc_bytes;
  size_t bytes;        // the workspace: bits, colc, rowc, each rounded up to 256 bytes
};

CASR_EDIT_HD inline int ea_diag_lo(int d, int tiles_c) { return d - (tiles_c - 1) > 0 ? d - (tiles_c - 1) : 0; }
// tiles of launch d per pair: ti from ea_diag_lo(d) up, tj = d - ti
CASR_EDIT_HD inline int ea_diag_tiles(int d, int tiles_r, int tiles_c) {
  const int hi = d < tiles_r - 1 ? d : tiles_r - 1;
  return hi - ea_diag_lo(d, tiles_c) + 1;
}
inline size_t ea_round256(size_t x) { return (x + 255) & ~(size_t)255; }

// bits = false: neither ops nor a map is asked for, no bits are kept
inline EaPlan edit_align_plan(int La, int Lb, int n, bool bits) {
  EaPlan p{false, 0, 0, 0, 0, 0, 0, 0};
  if (La < 1 || Lb < 1 || La > EA_MAX_LEN || Lb > EA_MAX_LEN || n < 0) return p;
  p.tiles_r = ea_tiles_r(La);
  p.tiles_c = ea_tiles_c(Lb);
  p.launches = p.tiles_r + p.tiles_c - 1;
  // (n < 2^31 and at most 2^17 tiles of 2^11 bytes: below 2^59)
  p.bits_bytes = bits ? (size_t)n * ea_bits_words(La, Lb) * sizeof(uint32_t) : 0;
  p.colc_bytes = (size_t)n * ea_colc_words(La) * sizeof(int32_t);
  p.rowc_bytes = (size_t)n * ea_rowc_words(Lb) * sizeof(int32_t);
  p.bytes = ea_round256(p.bits_bytes) + ea_round256(p.colc_bytes) + ea_round256(p.rowc_bytes);
  // every pair keeps a whole tile at least, so n is below 2^19 here and a launch's grid fits an int
  p.ok = (size_t)n * ea_bits_words(La, Lb) * sizeof(uint32_t) <= EA_BITS_LIMIT;
  return p;
}

// One pair in the order of the device: launch after launch, every tile of a launch on the state the
// launch before left.  Gives what ea_pair_rows gives; the tests hold the two against each other.
inline int32_t ea_pair_tiles(const int32_t* a, int m, const int32_t* b, int n, int32_t* ops, int32_t* b_of_a,
                             int32_t* a_of_b) {
  if (b_of_a) for (int i = 0; i < m; ++i) b_of_a[i] = -1;
  if (a_of_b) for (int j = 0; j < n; ++j) a_of_b[j] = -1;
  int32_t dist = m > n ? m : n;  // an empty row
  const int tiles_r = ea_tiles_r(m), tiles_c = ea_tiles_c(n);
  std::vector<uint32_t> bits(ea_bits_words(m, n), 0u);
  if (m > 0 && n > 0) {
    std::vector<int32_t> colc(ea_colc_words(m), 0), rowc(ea_rowc_words(n), 0);
    for (int d = 0; d < tiles_r + tiles_c - 1; ++d) {
      const int lo = ea_diag_lo(d, tiles_c), cnt = ea_diag_tiles(d, tiles_r, tiles_c);
      for (int x = cnt - 1; x >= 0; --x) {  // (any order within a launch)
        const int ti = lo + x, tj = d - ti;
        const int32_t v = ea_tile_host(a, m, b, n, ti, tj, colc.data(), rowc.data(),
                                       bits.data() + ea_tile_base(ti, tj, tiles_c));
        if (ti == tiles_r - 1 && tj == tiles_c - 1) dist = v;
      }
    }
  }
  ea_backtrace(bits.data(), tiles_c, m, n, ops, b_of_a, a_of_b);
  return dist;
}

}  // namespace casr
