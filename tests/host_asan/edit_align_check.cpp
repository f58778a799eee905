// csrc/edit_align_plan.h under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU: a program of
// its own (tests/test_edit_align_host_sanitizer.py builds and runs it).  Every row is read into a heap
// buffer of exactly the symbols the case file holds for it, and every map is a heap buffer of exactly
// its row's length, so a read or a write past a length is a heap-buffer-overflow.  Both host forms run:
// the rolling row (casr_edit_align_host's text) and the device's tile order; they must agree.
// Case file: int32 pairs, then per pair int32 m, n, int64 na, a[na], int64 nb, b[nb].
// Output: per pair "P dist ins del rep | b_of_a .. | a_of_b ..".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "edit_align_plan.h"

using namespace casr;

template <class T>
static T* read_exact(FILE* f, size_t n) {
  T* p = static_cast<T*>(std::malloc(n ? n * sizeof(T) : 1));
  if (n && std::fread(p, sizeof(T), n, f) != n) {
    std::fprintf(stderr, "edit_align_check: short case file\n");
    std::exit(2);
  }
  return p;
}

template <class T>
static T read_one(FILE* f) {
  T* p = read_exact<T>(f, 1);
  const T v = *p;
  std::free(p);
  return v;
}

static int32_t* row_of(size_t n) { return static_cast<int32_t*>(std::malloc(n ? n * sizeof(int32_t) : 1)); }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  FILE* o = std::fopen(argv[2], "w");
  if (!f || !o) return 2;
  const int32_t pairs = read_one<int32_t>(f);
  for (int32_t i = 0; i < pairs; ++i) {
    const int32_t m = read_one<int32_t>(f), n = read_one<int32_t>(f);
    const int64_t na = read_one<int64_t>(f);
    int32_t* a = read_exact<int32_t>(f, (size_t)na);
    const int64_t nb = read_one<int64_t>(f);
    int32_t* b = read_exact<int32_t>(f, (size_t)nb);
    int32_t ops[3] = {-1, -1, -1}, ops2[3] = {-1, -1, -1};
    int32_t *ba = row_of(m), *ab = row_of(n), *ba2 = row_of(m), *ab2 = row_of(n);
    const int32_t d = ea_pair_rows(a, m, b, n, ops, ba, ab);
    const int32_t d2 = ea_pair_tiles(a, m, b, n, ops2, ba2, ab2);
    const int32_t d3 = ea_pair_rows(a, m, b, n, nullptr, nullptr, nullptr);
    if (d != d2 || d != d3 || std::memcmp(ops, ops2, sizeof(ops)) || (m && std::memcmp(ba, ba2, m * sizeof(int32_t))) ||
        (n && std::memcmp(ab, ab2, n * sizeof(int32_t)))) {
      std::fprintf(stderr, "edit_align_check: pair %d: the tile order disagrees with the rolling row\n", i);
      return 4;
    }
    std::fprintf(o, "P %d %d %d %d |", d, ops[0], ops[1], ops[2]);
    for (int32_t x = 0; x < m; ++x) std::fprintf(o, " %d", ba[x]);
    std::fprintf(o, " |");
    for (int32_t x = 0; x < n; ++x) std::fprintf(o, " %d", ab[x]);
    std::fprintf(o, "\n");
    for (int32_t* p : {a, b, ba, ab, ba2, ab2}) std::free(p);
  }
  // the plan's arithmetic at its corners (UBSan: no overflow)
  const EaPlan top = edit_align_plan(EA_MAX_LEN, EA_MAX_LEN, 4, true);
  const EaPlan over = edit_align_plan(EA_MAX_LEN, EA_MAX_LEN, 5, true);
  const EaPlan many = edit_align_plan(EA_MAX_LEN, EA_MAX_LEN, 2147483647, true);
  const EaPlan none = edit_align_plan(EA_MAX_LEN + 1, 1, 1, true);
  if (!top.ok || top.bits_bytes != EA_BITS_LIMIT || top.launches != 767 || over.ok || many.ok || none.ok) return 3;
  if (ea_diag_tiles(0, top.tiles_r, top.tiles_c) != 1 || ea_diag_tiles(766, top.tiles_r, top.tiles_c) != 1 ||
      ea_diag_tiles(300, top.tiles_r, top.tiles_c) != 256)
    return 3;
  std::fclose(f);
  std::fclose(o);
  std::printf("edit_align_check ok\n");
  return 0;
}
