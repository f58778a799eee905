// csrc/segment_plan.h under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (host
// code only; tests/test_segment_host_sanitizer.py builds and runs it).  Every input array lives in a heap
// buffer of exactly the size the file states, and every recording is copied into a buffer of exactly
// its n rows, so a read past what the operation may touch is a sanitizer report.
//   segment_check <cases.bin> <out.bin>
// cases.bin: int32 count; per case ten int32 parameters (casr_segment_params order), int32 n, n_mels,
// s_max, chunk, then the fbank array: int64 element count + the floats (n n_mels of them, or fewer in the
// case that must be caught).
// out.bin: per case int32 thr, n_seg, then min(n_seg, s_max) (start, len) int32 pairs.
// Each case runs twice: whole-row runs, and runs clipped to `chunk` frames as the kernel's tiles hand
// them over; both must give the same segments.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "segment_plan.h"

using namespace casr;

#define CHECK(c)                                                             \
  do {                                                                       \
    if (!(c)) {                                                              \
      fprintf(stderr, "segment_check: %s failed (line %d)\n", #c, __LINE__); \
      exit(2);                                                               \
    }                                                                        \
  } while (0)

template <class T>
static std::unique_ptr<T[]> read_array(FILE* f, int64_t* n) {
  CHECK(fread(n, sizeof *n, 1, f) == 1);
  std::unique_ptr<T[]> p(new T[(size_t)*n]);  // exact size: no slack behind the data
  if (*n) CHECK(fread(p.get(), sizeof(T), (size_t)*n, f) == (size_t)*n);
  return p;
}

static void edge_cases() {
  casr_segment_params p = segment_default_params();
  CHECK(segment_params_valid(p));
  CHECK(segment_bound(60000, p) == (60000 + 20) / 25 + 60000 / 200);
  CHECK(segment_bound(-1, p) == -1);
  casr_segment_params big = p;
  big.min_speech = 1;
  big.min_pause = 1;
  big.pad = 0;
  big.min_frames = 1;
  CHECK(segment_bound(INT32_MAX, big) == -1);  // does not fit an int
  big.max_frames = INT32_MAX;  // the split and the merge add to it
  big.max_gap = INT32_MAX;
  big.rise_min = INT32_MAX;    // thr saturates
  std::unique_ptr<float[]> fb(new float[3 * 16]);
  for (int i = 0; i < 48; ++i) fb[i] = (float)(i / 16);
  int32_t st[4], ln[4], ns = -1, thr = -1;
  segment_row_host(fb.get(), 3, 16, big, 4, st, ln, &ns, &thr);
  CHECK(ns == 0 && thr == INT32_MAX);
  big.rise_min = 0;
  big.rel_q8 = 0;  // thr = lo: every frame is active
  segment_row_host(fb.get(), 3, 16, big, 4, st, ln, &ns, &thr);
  CHECK(ns == 1 && st[0] == 0 && ln[0] == 3);
  segment_row_host(fb.get(), 0, 16, big, 4, st, ln, &ns, &thr);  // n = 0 reads nothing
  CHECK(ns == 0 && thr == 0);
  CHECK(seg_key_cut(seg_cut_key(7, 12345)) == 12345 && seg_cut_key(7, 5) < seg_cut_key(7, 4) &&
        seg_cut_key(6, 4) < seg_cut_key(7, 5));
  CHECK(seg_level_bin(-1e30f, 1.f) == 0 && seg_level_bin(1e30f, 1.f) == 511 && seg_level_bin(-24.f, 1.f) == 0 &&
        seg_level_bin(39.9f, 1.f) == 511 && seg_level_bin(0.f, 1.f) == 192);
}

int main(int argc, char** argv) {
  edge_cases();
  if (argc < 3) {
    printf("segment_check ok (edge cases only)\n");
    return 0;
  }
  FILE* f = fopen(argv[1], "rb");
  CHECK(f);
  FILE* o = fopen(argv[2], "wb");
  CHECK(o);
  int32_t count;
  CHECK(fread(&count, sizeof count, 1, f) == 1);
  for (int i = 0; i < count; ++i) {
    casr_segment_params p;
    int32_t dims[4];
    CHECK(fread(&p, sizeof p, 1, f) == 1);
    CHECK(fread(dims, sizeof dims, 1, f) == 1);
    const int32_t n = dims[0], n_mels = dims[1], s_max = dims[2], chunk = dims[3];
    CHECK(segment_params_valid(p) && n >= 0 && n_mels > 0 && n_mels % SEG_LANES == 0 && s_max >= 0);
    int64_t sz;
    auto fb = read_array<float>(f, &sz);  // exactly the recording's rows (or what the file holds of them)
    std::unique_ptr<int32_t[]> st(new int32_t[(size_t)s_max]), ln(new int32_t[(size_t)s_max]);
    std::unique_ptr<int32_t[]> st2(new int32_t[(size_t)s_max]), ln2(new int32_t[(size_t)s_max]);
    int32_t ns = -1, thr = -1, ns2 = -1, thr2 = -1;
    segment_row_host(fb.get(), n, n_mels, p, s_max, st.get(), ln.get(), &ns, &thr);
    segment_row_host(fb.get(), n, n_mels, p, s_max, st2.get(), ln2.get(), &ns2, &thr2, chunk);
    const int32_t w = ns < s_max ? ns : s_max;
    CHECK(ns == ns2 && thr == thr2);
    CHECK(w == 0 || (memcmp(st.get(), st2.get(), sizeof(int32_t) * (size_t)w) == 0 &&
                     memcmp(ln.get(), ln2.get(), sizeof(int32_t) * (size_t)w) == 0));
    CHECK(ns <= segment_bound(n, p));
    CHECK(fwrite(&thr, sizeof thr, 1, o) == 1 && fwrite(&ns, sizeof ns, 1, o) == 1);
    for (int32_t k = 0; k < w; ++k) CHECK(fwrite(&st[k], 4, 1, o) == 1 && fwrite(&ln[k], 4, 1, o) == 1);
  }
  fclose(f);
  fclose(o);
  printf("segment_check ok\n");
  return 0;
}
