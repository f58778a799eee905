// The beam tree's reading rules (csrc/beam_tree.h) on the host, as a program of its own under
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_beam_tree_host.py builds and runs it): the
// text the kernels compile, on small hand-built trees in heap arrays of exactly the size the rules may
// read (B = 2, k = 3, L = 5), each rule against a literal restatement written out here.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "beam_tree.h"

using namespace casr;

#define CHECK(c)                                                               \
  do {                                                                         \
    if (!(c)) {                                                                \
      fprintf(stderr, "beam_tree_check: %s failed (line %d)\n", #c, __LINE__); \
      exit(2);                                                                 \
    }                                                                          \
  } while (0)

constexpr int B = 2, K = 3, L = 5, R = B * K, V = 50;
static int checks = 0;

// an exactly sized heap array (ASan sees one element past either end)
template <class T>
struct Heap {
  T* p;
  explicit Heap(size_t n) : p(static_cast<T*>(malloc(n * sizeof(T)))) { memset(p, 0, n * sizeof(T)); }
  ~Heap() { free(p); }
  Heap(const Heap&) = delete;
  T& operator[](size_t i) { return p[i]; }
};

struct Tree {
  Heap<int32_t> bp{(size_t)L * R}, tk{(size_t)L * R}, newdone{L}, rec_src{(size_t)B * L * K};
  Heap<float> rec_score{(size_t)B * L * K}, s0{R}, s1{R};
  Heap<uint8_t> rec_valid{(size_t)B * L * K};
  Heap<int32_t> err{1};
  Tree() {
    for (int st = 0; st < L; ++st)
      for (int r = 0; r < R; ++r) {
        bp[st * R + r] = (st * 7 + r * 5 + 1) % K;
        tk[st * R + r] = 10 * st + r;  // every node its own token
      }
  }
  BeamTree view() {
    return BeamTree{B, K, L, V, bp.p, tk.p, newdone.p, rec_score.p, rec_src.p, rec_valid.p, {s0.p, s1.p}, err.p};
  }
};

static void executed_steps() {
  Heap<int32_t> nd(L);
  const int at0[L] = {2, 0, 0, 0, 0}, mid[L] = {0, 1, 0, 1, 0}, never[L] = {0, 0, 1, 0, 0}, over[L] = {1, 0, 3, 0, 0};
  memcpy(nd.p, at0, sizeof(at0));
  CHECK(beam_executed_steps(nd.p, L, B) == 1);
  memcpy(nd.p, mid, sizeof(mid));
  CHECK(beam_executed_steps(nd.p, L, B) == 4);
  memcpy(nd.p, never, sizeof(never));
  CHECK(beam_executed_steps(nd.p, L, B) == L);
  memcpy(nd.p, over, sizeof(over));
  CHECK(beam_executed_steps(nd.p, L, B) == 3);
  Heap<int32_t> two(2);  // reached at step 1 of an array that ends there: nothing past it is read
  two[1] = 2;
  CHECK(beam_executed_steps(two.p, 2, B) == 2);
  checks += 5;
}

// the literal restatement of casr_beam's unfinished fallback
static int live_row_ref(const float* s0, const float* s1, int b, float lmw, float lenw, int steps, float* score) {
  const float* sf = (steps & 1) ? s1 : s0;
  const int ll = steps - 1;
  const float lw = (float)((double)lenw * (double)(ll + 1));
  int bj = 0;
  float bsv = 0.f;
  for (int j = 0; j < K; ++j) {
    const float s = (sf[b * K + j] + lmw * 0.f) + lw;
    if (j == 0 || s > bsv) {
      bsv = s;
      bj = j;
    }
  }
  *score = bsv;
  return bj;
}

static void live_row() {
  Tree t;
  const float a0[R] = {-3.5f, -1.25f, -1.25f, -7.f, -9.f, -8.f};  // utterance 0: a tie, the first wins
  const float a1[R] = {-2.f, -2.f, -0.5f, -4.f, -4.f, -4.f};      // utterance 1: all equal
  memcpy(t.s0.p, a0, sizeof(a0));
  memcpy(t.s1.p, a1, sizeof(a1));
  const BeamTree v = t.view();
  const int want[2][2] = {{1, 0}, {2, 0}};  // [parity][b]
  for (int steps = 1; steps <= L; ++steps)
    for (int b = 0; b < B; ++b)
      for (float lenw : {0.f, 0.3f, -1.7f}) {
        float s = 0.f, sr = 0.f;
        const int j = beam_live_row(v, b, 0.4f, lenw, steps, &s);
        const int jr = live_row_ref(t.s0.p, t.s1.p, b, 0.4f, lenw, steps, &sr);
        CHECK(j == jr && memcmp(&s, &sr, sizeof(s)) == 0);
        CHECK(j == want[steps & 1][b]);
        ++checks;
      }
}

// the literal walk over the workspaces' layout
static bool walk_ref(Tree& t, int b, int slot, int from, int32_t* out) {
  bool bad = false;
  for (int s = from; s >= 0; --s) {
    if ((unsigned)slot >= (unsigned)K) {
      bad = true;
      slot = 0;
    }
    const size_t ix = (size_t)s * R + b * K + slot;
    out[s] = t.tk[ix];
    slot = t.bp[ix];
  }
  return bad;
}

// stage `steps` steps of utterance b with `nthreads` threads into exactly sized arrays; returns the OR of
// the threads' reports
template <bool CLAMP>
static bool stage(const BeamTree& v, int b, int steps, int nthreads, Heap<int32_t>& sbp, Heap<int32_t>& stk,
                  std::vector<int>* seen) {
  bool bad = false;
  for (int tid = 0; tid < nthreads; ++tid)
    bad |= beam_stage_tree<CLAMP>(v, b, steps, sbp.p, stk.p, tid, nthreads, [&](int i, int32_t tok) {
      CHECK(tok == stk[i]);
      if (seen) ++(*seen)[i];
    });
  return bad;
}

// both layouts against the literal walk from every node, for a tree that may hold bad pointers; returns
// whether any global walk reported
static bool walks_agree(Tree& t, int steps, bool expect_stage_bad) {
  const BeamTree v = t.view();
  bool any = false;
  for (int b = 0; b < B; ++b)
    for (int nthreads : {1, 4, 64}) {
      Heap<int32_t> sbp((size_t)steps * K), stk((size_t)steps * K), raw((size_t)steps * K), rtk((size_t)steps * K);
      std::vector<int> seen(steps * K, 0);
      const bool sbad = stage<true>(v, b, steps, nthreads, sbp, stk, &seen);
      CHECK(!stage<false>(v, b, steps, nthreads, raw, rtk, nullptr));
      if (!expect_stage_bad) CHECK(!sbad);
      const TreeGlobal g(v, b);
      for (int st = 0; st < steps; ++st)
        for (int c = 0; c < K; ++c) {  // staged and global reads agree on every node
          const int i = st * K + c, p = t.bp[g.at(st, c)];
          CHECK(seen[i] == 1);
          CHECK(stk[i] == t.tk[g.at(st, c)] && rtk[i] == stk[i] && raw[i] == p);
          CHECK(sbp[i] == ((unsigned)p < (unsigned)K ? p : 0));
          ++checks;
        }
      for (int from = -1; from < steps; ++from)
        for (int slot = -1; slot <= K; ++slot) {
          Heap<int32_t> ref(L), og(L), os(L), orw(L);
          int calls = 0;
          const bool bref = walk_ref(t, b, slot, from, ref.p);
          const bool bg = beam_walk(g, K, slot, from, [&](int s, int32_t tok) { og[s] = tok, ++calls; });
          const TreeStaged<true> staged{sbp.p, stk.p, K};
          const TreeStaged<false> unclamped{raw.p, rtk.p, K};
          const bool bs = beam_walk(staged, K, slot, from, [&](int s, int32_t tok) { os[s] = tok; });
          const bool br = beam_walk(unclamped, K, slot, from, [&](int s, int32_t tok) { orw[s] = tok; });
          CHECK(calls == from + 1);
          CHECK(bg == bref && br == bref);
          // the clamped staging has nothing left to report but the start slot
          CHECK(bs == (from >= 0 && (unsigned)slot >= (unsigned)K));
          CHECK(memcmp(ref.p, og.p, L * sizeof(int32_t)) == 0 && memcmp(ref.p, os.p, L * sizeof(int32_t)) == 0 &&
                memcmp(ref.p, orw.p, L * sizeof(int32_t)) == 0);
          any |= bg;
          ++checks;
        }
    }
  return any;
}

static void walks() {
  Tree t;
  for (int steps = 1; steps <= L; ++steps) walks_agree(t, steps, false);
  for (int bad : {-1, K}) {
    {  // at a step >= 1: clamped and reported by the staging and by the walk that follows it
      Tree u;
      u.bp[2 * R + 1 * K + 1] = bad;  // step 2, utterance 1, slot 1
      const BeamTree w = u.view();
      Heap<int32_t> sbp((size_t)L * K), stk((size_t)L * K), out(L);
      CHECK(stage<true>(w, 1, L, 4, sbp, stk, nullptr) && sbp[2 * K + 1] == 0);
      CHECK(!stage<true>(w, 0, L, 4, sbp, stk, nullptr));    // the other utterance is whole
      CHECK(!stage<true>(w, 1, 2, 4, sbp, stk, nullptr));    // and so are the steps before it
      CHECK(beam_walk(TreeGlobal(w, 1), K, 1, 2, [&](int s, int32_t tok) { out[s] = tok; }));
      CHECK(out[2] == u.tk[2 * R + K + 1] && out[1] == u.tk[1 * R + K + 0]);  // went on from slot 0
      CHECK(!beam_walk(TreeGlobal(w, 1), K, 0, 2, [&](int s, int32_t tok) { out[s] = tok; }));  // not followed
      CHECK(walks_agree(u, L, true));
    }
    {  // at step 0: clamped, never reported (no predecessor node: the pointer is not followed)
      Tree u;
      for (int r = 0; r < R; ++r) u.bp[r] = bad;
      const BeamTree w = u.view();
      Heap<int32_t> sbp((size_t)L * K), stk((size_t)L * K);
      for (int b = 0; b < B; ++b) {
        CHECK(!stage<true>(w, b, L, 4, sbp, stk, nullptr));
        for (int c = 0; c < K; ++c) CHECK(sbp[c] == 0);
      }
      Tree clean;
      for (int b = 0; b < B; ++b)
        for (int from = 0; from < L; ++from)
          for (int slot = 0; slot < K; ++slot) {
            Heap<int32_t> o0(L), o1(L);
            CHECK(!beam_walk(TreeGlobal(w, b), K, slot, from, [&](int s, int32_t tok) { o0[s] = tok; }));
            CHECK(!walk_ref(clean, b, slot, from, o1.p));
            CHECK(memcmp(o0.p, o1.p, L * sizeof(int32_t)) == 0);
            ++checks;
          }
    }
    {  // a record's start slot: an empty record walks nothing and reports nothing
      Tree u;
      const size_t r0 = (size_t)(1 * L + 0) * K + 2, r3 = (size_t)(1 * L + 3) * K + 2;
      u.rec_src[r0] = bad;
      u.rec_src[r3] = bad;
      u.rec_src[r3 - 1] = 2;
      const BeamTree w = u.view();
      bool rep = false;
      CHECK(beam_record_slot(w, r0, 0, &rep) == 0 && !rep);
      int calls = 0;
      CHECK(!beam_walk(TreeGlobal(w, 1), K, u.rec_src[r0], 0 - 1, [&](int, int32_t) { ++calls; }) && calls == 0);
      CHECK(!beam_walk(TreeStaged<true>{nullptr, nullptr, K}, K, bad, -1, [&](int, int32_t) { ++calls; }) && calls == 0);
      CHECK(beam_record_slot(w, r3 - 1, 3, &rep) == 2 && !rep);
      CHECK(beam_record_slot(w, r3, 3, &rep) == 0 && rep);
      CHECK(beam_walk(TreeGlobal(w, 1), K, u.rec_src[r3], 3 - 1, [&](int, int32_t) { ++calls; }) && calls == 3);
      checks += 6;
    }
  }
}

int main() {
  executed_steps();
  live_row();
  walks();
  printf("beam_tree_check ok (%d checks)\n", checks);
  return 0;
}
