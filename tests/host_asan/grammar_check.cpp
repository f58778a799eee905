// csrc/grammar_plan.h (the acceptor's builder, its transition, the candidate rule, the sentence walk and
// the row rule, which the kernels of csrc/grammar.hip and csrc/beam_lm.hip compile too) under
// AddressSanitizer + UndefinedBehaviorSanitizer on the CPU: a program of its own
// (tests/test_grammar_host_sanitizer.py builds and runs it).  Every array is read into a heap buffer of
// exactly its length, and the built tables are copied into such buffers before they are queried, so a read
// past any of them is a heap-buffer-overflow.  Case file: int32 sets; per set int32 V, eos, S, the arrays
// arc_off [S + 1] (int64), int64 A, arc_tok [A], arc_next [A], is_final [S] (bytes), then int32 sentences,
// per sentence int32 l, int64 ny, y[ny], then int32 rows, per row int32 state, budget.  Output: per set a
// line "G rc states" and (rc 0) "D" with the S distances, per sentence "S consumed state accepted", per
// row "R bad" followed by the V bits of the row.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "grammar_plan.h"

using namespace casr;

template <class T>
static T* read_exact(FILE* f, size_t n) {
  T* p = static_cast<T*>(std::malloc(n ? n * sizeof(T) : 1));
  if (n && std::fread(p, sizeof(T), n, f) != n) {
    std::fprintf(stderr, "grammar_check: short case file\n");
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

template <class T>
static T* exact_copy(const std::vector<T>& v) {
  T* p = static_cast<T*>(std::malloc(v.size() ? v.size() * sizeof(T) : 1));
  if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  FILE* o = std::fopen(argv[2], "w");
  if (!f || !o) return 2;
  const int32_t sets = read_one<int32_t>(f);
  for (int32_t i = 0; i < sets; ++i) {
    const int32_t V = read_one<int32_t>(f), eos = read_one<int32_t>(f), S = read_one<int32_t>(f);
    int64_t* off = read_exact<int64_t>(f, (size_t)S + 1);
    const int64_t A = read_one<int64_t>(f);
    int32_t* tok = read_exact<int32_t>(f, (size_t)A);
    int32_t* nxt = read_exact<int32_t>(f, (size_t)A);
    uint8_t* fin = read_exact<uint8_t>(f, (size_t)S);
    int32_t *doff = nullptr, *dtok = nullptr, *dnext = nullptr, *dadist = nullptr, *ddist = nullptr;
    uint8_t* dfin = nullptr;
    int rc, states = 0;
    {
      GrammarTables t;
      std::string why;
      rc = gram_build(V, eos, S, off, tok, nxt, fin, &t, &why);
      if (rc == GRAM_OK) {
        states = t.n_states();
        doff = exact_copy(t.arc_off);
        dtok = exact_copy(t.arc_tok);
        dnext = exact_copy(t.arc_next);
        dadist = exact_copy(t.arc_dist);
        ddist = exact_copy(t.dist);
        dfin = exact_copy(t.is_final);
      }
    }
    std::fprintf(o, "G %d %d\n", rc, states);
    const GrammarView m{V, eos, states, doff, dtok, dnext, dadist, ddist, dfin};
    for (int s = 0; rc == GRAM_OK && s < states; ++s)
      for (int q = doff[s]; q < doff[s + 1]; ++q)
        if (dadist[q] != ddist[dnext[q]]) {
          std::fprintf(stderr, "grammar_check: arc_dist and dist disagree at set %d arc %d\n", i, q);
          return 1;
        }
    if (rc == GRAM_OK) {
      std::fprintf(o, "D");
      for (int s = 0; s < states; ++s) std::fprintf(o, " %d", ddist[s]);
      std::fprintf(o, "\n");
    }
    const int32_t ns = read_one<int32_t>(f);
    for (int32_t s = 0; s < ns; ++s) {
      const int32_t l = read_one<int32_t>(f);
      const int64_t ny = read_one<int64_t>(f);
      int32_t* y = read_exact<int32_t>(f, (size_t)ny);
      if (rc == GRAM_OK) {
        int32_t consumed = -1, state = -1;
        uint8_t ok = 2;
        gram_sentence(m, y, l, &consumed, &state, &ok);
        std::fprintf(o, "S %d %d %d\n", consumed, state, (int)ok);
      }
      std::free(y);
    }
    const int32_t nr = read_one<int32_t>(f);
    for (int32_t r = 0; r < nr; ++r) {
      const int32_t state = read_one<int32_t>(f), budget = read_one<int32_t>(f);
      if (rc != GRAM_OK) continue;
      const int GW = gram_mask_words(V);
      uint32_t* mask = static_cast<uint32_t*>(std::malloc((size_t)GW * sizeof(uint32_t)));
      std::memset(mask, 0xff, (size_t)GW * sizeof(uint32_t));
      bool bad = false;
      gram_row_host(m, state, budget, mask, &bad);
      std::fprintf(o, "R %d ", (int)bad);
      for (int v = 0; v < 32 * GW; ++v) {
        const int bit = (mask[v >> 5] >> (v & 31)) & 1;
        const bool in = state >= 0 && state < states;
        if (v >= V ? bit != 0 : bit != (in && gram_allows(m, state, v, budget) ? 1 : 0)) {
          std::fprintf(stderr, "grammar_check: the row and the candidate rule disagree at set %d state %d token %d\n", i,
                       state, v);
          return 1;
        }
        if (v < V) std::fputc('0' + bit, o);
      }
      std::fprintf(o, "\n");
      std::free(mask);
    }
    std::free(off);
    std::free(tok);
    std::free(nxt);
    std::free(fin);
    std::free(doff);
    std::free(dtok);
    std::free(dnext);
    std::free(dadist);
    std::free(ddist);
    std::free(dfin);
  }
  std::fclose(f);
  std::fclose(o);
  std::printf("grammar_check ok\n");
  return 0;
}
