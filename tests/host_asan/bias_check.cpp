// csrc/bias_plan.h (the phrase automaton's builder, its transition, the sentence walk and the row rule,
// which the kernels of csrc/bias.hip and csrc/beam_lm.hip compile too) under AddressSanitizer +
// UndefinedBehaviorSanitizer on the CPU: a program of its own (tests/test_bias_host_sanitizer.py builds
// and runs it).  Every array is read into a heap buffer of exactly its length, and the built tables are
// copied into such buffers before they are queried, so a read past any of them is a
// heap-buffer-overflow.  Case file: int32 sets; per set int32 V, P, the arrays lens [P], boost [P],
// int64 nt, tokens [nt], then int32 sentences, per sentence int32 l, int64 ny, y[ny].  Output: per set a
// line "B rc nodes", and per sentence "S full tail state" and "R" with the V gains of that state's row
// followed by the V successor states.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bias_plan.h"

using namespace casr;

template <class T>
static T* read_exact(FILE* f, size_t n) {
  T* p = static_cast<T*>(std::malloc(n ? n * sizeof(T) : 1));
  if (n && std::fread(p, sizeof(T), n, f) != n) {
    std::fprintf(stderr, "bias_check: short case file\n");
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
    const int32_t V = read_one<int32_t>(f), P = read_one<int32_t>(f);
    int32_t* lens = read_exact<int32_t>(f, (size_t)P);
    int32_t* boost = read_exact<int32_t>(f, (size_t)P);
    const int64_t nt = read_one<int64_t>(f);
    int32_t* tokens = read_exact<int32_t>(f, (size_t)nt);
    BiasNode* node = nullptr;
    int32_t *ctok = nullptr, *cnext = nullptr, *rnext = nullptr, *rgain = nullptr;
    int rc, nodes = 0;
    {
      BiasTables t;
      std::string why;
      rc = bias_build(V, P, tokens, lens, boost, &t, &why);
      if (rc == BIAS_OK) {
        nodes = (int)t.node.size();
        node = exact_copy(t.node);
        ctok = exact_copy(t.ctok);
        cnext = exact_copy(t.cnext);
        rnext = exact_copy(t.root_next);
        rgain = exact_copy(t.root_gain);
      }
    }
    std::fprintf(o, "B %d %d\n", rc, nodes);
    const BiasView m{V, nodes, node, ctok, cnext, rnext, rgain};
    const int32_t ns = read_one<int32_t>(f);
    for (int32_t s = 0; s < ns; ++s) {
      const int32_t l = read_one<int32_t>(f);
      const int64_t ny = read_one<int64_t>(f);
      int32_t* y = read_exact<int32_t>(f, (size_t)ny);
      if (rc == BIAS_OK) {
        int32_t full = -1, tail = -1, state = -1;
        bias_sentence(m, y, l, &full, &tail, &state);
        std::fprintf(o, "S %d %d %d\n", full, tail, state);
        int32_t* gain = static_cast<int32_t*>(std::malloc((size_t)V * sizeof(int32_t)));
        int32_t* next = static_cast<int32_t*>(std::malloc((size_t)V * sizeof(int32_t)));
        bias_row_host(m, state, gain, next);
        std::fprintf(o, "R");
        for (int v = 0; v < V; ++v) {
          if (gain[v] != bias_gain(m, state, v) || next[v] != bias_delta(m, state, v)) {
            std::fprintf(stderr, "bias_check: the row and the transition disagree at set %d state %d token %d\n", i,
                         state, v);
            return 1;
          }
          std::fprintf(o, " %d", gain[v]);
        }
        for (int v = 0; v < V; ++v) std::fprintf(o, " %d", next[v]);
        std::fprintf(o, "\n");
        std::free(gain);
        std::free(next);
      }
      std::free(y);
    }
    std::free(lens);
    std::free(boost);
    std::free(tokens);
    std::free(node);
    std::free(ctok);
    std::free(cnext);
    std::free(rnext);
    std::free(rgain);
  }
  std::fclose(f);
  std::fclose(o);
  std::printf("bias_check ok\n");
  return 0;
}
