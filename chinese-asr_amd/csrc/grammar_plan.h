// Grammar-constrained decoding (include/casr.h casr_grammar_*, casr_beam_grammar): the acceptor's view,
// its transition, the candidate rule, the sentence walk and the mask row of a state, once, as plain C++
// that the kernels (grammar.hip, beam_lm.hip), the host entry points and the sanitizer program
// (tests/host_asan/grammar_check.cpp) all compile.  The builder (host only) is at the end.  The rules
// are casr.h's; tests/grammar_ref.py restates them by enumeration, with no automaton of its own kind.
//
// The grammar is a deterministic finite acceptor over token ids.  State s keeps its arcs as a range
// [arc_off[s], arc_off[s + 1]) of (token, next) pairs strictly ascending in token, a flag is_final, and
//   dist   the fewest tokens from s to a final state (0 at a final state), by backward breadth-first
//          search over the arcs; the builder refuses a state that reaches none, so dist is finite
// eos is never an arc label: a row may end (choose eos) exactly in a final state.  A candidate (s, v) with
// v != eos exists when there is an arc (s, v, d) and the row could still finish in time, dist[d] <= budget.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#if defined(__HIPCC__)
#define CASR_GRAM_HD __host__ __device__
#else
#define CASR_GRAM_HD
#endif

namespace casr {

constexpr int GRAM_MAX_STATES = 1 << 20;
constexpr int GRAM_MAX_ARCS = 1 << 24;
constexpr int GRAM_MAX_SENT = 512;  // longest sentence of casr_grammar_accept
constexpr int GRAM_DEAD = -1;       // the state of a dead beam row: no arcs, not final

struct GrammarView {
  int V, eos, n_states;
  const int32_t* arc_off;   // [n_states + 1]
  const int32_t* arc_tok;   // tokens, strictly ascending within a state
  const int32_t* arc_next;  // ... and the states they lead to
  const int32_t* arc_dist;  // ... and those states' dist, beside the tokens (the row kernel reads no other)
  const int32_t* dist;      // [n_states]
  const uint8_t* is_final;  // [n_states]
};

// words of a mask row: 4 ceil(V / 128), so rows are 16-byte aligned; bit v of word v >> 5 is token v
CASR_GRAM_HD inline int gram_mask_words(int V) { return 4 * ((V + 127) / 128); }

// the state under token v from state s, or -1 (binary search of an ascending range).  s must be a state;
// an id outside [0, V) has no arc.
CASR_GRAM_HD inline int gram_next(const GrammarView& m, int s, int v) {
  if ((unsigned)v >= (unsigned)m.V) return -1;
  int lo = m.arc_off[s], hi = m.arc_off[s + 1];
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int t = m.arc_tok[mid];
    if (t == v) return m.arc_next[mid];
    if (t < v) lo = mid + 1;
    else hi = mid;
  }
  return -1;
}

// is (s, v) a candidate under the budget: eos exactly in a final state, whatever the budget; another
// token when its arc leads to a state that reaches a final one within budget tokens.  s must be a state.
CASR_GRAM_HD inline bool gram_allows(const GrammarView& m, int s, int v, int budget) {
  if (v == m.eos) return m.is_final[s] != 0;
  const int d = gram_next(m, s, v);
  return d >= 0 && m.dist[d] <= budget;
}

// one sentence y[0..l) from state 0: the tokens walked before the first one without an arc (or l), the
// state after them, and accepted = all walked and that state final
CASR_GRAM_HD inline void gram_sentence(const GrammarView& m, const int32_t* y, int l, int32_t* consumed,
                                       int32_t* state, uint8_t* accepted) {
  int s = 0, j = 0;
  for (; j < l; ++j) {
    const int d = gram_next(m, s, y[j]);
    if (d < 0) break;
    s = d;
  }
  *consumed = j;
  *state = s;
  *accepted = (j == l && m.is_final[s]) ? 1 : 0;
}

// The row rule: the mask [gram_mask_words(V)] of state s under a budget.  Bit v is set iff (s, v) is a
// candidate (gram_allows); bits at and past V are 0.  The dead state gives a zero row; any other state
// outside [0, n_states) gives a zero row and *bad.
inline void gram_row_host(const GrammarView& m, int s, int budget, uint32_t* mask, bool* bad) {
  const int GW = gram_mask_words(m.V);
  for (int w = 0; w < GW; ++w) mask[w] = 0u;
  if (s == GRAM_DEAD) return;
  if ((unsigned)s >= (unsigned)m.n_states) {
    *bad = true;
    return;
  }
  for (int q = m.arc_off[s]; q < m.arc_off[s + 1]; ++q) {
    const int t = m.arc_tok[q];
    if (m.dist[m.arc_next[q]] <= budget) mask[t >> 5] |= 1u << (t & 31);
  }
  if (m.is_final[s]) mask[m.eos >> 5] |= 1u << (m.eos & 31);
}

// ---------------------------------------------------------------- the builder (host)
enum { GRAM_OK = 0, GRAM_ERR_ARG = 1, GRAM_ERR_UNSUPPORTED = 4 };  // casr.h's CASR_OK / CASR_ERR_*

struct GrammarTables {
  int V = 0, eos = 0;
  std::vector<int32_t> arc_off, arc_tok, arc_next, arc_dist, dist;
  std::vector<uint8_t> is_final;
  int n_states() const { return (int)is_final.size(); }
  GrammarView view() const {
    return GrammarView{V, eos, n_states(), arc_off.data(), arc_tok.data(), arc_next.data(), arc_dist.data(),
                       dist.data(), is_final.data()};
  }
};

// arc_off [S + 1] (int64, arc_off[0] = 0, ascending), arc_tok / arc_next [arc_off[S]], is_final [S]
inline int gram_build(int V, int eos, int S, const int64_t* arc_off, const int32_t* arc_tok, const int32_t* arc_next,
                      const uint8_t* is_final, GrammarTables* out, std::string* why) {
  auto bad = [&](int code, const std::string& s) {
    if (why) *why = s;
    return code;
  };
  const auto str = [](long long x) { return std::to_string(x); };
  if (V < 1) return bad(GRAM_ERR_ARG, "vocab " + str(V) + " < 1");
  if (eos < 0 || eos >= V) return bad(GRAM_ERR_ARG, "eos_token " + str(eos) + " outside [0, " + str(V) + ")");
  if (S < 1) return bad(GRAM_ERR_ARG, "n_states " + str(S) + " < 1");
  if (!arc_off || !is_final) return bad(GRAM_ERR_ARG, "a NULL array");
  if (S > GRAM_MAX_STATES) return bad(GRAM_ERR_UNSUPPORTED, "more than " + str(GRAM_MAX_STATES) + " states");
  if (arc_off[0] != 0) return bad(GRAM_ERR_ARG, "arc_off[0] = " + str(arc_off[0]) + ", not 0");
  for (int s = 0; s < S; ++s) {
    if (arc_off[s + 1] < arc_off[s])
      return bad(GRAM_ERR_ARG, "state " + str(s) + " has a negative arc count (arc_off descends)");
    if (arc_off[s + 1] > GRAM_MAX_ARCS) return bad(GRAM_ERR_UNSUPPORTED, "more than " + str(GRAM_MAX_ARCS) + " arcs");
  }
  const int A = (int)arc_off[S];
  if (A > 0 && (!arc_tok || !arc_next)) return bad(GRAM_ERR_ARG, "a NULL array");
  bool any_final = false;
  for (int s = 0; s < S; ++s) {
    any_final = any_final || is_final[s];
    for (int q = (int)arc_off[s]; q < (int)arc_off[s + 1]; ++q) {
      const std::string at = "arc " + str(q) + " of state " + str(s);
      const int32_t t = arc_tok[q];
      if (t < 0 || t >= V) return bad(GRAM_ERR_ARG, at + " has token " + str(t) + " outside [0, " + str(V) + ")");
      if (t == eos) return bad(GRAM_ERR_ARG, at + " has the eos token " + str(t) + " as its label");
      if (q > (int)arc_off[s] && arc_tok[q - 1] >= t)
        return bad(GRAM_ERR_ARG, at + " has token " + str(t) + " after " + str(arc_tok[q - 1]) +
                                     ": tokens must ascend strictly within a state");
      if (arc_next[q] < 0 || arc_next[q] >= S)
        return bad(GRAM_ERR_ARG, at + " leads to state " + str(arc_next[q]) + " outside [0, " + str(S) + ")");
    }
  }
  if (!any_final) return bad(GRAM_ERR_ARG, "no final state");
  // dist by breadth-first search over the reversed arcs from all final states at once
  std::vector<int32_t> roff(S + 1, 0), rsrc(A);
  for (int q = 0; q < A; ++q) ++roff[arc_next[q] + 1];
  for (int s = 0; s < S; ++s) roff[s + 1] += roff[s];
  {
    std::vector<int32_t> fill(roff.begin(), roff.end() - 1);
    for (int s = 0; s < S; ++s)
      for (int q = (int)arc_off[s]; q < (int)arc_off[s + 1]; ++q) rsrc[fill[arc_next[q]]++] = s;
  }
  std::vector<int32_t> dist(S, -1), order;
  order.reserve(S);
  for (int s = 0; s < S; ++s)
    if (is_final[s]) {
      dist[s] = 0;
      order.push_back(s);
    }
  for (size_t h = 0; h < order.size(); ++h) {
    const int d = order[h];
    for (int q = roff[d]; q < roff[d + 1]; ++q) {
      const int s = rsrc[q];
      if (dist[s] < 0) {
        dist[s] = dist[d] + 1;
        order.push_back(s);
      }
    }
  }
  for (int s = 0; s < S; ++s)
    if (dist[s] < 0) return bad(GRAM_ERR_ARG, "state " + str(s) + " reaches no final state (trim it out)");
  GrammarTables& t = *out;
  t.V = V;
  t.eos = eos;
  t.arc_off.resize(S + 1);
  for (int s = 0; s <= S; ++s) t.arc_off[s] = (int32_t)arc_off[s];
  t.arc_tok.clear();
  t.arc_next.clear();
  if (A > 0) {
    t.arc_tok.assign(arc_tok, arc_tok + A);
    t.arc_next.assign(arc_next, arc_next + A);
  }
  t.dist = dist;
  t.arc_dist.resize(A);
  for (int q = 0; q < A; ++q) t.arc_dist[q] = dist[arc_next[q]];
  t.is_final.resize(S);
  for (int s = 0; s < S; ++s) t.is_final[s] = is_final[s] ? 1 : 0;
  return GRAM_OK;
}

}  // namespace casr
