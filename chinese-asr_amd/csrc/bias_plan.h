// Hotword biasing (include/casr.h casr_bias_*, casr_beam_bias): the phrase automaton's view, its
// transition, the gain of a candidate, the dense row of a state and the sentence walk, once, as plain
// C++ that the kernels (bias.hip, beam_lm.hip), the host entry points and the sanitizer program
// (tests/host_asan/bias_check.cpp) all compile.  The builder (host only) is at the end.  The formulas
// are casr.h's; tests/bias_ref.py restates full and tail by brute force, with no automaton.
//
// The automaton is Aho-Corasick over the phrases.  Node 0 is the root (the empty match).  A node keeps
//   fail, depth
//   out_sum  the sum of n_p b_p over the phrases that end at the node or on its fail chain: what every
//            occurrence ending at this position adds to full
//   tail     the maximum over the node and its fail chain of depth x (the largest b_p among the phrases
//            that pass PROPERLY through the node, i.e. are longer than its depth): tail(y) of a
//            sequence that leaves the automaton here
//   its children as a range of (token, node) pairs ascending in token
// and the root's children are two dense arrays root_next [V] / root_gain [V], so the usual candidate (no
// match in progress continues) costs one read.  All arithmetic is int32: with b_p <= 4096 and n_p <= 16
// a position adds at most sum_{n <= 16} 4096 n = 557,056 (one phrase per length can end there), so 512
// positions stay below 2^31 with room for a tail (<= 15 x 4096).
#pragma once
#include <stdint.h>

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "casr.h"

#if defined(__HIPCC__)
#define CASR_BIAS_HD __host__ __device__
#else
#define CASR_BIAS_HD
#endif

namespace casr {

constexpr int BIAS_MAX_LEN = CASR_BIAS_MAX_LEN;  // tokens of a phrase; also the longest fail chain
constexpr int BIAS_MAX_BOOST = 4096;             // units of 1/256 nat per token
constexpr int BIAS_MAX_TOKENS = 1 << 20;         // tokens of all phrases
constexpr int BIAS_MAX_SENT = 512;               // longest sentence of casr_bias_score (the int32 bound above)

struct BiasNode {
  int32_t fail, depth, out_sum, tail;
  int32_t child_off, child_cnt;  // its children: ctok / cnext [child_off, child_off + child_cnt)
};

struct BiasView {
  int V, n_nodes;
  const BiasNode* node;
  const int32_t* ctok;   // children's tokens, ascending within a node
  const int32_t* cnext;  // ... and the nodes they lead to
  const int32_t* root_next;  // [V] the root's child under v, or 0
  const int32_t* root_gain;  // [V] out_sum + tail of that node (0 at the root)
};

// the child of node u under token v, or -1 (binary search of an ascending range)
CASR_BIAS_HD inline int bias_child(const BiasView& m, int u, int v) {
  const BiasNode nd = m.node[u];
  int lo = nd.child_off, hi = nd.child_off + nd.child_cnt;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int t = m.ctok[mid];
    if (t == v) return m.cnext[mid];
    if (t < v) lo = mid + 1;
    else hi = mid;
  }
  return -1;
}

// delta(s, v): the first node on s, fail(s), ... (root excluded) that has child v, else the root's
// child.  A token outside [0, V) matches nothing: the root.  s must be a node.
CASR_BIAS_HD inline int bias_delta(const BiasView& m, int s, int v) {
  if ((unsigned)v >= (unsigned)m.V) return 0;
  for (int u = s; u != 0; u = m.node[u].fail) {
    const int c = bias_child(m, u, v);
    if (c >= 0) return c;
  }
  return m.root_next[v];
}

CASR_BIAS_HD inline int bias_gain_of(const BiasView& m, int node) { return m.node[node].out_sum + m.node[node].tail; }

// gain(s, v) = out_sum(delta) + tail(delta): what candidate v adds to C_r under bias_open
CASR_BIAS_HD inline int bias_gain(const BiasView& m, int s, int v) { return bias_gain_of(m, bias_delta(m, s, v)); }

// the row rule: (s, C) after token v is (delta, C + out_sum(delta))
CASR_BIAS_HD inline void bias_advance(const BiasView& m, int v, int* s, int* C) {
  const int d = bias_delta(m, *s, v);
  *s = d;
  *C += m.node[d].out_sum;
}

// a state outside the automaton is the root (the callers report it)
CASR_BIAS_HD inline int bias_clamp_state(const BiasView& m, int s, bool* bad) {
  if ((unsigned)s >= (unsigned)m.n_nodes) {
    *bad = true;
    return 0;
  }
  return s;
}

// the non-root nodes of s's fail chain, s first (at most BIAS_MAX_LEN: depths fall strictly)
CASR_BIAS_HD inline int bias_chain(const BiasView& m, int s, int32_t* chain) {
  int n = 0;
  for (int u = s; u != 0 && n < BIAS_MAX_LEN; u = m.node[u].fail) chain[n++] = u;
  return n;
}

// The dense row of state s: gain [V] and next [V] (or null).  The root's arrays first, then the chain's
// children from the node nearest the root to s itself, so the deepest wins: the first node of the chain
// that has child v is delta's.
inline void bias_row_host(const BiasView& m, int s, int32_t* gain, int32_t* next) {
  for (int v = 0; v < m.V; ++v) {
    gain[v] = m.root_gain[v];
    if (next) next[v] = m.root_next[v];
  }
  int32_t chain[BIAS_MAX_LEN];
  const int n = bias_chain(m, s, chain);
  for (int i = n - 1; i >= 0; --i) {
    const BiasNode nd = m.node[chain[i]];
    for (int q = nd.child_off; q < nd.child_off + nd.child_cnt; ++q) {
      gain[m.ctok[q]] = bias_gain_of(m, m.cnext[q]);
      if (next) next[m.ctok[q]] = m.cnext[q];
    }
  }
}

// one sentence y[0..l): full, tail and the final state
CASR_BIAS_HD inline void bias_sentence(const BiasView& m, const int32_t* y, int l, int32_t* full, int32_t* tail,
                                       int32_t* state) {
  int s = 0, C = 0;
  for (int j = 0; j < l; ++j) bias_advance(m, y[j], &s, &C);
  *full = C;
  *tail = m.node[s].tail;
  *state = s;
}

// ---------------------------------------------------------------- the builder (host)
enum { BIAS_OK = 0, BIAS_ERR_ARG = 1, BIAS_ERR_UNSUPPORTED = 4 };  // casr.h's CASR_OK / CASR_ERR_*

struct BiasTables {
  int V = 0;
  std::vector<BiasNode> node;
  std::vector<int32_t> ctok, cnext, root_next, root_gain;
  BiasView view() const {
    return BiasView{V, (int)node.size(), node.data(), ctok.data(), cnext.data(), root_next.data(), root_gain.data()};
  }
};

// tokens: the phrases back to back, lens [P], boost [P]
inline int bias_build(int V, int P, const int32_t* tokens, const int32_t* lens, const int32_t* boost, BiasTables* out,
                      std::string* why) {
  auto bad = [&](int code, const std::string& s) {
    if (why) *why = s;
    return code;
  };
  if (V < 1) return bad(BIAS_ERR_ARG, "vocab " + std::to_string(V) + " < 1");
  if (P < 0 || (P > 0 && (!tokens || !lens || !boost))) return bad(BIAS_ERR_ARG, "n_phrases < 0 or a NULL array");
  long long total = 0;
  for (int p = 0; p < P; ++p) {
    if (lens[p] < 1 || lens[p] > BIAS_MAX_LEN)
      return bad(BIAS_ERR_ARG, "phrase " + std::to_string(p) + " has length " + std::to_string(lens[p]) +
                                   " outside [1, " + std::to_string(BIAS_MAX_LEN) + "]");
    if (boost[p] < 1 || boost[p] > BIAS_MAX_BOOST)
      return bad(BIAS_ERR_ARG, "phrase " + std::to_string(p) + " has boost " + std::to_string(boost[p]) +
                                   " outside [1, " + std::to_string(BIAS_MAX_BOOST) + "]");
    total += lens[p];
    if (total > BIAS_MAX_TOKENS)
      return bad(BIAS_ERR_UNSUPPORTED, "more than " + std::to_string(BIAS_MAX_TOKENS) + " tokens in the phrases");
  }
  // the trie; own[u]: n_p b_p of the phrase ending at u (0: none), thru[u]: the largest boost among
  // the phrases longer than depth(u) that pass through u
  std::vector<std::map<int32_t, int32_t>> kids(1);
  std::vector<int32_t> depth(1, 0), own(1, 0), thru(1, 0);
  size_t at = 0;
  for (int p = 0; p < P; ++p) {
    int u = 0;
    for (int j = 0; j < lens[p]; ++j) {
      const int32_t t = tokens[at + j];
      if (t < 0 || t >= V)
        return bad(BIAS_ERR_ARG, "phrase " + std::to_string(p) + " has id " + std::to_string(t) + " outside [0, " +
                                     std::to_string(V) + ")");
      if (boost[p] > thru[u]) thru[u] = boost[p];
      auto it = kids[u].find(t);
      if (it == kids[u].end()) {
        const int32_t nu = (int32_t)kids.size();
        kids[u].emplace(t, nu);
        kids.emplace_back();
        depth.push_back(depth[u] + 1);
        own.push_back(0);
        thru.push_back(0);
        u = nu;
      } else {
        u = it->second;
      }
    }
    if (own[u]) return bad(BIAS_ERR_ARG, "phrase " + std::to_string(p) + " is a duplicate");
    own[u] = lens[p] * boost[p];
    at += lens[p];
  }
  const int N = (int)kids.size();
  BiasTables& t = *out;
  t.V = V;
  t.node.assign(N, BiasNode{0, 0, 0, 0, 0, 0});
  t.ctok.clear();
  t.cnext.clear();
  // breadth first: a node's fail link is shallower, so it is final when the node is reached
  std::vector<int32_t> order(1, 0);
  order.reserve(N);
  for (size_t h = 0; h < order.size(); ++h) {
    const int u = order[h];
    BiasNode& nd = t.node[u];
    nd.depth = depth[u];
    nd.out_sum = own[u] + (u ? t.node[nd.fail].out_sum : 0);
    const int here = depth[u] * thru[u], up = u ? t.node[nd.fail].tail : 0;
    nd.tail = here > up ? here : up;
    for (const auto& kv : kids[u]) {
      const int c = kv.second;
      int f = 0;  // fail(c): delta(fail(u), token) over the finished shallower nodes
      if (u) {
        int w = nd.fail;
        for (;;) {
          auto it = kids[w].find(kv.first);
          if (it != kids[w].end()) {
            f = it->second;
            break;
          }
          if (!w) break;
          w = t.node[w].fail;
        }
      }
      t.node[c].fail = f;
      order.push_back(c);
    }
  }
  for (int u = 0; u < N; ++u) {
    t.node[u].child_off = (int32_t)t.ctok.size();
    t.node[u].child_cnt = (int32_t)kids[u].size();
    for (const auto& kv : kids[u]) {  // (a map: ascending in token)
      t.ctok.push_back(kv.first);
      t.cnext.push_back(kv.second);
    }
  }
  t.root_next.assign(V, 0);
  t.root_gain.assign(V, 0);
  for (const auto& kv : kids[0]) {
    t.root_next[kv.first] = kv.second;
    t.root_gain[kv.first] = t.node[kv.second].out_sum + t.node[kv.second].tail;
  }
  return BIAS_OK;
}

}  // namespace casr
