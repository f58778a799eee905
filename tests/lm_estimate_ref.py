"""Yardstick of the Kneser-Ney estimate (include/casr.h casr_lm_estimate*), written from the definition
and sharing no code with the product: Counters and dicts keyed by id tuples, Python floats (IEEE
float64, one operation at a time, never an fma) in the evaluation orders the definition states.  Also
the seeded corpora of the CPU and GPU tests and the normalisation check through ngram_ref.RefLM.

LM ids: 0 .. V - 1 the ASR token ids, V = <s>, V + 1 = </s>, V + 2 = <unk>."""
from collections import Counter

import numpy as np

import ngram_ref as R

F = np.float32
FALLBACK = (0.5, 1.0, 1.5)


def discounts(t):
    """t = (t1, t2, t3, t4) -> ((D1, D2, D3), fallback)."""
    if all(x > 0 for x in t):
        Y = float(t[0]) / (float(t[0]) + 2.0 * float(t[1]))
        D = tuple(float(k) - ((float(k + 1) * Y) * float(t[k])) / float(t[k - 1]) for k in (1, 2, 3))
        if all(0.0 < D[k - 1] <= float(k) for k in (1, 2, 3)):
            return D, False
    return FALLBACK, True


class Estimate:
    """sentences: id lists (ids in [0, V) or V + 2).  Per order n: raw[n-1], adj[n-1] {gram: int}, p[n-1]
    {gram: float} (without the unigram <s>), gamma[n-1] {context gram of order n: gamma_{n+1}}; gamma0
    (the empty context's), D [order][3], fallback [order], t [order][4], W."""

    def __init__(self, sentences, order, V):
        self.order, self.V = N, V = order, V
        bos, eos, unk = V, V + 1, V + 2
        padded = [[bos] + [int(x) for x in s] + [eos] for s in sentences]
        self.positions = sum(len(s) - 1 for s in padded)
        raw = [Counter() for _ in range(N)]
        for s in padded:
            for n in range(1, N + 1):
                for i in range(len(s) - n + 1):
                    raw[n - 1][tuple(s[i:i + n])] += 1
        adj = []
        for n in range(1, N + 1):
            if n == N:
                adj.append(dict(raw[n - 1]))
                continue
            ext = Counter(g[1:] for g in raw[n])
            adj.append({g: (c if g[0] == bos else ext[g]) for g, c in raw[n - 1].items()})
        self.raw, self.adj = [dict(r) for r in raw], adj
        pred = [{g: a for g, a in adj[n].items() if g != (bos,)} for n in range(N)]
        self.t = [[sum(1 for a in pred[n].values() if a == k) for k in (1, 2, 3, 4)] for n in range(N)]
        self.D, self.fallback = zip(*(discounts(t) for t in self.t))
        self.W = len([g for g in raw[0] if g not in ((bos,), (unk,))]) + 1
        self.p, self.gamma = [], []
        for n in range(1, N + 1):
            D = self.D[n - 1]
            S, Nk = Counter(), {}
            for g, a in pred[n - 1].items():
                S[g[:-1]] += a
                Nk.setdefault(g[:-1], [0, 0, 0])[min(a, 3) - 1] += 1
            gam = {c: ((D[0] * float(k[0]) + D[1] * float(k[1])) + D[2] * float(k[2])) / float(S[c]) for c, k in Nk.items()}
            p = {}
            for g, a in pred[n - 1].items():
                u = (float(a) - D[min(a, 3) - 1]) / float(S[g[:-1]])
                if n == 1:
                    p[g] = u + gam[()] / float(self.W)
                else:
                    p[g] = u + gam[g[:-1]] * self.p[n - 2][g[1:]]
            if n == 1:
                self.gamma0 = gam[()]
                if (unk,) not in p:  # never seen: a = 0, u = 0
                    p[(unk,)] = 0.0 + gam[()] / float(self.W)
                    self.raw[0][(unk,)] = 0
                    self.adj[0][(unk,)] = 0
            else:
                self.gamma.append(gam)  # contexts of order n - 1
            self.p.append(p)
        self.gamma.append({})

    def keys(self, n):
        return sorted(self.raw[n - 1])

    def gamma_of(self, n, g):
        """gamma_{n+1}(g) of an n-gram g as a context; 0.0 where nothing follows it."""
        return self.gamma[n - 1].get(g, 0.0) if n < self.order else 0.0

    def stored(self):
        """ngram_ref's grams: per order {gram: (f32 log10 p, f32 log10 gamma or 0)}; <s>: prob -99."""
        out = []
        for n in range(1, self.order + 1):
            d = {}
            for g in self.keys(n):
                gm = self.gamma_of(n, g)
                prob = F(-99.0) if g == (self.V,) else F(np.log10(self.p[n - 1][g]))
                d[g] = (prob, F(np.log10(gm)) if gm > 0.0 else F(0.0))
            out.append(d)
        return out


def normalisation(ref, ctx, words):
    """sum over ``words`` (LM ids) of 10^term after the context (oldest first) through a RefLM; the f32
    terms summed in float64."""
    ctx = [ref.lm_id(int(c)) for c in ctx]
    return float(sum(10.0 ** float(ref.term(ctx, ref.lm_id(int(w)))) for w in words))


# ---------------------------------------------------------------------------- corpora
def split(tokens, lens):
    out, at = [], 0
    for n in lens:
        out.append([int(x) for x in tokens[at:at + int(n)]])
        at += int(n)
    return out


def zipf_corpus(V=120, n=800, max_len=15, exponent=1.5, seed=3):
    """n sentences of 0..max_len tokens from a Zipf law over V ids (numpy.random.default_rng(seed))."""
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, V + 1) ** exponent
    w /= w.sum()
    return [[int(x) for x in rng.choice(V, size=int(rng.integers(0, max_len + 1)), p=w)] for _ in range(n)]


def small_corpus(V, n, max_len, seed, unk=0.0, ids=None):
    """n sentences of 0..max_len ids drawn uniformly from ``ids`` (default all of [0, V)), each replaced
    by <unk> with probability ``unk``."""
    rng = np.random.default_rng(seed)
    ids = np.arange(V) if ids is None else np.asarray(ids)
    lens = rng.integers(0, max_len + 1, size=n)
    tokens = ids[rng.integers(0, len(ids), size=int(lens.sum()))]
    tokens = np.where(rng.random(tokens.shape) < unk, V + 2, tokens)
    return split(tokens, lens)
