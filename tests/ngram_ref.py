"""Yardstick of the backoff n-gram LM (include/casr.h casr_lm_*), written from the definition and
sharing no code with the product: dicts keyed by id tuples, np.float32 adds in the stated order,
Python floats for the second pass's combination.  Also an ARPA writer and a seeded random-model
generator for the CPU and GPU tests.

LM ids: 0 .. V - 1 the ASR token ids, V = <s>, V + 1 = </s>, V + 2 = <unk>."""
from collections import Counter

import numpy as np

F = np.float32


class RefLM:
    """grams[n - 1]: {id tuple of length n: (prob, backoff)} for n = 1 .. order."""

    def __init__(self, order, V, grams):
        self.order, self.V = order, V
        self.grams = [dict(g) for g in grams]
        assert len(self.grams) == order
        self.bos, self.eos, self.unk = V, V + 1, V + 2
        if (self.unk,) not in self.grams[0]:
            self.grams[0][(self.unk,)] = (F(-100.0), F(0.0))
        self.branches = Counter()

    def lm_id(self, t):
        return t if 0 <= t < self.V + 3 and (t,) in self.grams[0] else self.unk

    def term(self, ctx, w):
        """ctx: the LM ids before w, oldest first (any length); w an LM id.  Both already lm_id'd."""
        ctx = tuple(ctx)[-(self.order - 1):] if self.order > 1 else ()
        m = max(n for n in range(1, len(ctx) + 2) if ctx[len(ctx) - (n - 1):] + (w,) in self.grams[n - 1])
        p = F(self.grams[m - 1][ctx[len(ctx) - (m - 1):] + (w,)][0])
        self.branches["m", m] += 1
        for j in range(m, len(ctx) + 1):
            c = ctx[len(ctx) - j:]
            if c in self.grams[j - 1]:
                p = F(p + F(self.grams[j - 1][c][1]))
                self.branches["bo_hit", j] += 1
            else:
                self.branches["bo_miss", j] += 1
        return p

    def sentence(self, tokens, bos=True):
        ids = [self.lm_id(int(t)) for t in tokens]
        hist = [self.lm_id(self.bos)] if bos else []
        q = None
        for w in ids + [self.lm_id(self.eos)]:
            t = self.term(hist, w)
            q = t if q is None else F(q + t)
            hist.append(w)
        return q

    def expected_branches(self):
        """Every branch class a model of this order has."""
        N = self.order
        return ([("m", m) for m in range(1, N + 1)] + [("bo_hit", j) for j in range(1, N)] +
                [("bo_miss", j) for j in range(2, N)])


def second_pass_choice(records, lm, lm_weight, length_weight):
    """records: [(tokens, logp)] of one utterance in (step, rank) order.  Returns (index, [q]): comb =
    (logp + lm_w q) + len_w len on Python floats, first maximum (np.argmax: the first NaN if any)."""
    qs = [lm.sentence(t, bos=True) for t, _ in records]
    comb = [(float(s) + lm_weight * float(q)) + length_weight * float(len(t)) for (t, s), q in zip(records, qs)]
    return int(np.argmax(comb)), qs


# ---------------------------------------------------------------------------- models and files
def word_of(i, V, int2word=None):
    if i >= V:
        return ("<s>", "</s>", "<unk>")[i - V]
    return int2word[i] if int2word is not None else f"w{i}"


def random_model(order, V, seed, n_uni=None, n_high=2000, seeds=(), with_unk=True, uni_ids=None, p_lo=-6.0,
                 b_lo=-2.0):
    """A seeded random model: unigrams for n_uni of the V ASR ids (default 3/4 of them; the rest
    score as <unk>) plus <s>, </s> and (with_unk) <unk>; per higher order n_high random n-grams over
    ids that have unigrams, half of them extensions of an n-gram of the order below (so backoff
    contexts exist), plus every tuple of ``seeds`` of that length.  Values: prob in [p_lo, -0.1],
    backoff in [b_lo, 0] with one in eight exactly 0, as float32."""
    rs = np.random.RandomState(seed)
    n_uni = (3 * V) // 4 if n_uni is None else n_uni
    if uni_ids is None:
        uni_ids = rs.choice(V, size=min(n_uni, V), replace=False)
    ids1 = sorted(int(i) for i in uni_ids) + [V, V + 1] + ([V + 2] if with_unk else [])

    def values(n):
        p = (p_lo + (-0.1 - p_lo) * rs.rand(n)).astype(F)
        b = (b_lo * rs.rand(n)).astype(F)
        b[rs.rand(n) < 0.125] = 0.0
        return p, b

    p, b = values(len(ids1))
    grams = [{(i,): (p[e], b[e]) for e, i in enumerate(ids1)}]
    pool = np.array([i for i in ids1 if i != V + 1])  # </s> only ever ends an n-gram
    lastp = np.array([i for i in ids1 if i != V])     # <s> only ever starts one
    for n in range(2, order + 1):
        keys = set(tuple(int(x) for x in s) for s in seeds if len(s) == n)
        prev = list(grams[n - 2].keys())
        want = len(keys) + n_high
        while len(keys) < want:
            if rs.rand() < 0.5 and prev:
                g = prev[rs.randint(len(prev))]
                if g[-1] == V + 1:
                    continue
                keys.add(g + (int(lastp[rs.randint(len(lastp))]),))
            else:
                keys.add(tuple(int(x) for x in pool[rs.randint(len(pool), size=n - 1)]) +
                         (int(lastp[rs.randint(len(lastp))]),))
        keys = sorted(keys)
        p, b = values(len(keys))
        if n == order:
            b[:] = 0.0
        grams.append({g: (p[e], b[e]) for e, g in enumerate(keys)})
    return grams


def arrays_of(grams):
    """casr_lm_create's arguments: per order (ids int32 [count, n], prob, backoff)."""
    ids = [np.array(sorted(g.keys()), np.int32).reshape(-1, n) for n, g in enumerate(grams, 1)]
    prob = [np.array([g[tuple(k)][0] for k in a.tolist()], F) for a, g in zip(ids, grams)]
    back = [np.array([g[tuple(k)][1] for k in a.tolist()], F) for a, g in zip(ids, grams)]
    return ids, prob, back


def write_arpa(path, grams, V, int2word=None, sep="\t", backoff_column=True):
    """The model as an ARPA file.  repr(float(x)) of a float32 reads back to the same float32.  The
    top order's lines have no backoff column; lower orders' omit it where it is 0 unless
    backoff_column."""
    order = len(grams)
    with open(path, "w", encoding="utf-8") as f:
        f.write("\\data\\\n")
        for n, g in enumerate(grams, 1):
            f.write(f"ngram {n}={len(g)}\n")
        for n, g in enumerate(grams, 1):
            f.write(f"\n\\{n}-grams:\n")
            for k in sorted(g.keys()):
                p, b = g[k]
                fields = [repr(float(p))] + [" ".join(word_of(i, V, int2word) for i in k)]
                if n < order and (backoff_column or float(b) != 0.0):
                    fields.append(repr(float(b)))
                f.write(sep.join(fields) + "\n")
        f.write("\n\\end\\\n")


def sentences_from(grams, V, n, L, seed, lengths=(0, 1, 2, 3, 40)):
    """n sentences of at most L ASR ids: the fixed lengths first, then random ones; half are chains of
    the model's own n-grams (ASR-id parts), half uniformly random ids (some without a unigram)."""
    rs = np.random.RandomState(seed)
    pools = [[k for k in g.keys() if all(i < V for i in k)] for g in grams]
    tokens = np.zeros((n, L), np.int32)
    lens = np.zeros(n, np.int32)
    for i in range(n):
        ln = min(L, lengths[i] if i < len(lengths) else int(rs.randint(0, L + 1)))
        if i % 2 == 0:
            row = []
            while len(row) < ln:
                pool = pools[rs.randint(len(pools))]
                if pool:
                    row.extend(pool[rs.randint(len(pool))])
                if rs.rand() < 0.15:
                    row.append(int(rs.randint(V)))
            row = row[:ln]
        else:
            row = rs.randint(V, size=ln).tolist()
        tokens[i, :ln] = row
        lens[i] = ln
    return tokens, lens
