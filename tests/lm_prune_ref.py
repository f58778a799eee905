"""Relative-entropy pruning of a backoff n-gram LM, restated in Python from the definition in
include/casr.h (casr_lm_prune): dictionaries in place of hash tables, numpy float64 scalars in place of
C doubles, the same operations in the same order.  ``exp10`` and ``log`` repeat csrc/lm_prune_plan.h's
lmp_exp10 and lmp_log operation by operation, so the host entry, the kernels and this file give the
same bits.  Test infrastructure: nothing here is fast."""
import math

import numpy as np

F = np.float64
INF = F(np.inf)
NAN = F(np.nan)


def _h(s):
    return F(float.fromhex(s))


_EXP = [_h(s) for s in ("0x1.6124613a86d09p-33", "0x1.1eed8eff8d898p-29", "0x1.ae64567f544e4p-26",
                        "0x1.27e4fb7789f5cp-22", "0x1.71de3a556c734p-19", "0x1.a01a01a01a01ap-16",
                        "0x1.a01a01a01a01ap-13", "0x1.6c16c16c16c17p-10", "0x1.1111111111111p-7",
                        "0x1.5555555555555p-5", "0x1.5555555555555p-3", "0x1p-1", "0x1p0", "0x1p0")]
_LOG = [_h(s) for s in ("0x1.642c8590b2164p-5", "0x1.8618618618618p-5", "0x1.af286bca1af28p-5",
                        "0x1.e1e1e1e1e1e1ep-5", "0x1.1111111111111p-4", "0x1.3b13b13b13b14p-4",
                        "0x1.745d1745d1746p-4", "0x1.c71c71c71c71cp-4", "0x1.2492492492492p-3",
                        "0x1.999999999999ap-3", "0x1.5555555555555p-2", "0x1p0")]
_LOG2_10, _LOG10_2_HI, _LOG10_2_LO = _h("0x1.a934f0979a371p+1"), _h("0x1.3441350800000p-2"), _h("0x1.f79fef311f12bp-34")
_LN10, _LN2_HI, _LN2_LO = _h("0x1.26bb1bbb55516p+1"), _h("0x1.62e42fec00000p-1"), _h("0x1.d1cf79abc9e3bp-32")
_SQRT2 = _h("0x1.6a09e667f3bcdp+0")


def exp10(x):
    x = F(x)
    if x != x:
        return x
    if x > 308.0:
        return INF
    if x < -307.0:
        return F(0.0)
    t = x * _LOG2_10
    k = int(t - F(0.5)) if t < 0.0 else int(t + F(0.5))
    kd = F(k)
    r = (x - kd * _LOG10_2_HI) - kd * _LOG10_2_LO
    z = r * _LN10
    p = _EXP[0]
    for c in _EXP[1:]:
        p = p * z + c
    return p * F(math.ldexp(1.0, k))


def log(x):
    x = F(x)
    if not x > 0.0:
        return NAN
    if x == INF:
        return x
    e = 0
    u = int(x.view(np.uint64))
    if u < 0x0010000000000000:
        x = x * F(2.0 ** 54)
        u = int(x.view(np.uint64))
        e = -54
    e += (u >> 52) - 1023
    m = np.uint64((u & 0x000fffffffffffff) | 0x3ff0000000000000).view(np.float64)
    if m > _SQRT2:
        m = m * F(0.5)
        e += 1
    f = m - F(1.0)
    s = f / (F(2.0) + f)
    z = s * s
    p = _LOG[0]
    for c in _LOG[1:]:
        p = p * z + c
    ed = F(e)
    return ed * _LN2_HI + ((F(2.0) * s) * p + ed * _LN2_LO)


def sum64(xs):
    """The one association of a sum; an entry None keeps its place and adds nothing."""
    s = [F(0.0)] * 64
    for i, x in enumerate(xs):
        if x is not None:
            s[i % 64] = s[i % 64] + x
    d = 32
    while d >= 1:
        for l in range(d):
            s[l] = s[l] + s[l + d]
        d //= 2
    return s[0]


def _pos_finite(x):
    return bool(x > 0.0 and x < INF)


class Model:
    """ids[n-1] [count, n] LM ids, prob[n-1], backoff[n-1] float32 (casr_lm_create's arguments)."""

    def __init__(self, ids, prob, backoff, V):
        self.V, self.N = int(V), len(ids)
        V = self.V
        self.given = [[tuple(int(t) for t in g) for g in np.asarray(a).reshape(-1, n)] for n, a in enumerate(ids, 1)]
        self.prob = [dict(zip(g, np.asarray(p, np.float32))) for g, p in zip(self.given, prob)]
        self.backoff = [dict(zip(g, np.asarray(b, np.float32))) for g, b in zip(self.given, backoff)]
        for g in self.backoff[self.N - 1]:
            self.backoff[self.N - 1][g] = np.float32(0.0)  # (the top order's is never read)
        self.has_uni = {g[0] for g in self.given[0]} | {V + 2}
        # the table's unigrams: <unk> defaults to (-100, 0)
        uni_p, uni_b = dict(self.prob[0]), dict(self.backoff[0])
        uni_p.setdefault((V + 2,), np.float32(-100.0))
        uni_b.setdefault((V + 2,), np.float32(0.0))
        for t in range(V + 3):
            if t not in self.has_uni:
                uni_p[(t,)], uni_b[(t,)] = uni_p[(V + 2,)], uni_b[(V + 2,)]
        self.P = [{g: exp10(p) for g, p in uni_p.items()}] + [{g: exp10(p) for g, p in d.items()} for d in self.prob[1:]]
        self.B = [{g: exp10(b) for g, b in uni_b.items()}] + [{g: exp10(b) for g, b in d.items()} for d in self.backoff[1:]]
        self.succ = [None, None] + [dict() for _ in range(2, self.N + 1)]
        for n in range(2, self.N + 1):
            for g in self.given[n - 1]:
                if self.reachable(g):
                    self.succ[n].setdefault(g[:-1], []).append(g[-1])
            for ws in self.succ[n].values():
                ws.sort()

    def reachable(self, g):
        return all(t in self.has_uni for t in g)

    def query(self, c, w, keep=None, Bn=None):
        """Q(w | c), c oldest first.  keep / Bn: the pruned model."""
        B = self.B if Bn is None else Bn
        p, m = self.P[0][(w,)], 1
        for j in range(1, len(c) + 1):
            g = c[len(c) - j:] + (w,)
            if g in self.P[j] and (keep is None or keep[j][g]):
                p, m = self.P[j][g], j + 1
        for j in range(m, len(c) + 1):
            h = c[len(c) - j:]
            if j == 1 or (h in self.P[j - 1] and (keep is None or keep[j - 1][h])):
                p = p * B[j - 1][h]
        return p

    def ph(self, h):
        ph = F(1.0)
        for i in range(len(h)):
            f = self.P[0][(self.V + 1,)] if h[i] == self.V else self.query(h[:i], h[i])
            ph = ph * f
        return ph


def handmade(V=136, seed=11):
    """(ids, prob, backoff) of an order-3 model made by hand for the edges: bigram contexts holding
    exactly 130, 65, 64 and 1 successors (the words 0, 1, 2, 3), trigram contexts holding 65 and 1, no
    <unk> unigram, and the word V - 1 without a unigram inside a bigram, a trigram whose prefix it so
    protects, and a bigram context.  Every context gives its successors 0.8 in all and backs off with
    the rest, so the model is close to normalised and the decisions are spread around any theta."""
    rng = np.random.default_rng(seed)
    words = list(range(132)) + [V, V + 1]  # (ids 132 .. V - 1 and <unk> have no unigram)
    p1 = rng.random(len(words)) + 0.05
    p1[-2] = 0.0
    p1 /= p1.sum()
    uni = {w: p for w, p in zip(words, p1)}
    grams = [dict(), dict(), dict()]
    for w in words:
        grams[0][(w,)] = [np.log10(uni[w]) if w != V else -99.0, 0.0]

    def fill(h, succ, lower):
        r = rng.random(len(succ)) ** 3 + 1e-4
        r = 0.8 * r / r.sum()
        for w, p in zip(succ, r):
            grams[len(h)][h + (w,)] = [np.log10(p), 0.0]
        grams[len(h) - 1][h][1] = np.log10(0.2 / (1.0 - sum(lower(w) for w in succ)))

    for h, k in ((0, 130), (1, 65), (2, 64), (3, 1), (V, 7)):
        fill((h,), [V + 1] + list(range(1, k)) if k > 1 else [5], lambda w: uni[w])
    p2 = lambda h, w: 10.0 ** grams[1][(h, w)][0] if (h, w) in grams[1] else 10.0 ** grams[0][(h,)][1] * uni[w]  # noqa: E731
    fill((0, 1), [V + 1] + list(range(64)), lambda w: p2(1, w))
    fill((0, 2), [9], lambda w: p2(2, w))
    fill((V, 1), [0, 3, 7], lambda w: p2(1, w))
    grams[2][(4, 5, 6)] = [-1.0, 0.0]  # (its context (4, 5) is no bigram of the model)
    grams[1][(5, V - 1)] = [-2.0, -0.1]
    grams[1][(V - 1, 2)] = [-1.5, -0.2]
    grams[2][(0, 3, V - 1)] = [-1.25, 0.0]  # passes through and protects (0, 3)
    ids = [np.array(sorted(g), np.int32).reshape(-1, n + 1) for n, g in enumerate(grams)]
    prob = [np.array([g[tuple(k)][0] for k in a.tolist()], np.float32) for a, g in zip(ids, grams)]
    back = [np.array([g[tuple(k)][1] for k in a.tolist()], np.float32) for a, g in zip(ids, grams)]
    return ids, prob, back


def delta(ph, p, q, a, num, den):
    np_, dq = num + p, den + q
    if not (_pos_finite(p) and _pos_finite(q) and _pos_finite(a) and _pos_finite(np_) and _pos_finite(dq)):
        return INF
    a1 = np_ / dq
    la1 = log(a1)
    t0 = p * ((log(q) + la1) - log(p))
    t1 = num * (la1 - log(a))
    return -ph * (t0 + t1)


def backoff(sp, sq):
    num, den = F(1.0) - sp, F(1.0) - sq
    if not (_pos_finite(num) and _pos_finite(den)):
        return F(0.0)
    b = num / den
    return b if _pos_finite(b) else F(0.0)


def prune(m, theta):
    """dict(tau, removed_any, keys, delta, kept, b64, n_degenerate, count_out, n_protected): per order
    (index n - 1) over the n-grams as given in ascending tuple order; b64 the output backoff in float64
    (B', or exp10 of the stored one where it was not renewed)."""
    with np.errstate(all="ignore"):
        return _prune(m, theta)


def _prune(m, theta):
    N, one = m.N, F(1.0)
    tau = log(one + F(theta))
    keys = [sorted(g) for g in m.given]
    dl = [{g: NAN for g in k} for k in keys]
    keep = [{g: True for g in k} for k in keys]
    protect = [set() for _ in range(N)]
    for n in range(3, N + 1):
        for g in keys[n - 1]:
            if not m.reachable(g) and g[:-1] in m.P[n - 2]:
                protect[n - 2].add(g[:-1])
    removed = 0
    for n in range(N, 1, -1):
        for h, ws in m.succ[n].items():
            ps = [m.P[n - 1][h + (w,)] for w in ws]
            qs = [m.query(h[1:], w) for w in ws]
            num, den = one - sum64(ps), one - sum64(qs)
            a = m.B[n - 2][h] if h in m.P[n - 2] else one
            ph = m.ph(h)
            any_kept = False
            for w, p, q in zip(ws, ps, qs):
                g = h + (w,)
                d = delta(ph, p, q, a, num, den)
                k = g in protect[n - 1] or not bool(d < tau)
                dl[n - 1][g], keep[n - 1][g] = d, k
                any_kept = any_kept or k
                removed += not k
            if any_kept and n >= 3 and h in m.P[n - 2]:
                protect[n - 2].add(h)
    Bn = [{g: one for g in d} for d in m.P]
    if removed:
        for n in range(2, N + 1):
            for h, ws in m.succ[n].items():
                if h not in m.P[n - 2] or not (n == 2 or keep[n - 2][h]):
                    continue
                ps = [m.P[n - 1][h + (w,)] if keep[n - 1][h + (w,)] else None for w in ws]
                qs = [m.query(h[1:], w, keep, Bn) if keep[n - 1][h + (w,)] else None for w in ws]
                Bn[n - 2][h] = backoff(sum64(ps), sum64(qs))
    out = dict(tau=tau, removed_any=bool(removed), keys=keys, delta=[], kept=[], b64=[], n_degenerate=0,
               count_out=[], n_protected=[])
    for n in range(1, N + 1):
        d = np.array([dl[n - 1][g] for g in keys[n - 1]], np.float64)
        k = np.array([keep[n - 1][g] for g in keys[n - 1]], bool)
        b64 = np.array([exp10(m.backoff[n - 1][g]) for g in keys[n - 1]], np.float64)
        if removed:
            for i, g in enumerate(keys[n - 1]):
                if n == N:
                    b64[i] = one
                elif n == 1 or d[i] == d[i]:
                    b64[i] = Bn[n - 1][g]
                    out["n_degenerate"] += int(k[i] and not b64[i] > 0.0)
        out["delta"].append(d)
        out["kept"].append(k)
        out["b64"].append(b64)
        out["count_out"].append(int(k.sum()))
        out["n_protected"].append(int((k & (d < tau)).sum()))
    return out
