"""The N-best and confusion-network formulas of include/casr.h (casr_posterior_units_host, casr_nbest_host,
casr_confusion*) restated in plain Python over a full D matrix, and the cases the tests share.  Nothing
here is the library's text: the backtrace is casr.h's rule list from (m, n), a cell at a time."""
import math

import numpy as np

EPS, NONE = -1, -2
ONE = 1 << 32
L, K, V = 10, 4, 8          # the seeded recipe: L = 10, k = 4, alphabets of 2..8 symbols
UNITS = (0, 1, 12345, 1 << 31, 1 << 32)


# ---------------------------------------------------------------------------- formulas
def comb(s, q, l, lm_weight, length_weight):
    return (np.float64(np.float32(s)) + np.float64(lm_weight) * np.float64(np.float32(q))) \
        + np.float64(length_weight) * np.float64(l)


def units_of(c, scale):
    """u_i = floor(exp(scale (c_i - c_max)) 2^32), 0 for a NaN."""
    ok = [x for x in c if x == x]
    cmax = max(ok) if ok else float("nan")
    out = []
    for x in c:
        with np.errstate(all="ignore"):
            d = np.float64(x) - np.float64(cmax)
            e = np.float64(scale) * d
        w = float("nan") if e != e else (float("inf") if e > 700 else math.exp(e))
        out.append(0 if w != w else min(max(int(math.floor(w * 4294967296.0)), 0), ONE))
    return out


def nbest_order(c, flat):
    """Positions under the total order: no NaN before a NaN, the larger c, the lower flat index."""
    return sorted(range(len(c)), key=lambda p: (c[p] != c[p], -c[p] if c[p] == c[p] else 0.0, flat[p]))


def votes_of(a, b):
    """One vote per slot of the pivot a (2 len(a) + 1 slots) from the record b."""
    m, n = len(a), len(b)
    D = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(m + 1):
        D[i][0] = i
    for j in range(n + 1):
        D[0][j] = j
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            D[i][j] = D[i - 1][j - 1] if a[i - 1] == b[j - 1] else 1 + min(D[i - 1][j - 1], D[i - 1][j], D[i][j - 1])
    v = [EPS] * (2 * m + 1)
    i, j = m, n
    while i > 0 or j > 0:
        if i > 0 and j > 0 and (a[i - 1] == b[j - 1] or D[i][j] == D[i - 1][j - 1] + 1):
            v[2 * i - 1] = b[j - 1]
            i, j = i - 1, j - 1
        elif i > 0 and D[i][j] == D[i - 1][j] + 1:
            v[2 * i - 1] = EPS
            i -= 1
        else:
            v[2 * i] = b[j - 1]  # a later (smaller j) insert into the same gap overwrites
            j -= 1
    return v


def clean(t, vocab):
    return t if 0 <= t < vocab else 0


def records_of(rt, rv, b):
    """(flat indices, token lists) of utterance b's valid records in (step, rank) order."""
    k = rt.shape[2]
    flat = [i for i in range(rt.shape[1] * k) if rv[b].reshape(-1)[i]]
    return flat, [rt[b, i // k, i % k, :i // k].tolist() for i in flat]


def confusion(rt, rv, ru, pivot, vocab, M):
    """The outputs of casr_confusion_host as a dict of arrays, and ``full``: per utterance a list, per slot
    the dict token -> mass over ALL tokens."""
    B, Lr, k = rt.shape[:3]
    S = 2 * Lr + 1
    out = dict(n_slots=np.zeros(B, np.int32), slot_token=np.full((B, S, M), NONE, np.int32),
               slot_mass=np.zeros((B, S, M), np.int64), pivot_mass=np.zeros((B, Lr), np.int64),
               total=np.zeros(B, np.int64))
    full = []
    for b in range(B):
        flat, toks = records_of(rt, rv, b)
        toks = [[clean(t, vocab) for t in r] for r in toks]
        u = [min(max(int(ru[b].reshape(-1)[i]), 0), ONE) for i in flat]
        out["total"][b] = sum(u)
        pv = int(pivot[b])
        if pv not in flat:
            full.append([])
            continue
        a = toks[flat.index(pv)]
        votes = [votes_of(a, r) for r in toks]
        out["n_slots"][b] = 2 * len(a) + 1
        slots = []
        for s in range(2 * len(a) + 1):
            mass = {}
            for p in range(len(flat)):
                mass[votes[p][s]] = mass.get(votes[p][s], 0) + u[p]
            slots.append(mass)
            top = sorted(((t, w) for t, w in mass.items() if w > 0), key=lambda e: (-e[1], e[0]))[:M]
            for r, (t, w) in enumerate(top):
                out["slot_token"][b, s, r] = t
                out["slot_mass"][b, s, r] = w
            if s & 1:
                out["pivot_mass"][b, s >> 1] = mass.get(a[s >> 1], 0)
        full.append(slots)
    return out, full


def nbest(rt, rs, rv, rl, N, lm_weight, length_weight):
    B, Lr, k = rt.shape[:3]
    out = dict(index=np.full((B, N), -1, np.int32), tokens=np.full((B, N, Lr), -1, np.int32),
               length=np.zeros((B, N), np.int32), comb=np.zeros((B, N), np.float64))
    for b in range(B):
        flat, toks = records_of(rt, rv, b)
        c = [comb(rs[b].reshape(-1)[i], 0.0 if rl is None else rl[b].reshape(-1)[i], i // k, lm_weight, length_weight)
             for i in flat]
        for r, p in enumerate(nbest_order(c, flat)[:N]):
            out["index"][b, r] = flat[p]
            out["length"][b, r] = len(toks[p])
            out["tokens"][b, r, :len(toks[p])] = toks[p]
            out["comb"][b, r] = c[p]
    return out


def posterior_units(rs, rv, rl, scale, lm_weight, length_weight):
    B, Lr, k = rs.shape
    unit = np.zeros((B, Lr, k), np.int64)
    for b in range(B):
        flat = [i for i in range(Lr * k) if rv[b].reshape(-1)[i]]
        c = [comb(rs[b].reshape(-1)[i], 0.0 if rl is None else rl[b].reshape(-1)[i], i // k, lm_weight, length_weight)
             for i in flat]
        for i, u in zip(flat, units_of(c, scale)):
            unit[b].reshape(-1)[i] = u
    return unit


# ---------------------------------------------------------------------------- cases
def _empty(B):
    return (np.full((B, L, K, L), -1, np.int32), np.zeros((B, L, K), np.uint8), np.zeros((B, L, K), np.int64),
            np.full(B, -1, np.int32))


def _put(rt, rv, ru, b, step, rank, toks, unit):
    assert len(toks) == step
    rt[b, step, rank, :step] = toks
    rv[b, step, rank] = 1
    ru[b, step, rank] = unit


def seeded_cases(n=200, seed=2024):
    """The recipe: an alphabet of 2..8 symbols, a record valid with probability 0.3, units from UNITS, a
    random valid pivot (-1 where no record is valid).  One utterance per case."""
    rs = np.random.RandomState(seed)
    rt, rv, ru, pv = _empty(n)
    for b in range(n):
        alphabet = 2 + b % 7
        for step in range(L):
            for rank in range(K):
                if rs.rand() < 0.3:
                    _put(rt, rv, ru, b, step, rank, rs.randint(0, alphabet, size=step), UNITS[rs.randint(len(UNITS))])
        flat = np.flatnonzero(rv[b].reshape(-1))
        if flat.size:
            pv[b] = flat[rs.randint(flat.size)]
    return rt, rv, ru, pv


HAND = ["no record", "one record", "empty pivot", "pivot -1", "pivot on an invalid record", "token outside [0, V)",
        "pivot index past the tree"]


def hand_cases():
    """One utterance per entry of HAND, in that order."""
    rt, rv, ru, pv = _empty(len(HAND))
    _put(rt, rv, ru, 1, 3, 1, [1, 2, 3], 12345)
    pv[1] = 3 * K + 1
    _put(rt, rv, ru, 2, 0, 2, [], ONE)          # the pivot: no token, S = 1
    _put(rt, rv, ru, 2, 2, 0, [4, 5], 7)
    _put(rt, rv, ru, 2, 1, 1, [6], 9)
    pv[2] = 2
    for b in (3, 4, 6):
        _put(rt, rv, ru, b, 2, 0, [1, 1], 5)
        _put(rt, rv, ru, b, 3, 3, [1, 2, 1], ONE)
    pv[3], pv[4], pv[6] = -1, 2 * K + 1, L * K
    _put(rt, rv, ru, 5, 3, 0, [1, V, 2], ONE)    # V and -5 count as 0, the alignment included
    _put(rt, rv, ru, 5, 3, 1, [1, 0, 2], 3)
    _put(rt, rv, ru, 5, 4, 2, [1, -5, 2, 2], 1 << 31)
    pv[5] = 3 * K
    return rt, rv, ru, pv


def scored_cases(n=60, seed=77):
    """Records with scores for the N-best order and the units: ties, a NaN and infinities among them."""
    rs = np.random.RandomState(seed)
    rt, rv, _, _ = _empty(n)
    sc = np.zeros((n, L, K), np.float32)
    lm = np.zeros((n, L, K), np.float32)
    for b in range(n):
        for step in range(L):
            for rank in range(K):
                if rs.rand() < (0.0 if b == 0 else 0.4):
                    rt[b, step, rank, :step] = rs.randint(0, V, size=step)
                    rv[b, step, rank] = 1
                    sc[b, step, rank] = np.float32(-rs.randint(0, 6)) if b % 3 == 0 else np.float32(-10 * rs.rand())
                    lm[b, step, rank] = np.float32(-rs.randint(0, 3)) if b % 3 == 0 else np.float32(-5 * rs.rand())
        if b % 10 == 5:
            sc[b][rv[b] > 0] = np.where(rs.rand(int(rv[b].sum())) < 0.2, np.float32("nan"), sc[b][rv[b] > 0])
        if b % 10 == 7 and rv[b].any():
            i = np.flatnonzero(rv[b].reshape(-1))[0]
            sc[b].reshape(-1)[i] = -np.inf
    return rt, sc, rv, lm


def slot_stats(full):
    """(>= 2 entries, gap slots with a non-EPS entry, odd slots with an EPS entry, > 4 distinct tokens, a mass
    tie, slots) over the reference's full masses."""
    two = gap = odd = many = tie = slots = 0
    for utt in full:
        for s, mass in enumerate(utt):
            pos = {t: w for t, w in mass.items() if w > 0}
            slots += 1
            two += len(pos) >= 2
            gap += s % 2 == 0 and any(t != EPS for t in pos)
            odd += s % 2 == 1 and EPS in pos
            many += len(pos) > 4
            tie += len(set(pos.values())) < len(pos)
    return two, gap, odd, many, tie, slots
