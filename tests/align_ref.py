"""The monotone attention path of include/casr.h (casr_align_path*) restated in numpy: the weight (a),
the recurrence (b) as the plain sequential double loop over a full D matrix, the backtrack (c) and
the edges (d); plus the case generators the host, sanitizer and GPU tests share.  Nothing here is
vectorised along a row: the stay move is taken cell by cell, as the definition says."""
import numpy as np

FLOOR = -3072
DIAG, VERT, STAY = 0, 1, 2


def quant(x):
    """(a): float32 array -> int32 weights."""
    x = np.asarray(x, np.float32)
    q = (x.view(np.uint32) >> 16).astype(np.int64) - (127 << 7)
    q = np.clip(q, FLOOR, 0)
    with np.errstate(invalid="ignore"):
        q = np.where(x > 0, q, FLOOR)
    return q.astype(np.int32)


def path_one(a, T, n):
    """One utterance: a [L, Tp] float32, T frames, n tokens (both already clamped) ->
    (first, last, peak [L], score, cells) with cells the path as [(l, t)] from the start."""
    L = a.shape[0]
    first, last, peak = (np.full(L, -1, np.int32) for _ in range(3))
    if n == 0 or T == 0:
        return first, last, peak, 0, []
    q = quant(a[:n, :T]).astype(np.int64)
    D = np.zeros((n, T), np.int64)
    mv = np.zeros((n, T), np.int8)
    for l in range(n):
        for t in range(T):
            if l == 0 and t == 0:
                D[0, 0] = q[0, 0]
                continue
            cand = []  # in the tie order: diagonal, vertical, stay
            if l > 0 and t > 0:
                cand.append((D[l - 1, t - 1], DIAG))
            if l > 0:
                cand.append((D[l - 1, t], VERT))
            if t > 0:
                cand.append((D[l, t - 1], STAY))
            best = cand[0]
            for c in cand[1:]:
                if c[0] > best[0]:
                    best = c
            D[l, t] = q[l, t] + best[0]
            mv[l, t] = best[1]
    l, t = n - 1, T - 1
    cells = [(l, t)]
    while (l, t) != (0, 0):
        m = mv[l, t]
        if m == DIAG:
            l, t = l - 1, t - 1
        elif m == VERT:
            l -= 1
        else:
            t -= 1
        cells.append((l, t))
    cells.reverse()
    for l in range(n):
        ts = [t for (ll, t) in cells if ll == l]
        first[l], last[l] = min(ts), max(ts)
        span = q[l, first[l]:last[l] + 1]
        peak[l] = first[l] + int(np.argmax(span))  # (argmax: the first of equal maxima)
    return first, last, peak, int(D[n - 1, T - 1]), cells


def path(align, enc_len, tgt_len):
    """align [L, Tp, B] -> dict(first, last, peak [B, L] int32, path_score [B] int32), lengths clamped (d)."""
    align = np.asarray(align, np.float32)
    L, Tp, B = align.shape
    out = dict(first=np.full((B, L), -1, np.int32), last=np.full((B, L), -1, np.int32),
               peak=np.full((B, L), -1, np.int32), path_score=np.zeros(B, np.int32))
    for b in range(B):
        T, n = min(max(int(enc_len[b]), 0), Tp), min(max(int(tgt_len[b]), 0), L)
        f, la, p, s, _ = path_one(align[:, :, b], T, n)
        out["first"][b], out["last"][b], out["peak"][b], out["path_score"][b] = f, la, p, s
    return out


def check_invariants(align, enc_len, tgt_len, r):
    """The properties every result has (include/casr.h): asserts."""
    L, Tp, B = align.shape
    for b in range(B):
        T, n = min(max(int(enc_len[b]), 0), Tp), min(max(int(tgt_len[b]), 0), L)
        f, la, p = r["first"][b], r["last"][b], r["peak"][b]
        if n == 0 or T == 0:
            assert (f == -1).all() and (la == -1).all() and (p == -1).all() and r["path_score"][b] == 0
            continue
        assert (f[n:] == -1).all() and (la[n:] == -1).all() and (p[n:] == -1).all()
        assert f[0] == 0 and la[n - 1] == T - 1
        assert ((f[:n] <= p[:n]) & (p[:n] <= la[:n])).all()
        for l in range(n - 1):
            assert f[l + 1] in (la[l], la[l] + 1), (b, l)
        q = quant(align[:n, :T, b]).astype(np.int64)
        assert r["path_score"][b] == sum(int(q[l, f[l]:la[l] + 1].sum()) for l in range(n)), b


# ---------------------------------------------------------------------------- generators
def lengths(rs, B, L, Tp):
    """enc_len, tgt_len per utterance, the corners 0, 1, Tp and L among them."""
    enc = rs.randint(1, Tp + 1, size=B)
    tgt = rs.randint(1, L + 1, size=B)
    for i, (e, t) in enumerate([(Tp, L), (1, L), (Tp, 1), (0, L), (Tp, 0), (1, 1)]):
        if i < B and rs.rand() < 0.7:
            enc[(i * 5) % B], tgt[(i * 5) % B] = e, t
    return enc.astype(np.int32), tgt.astype(np.int32)


def softmax_rows(rs, B, L, Tp, sharp=4.0):
    x = rs.randn(L, Tp, B) * sharp
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def constant_rows(rs, B, L, Tp):
    """every cell equal: every tie rule decides"""
    return np.full((L, Tp, B), rs.choice([0.5, 1.0, 0.001, 0.0]), np.float32)


def onehot_rows(rs, B, L, Tp):
    a = np.zeros((L, Tp, B), np.float32)
    for b in range(B):
        a[np.arange(L), rs.randint(0, Tp, size=L), b] = 1.0
    return a


def special_rows(rs, B, L, Tp):
    """0, denormals, NaN, infinities, negatives and values > 1 among ordinary weights"""
    pool = np.array([0.0, -0.0, 1e-40, 1.4e-45, np.nan, -1.0, -np.inf, np.inf, 2.0, 1.0, 0.5, 0.75, 2.0 ** -24,
                     2.0 ** -25, 3e-3, 0.2], np.float32)
    return pool[rs.randint(0, len(pool), size=(L, Tp, B))]


def planted(rs, B, L, Tp):
    """T >= n: spans of >= 1 frame that tile [0, T); alpha = 0.5 on a token's own span and 2^-10
    elsewhere.  Returns (align, enc_len, tgt_len, first, last) with -1 past n."""
    a = np.full((L, Tp, B), 2.0 ** -10, np.float32)
    enc, tgt = np.zeros(B, np.int32), np.zeros(B, np.int32)
    first, last = np.full((B, L), -1, np.int32), np.full((B, L), -1, np.int32)
    for b in range(B):
        n = rs.randint(1, min(L, Tp) + 1)
        T = rs.randint(n, Tp + 1)
        cuts = np.sort(rs.choice(np.arange(1, T), size=n - 1, replace=False)) if n > 1 else np.array([], int)
        edges = np.r_[0, cuts, T]
        for l in range(n):
            a[l, edges[l]:edges[l + 1], b] = 0.5
            first[b, l], last[b, l] = edges[l], edges[l + 1] - 1
        enc[b], tgt[b] = T, n
    return a, enc, tgt, first, last


GENERATORS = (softmax_rows, constant_rows, onehot_rows, special_rows)


def seeded_case(seed, B, L, Tp):
    """(align, enc_len, tgt_len) of one of the generators, by seed."""
    rs = np.random.RandomState(seed)
    gen = GENERATORS[seed % len(GENERATORS)]
    a = gen(rs, B, L, Tp)
    enc, tgt = lengths(rs, B, L, Tp)
    return a, enc, tgt
