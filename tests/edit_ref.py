"""The MBR formulas of include/casr.h (casr_mbr_host, casr_beam_mbr) restated in numpy, and helpers that
make cases for the edit-distance tests.  Distances and operation counts are not restated: they come
from casr.results.edit_distance / edit_ops, the Python the device replaces."""
import numpy as np

from casr.results import edit_distance, edit_ops

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


# ---------------------------------------------------------------------------- pairs
def edited_pair(rs, length, alphabet, edits):
    """A reference of ``length`` symbols below ``alphabet`` and a copy with ``edits`` random edits."""
    ref = rs.randint(0, alphabet, size=length).tolist()
    pred = list(ref)
    for _ in range(edits):
        op = rs.randint(3)
        if op == 0 and pred:
            pred[rs.randint(len(pred))] = int(rs.randint(alphabet))
        elif op == 1 and pred:
            del pred[rs.randint(len(pred))]
        else:
            pred.insert(rs.randint(len(pred) + 1), int(rs.randint(alphabet)))
    return pred, ref


def seeded_pairs(n, seed, max_len=70, alphabets=(2, 5, 300)):
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        alphabet = alphabets[i % len(alphabets)]
        length = int(rs.randint(0, max_len - 9))
        out.append(edited_pair(rs, length, alphabet, int(rs.randint(0, 10))))
    return [(p[:max_len], r) for p, r in out]


def hand_pairs():
    """Lengths (0,0), (0,1), (1,0), (1,1); equal and disjoint rows; the strip boundary 63/64/65 against
    1/64/65; the extreme symbols."""
    rs = np.random.RandomState(5)
    pairs = [([], []), ([], [7]), ([7], []), ([7], [7]), ([7], [8]),
             (list(range(30)), list(range(30))), (list(range(30)), list(range(100, 125))),
             ([-1, INT32_MIN, INT32_MAX, 0], [INT32_MAX, -1, INT32_MIN, 0, -1]),
             ([INT32_MIN] * 5, [INT32_MIN] * 3 + [INT32_MAX])]
    for la in (63, 64, 65):
        for lb in (1, 64, 65):
            a = rs.randint(0, 4, size=la).tolist()
            b = (a + rs.randint(0, 4, size=70).tolist())[:lb]
            if lb > 1:
                b[lb // 2] = 9
            pairs.append((a, b))
    return pairs


def pad_pairs(pairs, La=None, Lb=None):
    """(a [n, La], a_len, b [n, Lb], b_len) int32, rows padded with a symbol no row holds."""
    La = max([1] + [len(p) for p, _ in pairs]) if La is None else La
    Lb = max([1] + [len(r) for _, r in pairs]) if Lb is None else Lb
    a = np.full((len(pairs), La), -77, np.int32)
    b = np.full((len(pairs), Lb), -78, np.int32)
    for i, (p, r) in enumerate(pairs):
        a[i, :len(p)] = p
        b[i, :len(r)] = r
    return (a, np.array([len(p) for p, _ in pairs], np.int32), b, np.array([len(r) for _, r in pairs], np.int32))


def reference(pairs):
    """(dist [n], ops [n, 3]) of casr.results.edit_distance / edit_ops."""
    dist = np.array([edit_distance(p, r) for p, r in pairs], np.int32)
    ops = np.array([edit_ops(p, r) for p, r in pairs], np.int32).reshape(len(pairs), 3)
    return dist, ops


def dp_matrix(a, b):
    m, n = len(a), len(b)
    d = np.zeros((m + 1, n + 1), np.int64)
    d[:, 0] = np.arange(m + 1)
    d[0, :] = np.arange(n + 1)
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            d[i, j] = d[i - 1, j - 1] if a[i - 1] == b[j - 1] else 1 + min(d[i - 1, j - 1], d[i - 1, j], d[i, j - 1])
    return d


def backtrace(a, b, order=("match", "replace", "delete", "insert"), branches=None):
    """(insert, delete, replace) under a tie order of the backtrace's rules (edit_ops' is the
    default); ``branches`` counts which rule was taken, boundary moves apart."""
    d = dp_matrix(a, b)
    i, j, cnt = len(a), len(b), dict(insert=0, delete=0, replace=0)

    def ok(rule):
        if rule == "match":
            return i > 0 and j > 0 and a[i - 1] == b[j - 1]
        if rule == "replace":
            return i > 0 and j > 0 and a[i - 1] != b[j - 1] and d[i, j] == d[i - 1, j - 1] + 1
        if rule == "delete":
            return i > 0 and d[i, j] == d[i - 1, j] + 1 and not (j > 0 and a[i - 1] == b[j - 1])
        return j > 0 and d[i, j] == d[i, j - 1] + 1 and not (i > 0 and a[i - 1] == b[j - 1])

    while i > 0 or j > 0:
        rule = next(r for r in order if ok(r))
        if branches is not None:
            key = rule if (i > 0 and j > 0) else rule + "_edge"
            branches[key] = branches.get(key, 0) + 1
        if rule != "match":
            cnt[rule] += 1
        if rule in ("match", "replace"):
            i, j = i - 1, j - 1
        elif rule == "delete":
            i -= 1
        else:
            j -= 1
    return cnt["insert"], cnt["delete"], cnt["replace"]


# ---------------------------------------------------------------------------- MBR
def mbr_utterance(tokens, scores, lms, scale, lm_weight, length_weight):
    """The formulas of casr.h on one utterance's records (token lists in (step, rank) order, float32
    scores and LM scores): (choice or -1, risk [n] float64, c [n] float64, dist [n, n])."""
    n = len(tokens)
    if n == 0:
        return -1, np.zeros(0), np.zeros(0), np.zeros((0, 0), np.int64)
    s = np.asarray(scores, np.float32).astype(np.float64)
    q = np.asarray(lms, np.float32).astype(np.float64)
    l = np.array([len(t) for t in tokens], np.float64)
    c = (s + np.float64(lm_weight) * q) + np.float64(length_weight) * l
    cmax = np.fmax.reduce(c)
    w = np.exp(np.float64(scale) * (c - cmax))
    dist = np.zeros((n, n), np.int64)
    for i in range(n):
        for j in range(i):
            dist[i, j] = dist[j, i] = edit_distance(tokens[i], tokens[j])
    risk = np.zeros(n, np.float64)
    for i in range(n):
        r = np.float64(0.0)
        for j in range(n):
            r = r + w[j] * np.float64(dist[i, j])
        risk[i] = r
    best = -1
    for i in range(n):  # no NaN beats a NaN, then the smaller risk, then the lower index
        if best < 0 or (np.isnan(risk[best]) and not np.isnan(risk[i])) or risk[i] < risk[best]:
            best = i
    return best, risk, c, dist


def near_tie(risk, best, rel=1e-12):
    """Another record's risk is within ``rel`` relative of the minimum but not bit-equal to it: the
    choice may then legitimately differ where exp differs in its last bit."""
    r = np.asarray(risk, np.float64)
    if best < 0 or np.isnan(r[best]):
        return False
    close = np.abs(r - r[best]) <= rel * max(abs(r[best]), np.finfo(np.float64).tiny)
    return bool(np.any(close & (r != r[best])))


def random_record_set(rs, n, L, k, alphabet=6, equal_scores=False):
    """One utterance's arrays as casr_beam_records lays them out: (rec_tokens [L, k, L], rec_score
    [L, k] float32, rec_valid [L, k] uint8, rec_lm [L, k] float32) with n valid records (at most k per
    step, a record at step l holding l tokens) that are edits of one another, so distances are small
    and ties frequent."""
    rt = np.full((L, k, L), -1, np.int32)
    sc = np.zeros((L, k), np.float32)
    va = np.zeros((L, k), np.uint8)
    lm = np.zeros((L, k), np.float32)
    slots = [(l, c) for l in range(L) for c in range(k)]
    pick = sorted(rs.choice(len(slots), size=n, replace=False).tolist()) if n else []
    base = rs.randint(0, alphabet, size=L)
    for s in pick:
        l, c = slots[s]
        t = base[:l].copy()
        for _ in range(int(rs.randint(0, 4))):
            if l:
                t[rs.randint(l)] = rs.randint(alphabet)
        rt[l, c, :l] = t
        va[l, c] = 1
        sc[l, c] = np.float32(0.0 if equal_scores else -rs.rand() * 6.0)
        lm[l, c] = np.float32(0.0 if equal_scores else -rs.rand() * 20.0)
    return rt, sc, va, lm


def records_of(rt, sc, va, lm, k):
    """The valid records of one utterance in (step, rank) order: (flat indices, token lists, scores, lms)."""
    flat = np.flatnonzero(va.reshape(-1))
    toks = [rt.reshape(-1, rt.shape[-1])[i, :i // k].tolist() for i in flat]
    return flat, toks, sc.reshape(-1)[flat], lm.reshape(-1)[flat]
