"""The backtrace of casr_edit_align (include/casr.h) restated in plain Python: casr.results.edit_ops'
table and its rules in its order, returning also the two maps.  Nothing here comes from the C++."""
import numpy as np

import edit_ref as R

RULES = ("match", "replace", "delete", "insert")


def align(a, b, order=RULES, branches=None):
    """(dist, (insert, delete, replace), b_of_a [len(a)], a_of_b [len(b)]) of the script turning a into
    b: at (i, j) the first rule of ``order`` that holds (edit_ops' order by default); a diagonal step
    through cell (i - 1, j - 1) sets b_of_a[i - 1] = j - 1 and a_of_b[j - 1] = i - 1, everything else
    stays -1.  ``branches`` counts the rules taken, the moves along an edge of the table apart."""
    d = R.dp_matrix(a, b)
    i, j = len(a), len(b)
    ins = dele = rep = 0
    b_of_a, a_of_b = [-1] * i, [-1] * j

    def holds(rule):
        if rule == "match":
            return i > 0 and j > 0 and a[i - 1] == b[j - 1] and d[i, j] == d[i - 1, j - 1]
        if rule == "replace":
            return i > 0 and j > 0 and a[i - 1] != b[j - 1] and d[i, j] == d[i - 1, j - 1] + 1
        if rule == "delete":
            return i > 0 and d[i, j] == d[i - 1, j] + 1 and not (j > 0 and a[i - 1] == b[j - 1])
        return j > 0 and d[i, j] == d[i, j - 1] + 1 and not (i > 0 and a[i - 1] == b[j - 1])

    while i > 0 or j > 0:
        rule = next(r for r in order if holds(r))
        if branches is not None:
            key = rule if (i > 0 and j > 0) else rule + "_edge"
            branches[key] = branches.get(key, 0) + 1
        if rule in ("match", "replace"):
            rep += rule == "replace"
            i, j = i - 1, j - 1
            b_of_a[i], a_of_b[j] = j, i
        elif rule == "delete":
            dele += 1
            i -= 1
        else:
            ins += 1
            j -= 1
    return int(d[len(a), len(b)]), (ins, dele, rep), b_of_a, a_of_b


def reference(pairs, La=None, Lb=None):
    """dict of dist [n], ops [n, 3], b_of_a [n, La], a_of_b [n, Lb] as the entries lay them out."""
    La = max([1] + [len(p) for p, _ in pairs]) if La is None else La
    Lb = max([1] + [len(r) for _, r in pairs]) if Lb is None else Lb
    n = len(pairs)
    out = dict(dist=np.zeros(n, np.int32), ops=np.zeros((n, 3), np.int32), b_of_a=np.full((n, La), -1, np.int32),
               a_of_b=np.full((n, Lb), -1, np.int32))
    for k, (p, r) in enumerate(pairs):
        dist, ops, ba, ab = align(p, r)
        out["dist"][k], out["ops"][k] = dist, ops
        out["b_of_a"][k, :len(p)] = ba
        out["a_of_b"][k, :len(r)] = ab
    return out


def same(got, want):
    return all(np.array_equal(np.asarray(got[k]), want[k]) for k in ("dist", "ops", "b_of_a", "a_of_b"))


def edited_copy(rs, length, alphabet, edits):
    """(copy, row): a row of ``length`` symbols below ``alphabet`` and a copy with ``edits`` random edits."""
    ref = rs.randint(0, alphabet, size=length).astype(np.int32)
    pred = ref.tolist()
    for _ in range(edits):
        op = rs.randint(3)
        if op == 0 and pred:
            pred[rs.randint(len(pred))] = int(rs.randint(alphabet))
        elif op == 1 and pred:
            del pred[rs.randint(len(pred))]
        else:
            pred.insert(rs.randint(len(pred) + 1), int(rs.randint(alphabet)))
    return pred, ref.tolist()
