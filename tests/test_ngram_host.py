"""The backoff n-gram LM on the host (include/casr.h casr_lm_create / casr_lm_score_host,
casr/ngram.py): a hand-derived known-answer file, bitwise comparison with the independent reference
(tests/ngram_ref.py) on random models of every order, the table's edge cases, every refusal, the ARPA
reader, and the unchanged host second pass consuming the new object.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import ngram_ref as R
from casr import lib as L
from casr.ngram import NgramLM, read_arpa
from casr.results import second_pass_arrays

HERE = os.path.dirname(os.path.abspath(__file__))
TINY = os.path.join(HERE, "golden", "tiny_3gram.arpa")
V = 5004


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_known_answers_of_the_tiny_3gram():
    """tests/golden/tiny_3gram.arpa over the ASR words a = 0, b = 1, c = 2, d = 3 (d has no unigram),
    derived by hand from the definition (t(w | ctx); bo = backoff):

      "a b"            t(a|<s>) = P(<s> a) = -0.5;  t(b|<s> a) = P(<s> a b) = -0.25 (trigram hit);
                       t(</s>|a b) = P(a b </s>) = -0.0625                            q = -0.8125
      "a b c"          -0.5, -0.25, then t(c|a b): no trigram, P(b c) = -0.375 + bo(a b) = -0.375
                       -> -0.75 (bigram hit, one backoff);  t(</s>|b c): no trigram, no bigram,
                       P(</s>) = -1.5 + bo(c) = -1.0 + bo(b c) = 0 -> -2.5 (unigram, two backoffs)
                                                                                      q = -4.0
      "a c"            -0.5;  t(c|<s> a) = P(c) -1.75 + bo(a) -0.5 + bo(<s> a) -0.25 = -2.5;
                       t(</s>|a c) = -1.5 + bo(c) -1.0, the context (a c) is absent -> -2.5
                                                                                      q = -5.5
      "a zzz", "a d"   an OOV word, and an ASR id without a unigram, score as <unk>: -0.5;
                       t(<unk>|<s> a) = -2.0 - 0.5 - 0.25 = -2.75;  t(</s>|a <unk>) = -1.5 + bo(<unk>)
                       -0.25, (a <unk>) absent -> -1.75                               q = -5.0
      "c a b"          t(c|<s>) = -1.75 + bo(<s>) -0.5 = -2.25;  t(a|<s> c) = P(c a) = -1.125, (<s> c)
                       absent;  t(b|c a) = P(a b) -0.625 + bo(c a) -2.0 = -2.625;  -0.0625
                                                                                      q = -6.0625
      ""               t(</s>|<s>) = P(</s>) -1.5 + bo(<s>) -0.5                      q = -2.0
      bos=False "a b"  t(a|) = P(a) = -0.75;  t(b|a) = P(a b) = -0.625;  -0.0625      q = -1.4375
      bos=False ""     P(</s>)                                                        q = -1.5
    """
    lm = NgramLM(TINY, {"a": 0, "b": 1, "c": 2, "d": 3}, 4)
    assert lm.order == 3
    want = {"a b": -0.8125, "a b c": -4.0, "a c": -5.5, "a zzz": -5.0, "a d": -5.0, "c a b": -6.0625, "": -2.0,
            "  a\tb ": -0.8125}
    for s, q in want.items():
        assert lm.score(s, bos=True) == q, s
        assert lm.score(s) == q, s
    assert lm.score("a b", bos=False) == -1.4375
    assert lm.score("", bos=False) == -1.5
    # the reference reads the same answers out of the same file
    secs = read_arpa(TINY)
    ids = {"a": 0, "b": 1, "c": 2, "<s>": 4, "</s>": 5, "<unk>": 6}
    ref = R.RefLM(3, 4, [{tuple(ids[w] for w in g): (p[i], b[i]) for i, g in enumerate(gr)} for gr, p, b in secs])
    assert ref.sentence([0, 1, 2]) == np.float32(-4.0) and ref.sentence([0, 3]) == np.float32(-5.0)


def _sentences(order, seed):
    grams = R.random_model(order, V, seed)
    tokens, lens = R.sentences_from(grams, V, 500, 40, seed + 1)
    return grams, tokens, lens


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_host_scores_equal_the_reference_bit_for_bit(order):
    """Random models over V = 5004, 500 sentences (lengths 0, 1, 2, 3 and 40 among them), both bos
    values; the reference counts that every branch of the query was taken."""
    grams, tokens, lens = _sentences(order, 100 + order)
    assert set((0, 1, 2, 3, 40)) <= set(lens.tolist())
    ref = R.RefLM(order, V, grams)
    lm = NgramLM.from_ids(*R.arrays_of(grams), {}, V)
    for bos in (True, False):
        want = np.array([ref.sentence(tokens[i, :lens[i]], bos) for i in range(len(lens))], np.float32)
        got = lm.score_ids(tokens, lens, bos)
        assert np.array_equal(bits(got), bits(want)), (order, bos)
    for key in ref.expected_branches():
        assert ref.branches[key] > 0, (order, key)
    # .score through words: the same bits as the id rows
    w2i = {f"w{i}": i for i in range(V)}
    lm2 = NgramLM.from_ids(*R.arrays_of(grams), w2i, V)
    for i in (0, 1, 4, 5, 6, 7):
        s = " ".join(f"w{t}" for t in tokens[i, :lens[i]])
        assert np.float32(lm2.score(s)) == ref.sentence(tokens[i, :lens[i]], True)


def _create(order, vocab, ids, prob, back, lib=None):
    lib = lib or L.load()
    count = np.array([len(a) for a in ids], np.int64)

    def ptrs(arrs):
        out = (ctypes.c_void_p * len(arrs))()
        for i, a in enumerate(arrs):
            out[i] = None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        return out

    lm = ctypes.c_void_p()
    rc = lib.casr_lm_create(-1, order, vocab, count.ctypes.data_as(ctypes.c_void_p), ptrs(ids), ptrs(prob),
                            ptrs(back), ctypes.byref(lm))
    return rc, lm


def _check_model(grams, vocab, seed, n=200, Lmax=12):
    order = len(grams)
    ref = R.RefLM(order, vocab, grams)
    lm = NgramLM.from_ids(*R.arrays_of(grams), {}, vocab)
    tokens, lens = R.sentences_from(grams, vocab, n, Lmax, seed)
    want = np.array([ref.sentence(tokens[i, :lens[i]]) for i in range(n)], np.float32)
    assert np.array_equal(bits(lm.score_ids(tokens, lens)), bits(want))


def test_table_edges():
    """One n-gram at an order; a count that is exactly a power of two; 50,000 random 4-grams; the ids
    V - 1, V (<s>), V + 1 (</s>) and V + 2 (<unk>) inside n-grams."""
    f = np.float32
    base = R.random_model(1, V, 7)
    one = base + [{(5, 9): (f(-0.5), f(-0.25))}, {(5, 9, 11): (f(-0.75), f(-0.5))}, {(5, 9, 11, 5): (f(-1.5), f(0))}]
    for g in one[1:]:
        for k in g:
            for i in k:
                one[0].setdefault((i,), (f(-3.0), f(-0.125)))
    _check_model(one, V, 1)
    ref = R.RefLM(4, V, one)
    lm = NgramLM.from_ids(*R.arrays_of(one), {}, V)
    row = np.array([[5, 9, 11, 5]], np.int32)
    assert np.array_equal(bits(lm.score_ids(row, [4])), bits([ref.sentence(row[0])]))
    pow2 = R.random_model(3, V, 8, n_high=1024)
    assert len(pow2[1]) == 1024 and len(pow2[2]) == 1024
    _check_model(pow2, V, 2)
    big = R.random_model(4, V, 9, n_high=50000)
    assert len(big[3]) == 50000
    _check_model(big, V, 3, n=300, Lmax=40)
    # the largest ids in every field of a key
    edge = R.random_model(1, V, 10, uni_ids=[V - 1, V - 2, 0])
    edge += [{(V, V - 1): (f(-0.5), f(-0.25)), (V - 1, V + 2): (f(-0.625), f(-0.5)), (V - 1, V + 1): (f(-0.375), f(0))},
             {(V, V - 1, V - 1): (f(-0.25), f(-1.0)), (V - 1, V - 1, V + 1): (f(-0.125), f(-2.0)),
              (V + 2, V - 1, V + 2): (f(-0.0625), f(-0.5))},
             {(V, V - 1, V - 1, V - 1): (f(-1.0), f(0)), (V - 1, V - 1, V - 1, V + 1): (f(-2.0), f(0)),
              (V - 1, V + 2, V - 1, V + 2): (f(-4.0), f(0))}]
    ref = R.RefLM(4, V, edge)
    lm = NgramLM.from_ids(*R.arrays_of(edge), {}, V)
    rows = np.array([[V - 1, V - 1, V - 1, 0], [V - 1, 7, V - 1, 7], [V - 1, V + 2, V - 1, V + 2], [V - 2, V - 1, 3, 3]],
                    np.int32)
    lens = np.array([3, 4, 4, 2], np.int32)
    want = np.array([ref.sentence(r[:n]) for r, n in zip(rows, lens)], np.float32)
    assert np.array_equal(bits(lm.score_ids(rows, lens)), bits(want))
    assert ref.branches["m", 4] >= 2


def test_refusals():
    lib = L.load()
    f = np.float32
    uni = np.array([[0], [1], [5], [6]], np.int32)  # V = 5: <s> = 5, </s> = 6
    p1, b1 = np.array([-1, -1, -1, -1], f), np.zeros(4, f)
    bi = np.array([[0, 1], [1, 0]], np.int32)
    p2 = np.array([-0.5, -0.25], f)
    ok = lambda *a: _create(*a)[0]
    rc, lm = _create(2, 5, [uni, bi], [p1, p2], [b1, None])
    assert rc == 0 and lm.value
    lib.casr_lm_destroy(lm)
    lib.casr_lm_destroy(None)
    five = [uni, bi, bi[:0].reshape(0, 3), bi[:0].reshape(0, 4), bi[:0].reshape(0, 5)]
    assert ok(5, 5, five, [p1, p2, p2[:0], p2[:0], p2[:0]], [b1] * 5) == 4  # order > 4
    assert b"order" in lib.casr_last_error(None)
    rc, lm = _create(1, 65532, [uni], [p1], [b1])  # V + 3 = 65535 is the last size accepted
    assert rc == 0
    lib.casr_lm_destroy(lm)
    assert ok(1, 65533, [uni], [p1], [b1]) == 4
    assert ok(0, 5, [], [], []) == 1
    dup = np.array([[0, 1], [1, 0], [0, 1]], np.int32)
    assert ok(2, 5, [uni, dup], [p1, np.array([-1, -1, -1], f)], [b1, None]) == 1
    assert b"duplicate" in lib.casr_last_error(None)
    assert ok(1, 5, [np.array([[0], [0]], np.int32)], [p1[:2]], [b1[:2]]) == 1  # duplicate unigram
    for bad in (-1, 8):  # V + 3 = 8 ids
        assert ok(2, 5, [uni, np.array([[0, bad]], np.int32)], [p1, p2[:1]], [b1, None]) == 1
    assert ok(1, 5, [np.array([[8]], np.int32)], [p1[:1]], [b1[:1]]) == 1
    for v in (np.inf, -np.inf, np.nan):
        assert ok(2, 5, [uni, bi], [p1, np.array([v, -1], f)], [b1, None]) == 1
        assert ok(2, 5, [uni, bi], [p1, p2], [np.array([0, v, 0, 0], f), None]) == 1
    assert b"non-finite" in lib.casr_last_error(None)
    assert lib.casr_lm_create(-1, 1, 5, None, None, None, None, None) == 1
    # scoring: NULL arguments and a length past L
    rc, lm = _create(2, 5, [uni, bi], [p1, p2], [b1, None])
    q = np.zeros(1, f)
    tok = np.zeros((1, 2), np.int32)
    ln = np.array([3], np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.casr_lm_score_host(lm, vp(tok), vp(ln), 1, 2, 1, vp(q)) == 1
    assert lib.casr_lm_score_host(None, vp(tok), vp(ln), 1, 2, 1, vp(q)) == 1
    assert lib.casr_lm_score_host(lm, vp(tok), vp(ln), 1, 2, 1, None) == 1
    ln[0] = 2
    assert lib.casr_lm_score_host(lm, vp(tok), vp(ln), 1, 2, 1, vp(q)) == 0
    # a host-only LM is refused by the device entry points before they touch the handle's device
    lib.casr_lm_destroy(lm)


def test_read_arpa_round_trip_and_errors(tmp_path):
    grams = R.random_model(3, 50, 21, n_high=40)
    for sep, col in (("\t", True), (" ", False)):
        path = str(tmp_path / f"m{col}.arpa")
        R.write_arpa(path, grams, 50, sep=sep, backoff_column=col)
        secs = read_arpa(path)
        assert [len(s[0]) for s in secs] == [len(g) for g in grams]
        w2i = {f"w{i}": i for i in range(50)}
        lm = NgramLM(path, w2i, 50)
        ref = R.RefLM(3, 50, grams)
        tokens, lens = R.sentences_from(grams, 50, 100, 10, 5)
        want = np.array([ref.sentence(tokens[i, :lens[i]]) for i in range(100)], np.float32)
        assert np.array_equal(bits(lm.score_ids(tokens, lens)), bits(want))
        # n-grams with a word outside the ASR vocabulary are dropped
        small = NgramLM(path, {f"w{i}": i for i in range(25)}, 25)
        kept = [{k: v for k, v in g.items() if all(i < 25 or i >= 50 for i in k)} for g in grams]
        kept = [{tuple(i if i < 50 else i - 25 for i in k): v for k, v in g.items()} for g in kept]
        ref25 = R.RefLM(3, 25, kept)
        t25 = tokens % 25
        want = np.array([ref25.sentence(t25[i, :lens[i]]) for i in range(100)], np.float32)
        assert np.array_equal(bits(small.score_ids(t25, lens)), bits(want))
    text = open(TINY).read()

    def bad(edit, match):
        p = tmp_path / "bad.arpa"
        p.write_text(edit(text))
        with pytest.raises(ValueError, match=match):
            read_arpa(str(p))

    bad(lambda t: t.replace("ngram 2=5", "ngram 2=6"), r"bad.arpa:\d+: .*2-grams.*has 5")
    bad(lambda t: t.replace("-0.625\ta b\t-0.375", "-0.625\ta\t-0.375\t1\t2"), r"bad.arpa:18: ")
    bad(lambda t: t.replace("-0.625\ta b", "x\ta b"), r"bad.arpa:18: not a number")
    bad(lambda t: t.replace("-0.625\ta b", "-inf\ta b"), r"bad.arpa:18: non-finite")
    bad(lambda t: t.replace("\\end\\", ""), r"no \\end\\")
    bad(lambda t: t.replace("\\3-grams:", "\\4-grams:"), r"bad.arpa:23: section")


class _ScoreOnly:
    def __init__(self, lm):
        self.lm, self.calls = lm, 0

    def score(self, s, bos=True):
        self.calls += 1
        return self.lm.score(s, bos=bos)


def test_second_pass_arrays_consumes_an_ngram_lm():
    """The unchanged host second pass (casr.results.second_pass_arrays) with an NgramLM as lm_model,
    on synthetic record arrays, against the reference's choice."""
    Vs, B, Lm, k = 60, 5, 8, 3
    grams = R.random_model(3, Vs, 33, n_high=300)
    i2w = {i: f"w{i}" for i in range(Vs)}
    lm = NgramLM.from_ids(*R.arrays_of(grams), {w: i for i, w in i2w.items()}, Vs)
    ref = R.RefLM(3, Vs, grams)
    rs = np.random.RandomState(4)
    rt = np.full((B, Lm, k, Lm), -1, np.int32)
    sc = np.zeros((B, Lm, k), np.float32)
    rv = np.zeros((B, Lm, k), np.uint8)
    for b in range(B):
        for l in range(Lm):
            for c in range(k):
                if b != 1 and rs.rand() < (0.5 if b else 0.05):
                    rv[b, l, c] = 1
                    rt[b, l, c, :l] = rs.randint(4, Vs, size=l)
                    sc[b, l, c] = np.float32(-rs.rand() * 3)
    got = second_pass_arrays(rt, sc, rv, i2w, lm, 1.5, 1.5)
    wrapped = second_pass_arrays(rt, sc, rv, i2w, _ScoreOnly(lm), 1.5, 1.5)
    assert got == wrapped and 1 not in got
    changed = 0
    for b in got:
        recs = [(rt[b, l, c, :l].tolist(), float(sc[b, l, c])) for l in range(Lm) for c in range(k) if rv[b, l, c]]
        i, _ = R.second_pass_choice(recs, ref, 1.5, 1.5)
        assert got[b] == recs[i]
        changed += recs[i] != recs[int(np.argmax([s for _, s in recs]))]
    assert changed > 0
