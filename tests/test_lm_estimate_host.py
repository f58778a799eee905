"""casr_lm_estimate_host (include/casr.h) against the Python restatement tests/lm_estimate_ref.py.  No GPU.

Exact: the n-gram sets, raw and adjusted counts, fallback flags and |W|.  Bit for bit: the discounts and
the float64 p and gamma (the same IEEE operations in the same order).  The stored float32 logs: within
1 float32 ulp of numpy.log10 of the restatement's float64 (libm and numpy may differ in the last bit of
the float64 logarithm, which moves a float32 rounding by at most one step).  Then the LM query on a real
distribution for the first time: the terms of every word after a context sum to 1."""
import ctypes
import itertools

import numpy as np
import pytest

import lm_estimate_ref as E
import ngram_ref as R
from casr import lib as L
from casr import ngram
from casr.ngram import NgramLM


def _ulps(got, want64):
    """float32 steps between got and float32(want64); every value is <= 0 (a log10 of a p or gamma <= 1)."""
    w = np.asarray(want64, np.float64).astype(np.float32)
    return np.abs(np.asarray(got, np.float32).view(np.int32).astype(np.int64) - w.view(np.int32).astype(np.int64))


def _against_ref(sents, order, V):
    ref = E.Estimate(sents, order, V)
    tokens, offsets = ngram.flatten(sents, V)
    est = ngram.estimate_host(tokens, offsets, order, V)
    assert est.order == order and est.positions == ref.positions == len(tokens) + len(sents)
    assert est.n_types == ref.W
    assert est.fallback.tolist() == list(ref.fallback)
    assert np.array_equal(est.discounts.view(np.uint64), np.array(ref.D, np.float64).view(np.uint64))
    for n in range(1, order + 1):
        keys = ref.keys(n)
        assert [tuple(r) for r in est.ids[n - 1].tolist()] == keys, n  # the set, in ascending key order
        assert est.raw[n - 1].tolist() == [ref.raw[n - 1][g] for g in keys], n
        assert est.adjusted[n - 1].tolist() == [ref.adj[n - 1][g] for g in keys], n
        p = np.array([ref.p[n - 1].get(g, 0.0) for g in keys], np.float64)  # (0 for the unigram <s>)
        gm = np.array([ref.gamma_of(n, g) for g in keys], np.float64)
        assert np.array_equal(est.p[n - 1].view(np.uint64), p.view(np.uint64)), n
        assert np.array_equal(est.gamma[n - 1].view(np.uint64), gm.view(np.uint64)), n
        bos = np.array([g == (V,) for g in keys], bool)
        assert np.all(est.prob[n - 1][bos] == np.float32(-99.0))
        assert _ulps(est.prob[n - 1][~bos], np.log10(p[~bos])).max(initial=0) <= 1, n
        ctx = gm > 0.0
        assert np.all(est.backoff[n - 1][~ctx] == 0.0)
        assert _ulps(est.backoff[n - 1][ctx], np.log10(gm[ctx])).max(initial=0) <= 1, n
    for n in range(order):  # t_{n,k}, recounted from the adjusted counts the entry reports (without the unigram <s>)
        skip = (est.ids[n][:, 0] == V) if n == 0 else np.zeros(len(est.ids[n]), bool)
        assert [int(np.sum((est.adjusted[n] == k) & ~skip)) for k in (1, 2, 3, 4)] == ref.t[n]
    return est, ref


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_zipf_corpus_uses_estimated_discounts_at_every_order(order):
    est, ref = _against_ref(E.zipf_corpus(), order, 120)
    assert est.positions == 6971
    assert not est.fallback.any()  # so D = k - (k + 1) Y t_{k+1} / t_k is what the test exercises
    assert np.all(est.discounts > 0) and np.all(est.discounts <= [1.0, 2.0, 3.0])


def test_vocabulary_of_four_falls_back_where_it_must():
    est, ref = _against_ref(E.small_corpus(4, 40, 6, 1), 4, 4)
    # order 1: six types, t = (0, 0, 0, 1); order 4: D_4(3) = 3 - 4 Y t4 / t3 < 0
    assert est.fallback.tolist() == [True, False, False, True]
    assert ref.t[0][0] == 0 and ref.t[3][2] > 0
    assert np.array_equal(est.discounts[0], E.FALLBACK) and np.array_equal(est.discounts[3], E.FALLBACK)


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_short_sentences_only(order):
    """Lengths 0, 1 and N - 1: windows that are all padding, or that just reach from <s> to </s>."""
    rng = np.random.default_rng(order)
    sents = [[int(x) for x in rng.integers(0, 9, size=ln)] for ln in [0, 1, max(order - 1, 0)] * 15]
    _against_ref(sents, order, 9)


def test_one_sentence_and_one_empty_sentence():
    _against_ref([[3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5]], 4, 10)
    est, _ = _against_ref([[]], 4, 10)
    assert [len(a) for a in est.ids] == [3, 1, 0, 0] and est.positions == 1


def test_one_repeated_token():
    est, _ = _against_ref([[7] * 300, [7] * 2, [7]], 4, 10)
    assert est.raw[3].max() == 297 and est.fallback.all()


def test_ids_zero_and_last():
    V = 5003
    est, _ = _against_ref(E.small_corpus(V, 60, 9, 4, ids=[0, 1, V - 1]), 4, V)
    assert est.ids[0][0, 0] == 0 and (V - 1) in est.ids[0][:, 0]


def test_unk_in_the_input_and_absent_from_it():
    V = 12
    with_unk = E.small_corpus(V, 80, 8, 6, unk=0.08)
    assert any(V + 2 in s for s in with_unk)
    est, ref = _against_ref(with_unk, 3, V)
    assert ref.raw[0][(V + 2,)] > 0
    without = [[t for t in s if t != V + 2] for s in with_unk]
    est, ref = _against_ref(without, 3, V)
    i = est.ids[0][:, 0].tolist().index(V + 2)  # always a unigram: a = 0, u = 0, p = gamma_1 / |W|
    assert est.raw[0][i] == 0 and est.adjusted[0][i] == 0 and est.p[0][i] == ref.gamma0 / ref.W > 0


def test_refusals():
    lib = L.load()
    tok = np.array([0, 1, 2, 3], np.int32)

    def call(order, vocab, tokens, offsets, n=None):
        offsets = None if offsets is None else np.asarray(offsets, np.int64)
        out = ctypes.c_void_p()
        rc = lib.casr_lm_estimate_host(order, vocab, None if tokens is None else tokens.ctypes.data_as(ctypes.c_void_p),
                                       None if offsets is None else offsets.ctypes.data_as(ctypes.c_void_p),
                                       len(offsets) - 1 if n is None else n, ctypes.byref(out))
        assert (rc == 0) == bool(out.value)
        if rc == 0:
            lib.casr_lm_estimate_destroy(out)
        else:
            assert lib.casr_last_error(None)
        return L.STATUS[rc]

    assert call(2, 10, tok, [0, 4]) == "CASR_OK"
    for order in (0, 5, -1):
        assert call(order, 10, tok, [0, 4]) == "CASR_ERR_ARG"
    assert call(2, 10, tok, [0], n=0) == "CASR_ERR_ARG"
    assert call(2, 10, tok, [0, 4], n=-1) == "CASR_ERR_ARG"
    assert call(2, 10, None, [0, 4]) == "CASR_ERR_ARG"
    assert call(2, 10, tok, None, n=1) == "CASR_ERR_ARG"
    assert lib.casr_lm_estimate_host(2, 10, tok.ctypes.data_as(ctypes.c_void_p), tok.ctypes.data_as(ctypes.c_void_p), 1,
                                     None) == 1
    assert call(2, 10, tok, [1, 4]) == "CASR_ERR_ARG"      # does not start at 0
    assert call(2, 10, tok, [0, 3, 2, 4]) == "CASR_ERR_ARG"  # descends
    for bad in (10, 11, 13, -1):  # <s>, </s>, one past <unk>, negative
        t = tok.copy()
        t[2] = bad
        assert call(2, 10, t, [0, 4]) == "CASR_ERR_ARG", bad
    t = tok.copy()
    t[2] = 12  # <unk> is a word
    assert call(2, 10, t, [0, 4]) == "CASR_OK"
    assert call(2, 65532, tok, [0, 4]) == "CASR_OK"
    assert call(2, 65533, tok, [0, 4]) == "CASR_ERR_UNSUPPORTED"  # V + 3 > 65,535
    assert call(2, 10, tok, [0, 1 << 28]) == "CASR_ERR_UNSUPPORTED"  # P = 2^28 + 1 (nothing is read)
    with pytest.raises(L.CasrError, match="CASR_ERR_ARG"):
        ngram.estimate([[1, 2]], 5, 10)


def test_workspace_plan():
    assert ngram.workspace_bytes(4, 1) > 0
    big = ngram.workspace_bytes(4, 1 << 28)
    # 2^29 slots per order 2..4: 16 (slot) + 8 (p) bytes, and below the top order 16 (context) + 8 (gamma)
    assert big >= (1 << 29) * (24 * 3 + 24 * 2) and big < (1 << 29) * (48 * 4)
    assert ngram.workspace_bytes(4, (1 << 28) + 1) == -1
    assert ngram.workspace_bytes(0, 100) == -1 and ngram.workspace_bytes(5, 100) == -1 and ngram.workspace_bytes(2, 0) == -1
    assert ngram.workspace_bytes(1, 1000) < ngram.workspace_bytes(2, 1000) < ngram.workspace_bytes(4, 1000)


# ---------------------------------------------------------------------------- the query on a distribution
V6 = 6


@pytest.fixture(scope="module")
def model6():
    """V = 6, N = 4: the corpus holds ids 0..4 and <unk>; id 5 never occurs, so it has no unigram and its
    column of NgramLM.terms is the term of <unk>."""
    sents = E.small_corpus(V6, 120, 7, 5, unk=0.05, ids=range(5))
    assert any(V6 + 2 in s for s in sents) and not any(5 in s for s in sents)
    lm = ngram.estimate(sents, 4, V6)
    yield lm, sents
    lm.close()


def _mass(lm, ctx_oldest_first):
    """sum over W (ids 0..4, <unk> through the unseen id 5, </s>) of 10^term after the context: float32
    terms summed in float64."""
    c = list(ctx_oldest_first)[::-1]
    row = np.array([c + [0] * (3 - len(c))], np.int32)
    words = lm.terms(row, [len(c)])[0].astype(np.float64)
    eos = float(lm.terms(row, [len(c)], eos=0)[0, 0])
    return float(np.sum(10.0 ** words) + 10.0 ** eos)


def test_terms_sum_to_one_after_every_context(model6):
    """|W| = 8 terms of relative error 2^-24 ln 10 |log10 p| with |log10 p| < 3: under 4e-6 in all."""
    lm, _ = model6
    est = lm.estimate
    assert est.n_types == 7 and lm.terms(np.zeros((1, 3), np.int32), [0]).min() > -3.0
    seen = [()]
    for n in range(3):
        seen += [tuple(r) for r in est.ids[n][est.gamma[n] > 0.0].tolist()]
    assert len(seen) > 50 and any(V6 + 2 in c for c in seen) and any(len(c) == 3 for c in seen)
    known = set(seen)
    unseen = [c for c in itertools.product(range(5), repeat=3) if c not in known][:2]
    assert len(unseen) == 2
    for c in seen + unseen + [(V6 + 2, V6 + 2, 1), (V6, V6 + 2)]:
        assert abs(_mass(lm, c) - 1.0) < 1e-5, c


def test_scores_equal_the_reference_query_over_the_exported_model(model6):
    lm, _ = model6
    est = lm.estimate
    grams = [{tuple(g): (p, b) for g, p, b in zip(est.ids[n].tolist(), est.prob[n], est.backoff[n])} for n in range(4)]
    ref = R.RefLM(4, V6, grams)
    held = E.small_corpus(V6, 64, 12, 77, unk=0.1)  # (id 5 occurs here: scored as <unk>)
    lens = np.array([len(s) for s in held], np.int32)
    tokens = np.zeros((64, 12), np.int32)
    for i, s in enumerate(held):
        tokens[i, :len(s)] = s
    for bos in (True, False):
        want = np.array([ref.sentence(s, bos) for s in held], np.float32)
        assert np.array_equal(lm.score_ids(tokens, lens, bos).view(np.uint32), want.view(np.uint32))
    # a distribution over sentences too: no sentence is more likely than certain
    assert np.all(lm.score_ids(tokens, lens) < 0)


def test_arpa_round_trip(tmp_path, model6):
    """write_arpa keeps the n-grams and their order and 7 significant digits of every value: what comes
    back is float32(float('%.7g' % x)), within 6e-7 |x| of x; 0 and -99 come back exactly."""
    lm, sents = model6
    i2w = [f"w{i}" for i in range(V6)]
    w2i = {w: i for i, w in enumerate(i2w)}
    path = str(tmp_path / "lm.arpa")
    lm.write_arpa(path, i2w)
    back = NgramLM(path, w2i, V6)
    try:
        assert back.order == 4
        for n in range(4):
            assert np.array_equal(back._arrays[0][n], lm._arrays[0][n])
            for a, b in ((lm._arrays[1][n], back._arrays[1][n]), (lm._arrays[2][n], back._arrays[2][n])):
                want = np.array([np.float32(float("%.7g" % float(x))) for x in a], np.float32)
                assert np.array_equal(b.view(np.uint32), want.view(np.uint32))
                assert np.all(np.abs(b.astype(np.float64) - a.astype(np.float64)) <= 6e-7 * np.abs(a.astype(np.float64)))
                assert np.array_equal(b[a == 0], a[a == 0]) and np.array_equal(b[a == -99], a[a == -99])
        assert np.all(back._arrays[2][3] == 0)  # the top order has no backoff column
        text = open(path, encoding="utf-8").read()
        assert "\\4-grams:" in text and "<s>" in text and "<unk>" in text
        tokens, offsets = ngram.flatten(sents[:20], V6)
        rows = np.zeros((20, 8), np.int32)
        lens = np.diff(offsets).astype(np.int32)
        for i, s in enumerate(sents[:20]):
            rows[i, :len(s)] = s
        assert np.allclose(back.score_ids(rows, lens), lm.score_ids(rows, lens), rtol=1e-5, atol=0)
    finally:
        back.close()


def test_estimate_from_strings_carries_discounts(tmp_path):
    w2i = {ch: i for i, ch in enumerate("abcdefgh")}
    lm = ngram.estimate(["abc abd", "", "hz", "abcabc"], 3, 8, word2int=w2i)  # z is outside: <unk>
    try:
        assert lm.order == 3 and lm.discounts.shape == (3, 3) and lm.fallback.shape == (3,)
        assert lm.estimate.raw[0][lm.estimate.ids[0][:, 0].tolist().index(10)] == 1
        assert lm.ids_of("a b z") == [0, 1, 10] and lm.score("a b c") < 0
    finally:
        lm.close()


def test_library_exports_the_estimate_entries():
    lib = L.load()
    for name in L.EXPORTS:
        if name.startswith("casr_lm_estimate"):
            assert hasattr(lib, name)
    assert lib.casr_lm_estimate_combine(1) in (0, 1)
