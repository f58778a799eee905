"""Term rows of the backoff n-gram LM on the host (include/casr.h casr_lm_terms_host,
NgramLM.terms): every ASR token's term under one context, computed per row from the successor lists,
against the independent per-word reference (tests/ngram_ref.py RefLM.term) bit for bit, and
consistent with the sentence scores casr_lm_score_host gives.  No GPU."""
import numpy as np
import pytest

import ngram_ref as R
from casr.ngram import NgramLM

F = np.float32
V = 5004


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def ref_rows(ref, ctx, nc, eos):
    """RefLM's rows: contexts redirected as the product redirects them (an id outside [0, V + 3) or
    without a unigram is <unk>), nc clamped to [0, order - 1]; RefLM.term wants the oldest first."""
    out = np.empty((len(nc), ref.V), F)
    for i in range(len(nc)):
        n = min(max(int(nc[i]), 0), ref.order - 1)
        c = [ref.lm_id(int(t)) for t in ctx[i, :n]][::-1]
        for v in range(ref.V):
            out[i, v] = ref.term(c, ref.lm_id(ref.eos) if v == eos else ref.lm_id(v))
    return out


def contexts_of(grams, Vn, n, seed):
    """n contexts [n, 3] (nearest first) with nc 0..3 (past the order too: clamped): half are the
    leading words of the model's own n-grams (contexts with successor lists, <s> among them), the
    rest random ids (no list; not n-grams of the model; some without a unigram), plus ids out of range."""
    rs = np.random.RandomState(seed)
    ctx = rs.randint(0, Vn + 3, size=(n, 3)).astype(np.int32)
    nc = rs.randint(0, 4, size=n).astype(np.int32)
    for i in range(0, n, 2):
        g = grams[rs.randint(1, len(grams))] if len(grams) > 1 else None
        if g:
            key = list(g.keys())[rs.randint(len(g))]
            lead = list(key[:-1])[::-1]
            ctx[i, :len(lead)] = lead
            nc[i] = len(lead) if rs.rand() < 0.8 else rs.randint(0, 4)
    ctx[1] = (Vn, 0, 0)  # <s> alone
    nc[1] = 1
    ctx[3] = (Vn + 3, -1, 70000)  # outside [0, V + 3): <unk>
    nc[3] = 3
    nc[5], nc[7] = -2, 9  # clamped
    return ctx, nc


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_term_rows_equal_the_reference_bit_for_bit(order):
    """V = 37 (so a row check of every v is cheap and every word collides with many n-grams) and the
    standard V = 5004 random model; every branch class of the query occurs."""
    for Vn, n_high, n_ctx, seed in ((37, 150, 60, 10 + order), (V, 2000, 10, 20 + order)):
        grams = R.random_model(order, Vn, seed, n_high=n_high)
        ref = R.RefLM(order, Vn, grams)
        lm = NgramLM.from_ids(*R.arrays_of(grams), {}, Vn)
        ctx, nc = contexts_of(grams, Vn, n_ctx, seed + 100)
        eos = 3
        got = lm.terms(ctx, nc, eos)
        assert got.shape == (n_ctx, Vn)
        assert np.array_equal(bits(got), bits(ref_rows(ref, ctx, nc, eos))), (order, Vn)
        none = lm.terms(ctx, nc)  # no eos token: v scores as itself
        want = got.copy()
        want[:, eos] = ref_rows(ref, ctx, nc, -1)[:, eos]
        assert np.array_equal(bits(none), bits(want))
        if Vn == 37:
            for key in ref.expected_branches():
                assert ref.branches[key] > 0, (order, key)
        lm.close()


def test_terms_are_the_sentence_scores_terms():
    """q of a sentence (casr_lm_score_host) is the ascending f32 sum of the row entries of its words:
    row p's context is the up to three tokens before p, <s> first, and the closing </s> is the eos
    column."""
    grams = R.random_model(4, V, 31)
    lm = NgramLM.from_ids(*R.arrays_of(grams), {}, V)
    tokens, lens = R.sentences_from(grams, V, 12, 9, 32)
    eos = 4
    for i in range(len(lens)):
        sent = [int(t) for t in tokens[i, :lens[i]] if t != eos]
        hist = [V] + sent
        ctx = np.zeros((len(sent) + 1, 3), np.int32)
        nc = np.zeros(len(sent) + 1, np.int32)
        for p in range(len(sent) + 1):
            c = hist[:p + 1][::-1][:3]
            ctx[p, :len(c)] = c
            nc[p] = len(c)
        rows = lm.terms(ctx, nc, eos)
        q = None
        for p, w in enumerate(sent + [eos]):
            q = rows[p, w] if q is None else F(q + rows[p, w])
        row = np.array([sent + [0] * (9 - len(sent))], np.int32)
        assert bits(q) == bits(lm.score_ids(row, [len(sent)])[0]), i
    lm.close()


def _with_unigrams(grams, p=-3.0, b=-0.125):
    for g in grams[1:]:
        for k in g:
            for i in k:
                grams[0].setdefault((i,), (F(p), F(b)))
    return grams


def test_constructed_cases():
    Vn = 300
    base = R.random_model(1, Vn, 5, n_uni=Vn)  # every id has a unigram
    # (a) a context whose bigram successor list holds every unigram id: far longer than a wave
    everyone = {(7, w): (F(-0.5 - w / 1024.0), F(-0.25)) for w in list(range(Vn)) + [Vn + 1, Vn + 2]}
    # (b) word 11 as a 2-, 3- and 4-gram under the same context (9 8 7): the highest order wins; word
    # 12 as a 2- and 4-gram only; (c) <unk> and </s> as successors at every order
    tri = {(8, 7, 11): (F(-0.75), F(-0.5)), (8, 7, Vn + 2): (F(-1.25), F(-0.5)), (8, 7, Vn + 1): (F(-1.75), F(0)),
           (9, 8, 7): (F(-0.375), F(-1.5))}
    four = {(9, 8, 7, 11): (F(-0.125), F(0)), (9, 8, 7, 12): (F(-0.0625), F(0)), (9, 8, 7, Vn + 2): (F(-2.25), F(0)),
            (9, 8, 7, Vn + 1): (F(-2.5), F(0))}
    grams = _with_unigrams(base + [everyone, tri, four])
    ref = R.RefLM(4, Vn, grams)
    lm = NgramLM.from_ids(*R.arrays_of(grams), {}, Vn)
    ctx = np.array([[7, 8, 9], [7, 8, 9], [7, 8, 9], [7, 8, 9], [7, 5, 9], [8, 7, 9]], np.int32)
    nc = np.array([3, 2, 1, 0, 3, 3], np.int32)
    eos = 20
    got = lm.terms(ctx, nc, eos)
    assert np.array_equal(bits(got), bits(ref_rows(ref, ctx, nc, eos)))
    assert got[0, 11] == F(-0.125) and got[1, 11] == F(-0.75) and got[0, 12] == F(-0.0625)
    assert got[0, eos] == F(-2.5) and got[1, eos] == F(-1.75)
    lm.close()
    # (d) a model whose n-grams contain words without unigrams (test_gpu_ngram's _lm_from_records
    # recipe: the n-grams of sentences, one in eight of whose tokens has no unigram): they change nothing
    rs = np.random.RandomState(3)
    sents = [rs.randint(0, 60, size=rs.randint(1, 8)).tolist() for _ in range(40)]
    seen, toks = set(), set()
    for t in sents:
        ids = [V] + t + [V + 1]
        toks.update(t)
        for n in (2, 3, 4):
            seen.update(tuple(ids[i:i + n]) for i in range(len(ids) - n + 1))
    keep = [t for t in sorted(toks) if rs.rand() < 0.875]
    assert len(keep) < len(toks)
    uni = sorted(set(keep) | set(int(x) for x in rs.choice(V, size=500, replace=False)) - (toks - set(keep)))
    grams = R.random_model(4, V, 4, n_high=500, seeds=sorted(seen), uni_ids=uni, p_lo=-1.5, b_lo=-0.5)
    ref = R.RefLM(4, V, grams)
    lm = NgramLM.from_ids(*R.arrays_of(grams), {}, V)
    ctx, nc = [], []
    for t in sents[:8]:
        hist = ([V] + t)[::-1][:3]
        ctx.append(hist + [0] * (3 - len(hist)))
        nc.append(len(hist))
    ctx, nc = np.array(ctx, np.int32), np.array(nc, np.int32)
    got = lm.terms(ctx, nc, 1)
    assert np.array_equal(bits(got), bits(ref_rows(ref, ctx, nc, 1)))
    lm.close()


def test_refusals():
    import ctypes
    lm = NgramLM.from_ids(*R.arrays_of(R.random_model(2, 50, 1, n_high=20)), {}, 50)
    lib = lm._lib
    ctx, nc, out = np.zeros((1, 3), np.int32), np.zeros(1, np.int32), np.zeros((1, 50), F)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.casr_lm_terms_host(None, vp(ctx), vp(nc), 1, -1, vp(out)) == 1
    assert lib.casr_lm_terms_host(lm._host, None, vp(nc), 1, -1, vp(out)) == 1
    assert lib.casr_lm_terms_host(lm._host, vp(ctx), vp(nc), -1, -1, vp(out)) == 1
    assert lib.casr_lm_terms_host(lm._host, vp(ctx), vp(nc), 0, -1, None) == 0
    assert not out.any()
    with pytest.raises(ValueError):
        lm.terms(np.zeros((2, 2), np.int32), [0, 0])
    lm.close()
