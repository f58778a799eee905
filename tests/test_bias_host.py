"""Hotword biasing on the host (include/casr.h casr_bias_create, casr_bias_score_host,
casr_bias_rows_host; casr/bias.py PhraseBias): the automaton's full, tail and gain rows equal the brute
force of tests/bias_ref.py exactly, on hand cases and seeded sets; the create-time refusals; PhraseBias
parsing; and the conditions the shared beam case (bias_ref.bias_case) must meet before the device test
compares against the numpy restatement.  No GPU."""
import ctypes

import numpy as np
import pytest

import bias_ref as BR
from casr import lib as L
from casr.bias import PhraseBias, read_hotwords

V = 5004
# 北 京 大 学 and a few more as ids
BEI, JING, DA, XUE, A, B, C, X = 10, 11, 12, 13, 20, 21, 22, 30


def _bias(phrases, boosts, vocab=V):
    return PhraseBias(phrases, {}, vocab, [b / 256 for b in boosts])


def _score(pb, sents, L_=None):
    L_ = max([len(y) for y in sents] + [1]) if L_ is None else L_
    tok = np.zeros((len(sents), L_), np.int32)
    for i, y in enumerate(sents):
        tok[i, :len(y)] = y
    return pb.score_ids(tok, [len(y) for y in sents])


def _check(phrases, boosts, sents, vocab=V, rows=True):
    pb = _bias(phrases, boosts, vocab)
    try:
        full, tail, state = _score(pb, sents)
        for i, y in enumerate(sents):
            assert (int(full[i]), int(tail[i])) == (BR.full(y, phrases, boosts), BR.tail(y, phrases, boosts)), (i, y)
        if rows:
            gain, nxt = pb.rows(state, next=True)
            for i, y in enumerate(sents):
                want = BR.candidate_ints(y, phrases, boosts, vocab) - BR.full(y, phrases, boosts)
                assert np.array_equal(gain[i], want), (i, y)
                # next: the state the sentence walk reaches with one more token (where the row is not the root's)
                for v in np.nonzero(gain[i])[0][:6].tolist() + [0]:
                    assert _score(pb, [y + [v]])[2][0] == nxt[i, v], (i, y, v)
        return full, tail
    finally:
        pb.close()


# ---------------------------------------------------------------------------- hand cases
def test_nested_phrases_both_count():
    ph, bo = [[BEI, JING], [BEI, JING, DA, XUE]], [256, 512]
    full, tail = _check(ph, bo, [[BEI], [BEI, JING], [BEI, JING, DA], [BEI, JING, DA, XUE], [X, BEI, JING, DA, XUE, X]])
    assert full.tolist() == [0, 512, 512, 512 + 2048, 512 + 2048]
    assert tail.tolist() == [512, 1024, 1536, 0, 0]  # the longer phrase's boost, the larger, carries the partial


def test_suffix_phrase_reached_through_a_fail_link():
    # after A B the match of A B C is in progress; X breaks it, but B X is a phrase, found through fail(A B) = B
    ph, bo = [[A, B, C], [B, X]], [300, 200]
    full, tail = _check(ph, bo, [[A, B], [A, B, X], [A, B, C], [A, A, B, X, X]])
    assert full.tolist() == [0, 400, 900, 400]
    assert tail.tolist() == [600, 0, 0, 0]


def test_abac_inside_ababac():
    ph, bo = [[A, B, A, C]], [256]
    full, tail = _check(ph, bo, [[A, B, A, B, A, C], [A, B, A, B], [A, B, A, B, A]])
    assert full.tolist() == [1024, 0, 0]
    assert tail.tolist() == [0, 512, 768]


def test_partial_match_withdrawn():
    ph, bo = [[A, B, C]], [512]
    full, tail = _check(ph, bo, [[A], [A, B], [A, B, X], [A, B, A]])
    assert full.tolist() == [0, 0, 0, 0]
    assert tail.tolist() == [512, 1024, 0, 512]
    assert BR.withdrawn([A, B, X], ph) and not BR.withdrawn([A, B, C], ph)


def test_phrase_of_length_16_and_the_bound():
    p16 = list(range(100, 116))
    ph, bo = [p16, p16[:15], [100]], [4096, 4096, 4096]
    full, tail = _check(ph, bo, [p16, p16[:15], p16[:8], p16 + p16], rows=True)
    assert full[0] == 16 * 4096 + 15 * 4096 + 4096 and tail[1] == 15 * 4096
    # the header's bound: 512 tokens of one repeated token with one phrase per length, boost 4096
    ph = [[7] * n for n in range(1, 17)]
    bo = [4096] * 16
    pb = _bias(ph, bo)
    try:
        f, t, _ = _score(pb, [[7] * 512])
        want = sum(n * 4096 * (512 - n + 1) for n in range(1, 17))
        assert int(f[0]) == want and want + int(t[0]) < 2 ** 31 and int(t[0]) == 15 * 4096
    finally:
        pb.close()


def test_empty_set_and_unknown_ids():
    full, tail = _check([], [], [[], [1, 2, 3], [V, -1]])
    assert not full.any() and not tail.any()
    ph, bo = [[A, B]], [256]
    full, tail = _check(ph, bo, [[A, V, B], [A, -5], [A, 2 ** 31 - 1, A, B], [-1, A]], rows=False)
    assert full.tolist() == [0, 0, 512, 0] and tail.tolist() == [0, 0, 0, 256]


# ---------------------------------------------------------------------------- seeded sets
@pytest.mark.parametrize("chunk", range(4))
def test_seeded_sets_equal_the_brute_force(chunk):
    for seed in range(50 * chunk, 50 * chunk + 50):
        vocab, ph, bo, sents = BR.seeded_set(seed)
        _check(ph, bo, sents, vocab)
        # the restatement's per-candidate form against full + tail of the extended sentence
        for y in sents[:2]:
            want = [BR.full(y + [v], ph, bo) + BR.tail(y + [v], ph, bo) for v in range(vocab)]
            assert BR.candidate_ints(y, ph, bo, vocab).tolist() == want


# ---------------------------------------------------------------------------- refusals
def _create(vocab, phrases, boosts):
    lib = L.load()
    toks = np.array([t for p in phrases for t in p], np.int32)
    lens = np.array([len(p) for p in phrases], np.int32)
    bo = np.array(boosts, np.int32)
    out = ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None  # noqa: E731
    rc = lib.casr_bias_create(-1, vocab, len(phrases), p(toks), p(lens), p(bo), ctypes.byref(out))
    msg = (lib.casr_last_error(None) or b"").decode()
    if rc == 0:
        lib.casr_bias_destroy(out)
    return rc, msg


def test_create_refusals():
    assert _create(V, [[1, 2]], [256])[0] == 0
    rc, msg = _create(V, [[1, 2], [3], [1, 2]], [256, 256, 300])
    assert rc == 1 and "phrase 2 is a duplicate" in msg
    rc, msg = _create(V, [[1, V]], [256])
    assert rc == 1 and f"id {V}" in msg
    rc, msg = _create(V, [[-1]], [256])
    assert rc == 1 and "id -1" in msg
    for bad in (0, 4097, -3):
        rc, msg = _create(V, [[1]], [bad])
        assert rc == 1 and f"boost {bad}" in msg
    assert _create(V, [[1]], [4096])[0] == 0 and _create(V, [[1]], [1])[0] == 0
    rc, msg = _create(V, [list(range(17))], [256])
    assert rc == 1 and "length 17" in msg
    assert _create(V, [list(range(16))], [256])[0] == 0
    # more than 2^20 tokens (the lengths are read before any id: no token array of that size is needed)
    lib = L.load()
    n = (1 << 20) // 16 + 1
    lens = np.full(n, 16, np.int32)
    bo = np.full(n, 256, np.int32)
    toks = np.zeros(n * 16, np.int32)
    out = ctypes.c_void_p()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert lib.casr_bias_create(-1, V, n, vp(toks), vp(lens), vp(bo), ctypes.byref(out)) == 4
    assert "tokens" in lib.casr_last_error(None).decode()
    assert lib.casr_bias_create(-1, V, 1, None, vp(lens), vp(bo), ctypes.byref(out)) == 1
    assert lib.casr_bias_create(-1, V, 1, vp(toks), vp(lens), vp(bo), None) == 1
    for name in ("casr_bias_create", "casr_bias_score", "casr_bias_rows", "casr_beam_bias", "casr_beam_record_bias"):
        assert name in L.EXPORTS and hasattr(lib, name)


def test_host_entry_refusals():
    pb = _bias([[A, B]], [256])
    lib = L.load()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    tok, ln, out = np.zeros((1, 4), np.int32), np.array([5], np.int32), np.zeros(1, np.int32)
    assert lib.casr_bias_score_host(pb._host, vp(tok), vp(ln), 1, 4, vp(out), None, None) == 1  # a length past L
    assert lib.casr_bias_score_host(None, vp(tok), vp(ln), 1, 4, vp(out), None, None) == 1
    st, gain = np.array([99], np.int32), np.zeros((1, V), np.int32)
    assert lib.casr_bias_rows_host(pb._host, vp(st), 1, vp(gain), None) == 1  # a state outside the automaton
    assert "state[0] = 99" in lib.casr_last_error(None).decode()
    assert lib.casr_bias_rows_host(pb._host, None, 1, vp(gain), None) == 1
    assert lib.casr_bias_rows_host(pb._host, None, 0, None, None) == 0
    pb.close()


# ---------------------------------------------------------------------------- PhraseBias
def test_phrase_bias_parsing(tmp_path):
    w2i = {"北": BEI, "京": JING, "大": DA, "学": XUE}
    pb = PhraseBias(["北京", "北京大学", [DA, XUE]], w2i, V, boost=[1.0, 2.0, 0.5])
    assert pb.phrases == [[BEI, JING], [BEI, JING, DA, XUE], [DA, XUE]] and pb.boost_q == [256, 512, 128]
    f, t, _ = pb.score_ids([[BEI, JING, DA, XUE]], [4])
    assert (int(f[0]), int(t[0])) == (512 + 2048 + 256, 0)
    pb.close()
    pb = PhraseBias(["北京"], w2i, V, boost=1.3)  # quantised to 1/256
    assert pb.boost_q == [333]
    pb.close()
    with pytest.raises(ValueError, match="'海'"):
        PhraseBias(["北京", "上海"], dict(w2i, 上=40), V)
    with pytest.raises(ValueError, match="boost"):
        PhraseBias(["北京"], w2i, V, boost=17.0)
    with pytest.raises(ValueError, match="boost"):
        PhraseBias(["北京"], w2i, V, boost=0.0)
    with pytest.raises(ValueError, match="tokens"):
        PhraseBias(["北" * 17], w2i, V)
    with pytest.raises(ValueError, match="2 phrases but 1 boosts"):
        PhraseBias(["北京", "大学"], w2i, V, boost=[1.0])
    with pytest.raises(L.CasrError, match="duplicate"):
        PhraseBias(["北京", "北京"], w2i, V)
    path = tmp_path / "hot.txt"
    path.write_text("# names\n北京 2.5\n\n大学\n", encoding="utf-8")
    assert read_hotwords(path) == (["北京", "大学"], [2.5, None])
    pb = PhraseBias.coerce(str(path), w2i, V, 1.5)
    assert pb.phrases == [[BEI, JING], [DA, XUE]] and pb.boost_q == [640, 384]
    assert PhraseBias.coerce(pb, w2i, V) is pb and PhraseBias.coerce(None, w2i, V) is None
    pb.close()


def test_model_refuses_bias_with_mbr_or_a_second_pass():
    import model as M
    m = M.Model.__new__(M.Model)
    m.model = type("T", (), {"eval": lambda self: None})()
    pb = _bias([[A, B]], [256])
    with pytest.raises(ValueError, match="mbr"):
        M.Model.eval_one_batch_with_beam(m, None, 4, None, None, None, None, mbr=0.5, bias=pb)
    with pytest.raises(ValueError, match="second pass"):
        M.Model.eval_one_batch_with_beam(m, None, 4, None, None, None, None, second_pass=True, lm_model=object(), bias=pb)
    pb.close()


# ---------------------------------------------------------------------------- the shared beam case
@pytest.mark.parametrize("with_lm", [True, False])
def test_shared_beam_case_conditions(with_lm):
    """What tests/test_gpu_bias.py's comparison with the numpy restatement rests on, per width of
    bias_ref.GPU_K: adjacent ranked vals at least 1e-2 apart (fusion_ref.GPU_K's condition: a device
    whose am differs by rounding ranks the same), at least 6 steps, a choice the bias changes, a
    withdrawn partial match and a completed phrase of 3 or more tokens among the records."""
    case = BR.bias_case()
    ph = case["phrases"]
    assert len(ph) == len(set(map(tuple, ph))) and max(map(len, ph)) >= 3
    for k in BR.GPU_K:
        r = BR.biased_case(k, with_lm)
        plain = BR.biased_case(k, with_lm, 0.0)
        assert (r["gap"] >= 1e-2).all(), (k, r["gap"])
        assert r["steps"] >= 6
        assert sum(a != b for a, b in zip(r["tokens"], plain["tokens"])) >= 1
        recs = [t for v in r["records"].values() for t, *_ in v]
        assert any(BR.withdrawn(t, ph) for t in recs)
        assert any(len(p) >= 3 and BR.contains(t, p) for t in recs for p in ph)
        # a record's bias is bias_closed of its tokens
        for v in r["records"].values():
            for t, _, _, z in v:
                assert z == np.float32(BR.full(t, ph, case["boosts"])) / np.float32(256)
