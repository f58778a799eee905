"""Grammar-constrained decoding on the host (include/casr.h casr_grammar_create, casr_grammar_info,
casr_grammar_accept_host, casr_grammar_rows_host; casr/grammar.py Grammar): walks, mask rows and distances
equal the restatement of tests/grammar_ref.py exactly, on hand cases and seeded acceptors; every
create-time refusal; each builder's language equals brute-force enumeration; and the conditions the shared
beam cases (grammar_ref.grammar_case) must meet before the device test compares against the numpy
restatement.  No GPU."""
import ctypes
import itertools

import numpy as np
import pytest

import grammar_ref as GR
from casr import lib as L
from casr.grammar import Grammar, mask_bits

V = 5004
EOS = 2
SV = 12  # the small vocabulary of the seeded acceptors and the enumerations
BUDGETS = (-1, 0, 1, 5, 10 ** 6)
A, B, C, D, E = 3, 4, 5, 6, 7
W2I = {"a": A, "b": B, "c": C, "d": D, "e": E}


def _walk(g, sents):
    L_ = max([len(y) for y in sents] + [1])
    tok = np.zeros((len(sents), L_), np.int32)
    for i, y in enumerate(sents):
        tok[i, :len(y)] = y
    return g.walk(tok, [len(y) for y in sents])


def _check(arcs, finals, sents, vocab=SV, eos=EOS):
    g = Grammar(arcs, finals, vocab, eos)
    try:
        S = len(arcs)
        acc = GR.TripleAcceptor({(s, v, d) for s, row in enumerate(arcs) for v, d in row}, finals, S)
        assert g.dist.tolist() == acc.dist() and g.n_states == S and g.n_arcs == sum(map(len, arcs))
        consumed, state, ok = _walk(g, sents)
        for i, y in enumerate(sents):
            n, cur = acc.walk(y, vocab)
            assert (int(consumed[i]), {int(state[i])}) == (n, cur), (i, y)
            assert bool(ok[i]) == acc.accepts(y, vocab) == g.accepts(y), (i, y)
        states = list(range(S)) + [-1]
        for budget in BUDGETS:
            bits = mask_bits(g.rows(states, budget), vocab)
            raw = g.rows(states, budget)
            assert raw.shape == (S + 1, 4 * ((vocab + 127) // 128))
            assert not np.unpackbits(raw.view(np.uint8), axis=1, bitorder="little")[:, vocab:].any()
            for i, s in enumerate(states):
                assert np.array_equal(bits[i], acc.row(s, budget, vocab, eos)), (s, budget)
        return g.dist.tolist()
    finally:
        g.close()


# ---------------------------------------------------------------------------- hand cases
def test_a_chain_a_branch_and_a_loop():
    # 0 -a-> 1 -b-> 2 (final) -c-> 2; 0 -d-> 3 -e-> 4 -e-> 2
    arcs = [[(A, 1), (D, 3)], [(B, 2)], [(C, 2)], [(E, 4)], [(E, 2)]]
    dist = _check(arcs, [2], [[A, B], [A, B, C, C], [A], [D, E, E], [D, E], [A, C], [], [B], [A, B, EOS], [A, SV], [-1]])
    assert dist == [2, 1, 0, 2, 1]
    g = Grammar(arcs, [2], SV)
    try:
        # budget: from state 0, a needs dist[1] = 1 <= budget and d needs dist[3] = 2
        assert [mask_bits(g.rows([0], b), SV)[0].nonzero()[0].tolist() for b in (0, 1, 2)] == [[], [A], [A, D]]
        # eos exactly in the final state, whatever the budget
        assert mask_bits(g.rows([2, 2, 1], [-1, 5, 5]), SV)[:, EOS].tolist() == [True, True, False]
        assert mask_bits(g.rows([2], -1), SV)[0].nonzero()[0].tolist() == [EOS]
    finally:
        g.close()


def test_full_vocabulary_rows_and_the_mask_width():
    lib = L.load()
    assert lib.casr_grammar_mask_words(V) == 160 and lib.casr_grammar_mask_words(128) == 4
    assert lib.casr_grammar_mask_words(129) == 8 and lib.casr_grammar_mask_words(0) == 0
    g = Grammar.universal(V, EOS)
    try:
        assert g.n_states == 1 and g.n_arcs == V - 1 and g.dist.tolist() == [0]
        bits = mask_bits(g.rows([0, 0], [0, -1]), V)
        assert bits[0].all() and bits[1].nonzero()[0].tolist() == [EOS]
        assert g.accepts([V - 1, 0, 31, 32, 63, 64]) and not g.accepts([EOS]) and not g.accepts([V])
    finally:
        g.close()


# ---------------------------------------------------------------------------- seeded acceptors
@pytest.mark.parametrize("chunk", range(4))
def test_seeded_acceptors_equal_the_restatement(chunk):
    for seed in range(50 * chunk, 50 * chunk + 50):
        arcs, finals, sents = GR.seeded_acceptor(seed, SV, EOS)
        _check(arcs, finals, sents)


# ---------------------------------------------------------------------------- refusals
def _create(vocab, eos, arcs, finals, null=None, off=None):
    lib = L.load()
    S = len(arcs)
    o = np.zeros(S + 1, np.int64)
    o[1:] = np.cumsum([len(r) for r in arcs])
    o = o if off is None else np.array(off, np.int64)
    tok = np.array([t for r in arcs for t, _ in r] + [0], np.int32)
    nxt = np.array([d for r in arcs for _, d in r] + [0], np.int32)
    fin = np.zeros(max(S, 1), np.uint8)
    fin[np.array(sorted(finals), np.intp)] = 1
    out = ctypes.c_void_p()
    vp = lambda n, a: None if null == n else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = lib.casr_grammar_create(-1, vocab, eos, S, vp("off", o), vp("tok", tok), vp("next", nxt), vp("fin", fin),
                                 None if null == "out" else ctypes.byref(out))
    msg = (lib.casr_last_error(None) or b"").decode()
    if rc == 0:
        lib.casr_grammar_destroy(out)
    return rc, msg


def test_create_refusals():
    ok = [[(A, 1), (B, 0)], []]
    assert _create(V, EOS, ok, [1])[0] == 0
    for null in ("off", "tok", "next", "fin", "out"):
        assert _create(V, EOS, ok, [1], null=null)[0] == 1, null
    assert _create(V, EOS, [[]], [0], null="tok")[0] == 0  # no arcs: their arrays may be NULL
    rc, msg = _create(V, EOS, [[(V, 1)], []], [1])
    assert rc == 1 and f"token {V}" in msg and "arc 0 of state 0" in msg
    rc, msg = _create(V, EOS, [[(-1, 1)], []], [1])
    assert rc == 1 and "token -1" in msg
    rc, msg = _create(V, EOS, [[(A, 1)], [(EOS, 0)]], [1])
    assert rc == 1 and "eos" in msg and "arc 1 of state 1" in msg
    for row in ([(B, 1), (A, 1)], [(A, 1), (A, 0)]):  # descending, and a duplicate
        rc, msg = _create(V, EOS, [row, []], [1])
        assert rc == 1 and "ascend" in msg and "arc 1 of state 0" in msg
    for bad in (2, -1):
        rc, msg = _create(V, EOS, [[(A, bad)], []], [1])
        assert rc == 1 and f"state {bad}" in msg and "arc 0 of state 0" in msg
    rc, msg = _create(V, EOS, ok, [])
    assert rc == 1 and "no final state" in msg
    rc, msg = _create(V, EOS, [[(A, 1), (B, 2)], [], [(A, 2)]], [1])
    assert rc == 1 and "state 2 reaches no final state" in msg
    assert _create(V, V, ok, [1])[0] == 1 and _create(V, -1, ok, [1])[0] == 1 and _create(0, 0, ok, [1])[0] == 1
    assert _create(V, EOS, [], [])[0] == 1
    rc, msg = _create(V, EOS, ok, [1], off=[0, 2, 1])
    assert rc == 1 and "state 1" in msg
    assert _create(V, EOS, ok, [1], off=[1, 2, 2])[0] == 1
    # the limits: 2^20 states, 2^24 arcs (read off arc_off before any arc: no array of that size is needed)
    lib = L.load()
    out = ctypes.c_void_p()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    S = (1 << 20) + 1
    off, fin, few = np.zeros(S + 1, np.int64), np.ones(S, np.uint8), np.zeros(4, np.int32)
    assert lib.casr_grammar_create(-1, V, EOS, S, vp(off), vp(few), vp(few), vp(fin), ctypes.byref(out)) == 4
    assert "states" in lib.casr_last_error(None).decode()
    off = np.array([0, (1 << 24) + 1], np.int64)
    assert lib.casr_grammar_create(-1, V, EOS, 1, vp(off), vp(few), vp(few), vp(fin), ctypes.byref(out)) == 4
    assert "arcs" in lib.casr_last_error(None).decode()
    for name in ("casr_grammar_create", "casr_grammar_destroy", "casr_grammar_info", "casr_grammar_mask_words",
                 "casr_grammar_accept_host", "casr_grammar_accept", "casr_grammar_rows_host", "casr_grammar_rows",
                 "casr_beam_grammar"):
        assert name in L.EXPORTS and hasattr(lib, name)


def test_host_entry_refusals():
    g = Grammar([[(A, 0)]], [0], V)
    lib = L.load()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    tok, ln, out = np.zeros((1, 4), np.int32), np.array([5], np.int32), np.zeros(1, np.int32)
    assert lib.casr_grammar_accept_host(g._host, vp(tok), vp(ln), 1, 4, vp(out), None, None) == 1  # a length past L
    assert "lens[0] = 5" in lib.casr_last_error(None).decode()
    assert lib.casr_grammar_accept_host(None, vp(tok), vp(ln), 1, 4, vp(out), None, None) == 1
    st, bu, mask = np.array([1], np.int32), np.array([3], np.int32), np.zeros((1, 160), np.uint32)
    assert lib.casr_grammar_rows_host(g._host, vp(st), vp(bu), 1, vp(mask)) == 1  # a state outside the grammar
    assert "state[0] = 1" in lib.casr_last_error(None).decode()
    st[0] = -2
    assert lib.casr_grammar_rows_host(g._host, vp(st), vp(bu), 1, vp(mask)) == 1
    assert lib.casr_grammar_rows_host(g._host, None, vp(bu), 1, vp(mask)) == 1
    assert lib.casr_grammar_rows_host(g._host, None, None, 0, None) == 0
    assert lib.casr_grammar_info(None, None, None, None) == 1
    g.close()


# ---------------------------------------------------------------------------- the builders
ALPHA = [A, B, C, D]


def _language(g, longest=6):
    """Every sentence over ALPHA of at most ``longest`` tokens that the grammar accepts, by brute force."""
    sents = [list(y) for n in range(longest + 1) for y in itertools.product(ALPHA, repeat=n)]
    return {tuple(y) for y, ok in zip(sents, _walk(g, sents)[2]) if ok}


def _strings(words):
    return {tuple(W2I[ch] for ch in w) for w in words}


def _all_strings(parts_per_slot):
    return {tuple(t for p in combo for t in p) for combo in itertools.product(*parts_per_slot)}


def test_builders_languages_equal_enumeration(tmp_path):
    g = Grammar.from_phrases(["ab", "abc", "b", "abd", [C, C]], W2I, SV)
    assert _language(g) == _strings(["ab", "abc", "b", "abd", "cc"])
    g.close()
    g = Grammar.sequence([["a", "bb"], ["c"], ["d", "da", ""]], W2I, SV, optional=[1])
    first, mid, last = _strings(["a", "bb"]), _strings(["c", ""]), _strings(["d", "da", ""])
    assert _language(g) == {y for y in _all_strings([first, mid, last]) if len(y) <= 6}
    g.close()
    for lo, hi in ((1, 3), (0, 2), (2, 2), (3, 6)):
        g = Grammar.repeat(["a", "bc"], lo, hi, W2I, SV)
        unit = _strings(["a", "bc"])
        want = {y for n in range(lo, hi + 1) for y in _all_strings([unit] * n) if len(y) <= 6}
        assert _language(g) == want, (lo, hi)
        g.close()
    digits = Grammar.repeat([[t] for t in ALPHA], 3, 5, None, SV)
    assert _language(digits) == {y for n in (3, 4, 5) for y in itertools.product(ALPHA, repeat=n)}
    names = Grammar.from_phrases(["ab", "cd"], W2I, SV)
    u, starts = Grammar.union([digits, names])
    assert starts[0] == 0 and len(set(starts)) == 2
    assert _language(u) == _language(digits)  # sentences walked from state 0 are the first member's
    # the second member's language, from its own start state: the rows lead through it
    s, y = starts[1], []
    for t in (A, B):
        assert mask_bits(u.rows([s], 10), SV)[0].nonzero()[0].tolist() == ([A, C] if not y else [B])
        s = dict(u.arcs[s])[t]
        y.append(t)
    assert s in u.finals and mask_bits(u.rows([s], 10), SV)[0].nonzero()[0].tolist() == [EOS]
    for x in (digits, names, u):
        x.close()
    uni = Grammar.universal(SV, EOS)
    assert _language(uni, 3) == {y for n in range(4) for y in itertools.product(ALPHA, repeat=n)}
    uni.close()
    path = tmp_path / "menu.txt"
    path.write_text("# a menu\nab\n\ncd\n", encoding="utf-8")
    g = Grammar.from_file(path, W2I, SV)
    assert _language(g) == _strings(["ab", "cd"])
    assert Grammar.coerce(g, W2I, SV) is g and Grammar.coerce(None, W2I, SV) is None
    g2 = Grammar.coerce(["ab"], W2I, SV)
    assert g2.accepts("ab", W2I) and not g2.accepts("a", W2I) and not g2.accepts("xb", W2I)
    g.close()
    g2.close()
    with pytest.raises(ValueError, match="'x'"):
        Grammar.from_phrases(["ab", "ax"], W2I, SV)
    with pytest.raises(ValueError, match="vocabulary"):
        Grammar.from_phrases([[A, EOS]], W2I, SV)
    with pytest.raises(ValueError, match="empty"):
        Grammar.from_phrases([], W2I, SV)
    with pytest.raises(L.CasrError, match="ascend"):
        Grammar([[(A, 0), (A, 0)]], [0], SV)


def test_model_refuses_a_grammar_with_the_readers_of_a_plain_beam():
    import model as M
    m = M.Model.__new__(M.Model)
    m.model = type("T", (), {"eval": lambda self: None})()
    g = Grammar.from_phrases(["ab"], W2I, V)
    from casr.bias import PhraseBias
    pb = PhraseBias([[A, B]], {}, V)
    for kw, what in ((dict(bias=pb), "bias"), (dict(mbr=0.5), "mbr"), (dict(nbest=3), "nbest"),
                     (dict(alternatives=2), "alternatives"), (dict(second_pass=True, lm_model=object()), "second pass")):
        kw.setdefault("second_pass", False)
        with pytest.raises(ValueError, match=what):
            M.Model.eval_one_batch_with_beam(m, None, 4, None, None, None, None, grammar=g, **kw)
    g.close()
    pb.close()


# ---------------------------------------------------------------------------- the shared beam cases
def test_shared_beam_case_conditions():
    """What tests/test_gpu_grammar.py's comparison with the numpy restatement rests on: on fusion_ref.UTTS (B =
    6, T = 101), with the record language of grammar_ref.grammar_case (the oracle's k = 4 plain-beam
    records minus each utterance's best) and no LM, the smallest gap between vals adjacent in rank among
    the best 2k + 1 candidates is

        eos_bias   k = 2     k = 4     search steps
        18.0       0.108     0.045     5
        28.5       0.0168    0.0168    2

    so a device whose am differs by rounding (2e-3) ranks the same at every width of grammar_ref.GPU_K.
    At eos_bias 28.5 the plain search takes 3 steps and at k = 16 the gap falls below 1e-2 (1.5e-3), so k
    = 16 rests on the device test's invariants.  All six outputs are sentences of the language and, the
    plain choice being outside it, all six differ from the plain beam's (at least the two the condition
    asks for).  The with-LM variants (weights 1.5, 1.5) measured 0.052 / 0.052 (18.0) and 0.051 / 0.035
    (28.5) at k = 2 / 4 and are compared as well; at k = 16 they fall to 0.023 and 0.0048."""
    want = {(18.0, 2): (0.108, 5), (18.0, 4): (0.045, 5), (28.5, 2): (0.0168, 2), (28.5, 4): (0.0168, 2)}
    for eb in GR.EOS_BIASES:
        case = GR.grammar_case(eb)
        lang = case["lang"]
        assert all(not lang.member(t) for t in case["plain"]["tokens"])
        for k in GR.GPU_K:
            r = GR.constrained_case(eb, k)
            gap, steps = want[(eb, k)]
            assert r["gap"].min() >= 1e-2 and abs(r["gap"].min() - gap) <= 0.05 * gap, (eb, k, r["gap"])
            assert r["steps"] == steps
            assert r["complete"].all() and all(lang.member(t) for t in r["tokens"])
            assert sum(a != b for a, b in zip(r["tokens"], case["plain"]["tokens"])) >= 2
            assert all(lang.member(t) for v in r["records"].values() for t, *_ in v)
            rl = GR.constrained_case(eb, k, True)
            assert (rl["gap"] >= 1e-2).all(), (eb, k, rl["gap"])
            assert rl["complete"].all() and all(lang.member(t) for t in rl["tokens"])
    assert GR.grammar_case(28.5)["plain"]["steps"] == 3
    assert GR.constrained_case(28.5, 16)["gap"].min() < 1e-2


def test_the_horizon_on_the_restatement():
    """The horizon rule on the restatement alone: an eos that can never win (eos_bias -60), B = 2, T = 48, k
    = 4 and a loop over ten tokens: the search runs all max_len steps, every row stays able to finish, the
    records are at the last step only and every answer has max_len - 1 tokens.  A chain of exactly max_len -
    1 tokens is returned whole; a chain of max_len tokens has no candidate at all."""
    case = GR.horizon_case()
    Lmax = case["cfg"].max_len
    r = GR.constrained_beam(case["encoded"], case["dec_sd"], 4, GR.LoopLanguage(GR.LOOP_TOKENS))
    assert r["steps"] == Lmax and r["complete"].all()
    assert [len(t) for t in r["tokens"]] == [Lmax - 1] * 2
    assert all(l == Lmax - 1 for v in r["records"].values() for *_, l in v) and all(r["records"].values())
    chain = GR.chain_tokens(Lmax - 1)
    r = GR.constrained_beam(case["encoded"], case["dec_sd"], 4, GR.SetLanguage([chain]))
    assert r["tokens"] == [chain, chain] and r["complete"].all() and r["steps"] == Lmax
    r = GR.constrained_beam(case["encoded"], case["dec_sd"], 4, GR.SetLanguage([GR.chain_tokens(Lmax)]))
    assert r["tokens"] == [[], []] and not r["complete"].any() and r["steps"] == 1 and not r["score"].any()
