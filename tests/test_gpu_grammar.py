"""Grammar-constrained decoding on the device (include/casr.h casr_grammar_accept, casr_grammar_rows,
casr_beam_grammar).

Mask rows and walks against the host entries exactly; the universal grammar against casr_beam and
casr_beam_lm bit for bit (every width class, both arithmetics, the folded step); invariants on the
device's own records, where near ties of the search play no part (every record and every answer is a
sentence of the enumerated language, the best is the first maximum of the defined expression, rec_lm is the
reference sentence score); the numpy restatement (tests/grammar_ref.py) at the inputs whose rank gaps
tests/test_grammar_host.py checked; the horizon rule; refusals and state; Model and main.parse_batch."""
import numpy as np
import pytest
import torch

import grammar_ref as GR
import ngram_ref as R
from golden_util import fbank_for
from casr import lib as L
from casr.config import CasrConfig
from casr.grammar import Grammar, mask_bits
from casr.ngram import NgramLM
from casr.weights import synthetic_state_dicts

pytestmark = pytest.mark.gpu

CFG = CasrConfig()
V, EOS, LMAX = CFG.vocab, CFG.eos, CFG.max_len
B, T = 6, 101
F = np.float32
I2W = {i: f"w{i}" for i in range(V)}
W2I = {w: i for i, w in I2W.items()}
_PACKED = {}


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _engine(eos_bias, cfg=CFG):
    from casr.engine import Engine
    if eos_bias not in _PACKED:
        _PACKED[eos_bias] = L.pack_weights(CFG, *synthetic_state_dicts(CFG, peaked=True, eos_bias=eos_bias))
    return Engine(cfg, packed=_PACKED[eos_bias])


def _encode(e, nb=B, t=T, ids=None):
    ids = list(range(nb)) if ids is None else ids
    fb = torch.from_numpy(np.stack([fbank_for(b, t) for b in ids])).to(e.device)
    e.encode_fbank(fb, torch.full((len(ids),), t, dtype=torch.int32, device=e.device))


def _np(d):
    return {n: (v.cpu().numpy() if v is not None else None) for n, v in d.items()}


def _records(e):
    return [x.cpu().numpy() for x in e.beam_records()]


def _answers(r):
    return [r["tokens"][b, :r["length"][b]].tolist() for b in range(len(r["length"]))]


# ---------------------------------------------------------------------------- 1. rows and walks
def test_device_rows_and_walks_equal_the_host():
    from casr.engine import Engine
    rs = np.random.RandomState(3)
    toks = [v for v in range(V) if v != EOS]
    edge = [0, 31, 32, 63, 64, V - 1]
    counts = [0, 1, 2, 31, 32, 33, 64, V - 1]
    S = len(counts) + 3  # ... and three states further from a final one
    arcs = []
    rest = [v for v in toks if v not in edge]
    for n in counts:  # the edge tokens first, as many as fit
        ts = toks if n == V - 1 else edge[:n] + rs.choice(rest, size=max(n - len(edge), 0), replace=False).tolist()
        arcs.append([(int(t), int(rs.randint(S))) for t in sorted(ts)])
    arcs[1] = [(V - 1, 0)]
    arcs[2] = [(0, S - 1), (31, 2)]
    arcs += [[(32, 0), (63, S - 2)], [(64, S - 3)], [(5, S - 2), (V - 1, 1)]]
    assert [len(a) for a in arcs[:len(counts)]] == counts
    g = Grammar(arcs, [0, 3], V, EOS)
    n = 64
    state = rs.randint(0, S, size=n).astype(np.int32)
    state[:S] = np.arange(S)
    state[S] = -1
    e = Engine(CFG)  # no weights: the entries need none
    try:
        e.device_flags()
        assert g.mask_words == 160
        for budget in (-1, 0, 1, 5, 10 ** 6):
            want = g.rows(state, budget)
            got = e.grammar_rows(g, state, budget).cpu().numpy().view(np.uint32)
            assert np.array_equal(got, want), budget
            assert not np.unpackbits(got.view(np.uint8), axis=1, bitorder="little")[:, V:].any()
            assert not got[S].any()  # the dead state: a zero row
        mixed = rs.choice([-1, 0, 1, 5, 10 ** 6], size=n).astype(np.int32)
        assert np.array_equal(e.grammar_rows(g, state, mixed).cpu().numpy().view(np.uint32), g.rows(state, mixed))
        full = mask_bits(g.rows([len(counts) - 1], 10 ** 6), V)[0]
        assert full.sum() == V - 1 and not full[EOS]
        # walks: sentences through the grammar, some cut short by a token without an arc or an id outside [0, V)
        Ls = 24
        tok = np.zeros((n, Ls), np.int32)
        lens = rs.randint(0, Ls + 1, size=n).astype(np.int32)
        lens[:2] = (0, Ls)
        for i in range(n):
            s = 0
            for j in range(Ls):
                if not arcs[s] or rs.rand() < 0.05:
                    tok[i, j] = rs.choice([EOS, V, -1, 7])
                    continue
                tok[i, j], s = arcs[s][rs.randint(len(arcs[s]))]
        hc, hs, ha = g.walk(tok, lens)
        dc, ds, da = (x.cpu().numpy() for x in e.grammar_accept(g, tok, lens))
        assert np.array_equal(dc, hc) and np.array_equal(ds, hs) and np.array_equal(da, ha)
        assert ha.any() and not ha.all() and (hc < lens).any()
        assert e.device_flags() == 0
        # guard bit 1: a state outside the grammar gives a zero row; a length outside [0, L] is clamped
        st = state[:4].copy()
        st[1], st[2] = S, -2
        got = e.grammar_rows(g, st, 5).cpu().numpy().view(np.uint32)
        assert e.device_flags() == 1
        assert not got[1].any() and not got[2].any() and np.array_equal(got[[0, 3]], g.rows(st[[0, 3]], 5))
        bad = lens[:4].copy()
        bad[0], bad[3] = Ls + 3, -2
        dc, ds, da = (x.cpu().numpy() for x in e.grammar_accept(g, tok[:4], bad))
        assert e.device_flags() == 1
        bad[0], bad[3] = Ls, 0
        hc, hs, ha = g.walk(tok[:4], bad)
        assert np.array_equal(dc, hc) and np.array_equal(ds, hs) and np.array_equal(da, ha)
    finally:
        e.close()
        g.close()


# ---------------------------------------------------------------------------- 2. the universal grammar
def _same(z, zrecs, want, recs, names):
    print("steps", int(want["steps"][0]), "records", int(recs[2].sum()))
    assert int(want["steps"][0]) < LMAX  # (at the last step the horizon rule offers eos only)
    for n in ("tokens", "length", "steps"):
        assert np.array_equal(z[n], want[n]), n
    for n in names:
        assert np.array_equal(bits(z[n]), bits(want[n])), n
    assert np.array_equal(zrecs[0], recs[0]) and np.array_equal(bits(zrecs[1]), bits(recs[1]))
    assert np.array_equal(zrecs[2], recs[2])
    assert recs[2].any()
    assert z["complete"].all()


def _same_as_unconstrained(e, k, lm, uni):
    beam = _np(e.beam(k))
    recs = _records(e)
    fused = _np(e.beam_lm(lm, k, 1.5, 1.5))
    frecs, frq = _records(e), e.beam_record_lm().cpu().numpy()
    z = _np(e.beam_grammar(uni, k))  # no LM, length weight 0: casr_beam's
    _same(z, _records(e), beam, recs, ("score",))
    assert z["lm"] is None
    z = _np(e.beam_grammar(uni, k, lm, 1.5, 1.5))  # with the LM: casr_beam_lm's
    _same(z, _records(e), fused, frecs, ("score", "lm"))
    assert np.array_equal(bits(e.beam_record_lm().cpu().numpy()), bits(frq))


@pytest.mark.parametrize("k,precision", [(2, None), (4, None), (16, None), (4, "f32")])
def test_universal_grammar_reproduces_beam_and_beam_lm(k, precision):
    """fusion_ref.UTTS at eos_bias 28.5 with the LM of grammar_ref.grammar_case (built from the plain beam's
    records): casr_beam and casr_beam_lm both end after 3 steps, so no step is the last one, where the
    horizon rule offers eos only.  (Under a random LM at weight 1.5 casr_beam_lm runs all 40.)"""
    lm = NgramLM.from_ids(*R.arrays_of(GR.grammar_case(28.5)["grams"]), W2I, V)
    uni = Grammar.universal(V, EOS)
    e = _engine(28.5)
    try:
        if precision:
            e.set_precision(precision)
        _encode(e, ids=GR.UTTS)
        _same_as_unconstrained(e, k, lm, uni)
        assert e.device_flags() == 0
    finally:
        e.close()
        lm.close()
        uni.close()


def test_universal_grammar_reproduces_beam_on_the_folded_step():
    """B = 128, k = 8 (R = 1,024): casr_beam runs the folded step with its select inside the attention;
    the constrained beam runs the same steps with its select as a launch of its own.  eos_bias 40: the
    search of these 128 utterances ends after 2 steps (at 28.5 and at 33 it runs all 40, and the last step
    is the one the horizon rule changes)."""
    lm = NgramLM.from_ids(*R.arrays_of(GR.grammar_case(28.5)["grams"]), W2I, V)
    uni = Grammar.universal(V, EOS)
    e = _engine(40.0)
    try:
        _encode(e, 128, 48)
        _same_as_unconstrained(e, 8, lm, uni)
        assert e.device_flags() == 0
    finally:
        e.close()
        lm.close()
        uni.close()


def test_universal_grammar_over_all_forty_steps():
    """eos_bias 25: the plain search runs all max_len steps.  The horizon rule offers only eos at the last
    step, so the records of the steps before it equal casr_beam's and every answer is a record."""
    uni = Grammar.universal(V, EOS)
    e = _engine(25.0)
    try:
        _encode(e)
        beam = _np(e.beam(4))
        rt, rs, rv = _records(e)
        assert int(beam["steps"][0]) == LMAX
        z = _np(e.beam_grammar(uni, 4))
        zt, zs, zv = _records(e)
        assert int(z["steps"][0]) == LMAX and z["complete"].all() and rv[:, :LMAX - 1].any()
        assert np.array_equal(zv[:, :LMAX - 1], rv[:, :LMAX - 1]) and np.array_equal(zt[:, :LMAX - 1], rt[:, :LMAX - 1])
        assert np.array_equal(bits(zs[:, :LMAX - 1]), bits(rs[:, :LMAX - 1]))
        assert e.device_flags() == 0
    finally:
        e.close()
        uni.close()


# ---------------------------------------------------------------------------- 3. invariants
def _comb(a, q, l, with_lm, w=1.5, lw=1.5):
    r = F(a)
    if with_lm:
        r = F(r + F(F(w) * F(q)))
    return F(r + F(float(F(lw)) * float(l + 1)))


@pytest.mark.parametrize("k", [4, 16])
@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("eos_bias", GR.EOS_BIASES)
def test_invariants_on_the_devices_own_records(eos_bias, with_lm, k):
    case = GR.grammar_case(eos_bias)
    lang = case["lang"]
    g = Grammar.from_phrases(case["sentences"], {}, V, EOS)
    lm = NgramLM.from_ids(*R.arrays_of(case["grams"]), W2I, V) if with_lm else None
    ref = R.RefLM(4, V, case["grams"]) if with_lm else None
    e = _engine(eos_bias)
    try:
        _encode(e, ids=GR.UTTS)
        plain = _np(e.beam_lm(lm, k, 1.5, 1.5)) if with_lm else _np(e.beam(k, 0.0, 1.5))
        e.device_flags()
        r = _np(e.beam_grammar(g, k, lm, 1.5 if with_lm else 0.0, 1.5))
        rt, rs, rv = _records(e)
        rq = e.beam_record_lm().cpu().numpy() if with_lm else np.zeros_like(rs)
        assert e.device_flags() == 0
        steps = int(r["steps"][0])
        assert rv.any() and not rv[:, steps:].any() and r["complete"].all()
        for b, l, c in zip(*np.nonzero(rv)):
            y = rt[b, l, c, :l].tolist()
            assert (rt[b, l, c, l:] == -1).all() and lang.member(y), (b, l, c, y)
            if with_lm:
                assert bits(rq[b, l, c]) == bits(ref.sentence(y)), (b, l, c)
        differs = 0
        for b, got in enumerate(_answers(r)):
            assert lang.member(got) and (r["tokens"][b, r["length"][b]:] == -1).all()
            idx = [(l, c) for l in range(steps) for c in range(k) if rv[b, l, c]]
            vals = [_comb(rs[b, l, c], rq[b, l, c], l, with_lm) for l, c in idx]
            l, c = idx[int(np.argmax(vals))]
            assert got == rt[b, l, c, :l].tolist(), b
            assert bits(r["score"][b]) == bits(rs[b, l, c])
            if with_lm:
                assert bits(r["lm"][b]) == bits(rq[b, l, c])
            differs += got != plain["tokens"][b, :plain["length"][b]].tolist()
        assert differs >= 1, "the grammar never changed a choice"
        r2 = _np(e.beam_grammar(g, k, lm, 1.5 if with_lm else 0.0, 1.5))  # two runs: the same bits
        for n in r:
            if r[n] is not None:
                assert np.array_equal(r[n].view(np.uint8), r2[n].view(np.uint8)), n
        assert e.device_flags() == 0
    finally:
        e.close()
        g.close()
        if lm is not None:
            lm.close()


# ---------------------------------------------------------------------------- 4. against grammar_ref
@pytest.mark.parametrize("k", GR.GPU_K)
@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("eos_bias", GR.EOS_BIASES)
def test_constrained_beam_equals_the_numpy_restatement(eos_bias, with_lm, k):
    """Tokens and records exactly, scores within 2e-3, at the widths where tests/test_grammar_host.py has
    asserted that the restatement's smallest gap between adjacent ranked vals is >= 1e-2."""
    case = GR.grammar_case(eos_bias)
    want = GR.constrained_case(eos_bias, k, with_lm)
    assert (want["gap"] >= 1e-2).all()
    g = Grammar.from_phrases(case["sentences"], {}, V, EOS)
    lm = NgramLM.from_ids(*R.arrays_of(case["grams"]), W2I, V) if with_lm else None
    lw, nw = GR.WEIGHTS if with_lm else (0.0, 0.0)
    e = _engine(eos_bias)
    try:
        _encode(e, ids=GR.UTTS)
        r = _np(e.beam_grammar(g, k, lm, lw, nw))
        rt, rs, rv = _records(e)
        rq = e.beam_record_lm().cpu().numpy() if with_lm else None
        assert e.device_flags() == 0
        assert int(r["steps"][0]) == want["steps"] and r["complete"].all()
        for b, got in enumerate(_answers(r)):
            assert got == want["tokens"][b], b
            assert abs(r["score"][b] - want["score"][b]) <= 2e-3, b
            if with_lm:
                assert abs(r["lm"][b] - want["lm"][b]) <= 2e-3, b
            idx = [(l, c) for l in range(LMAX) for c in range(k) if rv[b, l, c]]
            assert [(rt[b, l, c, :l].tolist(), l) for l, c in idx] == [(t, l) for t, _, _, l in want["records"][b]], b
            for (l, c), (_, a, q, _) in zip(idx, want["records"][b]):
                assert abs(rs[b, l, c] - a) <= 2e-3, (b, l, c)
                if with_lm:
                    assert abs(rq[b, l, c] - q) <= 2e-3, (b, l, c)
    finally:
        e.close()
        g.close()
        if lm is not None:
            lm.close()


# ---------------------------------------------------------------------------- 5. the horizon
def test_the_horizon_keeps_every_row_able_to_finish():
    """An eos that can never win (eos_bias -60), B = 2, T = 48, k = 4 (tests/test_grammar_host.py checks the
    same on the restatement): a loop over ten tokens runs all max_len steps and ends with records at the last
    step only; a chain of exactly max_len - 1 tokens is returned whole (at k = 16 every list is shorter
    than 2k); a chain of max_len tokens has no candidate at all."""
    loop = Grammar([[(t, 0) for t in GR.LOOP_TOKENS]], [0], V, EOS)
    chain = GR.chain_tokens(LMAX - 1)
    fits = Grammar.from_phrases([chain], {}, V, EOS)
    longer = Grammar.from_phrases([GR.chain_tokens(LMAX)], {}, V, EOS)
    e = _engine(GR.HORIZON_EOS_BIAS)
    try:
        _encode(e, GR.HORIZON_B, GR.HORIZON_T)
        e.device_flags()
        r = _np(e.beam_grammar(loop, 4))
        rt, rs, rv = _records(e)
        assert int(r["steps"][0]) == LMAX and r["complete"].all()
        assert r["length"].tolist() == [LMAX - 1] * 2
        assert not rv[:, :LMAX - 1].any() and rv[:, LMAX - 1].all()
        assert all(set(y) <= set(GR.LOOP_TOKENS) for y in _answers(r))
        for k in (4, 16):
            r = _np(e.beam_grammar(fits, k))
            assert _answers(r) == [chain, chain] and r["complete"].all() and int(r["steps"][0]) == LMAX
            rt, rs, rv = _records(e)
            assert rv.sum() == 2 and rv[:, LMAX - 1, 0].all()
        r = _np(e.beam_grammar(longer, 4))
        assert r["length"].tolist() == [0, 0] and not r["complete"].any() and int(r["steps"][0]) == 1
        assert not r["score"].any() and (r["tokens"] == -1).all()
        assert not _records(e)[2].any()
        assert e.device_flags() == 0
    finally:
        e.close()
        for g in (loop, fits, longer):
            g.close()


@pytest.mark.parametrize("k", [2, 4])
def test_start_states_with_fewer_arcs_than_the_list_holds(k):
    """A start state with 1, 2k - 1, 2k or 2k + 1 arcs, each to a final state without arcs: the list of step
    0 is that short, step 1 offers one eos per live row, and the answer is the best of those records."""
    e = _engine(28.5)
    try:
        _encode(e)
        e.device_flags()
        for n in (1, 2 * k - 1, 2 * k, 2 * k + 1):
            toks = list(range(200, 200 + n))
            g = Grammar([[(t, 1) for t in toks], []], [1], V, EOS)
            r = _np(e.beam_grammar(g, k))
            assert r["complete"].all() and r["length"].tolist() == [1] * B
            assert int(r["steps"][0]) == 2
            rt, rs, rv = _records(e)
            assert not rv[:, 0].any() and (rv[:, 1].sum(axis=1) == min(k, n)).all() and not rv[:, 2:].any()
            for b, y in enumerate(_answers(r)):
                c = int(np.argmax(np.where(rv[b, 1], rs[b, 1], -np.inf)))
                assert y == rt[b, 1, c, :1].tolist() and y[0] in toks and bits(r["score"][b]) == bits(rs[b, 1, c])
            g.close()
        assert e.device_flags() == 0
    finally:
        e.close()


def test_two_utterances_answer_in_their_own_languages():
    case = GR.grammar_case(28.5)
    sents = case["sentences"]
    half = len(sents) // 2
    ga = Grammar.from_phrases(sents[:half], {}, V, EOS)
    gb = Grammar.from_phrases(sents[half:], {}, V, EOS)
    u, starts = Grammar.union([ga, gb])
    la, lb = GR.SetLanguage(sents[:half]), GR.SetLanguage(sents[half:])
    e = _engine(28.5)
    try:
        _encode(e, ids=GR.UTTS)
        e.device_flags()
        pick = [0, 1, 0, 1, 1, 0]
        r = _np(e.beam_grammar(u, 4, start=[starts[p] for p in pick]))
        assert r["complete"].all()
        for b, y in enumerate(_answers(r)):
            assert (lb if pick[b] else la).member(y) and not (la if pick[b] else lb).member(y), (b, y)
        assert e.device_flags() == 0
        # a start state outside the grammar: no candidate at all, and guard bit 1
        r = _np(e.beam_grammar(u, 4, start=[starts[0]] * 5 + [u.n_states]))
        assert r["complete"].tolist() == [1] * 5 + [0] and r["length"][5] == 0 and r["score"][5] == 0
        assert e.device_flags() == 1
    finally:
        e.close()
        for g in (ga, gb, u):
            g.close()


# ---------------------------------------------------------------------------- 6. refusals and state
def test_refusals_and_state():
    from casr.engine import Engine
    grams = R.random_model(3, V, 63)
    lm = NgramLM.from_ids(*R.arrays_of(grams), {}, V)
    g = Grammar.universal(V, EOS)
    small = Grammar.universal(100, EOS)
    other_eos = Grammar.universal(V, 5)
    e = _engine(28.5)
    e2 = Engine(CFG)
    try:
        e.device_flags()
        dev = e.device
        out = dict(t=torch.full((B, LMAX), 77, dtype=torch.int32, device=dev),
                   n=torch.full((B,), 77, dtype=torch.int32, device=dev), s=torch.full((B,), 77.0, device=dev),
                   q=torch.full((B,), 77.0, device=dev), c=torch.full((B,), 77, dtype=torch.uint8, device=dev),
                   st=torch.full((1,), 77, dtype=torch.int32, device=dev))
        ptr = lambda x: x.data_ptr()  # noqa: E731

        def call(eng, gp, k, lmp=None, c="c"):
            return eng.lib.casr_beam_grammar(eng.handle, gp, lmp, None, k, 1.5, 1.5, ptr(out["t"]), ptr(out["n"]),
                                             ptr(out["s"]), ptr(out["q"]), ptr(out[c]) if c else None, ptr(out["st"]),
                                             None)

        assert call(e, g.on(e), 4) == 3  # before an encode: CASR_ERR_STATE
        assert call(e2, g.on(e2), 4) == 3  # before weights are bound
        _encode(e)
        assert call(e, None, 4) == 1
        assert call(e, g._host, 4) == 1  # host-only
        assert call(e, small.on(e), 4) == 1  # vocab mismatch
        assert call(e, other_eos.on(e), 4) == 1  # eos mismatch
        assert "eos" in e.lib.casr_last_error(e.handle).decode()
        assert call(e, g.on(e), 4, lm._host) == 1  # a host-only LM
        assert call(e, g.on(e), 0) == 1 and call(e, g.on(e), 17) == 1
        assert call(e, g.on(e), 4, c=None) == 1  # a NULL output
        st = torch.zeros(2, dtype=torch.int32, device=dev)
        rows = torch.full((2, 160), 77, dtype=torch.int32, device=dev)
        for gp in (None, g._host, small.on(e), other_eos.on(e)):
            assert e.lib.casr_grammar_rows(e.handle, gp, ptr(st), ptr(st), 2, ptr(rows), None) == 1
            assert e.lib.casr_grammar_accept(e.handle, gp, ptr(rows), ptr(st), 2, 8, ptr(st), None, None, None) == 1
        assert e.lib.casr_grammar_rows(e.handle, g.on(e), None, ptr(st), 2, ptr(rows), None) == 1
        assert e.lib.casr_grammar_rows(e.handle, g.on(e), ptr(st), None, 2, ptr(rows), None) == 1
        for bad_l in (0, 513):
            assert e.lib.casr_grammar_accept(e.handle, g.on(e), ptr(rows), ptr(st), 2, bad_l, ptr(st), None, None,
                                             None) == 4
        torch.cuda.synchronize()
        assert all(bool((x == 77).all()) for x in out.values()) and bool((rows == 77).all())
        # state: the readers that assume a plain beam refuse a grammar beam; record_lm needs its LM
        e.beam_grammar(g, 4)
        e.beam_records()
        for refused in (lambda: e.beam_record_lm(), lambda: e.beam_rescore(lm, 1.5, 1.5), lambda: e.beam_mbr(0.5),
                        lambda: e.beam_nbest(3), lambda: e.beam_confusion(2), lambda: e.beam_record_bias()):
            with pytest.raises(L.CasrError, match="CASR_ERR_STATE"):
                refused()
        e.beam_grammar(g, 4, lm, 1.5, 1.5)
        e.beam_record_lm()
        e.beam_records()
        for refused in (lambda: e.beam_rescore(lm, 1.5, 1.5), lambda: e.beam_mbr(0.5), lambda: e.beam_nbest(3),
                        lambda: e.beam_confusion(2)):
            with pytest.raises(L.CasrError, match="casr_beam_grammar"):
                refused()
        e.beam(4)  # casr_beam restores the readers
        e.beam_rescore(lm, 1.5, 1.5)
        e.beam_mbr(0.5)
        e.beam_nbest(3)
        e.beam_confusion(2)
        assert e.device_flags() == 0
    finally:
        e.close()
        e2.close()
        lm.close()
        for x in (g, small, other_eos):
            x.close()


# ---------------------------------------------------------------------------- 7. the Python layers
def test_model_and_parse_batch_run_the_constrained_beam_on_request():
    import main as MAIN
    import model as M
    case = GR.grammar_case(28.5)
    lang = case["lang"]
    m = M.Model()
    m.load_state_dicts(case["enc_sd"], case["dec_sd"])
    dev = m.device
    feats = [torch.from_numpy(f).to(dev) for f in case["feats"]]
    lens = torch.tensor(case["lens"])
    first = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, second_pass=False)
    off = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, second_pass=False, grammar=None, grammar_start=None)
    assert off.pred_text == first.pred_text and off.score == first.score  # unchanged defaults: the plain results
    g = Grammar.from_phrases(case["sentences"], {}, V, EOS)
    kw = dict(second_pass=False, lm_weight=1.5, length_weight=1.5)
    got = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, grammar=g, **kw)
    r = _np(m.engine.beam_grammar(g, 4, None, 0.0, 1.5))
    want = ["".join(I2W[t] for t in y) for y in _answers(r)]
    assert got.pred_text == want and all(lang.member(y) for y in _answers(r))
    assert np.array_equal(bits(np.array(got.score, np.float32)), bits(r["score"]))
    assert got.pred_text != first.pred_text, "the grammar never changed a choice"
    timed = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, grammar=g, timestamps=True, **kw)
    assert timed.pred_text == want and [len(t) for t in timed.timing] == [len(w) for w in want]
    u, starts = Grammar.union([g, Grammar.universal(V, EOS)])
    per = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, grammar=u, grammar_start=[starts[0]] * B, **kw)
    assert per.pred_text == want
    from casr.bias import PhraseBias
    pb = PhraseBias([[5, 6]], {}, V)
    for bad in (dict(bias=pb), dict(mbr=0.5), dict(nbest=3), dict(alternatives=2)):
        with pytest.raises(ValueError):
            m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, grammar=g, **dict(kw, **bad))
    with pytest.raises(ValueError, match="second pass"):
        m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, grammar=g, second_pass=True, lm_model=object())

    # main.parse_batch: the same call behind the file front end (features_for and read_audio stubbed out)
    class _AB:
        int2word, word2int = I2W, W2I

    keep = MAIN.features_for, MAIN.read_audio
    MAIN.features_for, MAIN.read_audio = (lambda audios: (feats, lens)), (lambda paths: paths)
    try:
        assert MAIN.parse_batch(["a"] * B, m, _AB, bw=4, grammar=g) == want
        assert MAIN.parse(["a"], m, _AB, None, 4, grammar=g) == want[0]
    finally:
        MAIN.features_for, MAIN.read_audio = keep
    for x in (g, u, pb):
        x.close()
