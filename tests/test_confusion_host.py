"""The three host entries of the N-best / confusion-network operation (include/casr.h
casr_posterior_units_host, casr_nbest_host, casr_confusion_host; csrc/confusion_plan.h) against the Python
restatement of the formulas in tests/confusion_ref.py: hand cases and 200 seeded ones, every output exactly
(the units within 1: exp is the platform's).  No GPU."""
import numpy as np
import pytest

import confusion_ref as R
from casr import lib as L


@pytest.fixture(scope="module")
def seeded():
    rt, rv, ru, pv = R.seeded_cases()
    want, full = R.confusion(rt, rv, ru, pv, R.V, 4)
    return (rt, rv, ru, pv), want, full


def _same(got, want, what=""):
    for n in ("n_slots", "slot_token", "slot_mass", "pivot_mass", "total"):
        assert got[n].dtype == want[n].dtype and np.array_equal(got[n], want[n]), (what, n)


def test_seeded_cases_equal_the_reference_and_are_not_vacuous(seeded):
    (rt, rv, ru, pv), want, full = seeded
    _same(L.confusion_host(rt, rv, ru, pv, R.V, 4), want)
    two, gap, odd, many, tie, slots = R.slot_stats(full)
    print("slots", slots, "two", two, "gap", gap, "odd-eps", odd, "many", many, "tie", tie)
    assert min(two, gap, odd, many, tie) >= 100, (two, gap, odd, many, tie, slots)
    # every slot's masses over ALL tokens sum to U, and the entries are the head of that list
    for b, utt in enumerate(full):
        assert len(utt) == want["n_slots"][b]
        for mass in utt:
            assert sum(mass.values()) == want["total"][b]


@pytest.mark.parametrize("M", [1, 8])
def test_m_1_and_m_8(seeded, M):
    (rt, rv, ru, pv), _, _ = seeded
    want, _ = R.confusion(rt[:40], rv[:40], ru[:40], pv[:40], R.V, M)
    got = L.confusion_host(rt[:40], rv[:40], ru[:40], pv[:40], R.V, M)
    _same(got, want, M)
    assert got["slot_token"].shape == (40, 2 * R.L + 1, M)
    if M == 8:
        assert (got["slot_token"][:, :, 4:] != R.NONE).any()


def test_hand_cases():
    rt, rv, ru, pv = R.hand_cases()
    for M in (1, 4, 8):
        want, full = R.confusion(rt, rv, ru, pv, R.V, M)
        got = L.confusion_host(rt, rv, ru, pv, R.V, M)
        _same(got, want, M)
    h = {n: i for i, n in enumerate(R.HAND)}
    n_slots = got["n_slots"]
    for name in ("no record", "pivot -1", "pivot on an invalid record", "pivot index past the tree"):
        b = h[name]
        assert n_slots[b] == 0 and (got["slot_token"][b] == R.NONE).all() and not got["slot_mass"][b].any()
        assert not got["pivot_mass"][b].any()
    assert got["total"][h["no record"]] == 0 and got["total"][h["pivot -1"]] == 5 + R.ONE
    b = h["one record"]
    assert n_slots[b] == 7 and got["slot_token"][b, :7, 0].tolist() == [-1, 1, -1, 2, -1, 3, -1]
    assert (got["slot_mass"][b, :7, 0] == 12345).all() and got["pivot_mass"][b, :3].tolist() == [12345] * 3
    b = h["empty pivot"]  # S = 1: the gap holds EPS from the pivot and the records' first tokens
    assert n_slots[b] == 1 and got["slot_token"][b, 0, :3].tolist() == [-1, 6, 4]
    assert got["slot_mass"][b, 0, :3].tolist() == [R.ONE, 9, 7]
    b = h["token outside [0, V)"]  # V and -5 are 0: all three records agree on [1, 0, 2]
    assert got["slot_token"][b, 3, :2].tolist() == [0, R.NONE] and got["pivot_mass"][b, 1] == got["total"][b]


def test_units_and_nbest_against_the_reference():
    rt, sc, rv, lm = R.scored_cases()
    for scale, rl, lmw, lw in ((0.0, None, 0.0, 1.5), (0.5, lm, 0.4, 0.7), (1e6, lm, 0.4, 0.0), (1.0, None, 0.0, 0.0)):
        unit, total = L.posterior_units_host(sc, rv, scale, rec_lm=rl, lm_weight=lmw, length_weight=lw)
        want = R.posterior_units(sc, rv, rl, scale, lmw, lw)
        assert np.abs(unit - want).max() <= 1 and not unit[rv == 0].any()
        assert np.array_equal(total, unit.reshape(len(unit), -1).sum(1))
        if scale == 0.0:  # exp(0) = 1 exactly: every record with a c that is no NaN has the whole unit
            assert set(np.unique(unit[rv > 0])) <= {0, R.ONE}
        for N in (1, 5, 64):
            got = L.nbest_host(rt, sc, rv, N, rec_lm=rl, lm_weight=lmw, length_weight=lw)
            ref = R.nbest(rt, sc, rv, rl, N, lmw, lw)
            for n in ("index", "tokens", "length"):
                assert np.array_equal(got[n], ref[n]), (n, N)
            assert np.array_equal(got["comb"].view(np.int64), ref["comb"].view(np.int64)), N
    # the record at c_max has 2^32
    unit, _ = L.posterior_units_host(sc, rv, 0.5)
    for b in range(len(rv)):
        ok = rv[b].astype(bool) & ~np.isnan(sc[b])
        if ok.any() and np.isfinite(sc[b][ok].max()):
            assert unit[b][ok].max() == R.ONE
    assert not rv[0].any() and (L.nbest_host(rt, sc, rv, 3)["index"][0] == -1).all()


def test_argument_errors():
    rt, rv, ru, pv = R.hand_cases()
    sc = np.zeros(rv.shape, np.float32)
    for M in (0, 9):
        with pytest.raises(L.CasrError, match="CASR_ERR_ARG"):
            L.confusion_host(rt, rv, ru, pv, R.V, M)
    for N in (0, 65):
        with pytest.raises(L.CasrError, match="CASR_ERR_ARG"):
            L.nbest_host(rt, sc, rv, N)
    for scale in (-1.0, float("nan"), float("inf")):
        with pytest.raises(L.CasrError, match="CASR_ERR_ARG"):
            L.posterior_units_host(sc, rv, scale)
    with pytest.raises(L.CasrError, match="CASR_ERR_ARG"):
        L.confusion_host(rt, rv, ru, pv, 0, 4)


def test_confusion_slots_and_the_result_type():
    from casr.results import BeamEvalOutput, EvalOutput, confusion_slots
    rt, rv, ru, pv = R.hand_cases()
    b = R.HAND.index("empty pivot")
    ru[b, 0, 2] = 100  # the pivot no longer outweighs the inserts into its one gap
    got = L.confusion_host(rt, rv, ru, pv, R.V, 4)
    i2w = {i: chr(ord("a") + i) for i in range(R.V)}
    slots = confusion_slots(got["slot_token"], got["slot_mass"], got["n_slots"], got["total"], i2w)
    assert slots[R.HAND.index("no record")] == [] and slots[R.HAND.index("pivot -1")] == []
    assert slots[b] == [[("", 100 / 116), ("g", 9 / 116), ("e", 7 / 116)]]
    assert confusion_slots(got["slot_token"], got["slot_mass"], got["n_slots"], got["total"], i2w, min_gap=0.2)[b] == []
    one = slots[R.HAND.index("one record")]  # gaps of EPS alone are dropped, every pivot character stays
    assert one == [[("b", 1.0)], [("c", 1.0)], [("d", 1.0)]]
    base = EvalOutput(["x"], [0.5], None, None, 1, None, None, None)
    r = BeamEvalOutput(*base, nbest=[[("x", 0.5)]], alternatives=[[[("x", 1.0)]]])
    assert isinstance(r, EvalOutput) and len(r) == 9 and r._fields == EvalOutput._fields and r.timing is None
    pred_text, score, text, wer, n, alignment, audio_feat_len, text_len, timing = r
    assert pred_text == ["x"] and r.nbest == [[("x", 0.5)]] and r.alternatives[0][0] == [("x", 1.0)]
    import copy
    import pickle
    for q in (pickle.loads(pickle.dumps(r)), copy.copy(r), copy.deepcopy(r), r._replace(n=2)):
        assert type(q) is BeamEvalOutput and q.pred_text == ["x"] and q.nbest == r.nbest and q.alternatives == r.alternatives
    assert r._replace(n=2).n == 2 and r._replace(nbest=None).nbest is None and r._replace(nbest=None) == r
    made = BeamEvalOutput._make(base)  # a namedtuple's own constructor: the attributes read as not asked for
    assert made == base and made.nbest is None and made.alternatives is None
