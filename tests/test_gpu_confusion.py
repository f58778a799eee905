"""N-best lists and confusion networks on the device (include/casr.h casr_confusion, casr_beam_nbest,
casr_beam_confusion; csrc/confusion.hip) against the host entries, which tests/test_confusion_host.py pins
to the Python restatement of the formulas; and the drop-in Model's ``nbest`` / ``alternatives`` keywords.

The beam is test_gpu_ngram.py's batch (B = 6, T = 101, synthetic peaked weights, eos_bias 25): some
utterances finish many hypotheses, one finishes none."""
import numpy as np
import pytest
import torch

import confusion_ref as R
from golden_util import fbank_for
from casr import lib as L
from casr.results import confusion_slots, records_by_utterance
from casr.weights import synthetic_state_dicts
from test_gpu_ngram import B, CFG, I2W, T, _encode, _engine, _lm_from_records

pytestmark = pytest.mark.gpu

V = CFG.vocab
CN = ("n_slots", "slot_token", "slot_mass", "pivot_mass", "total")


def _np(d):
    return {n: (v.cpu().numpy() if v is not None else None) for n, v in d.items()}


def _same(got, want, what=""):
    for n in CN:
        assert got[n].dtype == want[n].dtype and np.array_equal(got[n], want[n]), (what, n)


def test_device_confusion_equals_host_on_the_seeded_and_hand_cases():
    from casr.engine import Engine
    e = Engine(CFG)  # no weights, no encode
    try:
        rt, rv, ru, pv = R.seeded_cases()
        _same(_np(e.confusion(rt, rv, ru, pv, R.V, 4)), L.confusion_host(rt, rv, ru, pv, R.V, 4), "seeded")
        assert e.device_flags() == 0
        rt, rv, ru, pv = R.hand_cases()
        bad = R.HAND.index("token outside [0, V)")
        keep = [b for b in range(len(pv)) if b != bad]
        for M in (1, 4, 8):
            _same(_np(e.confusion(rt[keep], rv[keep], ru[keep], pv[keep], R.V, M)),
                  L.confusion_host(rt[keep], rv[keep], ru[keep], pv[keep], R.V, M), M)
        assert e.device_flags() == 0
        got = _np(e.confusion(rt, rv, ru, pv, R.V, 8))
        _same(got, L.confusion_host(rt, rv, ru, pv, R.V, 8), "hand")
        assert e.device_flags() == 1  # the out-of-range ids, nothing else
        assert got["n_slots"].tolist() == [0, 7, 1, 0, 0, 7, 0]
        # the other path of the plan: 64 lanes past the LDS (52 work), both kernels past 64 KB, two align
        # workgroups per utterance
        rs = np.random.RandomState(3)
        Lb, kb, Vb = 100, 2, 9000
        rt = np.full((2, Lb, kb, Lb), -1, np.int32)
        rv = (rs.rand(2, Lb, kb) < 0.3).astype(np.uint8)
        ru = np.asarray(R.UNITS, np.int64)[rs.randint(len(R.UNITS), size=(2, Lb, kb))]
        base = rs.randint(0, Vb, size=Lb)
        for b, l, c in zip(*np.nonzero(rv)):
            rt[b, l, c, :l] = np.where(rs.rand(l) < 0.8, base[:l], rs.randint(0, Vb, size=l))
        assert rv[0].sum() > 52
        pv = np.array([np.flatnonzero(rv[b].reshape(-1))[-3] for b in range(2)], np.int32)
        got = _np(e.confusion(rt, rv, ru, pv, Vb, 4))
        _same(got, L.confusion_host(rt, rv, ru, pv, Vb, 4), "L = 100")
        assert (got["slot_token"][:, :, 1] >= 0).any() and e.device_flags() == 0
        for args in ((rt, rv, ru, pv, Vb, 0), (rt, rv, ru, pv, Vb, 9)):
            with pytest.raises(L.CasrError, match="CASR_ERR_ARG"):
                e.confusion(*args)
        with pytest.raises(L.CasrError, match="CASR_ERR_UNSUPPORTED"):
            e.confusion(rt, rv, ru, pv, 40000, 4)
    finally:
        e.close()


def _check_network(e, rt, rs, rv, M, scale, pivot, host_pivot, rec_lm, lmw, lw):
    """casr_beam_confusion against casr_confusion_host on the device's records and the device's units."""
    r = _np(e.beam_confusion(M, scale, lm_weight=lmw, length_weight=lw, pivot=pivot, units=True,
                             rec_lm=None if rec_lm is None else torch.from_numpy(rec_lm).to(e.device)))
    hu, _ = L.posterior_units_host(rs, rv, scale, rec_lm=rec_lm, lm_weight=lmw, length_weight=lw)
    assert np.abs(r["rec_unit"] - hu).max() <= 1 and not r["rec_unit"][rv == 0].any()
    assert np.array_equal(r["total"], r["rec_unit"].reshape(B, -1).sum(1))
    _same(r, L.confusion_host(rt, rv, r["rec_unit"], host_pivot, V, M), (M, scale))
    none = ~rv.reshape(B, -1).astype(bool).any(1)
    assert none.any() and not r["n_slots"][none].any() and (r["n_slots"][~none] > 0).all()
    return r


@pytest.mark.parametrize("k,precision", [(2, None), (4, None), (16, None), (4, "f32")])
def test_beam_nbest_and_confusion_equal_host_on_device_records(k, precision):
    e = _engine(25.0)
    try:
        if precision:
            e.set_precision(precision)
        _encode(e)
        e.beam(k, 1.5, 1.5)
        before = [x.cpu() for x in e.beam_records()]
        rt, rs, rv = (x.numpy() for x in before)
        recs = records_by_utterance(rt, rs, rv)
        count = np.array([len(recs.get(b, [])) for b in range(B)])
        assert (count >= 2).sum() >= 3 and (count == 0).any(), count  # else the test would pass vacuously
        e.device_flags()
        grams, lm, ref = _lm_from_records(recs, 900 + k)
        rec_lm = e.beam_rescore(lm, 1.5, 1.5, records=True)["rec_lm"].cpu().numpy()
        for N, rl, lmw, lw in ((1, None, 0.0, 0.0), (8, None, 0.0, 1.5), (64, rec_lm, 1.5, 1.5)):
            got = _np(e.beam_nbest(N, lm_weight=lmw, length_weight=lw,
                                   rec_lm=None if rl is None else torch.from_numpy(rl).to(e.device)))
            want = L.nbest_host(rt, rs, rv, N, rec_lm=rl, lm_weight=lmw, length_weight=lw)
            for n in ("index", "tokens", "length"):
                assert np.array_equal(got[n], want[n]), (n, N)
            assert np.array_equal(got["comb"].view(np.int64), want["comb"].view(np.int64)), N
            assert np.array_equal((got["index"] >= 0).sum(1), np.minimum(count, N))
        for scale in (0.0, 0.5, 1e6):
            top = L.nbest_host(rt, rs, rv, 1, length_weight=1.5)["index"][:, 0]
            r = _check_network(e, rt, rs, rv, 4, scale, None, top, None, 0.0, 1.5)
            if scale == 0.0:  # distinct records with equal units: some slot has two entries
                assert (r["slot_token"][:, :, 1] != L.CN_NONE).any()
            idx = e.beam_mbr(scale, length_weight=1.5)["index"]
            _check_network(e, rt, rs, rv, 8, scale, idx, idx.cpu().numpy(), None, 0.0, 1.5)
        top = L.nbest_host(rt, rs, rv, 1, rec_lm=rec_lm, lm_weight=1.5, length_weight=1.5)["index"][:, 0]
        _check_network(e, rt, rs, rv, 1, 0.5, None, top, rec_lm, 1.5, 1.5)
        assert e.device_flags() == 0
        after = [x.cpu() for x in e.beam_records()]  # the beam state is only read
        for x, y in zip(before, after):
            assert torch.equal(x, y)
        lm.close()
    finally:
        e.close()


def test_state_and_argument_errors():
    from casr.engine import Engine
    e = _engine(25.0)
    e2 = Engine(CFG)
    try:
        e2._B, e2._k = B, 4
        for call in (lambda: e2.beam_nbest(4), lambda: e2.beam_confusion(4)):
            with pytest.raises(L.CasrError, match="CASR_ERR_STATE"):
                call()
        _encode(e)
        e.beam(4)
        recs = records_by_utterance(*(x.cpu().numpy() for x in e.beam_records()))
        grams, lm, ref = _lm_from_records(recs, 78)
        for call in (lambda: e.beam_nbest(0), lambda: e.beam_nbest(65), lambda: e.beam_confusion(0),
                     lambda: e.beam_confusion(9), lambda: e.beam_confusion(4, -0.5),
                     lambda: e.beam_confusion(4, float("nan")), lambda: e.beam_confusion(4, float("inf"))):
            with pytest.raises(L.CasrError, match="CASR_ERR_ARG"):
                call()
        e.beam_lm(lm, 4, 0.5, 0.5)
        for call in (lambda: e.beam_nbest(4), lambda: e.beam_confusion(4)):
            with pytest.raises(L.CasrError, match="CASR_ERR_STATE"):
                call()
        e.beam(4)
        e.beam_nbest(4)
        e.beam_confusion(4)
        assert e.device_flags() == 0
        lm.close()
    finally:
        e.close()
        e2.close()


class _ScoreOnly:
    def score(self, s, bos=True):
        return 0.0


def test_model_nbest_and_alternatives_keywords():
    import model as M
    from oracle import casr_oracle as O
    m = M.Model()
    enc_sd, dec_sd = synthetic_state_dicts(CFG, peaked=True, eos_bias=25.0)
    m.load_state_dicts(enc_sd, dec_sd)
    dev = m.device
    feats = [torch.from_numpy(O.features_from_fbank(fbank_for(b, T))).to(dev) for b in range(B)]
    lens = torch.tensor([f.shape[0] for f in feats])
    plain = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, second_pass=False, length_weight=1.5)
    assert type(plain).__name__ == "EvalOutput"
    r = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, second_pass=False, length_weight=1.5, nbest=5,
                                   alternatives=4)
    assert type(r).__name__ == "BeamEvalOutput" and len(r) == 9 and r._fields[-1] == "timing"
    pred_text, score, text, wer, n, alignment, audio_feat_len, text_len, timing = r
    assert pred_text == plain.pred_text and score == plain.score and n == B
    rv = m.engine.beam_records()[2].cpu().numpy()
    count = rv.reshape(B, -1).sum(1)
    assert (count >= 2).sum() >= 3 and (count == 0).any()
    eng = _np(m.engine.beam_confusion(4, 1.0))
    assert r.alternatives == confusion_slots(eng["slot_token"], eng["slot_mass"], eng["n_slots"], eng["total"], I2W)
    nb = _np(m.engine.beam_nbest(5))
    several = 0
    for b in range(B):
        if not count[b]:  # the fallback text, nothing to list
            assert r.nbest[b] == [] and r.alternatives[b] == []
            continue
        assert len(r.nbest[b]) == min(5, count[b]) and r.nbest[b][0][0] == pred_text[b]
        comb = [c for _, c in r.nbest[b]]
        assert comb == sorted(comb, reverse=True)
        # the pivot is the answer: its characters join to pred_text, and each has a slot of its own
        pivot = nb["tokens"][b, 0, :nb["length"][b, 0]].tolist()
        assert "".join(I2W[t] for t in pivot) == pred_text[b] and eng["n_slots"][b] == 2 * len(pivot) + 1
        assert len(r.alternatives[b]) >= len(pivot) and (eng["pivot_mass"][b, :len(pivot)] > 0).all()
        for slot in r.alternatives[b]:
            probs = [p for _, p in slot]
            assert slot and all(0 < p <= 1 for p in probs) and sum(probs) <= 1 + 1e-12
            assert probs == sorted(probs, reverse=True)
        several += any(len(slot) > 1 for slot in r.alternatives[b])
    assert several >= 1
    # with mbr the pivot is the MBR choice
    rm = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, second_pass=False, length_weight=1.5, mbr=0.5,
                                    alternatives=2, posterior_scale=0.5)
    mb = _np(m.engine.beam_mbr(0.5, length_weight=1.5))
    eng = _np(m.engine.beam_confusion(2, 0.5, length_weight=1.5, pivot=torch.from_numpy(mb["index"])))
    assert rm.nbest is None
    assert rm.alternatives == confusion_slots(eng["slot_token"], eng["slot_mass"], eng["n_slots"], eng["total"], I2W)
    for b in range(B):
        assert eng["n_slots"][b] == (2 * mb["length"][b] + 1 if count[b] else 0)
    # with an NgramLM and second_pass the answer, the order and the posterior are the second pass's
    recs = records_by_utterance(*(x.cpu().numpy() for x in m.engine.beam_records()))
    grams, lm, ref = _lm_from_records(recs, 92)
    r2 = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, second_pass=True, lm_model=lm, lm_weight=1.5,
                                    length_weight=1.5, nbest=3)
    assert r2.alternatives is None
    for b in range(B):
        assert (r2.nbest[b][0][0] == r2.pred_text[b]) if count[b] else r2.nbest[b] == []
    with pytest.raises(TypeError):
        m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, lm_model=_ScoreOnly(), nbest=3)
    with pytest.raises(ValueError):
        m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, lm_model=lm, fusion=True, alternatives=3)
    lm.close()
