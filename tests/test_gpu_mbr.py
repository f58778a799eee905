"""The minimum-Bayes-risk choice over a beam's finished hypotheses on the device (include/casr.h
casr_beam_mbr; csrc/edit.hip) against casr_mbr_host on the device's own records, which
tests/test_edit_host.py pins to the numpy restatement of the formulas; and the drop-in Model: the WER of
an evaluation through wer_batch, and the ``mbr`` keyword.

The batch is test_gpu_ngram.py's (B = 6, T = 101, synthetic peaked weights, eos_bias 25): some
utterances finish many hypotheses, one finishes none and keeps casr_beam's fallback."""
import numpy as np
import pytest
import torch

import edit_ref as R
from golden_util import fbank_for
from casr import lib as L
from casr.results import get_wer, records_by_utterance
from casr.weights import synthetic_state_dicts
from test_gpu_ngram import B, CFG, I2W, T, _encode, _engine, _lm_from_records, bits

pytestmark = pytest.mark.gpu

MAXL = CFG.max_len


def _np(d):
    return {n: (v.cpu().numpy() if v is not None else None) for n, v in d.items()}


def _check_against_host(r, rt, rs, rv, beam, k, scale, rec_lm, lm_weight, length_weight):
    """The device's choice, tokens, score and risks against casr_mbr_host on the same records; returns
    how many utterances the near-tie rule excused."""
    best, risk = L.mbr_host(rt, rs, rv, scale, rec_lm=rec_lm, lm_weight=lm_weight, length_weight=length_weight,
                            risk=True)
    valid = rv.astype(bool)
    assert np.all(r["rec_risk"][~valid] == 0)
    assert np.allclose(r["rec_risk"][valid], risk[valid], rtol=1e-12, atol=0)
    excused = 0
    for b in range(B):
        i = int(r["index"][b])
        n = r["length"][b]
        assert (r["tokens"][b, n:] == -1).all()
        if not valid[b].any():  # no record: casr_beam's unfinished fallback, bit for bit
            assert i == -1 and best[b] == -1 and r["risk"][b] == 0
            assert np.array_equal(r["tokens"][b], beam["tokens"][b]) and n == beam["length"][b]
            assert bits(r["score"][b]) == bits(beam["score"][b])
            continue
        if i != best[b]:
            assert R.near_tie(risk[b].reshape(-1)[valid[b].reshape(-1)], int(valid[b].reshape(-1)[:best[b]].sum())), b
            excused += 1
        l, c = divmod(i, k)
        assert valid[b, l, c] and n == l
        assert r["tokens"][b, :n].tolist() == rt[b, l, c, :l].tolist()
        assert bits(r["score"][b]) == bits(rs[b, l, c])
        assert r["risk"][b] == r["rec_risk"][b, l, c]
    return excused


@pytest.mark.parametrize("k,precision", [(2, None), (4, None), (16, None), (4, "f32")])
def test_device_mbr_equals_host_on_device_records(k, precision):
    e = _engine(25.0)
    try:
        if precision:
            e.set_precision(precision)
        _encode(e)
        beam = _np(e.beam(k, 1.5, 1.5))
        before = [x.cpu() for x in e.beam_records()]
        rt, rs, rv = (x.numpy() for x in before)
        recs = records_by_utterance(rt, rs, rv)
        count = np.array([len(recs.get(b, [])) for b in range(B)])
        assert (count >= 2).sum() >= 3 and (count == 0).any(), count  # else the test would pass vacuously
        e.device_flags()
        excused = 0
        for scale in (0.0, 0.5, 1e6):
            r = _np(e.beam_mbr(scale, length_weight=1.5, records=True))
            excused += _check_against_host(r, rt, rs, rv, beam, k, scale, None, 0.0, 1.5)
            if scale == 0.5:
                half = r
        assert excused <= 3 * B // 100
        # both mappings: the same distances (the host's), the same risks bit for bit
        per_map = {}
        for mp in (1, 2):
            e.set_option("MBR_MAP", mp)
            r = _np(e.beam_mbr(0.5, length_weight=1.5, records=True))
            dist, n_rec = (x.cpu().numpy() for x in e.beam_mbr_distances())
            per_map[mp] = (r, dist)
            assert np.array_equal(n_rec, count)
        e.set_option("MBR_MAP", 0)
        assert np.array_equal(per_map[1][1], per_map[2][1])
        for n in ("tokens", "length", "index"):
            assert np.array_equal(per_map[1][0][n], per_map[2][0][n]) and np.array_equal(per_map[1][0][n], half[n])
        for n in ("risk", "rec_risk"):
            assert np.array_equal(per_map[1][0][n].view(np.int64), per_map[2][0][n].view(np.int64))
        for b in range(B):
            toks = [t for t, _ in recs.get(b, [])]
            n = len(toks)
            rows, ln, _, _ = R.pad_pairs([(t, []) for t in toks], MAXL, 1)
            i, j = (x.reshape(-1) for x in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
            want = L.edit_distance_host(rows[i], ln[i], rows[j], ln[j]).reshape(n, n)
            assert np.array_equal(per_map[1][1][b, :n, :n], want), b
            assert not per_map[1][1][b, n:].any() and not per_map[1][1][b, :, n:].any()
        assert e.device_flags() == 0
        _with_the_lm(e, k, beam, rt, rs, rv, recs, count)
        # the beam state is only read
        after = [x.cpu() for x in e.beam_records()]
        for x, y in zip(before, after):
            assert torch.equal(x, y)
    finally:
        e.close()


def _with_the_lm(e, k, beam, rt, rs, rv, recs, count):
    """With an NgramLM of test_gpu_ngram.py's recipe in c: scale = 1e6 is the second pass wherever its
    maximum is unique, and at scale = 0.5 at least one choice differs from the first pass's."""
    grams, lm, ref = _lm_from_records(recs, 500 + k)
    second = _np(e.beam_rescore(lm, 1.5, 1.5, records=True))
    r = _np(e.beam_mbr(1e6, lm, 1.5, 1.5, records=True))
    assert e.device_flags() == 0
    assert np.array_equal(bits(r["rec_lm"]), bits(second["rec_lm"]))
    excused = _check_against_host(r, rt, rs, rv, beam, k, 1e6, second["rec_lm"], 1.5, 1.5)
    unique = 0
    for b in range(B):
        v = rv[b].reshape(-1).astype(bool)
        if not v.any():
            continue
        ls = np.flatnonzero(v) // k
        c = (rs[b].reshape(-1)[v].astype(np.float64) + 1.5 * second["rec_lm"][b].reshape(-1)[v].astype(np.float64)) \
            + 1.5 * ls.astype(np.float64)
        if (c == c.max()).sum() == 1:
            unique += 1
            assert r["length"][b] == second["length"][b] and np.array_equal(r["tokens"][b], second["tokens"][b]), b
            assert bits(r["score"][b]) == bits(second["score"][b])
    assert unique >= 3
    half = _np(e.beam_mbr(0.5, lm, 1.5, 1.5, records=True))
    again = _np(e.beam_mbr(0.5, lm, 1.5, 1.5, records=True))
    for n in half:
        assert np.array_equal(half[n].view(np.uint8), again[n].view(np.uint8)), n  # a second call: the same bits
    excused += _check_against_host(half, rt, rs, rv, beam, k, 0.5, second["rec_lm"], 1.5, 1.5)
    assert excused <= 2 * B // 100
    first = np.array([int(np.argmax(np.where(rv[b].reshape(-1), rs[b].reshape(-1), -np.inf))) if count[b] else -1
                      for b in range(B)])
    assert (half["index"] != first).any(), "the MBR choice never differed from the first pass's"
    lm.close()


def test_mbr_state_errors():
    from casr.engine import Engine
    e = _engine(25.0)
    e2 = Engine(CFG)
    try:
        with pytest.raises(L.CasrError, match="CASR_ERR_STATE"):
            e2._B, e2._k = B, 4
            e2.beam_mbr(0.5)
        _encode(e)
        e.beam(4)
        recs = records_by_utterance(*(x.cpu().numpy() for x in e.beam_records()))
        grams, lm, ref = _lm_from_records(recs, 77)
        with pytest.raises(L.CasrError, match="CASR_ERR_STATE"):
            e.beam_mbr_distances()
        e.beam_mbr(0.5)
        e.beam_mbr_distances()
        for bad in (-0.5, float("nan"), float("inf")):
            with pytest.raises(L.CasrError, match="CASR_ERR_ARG"):
                e.beam_mbr(bad)
        e.beam_lm(lm, 4, 0.5, 0.5)
        with pytest.raises(L.CasrError, match="CASR_ERR_STATE"):
            e.beam_mbr(0.5)
        e.beam(4)
        e.beam_mbr(0.5)
        assert e.device_flags() == 0
        lm.close()
    finally:
        e.close()
        e2.close()


def _record_bytes(e):
    return [x.cpu().numpy().view(np.uint8) for x in e.beam_records()]


def test_readers_leave_the_tree_and_a_spent_beam_is_refused():
    """(a) the readers only read: the records before and after them are the same bits; (c) a refused
    casr_beam leaves the last beam readable; (b) casr_greedy and casr_score reuse the decode workspaces,
    so every reader after them is CASR_ERR_STATE, not the records of a tree that is gone."""
    e = _engine(25.0)
    try:
        _encode(e)
        e.beam(4)
        first = _record_bytes(e)
        assert first[2].any()  # some record is valid: else the comparisons below would pass vacuously
        recs = records_by_utterance(*(x.cpu().numpy() for x in e.beam_records()))
        grams, lm, ref = _lm_from_records(recs, 78)
        e.device_flags()
        e.beam_mbr(0.5)
        e.beam_nbest(3)
        e.beam_confusion()
        for x, y in zip(first, _record_bytes(e)):
            assert np.array_equal(x, y)
        with pytest.raises(L.CasrError, match="CASR_ERR_ARG"):
            e.beam(0)
        for x, y in zip(first, _record_bytes(e)):
            assert np.array_equal(x, y)
        targets = torch.full((B, 5), 7, dtype=torch.int32)
        for spend in (e.greedy, lambda: e.score(targets, torch.full((B,), 5, dtype=torch.int32))):
            e.beam(4)
            e.beam_records()
            spend()
            for reader in (e.beam_records, lambda: e.beam_rescore(lm, 1.5, 1.5), lambda: e.beam_mbr(0.5),
                           lambda: e.beam_nbest(3), e.beam_confusion):
                with pytest.raises(L.CasrError, match="CASR_ERR_STATE"):
                    reader()
        assert e.device_flags() == 0
        lm.close()
    finally:
        e.close()


class _ScoreOnly:
    def score(self, s, bos=True):
        return 0.0


def test_model_wer_through_wer_batch_and_the_mbr_keyword():
    import model as M
    from oracle import casr_oracle as O
    m = M.Model()
    enc_sd, dec_sd = synthetic_state_dicts(CFG, peaked=True, eos_bias=25.0)
    m.load_state_dicts(enc_sd, dec_sd)
    dev = m.device
    feats = [torch.from_numpy(O.features_from_fbank(fbank_for(b, T))).to(dev) for b in range(B)]
    lens = torch.tensor([f.shape[0] for f in feats])
    rs = np.random.RandomState(4)
    text = [rs.randint(3, CFG.vocab, size=rs.randint(1, 12)).tolist() for _ in range(B)]
    calls = []
    orig = m.engine.edit_distance
    m.engine.edit_distance = lambda *a, **kw: calls.append(1) or orig(*a, **kw)
    g = m.eval_one_batch_with_greedy(dev, feats, lens, I2W, text)
    want = np.mean([get_wer(p, t) for p, t in zip(g.pred_text, g.text)])
    assert len(calls) == 1 and type(g.wer) is type(want) and g.wer == want
    bm = m.eval_one_batch_with_beam(dev, 4, feats, lens, text, I2W, second_pass=False)
    want = np.mean([get_wer(p, t) for p, t in zip(bm.pred_text, bm.text)])
    assert len(calls) == 2 and bm.wer == want
    # mbr: the engine's choice on the same beam
    r = m.eval_one_batch_with_beam(dev, 4, feats, lens, text, I2W, second_pass=False, mbr=0.5, length_weight=1.5)
    eng = _np(m.engine.beam_mbr(0.5, length_weight=1.5))
    assert r.pred_text == ["".join(I2W[i] for i in eng["tokens"][b, :eng["length"][b]].tolist()) for b in range(B)]
    assert r.score == [float(s) for s in eng["score"]]
    assert r.wer == np.mean([get_wer(p, t) for p, t in zip(r.pred_text, r.text)])
    first = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, second_pass=False, length_weight=1.5)
    # with an NgramLM and second_pass the LM enters c
    recs = records_by_utterance(*(x.cpu().numpy() for x in m.engine.beam_records()))
    grams, lm, ref = _lm_from_records(recs, 91)
    r2 = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, second_pass=True, lm_model=lm, lm_weight=1.5,
                                    length_weight=1.5, mbr=0.5)
    eng2 = _np(m.engine.beam_mbr(0.5, lm, 1.5, 1.5))
    assert r2.pred_text == ["".join(I2W[i] for i in eng2["tokens"][b, :eng2["length"][b]].tolist()) for b in range(B)]
    assert r2.pred_text != first.pred_text, "the MBR choice never differed from the first pass's"
    with pytest.raises(TypeError):
        m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, lm_model=_ScoreOnly(), mbr=0.5)
    with pytest.raises(ValueError):
        m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, lm_model=lm, fusion=True, mbr=0.5)
    lm.close()
