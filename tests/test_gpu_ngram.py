"""The backoff n-gram LM on the device (include/casr.h casr_lm_score, casr_beam_rescore).

Sentence scores against the host function and the independent reference (tests/ngram_ref.py), bit
for bit; the second pass over the beam tree against the unchanged host path
(casr.results.second_pass_arrays) on the device's own records, so near ties of the beam search play
no part and no tolerance is needed; zero weights, an early stop, undisturbed state, and the drop-in
Model.  The LMs are built from the decoded records themselves (half of their n-grams plus random
ones, some tokens without a unigram), so every branch of the query occurs on real hypotheses."""
import numpy as np
import pytest
import torch

import ngram_ref as R
from golden_util import fbank_for
from casr import lib as L
from casr.config import CasrConfig
from casr.ngram import NgramLM
from casr.results import records_by_utterance, second_pass_arrays
from casr.weights import synthetic_state_dicts

pytestmark = pytest.mark.gpu

CFG = CasrConfig()
V = CFG.vocab
B, T = 6, 101
I2W = {i: f"w{i}" for i in range(V)}
W2I = {w: i for i, w in I2W.items()}
_PACKED = {}


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _engine(eos_bias):
    from casr.engine import Engine
    if eos_bias not in _PACKED:
        _PACKED[eos_bias] = L.pack_weights(CFG, *synthetic_state_dicts(CFG, peaked=True, eos_bias=eos_bias))
    return Engine(CFG, packed=_PACKED[eos_bias])


def _encode(e):
    fb = torch.from_numpy(np.stack([fbank_for(b, T) for b in range(B)])).to(e.device)
    e.encode_fbank(fb, torch.full((B,), T, dtype=torch.int32, device=e.device))


def _lm_from_records(recs, seed):
    """A 4-gram model seeded with half of the records' own 2-, 3- and 4-grams (<s> and </s> included);
    one in eight of their tokens is left without a unigram.  Log-probabilities in [-1.5, -0.1],
    backoffs in [-0.5, 0], and the empty sentence improbable (P(</s> | <s>) = -8), as a real LM has
    it: with this recipe's weights the empty record, whose first-pass score is near 0, wins the first
    pass everywhere (a token costs about -4.6), and the second pass must be able to overturn that."""
    rs = np.random.RandomState(seed)
    seen, toks = set(), set()
    for v in recs.values():
        for t, _ in v:
            ids = [V] + list(t) + [V + 1]
            toks.update(t)
            for n in (2, 3, 4):
                seen.update(tuple(ids[i:i + n]) for i in range(len(ids) - n + 1))
    seen = sorted(seen)
    half = [g for g in seen if rs.rand() < 0.5]
    keep = [t for t in sorted(toks) if rs.rand() < 0.875]
    uni = sorted(set(keep) | set(int(x) for x in rs.choice(V, size=500, replace=False)) - (toks - set(keep)))
    grams = R.random_model(4, V, seed + 1, n_high=500, seeds=half, uni_ids=uni, p_lo=-1.5, b_lo=-0.5)
    grams[1][(V, V + 1)] = (np.float32(-8.0), np.float32(0.0))
    return grams, NgramLM.from_ids(*R.arrays_of(grams), W2I, V), R.RefLM(4, V, grams)


# ---------------------------------------------------------------------------- 1. sentence scoring
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_device_sentence_scores_equal_host_and_reference(order):
    from casr.engine import Engine
    grams = R.random_model(order, V, 200 + order)
    tokens, lens = R.sentences_from(grams, V, 300, 40, 300 + order)
    assert set((0, 1, 2, 3, 40)) <= set(lens.tolist())
    lm, ref = NgramLM.from_ids(*R.arrays_of(grams), {}, V), R.RefLM(order, V, grams)
    e = Engine(CFG)  # no weights: scoring needs none
    try:
        e.device_flags()
        for bos in (True, False):
            got = e.lm_score(lm, tokens, lens, bos).cpu().numpy()
            want = np.array([ref.sentence(tokens[i, :lens[i]], bos) for i in range(len(lens))], np.float32)
            assert np.array_equal(bits(got), bits(want)), (order, bos)
            assert np.array_equal(bits(got), bits(lm.score_ids(tokens, lens, bos)))
        assert e.device_flags() == 0
        for key in ref.expected_branches():
            assert ref.branches[key] > 0, key
        # one id outside [0, V + 3): guard bit 1, scored as <unk>
        bad = tokens.copy()
        i = int(np.argmax(lens >= 3))
        bad[i, 1] = V + 3
        got = e.lm_score(lm, bad, lens, True).cpu().numpy()
        assert e.device_flags() == 1
        unk = bad.copy()
        unk[i, 1] = V + 2
        want = lm.score_ids(unk, lens, True)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got), bits(lm.score_ids(bad, lens, True)))
    finally:
        e.close()
        lm.close()


# ---------------------------------------------------------------------------- 2. the second pass
@pytest.mark.parametrize("k,precision", [(2, None), (4, None), (16, None), (4, "f32")])
def test_device_second_pass_equals_host_path_on_device_records(k, precision):
    e = _engine(25.0)
    try:
        if precision:
            e.set_precision(precision)
        _encode(e)
        beam = {n: v.cpu().numpy() for n, v in e.beam(k, 1.5, 1.5).items()}
        rt, rs, rv = (x.cpu().numpy() for x in e.beam_records())
        recs = records_by_utterance(rt, rs, rv)
        count = np.array([len(recs.get(b, [])) for b in range(B)])
        assert (count >= 2).sum() >= 3 and (count == 0).any(), count  # else the test would pass vacuously
        grams, lm, ref = _lm_from_records(recs, 500 + k)
        e.device_flags()
        r = {n: (v.cpu().numpy() if v is not None else None)
             for n, v in e.beam_rescore(lm, 1.5, 1.5, records=True).items()}
        assert e.device_flags() == 0
        # q of every valid record, bit for bit; 0 elsewhere
        want_q = np.zeros(rv.shape, np.float32)
        for b, l, c in zip(*np.nonzero(rv)):
            want_q[b, l, c] = ref.sentence(rt[b, l, c, :l].tolist())
        assert np.array_equal(bits(r["rec_lm"]), bits(want_q))
        for key in ref.expected_branches():
            assert ref.branches[key] > 0, key
        # the choice: the host path's on the same records
        host = second_pass_arrays(rt, rs, rv, I2W, lm, 1.5, 1.5)
        differs = 0
        for b in range(B):
            got = r["tokens"][b, :r["length"][b]].tolist()
            assert (r["tokens"][b, r["length"][b]:] == -1).all()
            if b in host:
                assert got == host[b][0], b
                assert bits(r["score"][b]) == bits(np.float32(host[b][1])), b
                i, qs = R.second_pass_choice(recs[b], ref, 1.5, 1.5)
                assert recs[b][i][0] == got and bits(r["lm"][b]) == bits(qs[i])
                differs += recs[b][i] != recs[b][int(np.argmax([s for _, s in recs[b]]))]
            else:  # no record: casr_beam's unfinished fallback, bit for bit
                assert np.array_equal(r["tokens"][b], beam["tokens"][b]) and r["length"][b] == beam["length"][b]
                assert bits(r["score"][b]) == bits(beam["score"][b]) and r["lm"][b] == 0
        assert differs >= 1, "the LM never changed a choice"
        lm.close()
    finally:
        e.close()


# ---------------------------------------------------------------------------- 3, 5. weights, state
def test_zero_weights_reproduce_beam_and_state_is_undisturbed():
    from casr.engine import Engine
    e = _engine(25.0)
    e2 = Engine(CFG)
    try:
        _encode(e)
        beam = {n: v.cpu() for n, v in e.beam(4).items()}
        before = [x.cpu() for x in e.beam_records()]
        recs = records_by_utterance(*(x.numpy() for x in before))
        grams, lm, ref = _lm_from_records(recs, 77)
        z = e.beam_rescore(lm, 0.0, 0.0)
        for n in ("tokens", "length", "score"):
            assert torch.equal(z[n].cpu(), beam[n]), n
        a = {n: v.cpu() for n, v in e.beam_rescore(lm, 1.5, 1.5, records=True).items()}
        b = {n: v.cpu() for n, v in e.beam_rescore(lm, 1.5, 1.5, records=True).items()}
        for n in a:
            assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), n
        after = [x.cpu() for x in e.beam_records()]
        for x, y in zip(before, after):
            assert torch.equal(x, y)
        # one LM object, two Engines on the device
        assert lm.on(e).value == lm.on(e2).value
        tokens, lens = R.sentences_from(grams, V, 64, 40, 9)
        q1, q2 = e.lm_score(lm, tokens, lens).cpu(), e2.lm_score(lm, tokens, lens).cpu()
        assert torch.equal(q1.view(torch.int32), q2.view(torch.int32))
        assert np.array_equal(bits(q1.numpy()), bits(lm.score_ids(tokens, lens)))
        assert e.device_flags() == 0 and e2.device_flags() == 0
        # refusals: before casr_beam, a host-only LM's vocab mismatch
        with pytest.raises(L.CasrError, match="CASR_ERR_STATE"):
            e2._B, e2._k = B, 4
            e2.beam_rescore(lm, 1.5, 1.5)
        small = NgramLM.from_ids(*R.arrays_of(R.random_model(2, 100, 3, n_high=10)), {}, 100)
        with pytest.raises(L.CasrError, match="CASR_ERR_ARG"):
            e.beam_rescore(small, 1.5, 1.5)
        small.close()
        lm.close()
    finally:
        e.close()
        e2.close()


# ---------------------------------------------------------------------------- 4. early stop
def test_early_stop_every_utterance_one_record_of_length_zero():
    e = _engine(35.0)
    try:
        _encode(e)
        beam = e.beam(4, 1.5, 1.5)
        assert int(beam["steps"][0]) == 1
        rt, rs, rv = (x.cpu().numpy() for x in e.beam_records())
        assert (rv.reshape(B, -1).sum(axis=1) == 1).all() and rv[:, 0].sum() == B
        grams = R.random_model(4, V, 61)
        lm, ref = NgramLM.from_ids(*R.arrays_of(grams), {}, V), R.RefLM(4, V, grams)
        r = e.beam_rescore(lm, 1.5, 1.5)
        assert e.device_flags() == 0
        assert (r["length"].cpu().numpy() == 0).all() and (r["tokens"].cpu().numpy() == -1).all()
        assert np.array_equal(bits(r["lm"].cpu().numpy()), bits(np.full(B, ref.sentence([]), np.float32)))
        assert np.array_equal(bits(r["score"].cpu().numpy()), bits(rs[rv.astype(bool)]))
        lm.close()
    finally:
        e.close()


# ---------------------------------------------------------------------------- 6. the drop-in Model
class _ScoreOnly:
    """The same LM behind the duck-typed host interface only: the host second pass."""

    def __init__(self, lm):
        self.lm = lm

    def score(self, s, bos=True):
        return self.lm.score(s, bos=bos)


def _same_results(got, want):
    """Packed results equal in lengths, score bits and the tokens up to each length (the host path
    leaves the first pass's tokens behind a shorter choice; the device writes -1 there)."""
    from casr.distributed import unpack_results
    (gt, gl, gs), (wt, wl, ws) = unpack_results(got, CFG.max_len), unpack_results(want, CFG.max_len)
    assert np.array_equal(gl, wl) and np.array_equal(bits(gs), bits(ws))
    for b in range(len(gl)):
        assert gt[b, :gl[b]].tolist() == wt[b, :wl[b]].tolist(), b


def test_shard_decoder_takes_the_device_path_for_an_ngram_lm():
    """BeamShardDecoder with an NgramLM (device second pass, no records fetched) against the same LM
    behind score() only (host second pass): identical packed results, on one Engine and on a
    two-handle StreamPipeline whose handles share the one device LM (batches of 4 + 2)."""
    from casr.distributed import BeamShardDecoder
    from casr.pipeline import StreamPipeline
    e = _engine(25.0)
    blob = torch.from_numpy(_PACKED[25.0]).cuda()
    fb = torch.from_numpy(np.stack([fbank_for(b, T) for b in range(B)])).cuda()
    fr = torch.full((B,), T, dtype=torch.int32, device=fb.device)
    torch.cuda.synchronize()
    try:
        _encode(e)
        e.beam(4)
        recs = records_by_utterance(*(x.cpu().numpy() for x in e.beam_records()))
        grams, lm, ref = _lm_from_records(recs, 123)
        host = BeamShardDecoder(e, 4, _ScoreOnly(lm), I2W, 1.5, 1.5, max_batch=4)
        want = host.finish(host.enqueue(fb, fr))
        assert host.stats["records"] > 0
        dev = BeamShardDecoder(e, 4, lm, I2W, 1.5, 1.5, max_batch=4)
        assert dev.device_lm and not host.device_lm
        got = dev.finish(dev.enqueue(fb, fr))
        assert dev.stats["records"] == 0 and dev.stats["batch_steps"] == host.stats["batch_steps"]
        assert e.device_flags() == 0
    finally:
        e.close()
    _same_results(got, want)
    pipe = StreamPipeline(CFG, blob, n=2)
    try:
        d2 = BeamShardDecoder(pipe, 4, lm, I2W, 1.5, 1.5, max_batch=4)
        got2 = d2.finish(d2.enqueue(fb, fr))
        assert pipe.device_flags() == 0
        assert len(lm._device) == 1  # one upload for every handle on the device
    finally:
        pipe.close()
    _same_results(got2, want)
    lm.close()


def test_model_takes_the_device_path_for_an_ngram_lm():
    import model as M
    from oracle import casr_oracle as O
    m = M.Model()
    enc_sd, dec_sd = synthetic_state_dicts(CFG, peaked=True, eos_bias=25.0)
    m.load_state_dicts(enc_sd, dec_sd)
    dev = m.device
    feats = [torch.from_numpy(O.features_from_fbank(fbank_for(b, T))).to(dev) for b in range(B)]
    lens = torch.tensor([f.shape[0] for f in feats])
    m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, second_pass=False)
    recs = records_by_utterance(*(x.cpu().numpy() for x in m.engine.beam_records()))
    grams, lm, ref = _lm_from_records(recs, 91)
    calls = []
    orig = m.engine.beam_records
    m.engine.beam_records = lambda: calls.append(1) or orig()
    dev_r = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, second_pass=True, lm_model=lm,
                                       lm_weight=1.5, length_weight=1.5)
    assert not calls, "the device path copies no records"
    host_r = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, second_pass=True, lm_model=_ScoreOnly(lm),
                                        lm_weight=1.5, length_weight=1.5)
    assert calls
    first = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, second_pass=False)
    assert dev_r.pred_text == host_r.pred_text and dev_r.score == host_r.score
    assert dev_r.pred_text != first.pred_text, "the LM never changed a choice"
    lm.close()
