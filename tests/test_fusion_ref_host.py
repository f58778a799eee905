"""The numpy restatement of the fused beam (tests/fusion_ref.py) checked on the CPU before the device
is compared with it (tests/test_gpu_fusion.py): with zero weights it is the oracle's beam search,
and the inputs chosen for the device comparison keep every pair of neighbouring candidates far enough
apart that the two arithmetics cannot rank them differently.  No GPU."""
import numpy as np
import pytest

import fusion_ref as FR
import ngram_ref as R
from golden_util import fbank_for
from oracle import casr_oracle as O
from casr.config import CasrConfig
from casr.weights import synthetic_state_dicts

CFG = CasrConfig()


def test_term_rows_of_the_restatement_are_the_references():
    """The vectorised rows (the m = 1 chain for words that only have a unigram) against RefLM.term
    word by word."""
    case = FR.fusion_case()
    ref = R.RefLM(4, CFG.vocab, case["grams"])
    rows = FR.TermRows(ref, CFG.eos)
    rec = next(t for t in FR.fused_case(4)["tokens"] if len(t) >= 1)
    for ctx in ([ref.bos], [ref.bos] + [ref.lm_id(t) for t in rec[:1]], [ref.lm_id(7), ref.lm_id(9), ref.lm_id(11)]):
        row = rows(ctx)
        for v in range(0, CFG.vocab, 3):
            want = ref.term(ctx, ref.lm_id(ref.eos) if v == CFG.eos else ref.lm_id(v))
            assert np.float32(row[v]).view(np.uint32) == np.float32(want).view(np.uint32), (ctx, v)


def test_zero_weights_are_the_oracles_beam():
    """eos_bias 25, utterances 0..5, k = 4: all 40 steps, finished and unfinished utterances."""
    enc_sd, dec_sd = synthetic_state_dicts(CFG, peaked=True, eos_bias=25.0)
    feats = [O.features_from_fbank(fbank_for(b, FR.T)) for b in range(FR.B)]
    lens = [f.shape[0] for f in feats]
    plain = O.beam_decode(feats, lens, enc_sd, dec_sd, 4)
    ref = R.RefLM(4, CFG.vocab, FR.lm_grams_from_records(plain["records"], CFG.vocab, 7))
    z = FR.fused_beam(FR.encode(feats, lens, enc_sd, dec_sd), dec_sd, 4, ref, 0.0, 0.0)
    assert z["tokens"] == plain["tokens"] and z["steps"] == plain["steps"] == 40
    assert np.array_equal(z["score"], np.array(plain["score"], np.float32))
    count = [len(v) for v in plain["records"].values()]
    assert max(count) > 50 and min(count) == 0
    for b in range(FR.B):
        assert [(t, float(a)) for t, a, _ in z["records"][b]] == plain["records"][b], b
        for t, _, q in z["records"][b][::9]:  # a record's lm is its sentence score
            assert np.float32(q).view(np.uint32) == np.float32(ref.sentence(t)).view(np.uint32)


@pytest.mark.parametrize("k", FR.GPU_K)
def test_inputs_of_the_device_comparison(k):
    """Every utterance's smallest gap between vals adjacent in rank among the best 2k + 1, over all
    steps, is >= 1e-2 (five times the 2e-3 score tolerance between arithmetics), and the LM changes at
    least one choice."""
    case = FR.fusion_case()
    f = FR.fused_case(k)
    assert (f["gap"] >= 1e-2).all(), f["gap"]
    plain = case["plain"].get(k) or O.beam_decode(case["feats"], case["lens"], case["enc_sd"], case["dec_sd"], k)
    assert sum(a != b for a, b in zip(f["tokens"], plain["tokens"])) >= 1
    assert f["steps"] >= 2 and all(len(v) >= 1 for v in f["records"].values())
