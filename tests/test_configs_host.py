"""CPU side of test_gpu_configs.py: the oracle's new encoder keywords, and that every search whose
tokens the device must share with the float32 oracle rests on no near tie.

test_gpu_configs.py asks the device for the oracle's tokens, lengths and finished flags at the cases
of config_cases.SEARCHES.  That is a fair demand only where the float32 oracle's own choice does not
rest on a near tie of two candidates: a float64 run of the same search must keep the same tokens (the
method of test_accuracy_budget_host.test_small_width_beam_tokens_rest_on_no_near_tie).  Every case
passes at the seed config_cases gives it (seed 0 everywhere but the max_len batch, whose draw was
chosen for an eos at step 0, not for a tie), so no case dropped its token comparison.  The
budget checks of the GPU file do not depend on ties.
"""
import numpy as np
import pytest

import config_cases as CC
from oracle import casr_oracle as O


@pytest.mark.parametrize("sid", list(CC.SEARCHES))
def test_search_tokens_rest_on_no_near_tie(sid):
    r32 = CC.oracle_search(sid, np.float32)
    r64 = CC.oracle_search(sid, np.float64)
    assert O.F32 is np.float32 and O.encoder_forward.__name__ == "encoder_forward"  # (the swaps were undone)
    assert r32["tokens"] == r64["tokens"]
    assert r32["steps"] == r64["steps"]
    if CC.SEARCHES[sid].kind == "greedy":
        # every executed step's argmax, also past an utterance's eos (the device feeds them on)
        assert np.array_equal(r32["all_tokens"], r64["all_tokens"])
        assert np.array_equal(r32["finished"], r64["finished"])
        np.testing.assert_allclose(r32["accum"], r64["accum"], rtol=0, atol=2e-4)
    else:
        np.testing.assert_allclose(r32["score"], r64["score"], rtol=0, atol=2e-4)


def test_max_len_one_has_a_finished_and_a_fallback_utterance():
    """At max_len = 1 the first step is the last: the 48-frame utterance's first candidate is the eos
    (a finished record, the empty hypothesis) and the others end on the unfinished fallback."""
    r = CC.oracle_search("len-L1-beam8")
    assert r["steps"] == 1
    assert [len(v) > 0 for v in r["records"].values()].count(True) >= 1
    assert [len(v) == 0 for v in r["records"].values()].count(True) >= 1
    g = CC.oracle_search("len-L1-greedy")
    assert g["finished"].any() and not g["finished"].all()


def test_oracle_decodes_take_the_encoder_keywords():
    """O.greedy_decode and O.beam_decode pass num_layers and residual to encoder_forward; the defaults
    are the deployed encoder's (the golden tests run them unchanged)."""
    cfg = CC.config(layers=2, residual=False)
    enc_sd, dec_sd = CC.weights(cfg, True)
    feats = [O.features_from_fbank(CC.fbank(b, t)) for b, t in enumerate((48, 30))]
    lens = [f.shape[0] for f in feats]
    seen = []
    real = O.encoder_forward

    def spy(feats, lens, enc_sd, num_layers=4, residual=True):
        seen.append((num_layers, residual))
        return real(feats, lens, enc_sd, num_layers, residual)

    O.encoder_forward = spy
    try:
        g = O.greedy_decode(feats, lens, enc_sd, dec_sd, num_layers=2, residual=False)
        b = O.beam_decode(feats, lens, enc_sd, dec_sd, 2, num_layers=2, residual=False)
        with pytest.raises(KeyError):  # the defaults ask for four layers
            O.greedy_decode(feats, lens, enc_sd, dec_sd)
    finally:
        O.encoder_forward = real
    assert seen == [(2, False), (2, False), (4, True)]
    assert len(g["tokens"]) == len(b["tokens"]) == 2


def test_plan_predicates_at_the_boundaries():
    """config_cases' restatement of the two vocabulary rules, at the four boundaries plan_check.cpp
    checks on the plan itself"""
    assert CC.projection_partials(5120) and not CC.projection_partials(5121)
    assert CC.greedy_folds(7168) and not CC.greedy_folds(7169)
    assert all(CC.projection_partials(V) and CC.greedy_folds(V) for V in (4, 36, 83, 5003, 5004))


def test_derived_case_rests_on_no_near_tie():
    """The LM and bias searches at V = 83, (sos, eos) = (82, 0) that test_gpu_configs.py compares with
    fusion_ref and bias_ref: every step's best 2k + 1 vals lie at least 1e-2 apart (the bound those
    comparisons use at the deployed config), the searches finish hypotheses, and the bias changes a choice."""
    case = CC.derived_case()
    fused, biased = case["fused"], case["biased"]
    L = case["cfg"].max_len
    assert (fused["gap"] >= 1e-2).all() and 1 < fused["steps"] < L
    assert all(len(v) > 1 for v in fused["records"].values())
    for with_lm in (True, False):
        assert (biased[with_lm]["gap"] >= 1e-2).all(), with_lm
        assert biased[with_lm]["tokens"] != fused["tokens"] and biased[with_lm]["bias"].max() > 0
        assert any(biased[with_lm]["records"].values())
    assert 1 < biased[False]["steps"] < L


@pytest.mark.parametrize("k", CC.DERIVED_IDENTITY_K)
def test_derived_plain_beam_ends_early_with_records(k):
    """The bit-for-bit identities of casr_beam_lm, casr_beam_bias and casr_beam_grammar with casr_beam at
    (sos, eos) = (82, 0) run where the plain search takes more than one step, finishes hypotheses for
    every utterance and ends before max_len: at the last step the grammar's horizon rule offers eos only."""
    r = CC.derived_plain_beam(k)
    assert 1 < r["steps"] < CC.DERIVED_CFG.max_len
    assert all(len(v) > 0 for v in r["records"].values())
