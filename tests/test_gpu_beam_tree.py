"""casr_beam's thread-per-utterance finalize (csrc/decoder.hip beam_finalize_kernel), the form the plan
takes when max_len x k is past the wave form's LDS (csrc/decode_plan.h fin_lds == 0): max_len = 320 at
k = 16 is the smallest such shape, and no other test reaches it.  It reads the tree by the same rules
(csrc/beam_tree.h) as the wave form and the readers, so it is held to the same results: its choice among
finished records against casr_beam_records on the same handle, bit for bit, and its unfinished fallback
against the CPU oracle's beam (tests/golden/beam_tree_len320.npz, captured by make_beam_tree_golden.py).

T = 101 frames, synthetic peaked weights."""
import os

import numpy as np
import pytest
import torch

from golden_util import GOLD, fbank_for, near_tie_beam_check, teacher_forced_score
from oracle import casr_oracle as O
from casr import lib as L
from casr.config import CasrConfig
from casr.weights import synthetic_state_dicts

pytestmark = pytest.mark.gpu

MAX_LEN, K, T = 320, 16, 101
CFG = CasrConfig(max_len=MAX_LEN)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _beam(eos_bias, B):
    """(beam results, records, device flags, weights) of one casr_beam at k = 16, max_len = 320"""
    from casr.engine import Engine
    enc_sd, dec_sd = synthetic_state_dicts(CFG, peaked=True, eos_bias=eos_bias)
    e = Engine(CFG, packed=L.pack_weights(CFG, enc_sd, dec_sd))
    try:
        fb = torch.from_numpy(np.stack([fbank_for(b, T) for b in range(B)])).to(e.device)
        e.encode_fbank(fb, torch.full((B,), T, dtype=torch.int32, device=e.device))
        r = {n: v.cpu().numpy() for n, v in e.beam(K).items()}
        rec = [x.cpu().numpy() for x in e.beam_records()]
        flags = e.device_flags()
    finally:
        e.close()
    return r, rec, flags, (enc_sd, dec_sd)


@pytest.mark.parametrize("eos_bias", [25.0, 17.0])
def test_thread_form_picks_the_first_best_record(eos_bias):
    """eos_bias 25 (test_gpu_ngram.py's weights): utterances finish.  For every utterance with a record,
    tokens, length and score are those of the first maximum of rec_score over its valid records in
    (step, rank) order, in bits; the row is padded with -1.  At 25 the empty record wins wherever there is
    one (its score is near 0 and a token costs about -4.6); at 17 the oracle's beam gives utterance 0 two
    tokens, so there the walk has steps to take."""
    B = 3
    r, (rt, rs, rv), flags, _ = _beam(eos_bias, B)
    assert flags == 0
    valid = rv.astype(bool).reshape(B, -1)
    assert valid.any(1).sum() >= 2, valid.sum(1)  # else the test would pass vacuously
    walked = 0
    for b in range(B):
        n = int(r["length"][b])
        assert (r["tokens"][b, n:] == -1).all() and (r["tokens"][b, :n] >= 0).all()
        if not valid[b].any():
            assert n == int(r["steps"][0])
            continue
        sc = rs[b].reshape(-1)
        best, bi = None, -1
        for i in np.flatnonzero(valid[b]):  # the first maximum, as the kernel compares
            if bi < 0 or sc[i] > best:
                best, bi = sc[i], int(i)
        step = bi // K
        print(f"utterance {b}: {int(valid[b].sum())} records, best (step, rank) = {divmod(bi, K)}, score {best}")
        assert n == step
        walked += step
        assert bits(r["score"][b]) == bits(best)
        assert np.array_equal(r["tokens"][b], rt[b].reshape(-1, MAX_LEN)[bi])
        assert (rt[b].reshape(-1, MAX_LEN)[bi, step:] == -1).all()
    assert eos_bias == 25.0 or walked > 0


def test_thread_form_unfinished_fallback_matches_the_oracle():
    """eos_bias -60: eos cannot win, so no record; all 320 steps run and the choice is among the live rows
    of the last one.  Tokens identical to the oracle's and scores within 2e-3, as test_gpu_guards.py
    compares beams with the oracle; at most one utterance may instead split at a near-tied pruning step
    (golden_util.near_tie_beam_check, both hypotheses rescored by the oracle)."""
    B = 2
    r, (_, _, rv), flags, (enc_sd, dec_sd) = _beam(-60.0, B)
    assert flags == 0
    assert not rv.any() and int(r["steps"][0]) == MAX_LEN
    assert (r["length"] == MAX_LEN).all() and r["tokens"].min() >= 0
    g = np.load(os.path.join(GOLD, "beam_tree_len320.npz"))
    gold = {"tokens": [t.tolist() for t in g["tokens"]], "score": g["score"].tolist()}
    print("score", r["score"].tolist(), "oracle", gold["score"])

    def rescore(b, tokens):
        return teacher_forced_score(O.features_from_fbank(fbank_for(b, T)), tokens, enc_sd, dec_sd)

    near_tie_beam_check([r["tokens"][b].tolist() for b in range(B)], r["score"], gold, atol=2e-3, rescore=rescore)
