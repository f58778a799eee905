"""CPU-side checks of teacher-forced scoring (casr_score): the C ABI declares and exports it and
refuses a NULL handle, and the host helpers of casr/results.py (label-smoothed loss against the
fixture captured from the reference's util.label_smoothing, token times on hand-made alignments,
target encoding)."""
import ctypes
import os
import re

import numpy as np
import pytest

from casr import lib as L
from casr.config import CasrConfig
from casr.results import encode_targets, label_smoothed_loss, score_outputs, token_times

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = CasrConfig()
SG = np.load(os.path.join(REPO, "tests", "golden", "score_golden.npz"))


def test_header_library_and_binding_have_casr_score():
    hdr = open(os.path.join(REPO, "include", "casr.h")).read()
    assert re.search(r"\bint casr_score\s*\(casr_handle\* h, const int32_t\* targets, const int32_t\* tgt_len, int L,", hdr)
    assert re.search(r"#define CASR_API_VERSION 3\b", hdr)
    assert "casr_score" in L.EXPORTS
    for variant in (None, "s16x1"):
        lib = L.load(variant=variant)
        assert hasattr(lib, "casr_score")
        assert lib.casr_api_version() == 3


def test_null_handle_is_an_argument_error():
    lib = L.load()
    buf = (ctypes.c_int32 * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.casr_score(None, p, p, 1, p, p, None, None, None, None, None) == 1
    assert b"casr_score" in lib.casr_last_error(None)


@pytest.mark.parametrize("name", ["plain", "peaked"])
@pytest.mark.parametrize("ls,key", [(0.0, "ls0"), (0.1, "ls01")])
def test_label_smoothed_loss_matches_reference_fixture(name, ls, key):
    """util.py:265-279 restated from the two terms the device returns: the fixture's token_logp and
    mean_logp are the log_softmax value of the target and mean(logits) - logsumexp of the same
    logits the reference's label_smoothing saw."""
    n = SG[f"{name}_tgt_len"]
    got = label_smoothed_loss(SG[f"{name}_token_logp"], SG[f"{name}_mean_logp"], n, CFG.vocab, ls)
    assert got.shape == (8, CFG.max_len) and got.dtype == np.float32
    np.testing.assert_allclose(got, SG[f"{name}_{key}"], rtol=0, atol=1e-5)
    mask = np.arange(CFG.max_len)[None, :] < n[:, None]
    assert not got[~mask].any()
    if ls == 0.0:  # no smoothing: the negative log-likelihood
        np.testing.assert_allclose(got, -SG[f"{name}_token_logp"], rtol=0, atol=1e-6)


def test_fixture_covers_the_empty_transcript_and_golden_scores():
    import json
    with open(os.path.join(REPO, "tests", "golden", "golden.json"), encoding="utf-8") as f:
        meta = json.load(f)
    assert SG["peaked_tgt_len"].tolist() == [40, 1, 6, 2, 40, 40, 1, 1]  # 40, 0, 5, 1, 40, 40, 0, 0 + eos
    for name in ("plain", "peaked"):
        _, score = score_outputs(SG[f"{name}_token_logp"], SG[f"{name}_tgt_len"], SG[f"{name}_finished"])
        np.testing.assert_allclose(score, meta[name]["greedy"]["score"][:8], rtol=0, atol=1e-4)


def test_score_outputs_totals_and_greedy_form():
    lp = np.array([[-1.0, -2.0, -4.0], [-0.5, 9.0, 9.0], [-3.0, -1.0, 9.0]], np.float32)
    totals, score = score_outputs(lp, [3, 1, 2], [0, 1, 1])
    assert totals.tolist() == [-7.0, -0.5, -4.0]
    # unfinished: / len; a lone eos: the empty transcript scores 0.0 (model.py:588-590); finished: / (len + 1)
    assert score == [-7.0 / 3, 0.0, -2.0]


def test_token_times_on_hand_made_alignments():
    Lq, Tp, B = 3, 6, 2
    a = np.zeros((Lq, Tp, B), np.float32)
    a[0, 4, 0] = 1.0                      # one-hot
    a[1, 1, 0] = a[1, 3, 0] = 0.5         # two equal peaks: the first wins, the mean sits between
    a[2, :, 0] = 1.0 / 6                  # past tgt_len[0] = 2: ignored
    a[0, :3, 1] = [0.2, 0.5, 0.3]
    a[0, 3:, 1] = 7.0                     # past enc_lens[1] = 3: a length-masked tail, never read
    a[1, 2, 1] = 1.0
    a[2, 0, 1] = 1.0
    r = token_times(a, enc_lens=[6, 3], tgt_len=[2, 3])
    assert r["frame"].tolist() == [[4, 1, -1], [1, 2, 0]]
    np.testing.assert_allclose(r["expect"], [[4.0, 2.0, 0.0], [1.1, 2.0, 0.0]], atol=1e-6)
    np.testing.assert_allclose(r["frame_s"], [[0.12, 0.03, 0.0], [0.03, 0.06, 0.0]], atol=1e-12)
    np.testing.assert_allclose(r["expect_s"], np.asarray(r["expect"]) * 0.03, atol=1e-12)
    # 8 kHz audio: a stacked frame is 60 ms
    assert token_times(a, [6, 3], [2, 3], sample_rate=8000)["frame_s"][0, 0] == pytest.approx(0.24)


def test_encode_targets_padding_eos_unk_and_bad_ids():
    w2i = {"<pad>": 0, "<sos>": 1, "<eos>": 2, "<unk>": 3, "a": 4, "b": 5}
    ids, n = encode_targets(["ab", "", "bxa"], w2i, eos=2, unk=3)
    assert ids.dtype == np.int32 and n.dtype == np.int32
    assert n.tolist() == [3, 1, 4]
    assert ids.tolist() == [[4, 5, 2, 0], [2, 0, 0, 0], [5, 3, 4, 2]]
    ids, n = encode_targets([["a", "b"], []], w2i, eos=None, unk=3)
    assert n.tolist() == [2, 0] and ids.tolist() == [[4, 5], [0, 0]]
    ids, n = encode_targets([""], w2i, eos=None, unk=3)  # L is at least 1 (casr_score: 1 <= L)
    assert ids.shape == (1, 1) and n.tolist() == [0]
    with pytest.raises(ValueError, match="outside"):
        encode_targets(["ab"], w2i, eos=2, unk=3, V=5)       # "b" = 5 is not below V
    with pytest.raises(ValueError, match="outside"):
        encode_targets(["a"], {"a": -1}, eos=None, unk=3, V=10)
    with pytest.raises(ValueError, match="outside"):
        encode_targets(["ax"], w2i, eos=2, unk=77)            # the unk id itself out of range
    with pytest.raises(ValueError, match="max_len"):
        encode_targets(["abab"], w2i, eos=2, unk=3, max_len=4)
