"""Kneser-Ney estimation on the device (include/casr.h casr_lm_estimate) against the host entry, which
tests/test_lm_estimate_host.py holds to the Python restatement: after sorting each order by key, the
n-grams, the raw and adjusted counts, the discounts, the fallback flags, |W| and the float64 p and
gamma are all EXACT (the float64 as bits).  Shapes are the smallest at which a kernel can go wrong:
every order, a vocabulary of 4 (every key hot), one token 5,000 times (one key through the combining),
one empty sentence, positions around a power of two (the capacity edge), ids 0 and V - 1 with <unk>,
sentence counts that are no multiple of the waves per workgroup, clamped input, another stream, and the
count kernel without its LDS combining.  Then end to end: the estimated model on the device scores and
fuses as the host-estimated one does."""
import numpy as np
import pytest
import torch

import lm_estimate_ref as E
from golden_util import fbank_for
from casr import lib as L
from casr import ngram
from casr.config import CasrConfig
from casr.weights import synthetic_state_dicts

pytestmark = pytest.mark.gpu

_ENGINES = {}


def _engine(V):
    """One weightless Engine per vocabulary (estimation needs no weights)."""
    from casr.engine import Engine
    if V not in _ENGINES:
        _ENGINES[V] = Engine(CasrConfig(max_num_words=V - 4))
    return _ENGINES[V]


def _same(dev, host, positions=True):
    dev.sorted()
    assert dev.order == host.order and dev.n_types == host.n_types
    assert dev.positions == host.positions or not positions
    assert np.array_equal(dev.discounts.view(np.uint64), host.discounts.view(np.uint64))
    assert np.array_equal(dev.fallback, host.fallback)
    for n in range(host.order):
        assert np.array_equal(dev.ids[n], host.ids[n]), n + 1
        assert np.array_equal(dev.raw[n], host.raw[n]), n + 1
        assert np.array_equal(dev.adjusted[n], host.adjusted[n]), n + 1
        assert np.array_equal(dev.p[n].view(np.uint64), host.p[n].view(np.uint64)), n + 1
        assert np.array_equal(dev.gamma[n].view(np.uint64), host.gamma[n].view(np.uint64)), n + 1
        assert np.array_equal(dev.prob[n].view(np.uint32), host.prob[n].view(np.uint32)), n + 1
        assert np.array_equal(dev.backoff[n].view(np.uint32), host.backoff[n].view(np.uint32)), n + 1


def _check(sents, order, V, flags=0):
    e = _engine(V)
    tokens, offsets = ngram.flatten(sents, V)
    e.device_flags()
    dev = e.lm_estimate(tokens, offsets, order)
    assert e.device_flags() == flags
    host = ngram.estimate_host(tokens, offsets, order, V)
    _same(dev, host)
    return dev, host


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_every_order_on_the_zipf_corpus(order):
    dev, _ = _check(E.zipf_corpus(), order, 120)
    assert dev.positions == 6971 and not dev.fallback.any()


def test_vocabulary_of_four():
    dev, _ = _check(E.small_corpus(4, 40, 6, 1), 4, 4)
    assert dev.fallback.tolist() == [True, False, False, True]


def test_one_token_five_thousand_times():
    dev, _ = _check([[7] * 5000], 4, 120)
    assert dev.raw[3].max() == 4997 and dev.fallback.all()
    _check([[7] * 50] * 100 + [[7]], 3, 120)


def test_one_empty_sentence():
    dev, _ = _check([[]], 4, 120)
    assert dev.positions == 1 and [len(a) for a in dev.ids] == [3, 1, 0, 0]  # <s>, </s>, <unk>; <s> </s>


@pytest.mark.parametrize("positions", [1023, 1024, 1025])
def test_positions_around_a_power_of_two(positions):
    """The tables have the power of two >= 2 P slots: 2048 at P = 1023 and 1024 (half full where every
    window differs), 4096 at 1025."""
    n = 29  # (no multiple of the 4 waves of a workgroup)
    rng = np.random.default_rng(positions)
    cuts = np.sort(rng.integers(0, positions - n + 1, size=n - 1))
    lens = np.diff(np.concatenate([[0], cuts, [positions - n]]))
    tokens = rng.integers(0, 5003, size=positions - n)
    dev, _ = _check(E.split(tokens, lens), 4, 5003)
    assert dev.positions == positions


def test_ids_zero_and_last_with_unk():
    V = 5003
    sents = E.small_corpus(V, 37, 9, 11, unk=0.1, ids=[0, 1, 2500, V - 1])
    assert any(V + 2 in s for s in sents) and any(0 in s for s in sents) and any(V - 1 in s for s in sents)
    _check(sents, 4, V)
    _check([[t for t in s if t != V + 2] for s in sents], 3, V)  # <unk> absent: its unigram is added


def test_bad_id_and_descending_offsets_are_clamped_and_flagged():
    V, e = 120, _engine(120)
    sents = E.small_corpus(V, 21, 8, 13)
    tokens, offsets = ngram.flatten(sents, V)
    bad = tokens.copy()
    bad[[3, 10, 17]] = [V, -5, V + 3]  # <s> itself, a negative id, one past <unk>
    e.device_flags()
    dev = e.lm_estimate(bad, offsets, 3)
    assert e.device_flags() == 1
    unk = bad.copy()
    unk[[3, 10, 17]] = V + 2
    _same(dev, ngram.estimate_host(unk, offsets, 3, V))
    # a descending offset: sentence i is [clamp(o[i], 0, total), clamp(o[i + 1], that start, total))
    off = offsets.copy()
    off[5] = off[3] - 1 if off[3] > 0 else 0
    off[9] = off[-1] + 7
    total = int(off[-1])
    want = []
    for i in range(len(off) - 1):
        s = min(max(int(off[i]), 0), total)
        t = min(max(int(off[i + 1]), s), total)
        want.append(tokens[s:t].tolist())
    dev = e.lm_estimate(tokens, off, 3)
    assert e.device_flags() == 1
    _same(dev, ngram.estimate_host(*ngram.flatten(want, V), 3, V), positions=False)  # (P is total + n as given)


def test_another_stream_and_no_combining_give_the_same():
    V, e = 120, _engine(120)
    sents = E.zipf_corpus(n=203, seed=9)
    tokens, offsets = ngram.flatten(sents, V)
    host = ngram.estimate_host(tokens, offsets, 4, V)
    st = torch.cuda.Stream(device=e.device)
    with torch.cuda.stream(st):
        _same(e.lm_estimate(tokens, offsets, 4), host)
    st.synchronize()
    assert e.lib.casr_lm_estimate_combine(0) == 1
    try:
        _same(e.lm_estimate(tokens, offsets, 4), host)
    finally:
        assert e.lib.casr_lm_estimate_combine(1) == 0
    assert e.device_flags() == 0


def test_refusals_launch_nothing():
    e = _engine(120)
    tok = torch.zeros(4, dtype=torch.int32, device=e.device)
    for order, off, code in ((0, [0, 4], "CASR_ERR_ARG"), (5, [0, 4], "CASR_ERR_ARG"), (2, [0, -1], "CASR_ERR_ARG"),
                             (2, [0, (1 << 28)], "CASR_ERR_UNSUPPORTED")):
        with pytest.raises(L.CasrError, match=code):
            e.lm_estimate(tok, off, order)
    with pytest.raises(L.CasrError, match="CASR_ERR_ARG"):
        e.lm_estimate(tok, [0], 2)  # n = 0
    assert e.device_flags() == 0


def test_estimated_model_scores_fuses_and_disturbs_nothing():
    from casr.engine import Engine
    cfg = CasrConfig()
    V, B, T = cfg.vocab, 6, 101
    e = Engine(cfg, packed=L.pack_weights(cfg, *synthetic_state_dicts(cfg, peaked=True, eos_bias=25.0)))
    try:
        fb = torch.from_numpy(np.stack([fbank_for(b, T) for b in range(B)])).to(e.device)
        e.encode_fbank(fb, torch.full((B,), T, dtype=torch.int32, device=e.device))
        before = {n: v.cpu() for n, v in e.greedy().items() if v is not None}
        sents = E.zipf_corpus(V=300, n=400, seed=21)
        lm_dev = ngram.estimate(sents, 3, V, engine=e)
        after = {n: v.cpu() for n, v in e.greedy().items() if v is not None}
        for n in before:
            assert torch.equal(before[n], after[n]), n
        lm_host = ngram.estimate(sents, 3, V)
        held = E.zipf_corpus(V=330, n=64, max_len=20, seed=22)  # (ids 300..329 were never seen: <unk>)
        tokens = np.zeros((64, 20), np.int32)
        lens = np.array([len(s) for s in held], np.int32)
        for i, s in enumerate(held):
            tokens[i, :len(s)] = s
        got = e.lm_score(lm_dev, tokens, lens).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), lm_host.score_ids(tokens, lens).view(np.uint32))
        assert e.check_flags() == 0
        out = e.beam_lm(lm_dev, 4, 0.5, 0.5)
        assert e.check_flags() == 0
        assert out["tokens"].shape[0] == B
        lm_dev.close()
        lm_host.close()
    finally:
        e.close()
