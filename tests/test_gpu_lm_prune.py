"""Relative-entropy pruning on the device (include/casr.h casr_lm_prune) against the host entry, which
tests/test_lm_prune_host.py holds to the Python restatement: after sorting each order by key, every
n-gram's dH and kept flag, every float64 backoff and the stored prob and backoff are all EXACT (the
floats as bits).  Shapes are the smallest at which a kernel can go wrong: every order, contexts of
exactly 1, 64, 65 and 130 successors (one wave's lanes, one more, two rounds and a part), a word without
a unigram, no <unk> unigram, a context that is no n-gram, a threshold that removes nothing, one that
removes everything above the unigrams, and a second call over the same workspace.  Then end to end: the
pruned model on the device scores, gives term rows and fuses as its host copy does."""
import ctypes

import numpy as np
import pytest
import torch

import lm_estimate_ref as E
import lm_prune_ref as PR
from golden_util import fbank_for
from casr import lib as L
from casr import ngram
from casr.config import CasrConfig
from casr.weights import synthetic_state_dicts

pytestmark = pytest.mark.gpu

_ENGINES = {}


def _engine(V):
    """One weightless Engine per vocabulary (pruning needs no weights)."""
    from casr.engine import Engine
    if V not in _ENGINES:
        _ENGINES[V] = Engine(CasrConfig(max_num_words=V - 4))
    return _ENGINES[V]


def _same(dev, host):
    dev.sorted()
    assert dev.order == host.order and dev.tau == host.tau and dev.n_degenerate == host.n_degenerate
    assert dev.count_in.tolist() == host.count_in.tolist() and dev.count_out.tolist() == host.count_out.tolist()
    assert dev.n_protected.tolist() == host.n_protected.tolist()
    for n in range(host.order):
        assert np.array_equal(dev.all_ids[n], host.all_ids[n]), n + 1
        assert np.array_equal(dev.delta[n].view(np.uint64), host.delta[n].view(np.uint64)), n + 1
        assert np.array_equal(dev.kept[n], host.kept[n]), n + 1
        assert np.array_equal(dev.ids[n], host.ids[n]), n + 1
        assert np.array_equal(dev.backoff_f64[n].view(np.uint64), host.backoff_f64[n].view(np.uint64)), n + 1
        assert np.array_equal(dev.prob[n].view(np.uint32), host.prob[n].view(np.uint32)), n + 1
        assert np.array_equal(dev.backoff[n].view(np.uint32), host.backoff[n].view(np.uint32)), n + 1


def _check(lm, theta):
    e = _engine(lm.vocab)
    e.device_flags()
    dev = e.lm_prune(lm, theta)
    assert e.device_flags() == 0  # guard bits are clean
    host = lm.prune(theta)
    _same(dev, host.pruned)
    host.close()
    return dev


@pytest.mark.parametrize("order,kept", [(3, [120, 681, 412]), (4, [120, 676, 391, 127])])
def test_zipf_model_at_1e_4(order, kept):
    lm = ngram.estimate(E.zipf_corpus(), order, 120)
    dev = _check(lm, 1e-4)
    assert dev.count_out.tolist() == kept
    assert dev.timing_ms[7] > 0.0
    lm.close()


def test_small_model_at_three_thresholds_and_a_second_call_gives_the_same_bits():
    lm = ngram.estimate(E.small_corpus(6, 300, 8, 6), 4, 6)
    first = [_check(lm, theta) for theta in (1e-5, 1e-4, 1e-3)]
    assert [d.count_out.tolist() for d in first][2] == [9, 48, 4, 0]
    again = _engine(6).lm_prune(lm, 1e-5)  # over the workspace the calls above left
    _same(again, first[0])
    assert _check(lm, 1e-2).count_out.tolist() == [9, 0, 0, 0]
    lm.close()


def test_handmade_edges():
    """Contexts of 1, 64, 65 and 130 successors, a word without a unigram, no <unk> unigram."""
    lm = ngram.NgramLM.from_ids(*PR.handmade(), {}, 136)
    for theta in (1e-3, 3e-2):
        dev = _check(lm, theta)
        assert 0 < dev.count_out[1] < dev.count_in[1] and np.isnan(dev.delta[2]).sum() == 1
    lm.close()


def test_order_2_order_1_and_nothing_removed():
    lm = ngram.estimate(E.zipf_corpus(), 2, 120)
    dev = _check(lm, 1e-4)
    assert dev.count_out[1] < dev.count_in[1]
    same = _check(lm, 1e-9)
    assert same.count_out.tolist() == same.count_in.tolist()
    for got, want in zip((same.prob, same.backoff), lm._arrays[1:]):
        for n in range(2):
            assert np.array_equal(got[n].view(np.uint32), want[n].view(np.uint32))
    lm.close()
    lm = ngram.estimate(E.zipf_corpus(), 1, 120)
    dev = _check(lm, 1e-2)
    assert dev.count_out.tolist() == [120] and np.array_equal(dev.backoff[0].view(np.uint32), lm._arrays[2][0].view(np.uint32))
    lm.close()


def test_refusals_launch_nothing():
    e = _engine(120)
    lm = ngram.estimate(E.zipf_corpus(), 2, 120)
    for theta in (-1.0, float("nan"), float("inf")):
        with pytest.raises(L.CasrError, match="CASR_ERR_ARG"):
            e.lm_prune(lm, theta)
    out = ctypes.c_void_p()
    # a host-only LM object
    rc = e.lib.casr_lm_prune(e.handle, lm._host, ctypes.c_double(1e-4), None, ctypes.byref(out))
    assert rc != 0 and not out.value
    assert e.lib.casr_lm_prune(e.handle, None, ctypes.c_double(1e-4), None, ctypes.byref(out)) != 0
    assert e.lib.casr_lm_prune(e.handle, lm.on(e), ctypes.c_double(1e-4), None, None) != 0
    # another vocabulary
    other = ngram.estimate(E.small_corpus(6, 50, 8, 6), 2, 6)
    with pytest.raises(L.CasrError, match="CASR_ERR_ARG"):
        e.lm_prune(other, 1e-4)
    assert e.device_flags() == 0
    other.close()
    lm.close()


def test_pruned_model_scores_gives_terms_and_fuses():
    from casr.engine import Engine
    cfg = CasrConfig()
    V, B, T = cfg.vocab, 6, 101
    e = Engine(cfg, packed=L.pack_weights(cfg, *synthetic_state_dicts(cfg, peaked=True, eos_bias=25.0)))
    try:
        fb = torch.from_numpy(np.stack([fbank_for(b, T) for b in range(B)])).to(e.device)
        e.encode_fbank(fb, torch.full((B,), T, dtype=torch.int32, device=e.device))
        full = ngram.estimate(E.zipf_corpus(V=300, n=400, seed=21), 3, V)
        lm = full.prune(1e-5, engine=e)
        host = full.prune(1e-5)
        assert 0 < lm.pruned.count_out[2] < lm.pruned.count_in[2]
        for a, b in zip(lm._arrays, host._arrays):
            for n in range(3):
                assert np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32))
        held = E.zipf_corpus(V=330, n=64, max_len=20, seed=22)  # (ids 300..329 were never seen: <unk>)
        tokens = np.zeros((64, 20), np.int32)
        lens = np.array([len(s) for s in held], np.int32)
        for i, s in enumerate(held):
            tokens[i, :len(s)] = s
        got = e.lm_score(lm, tokens, lens).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), lm.score_ids(tokens, lens).view(np.uint32))
        ctx = np.array([[3, 1, 0], [V, 0, 0], [7, 2, 0], [299, 5, 0]], np.int32)
        nc = np.array([2, 1, 2, 0], np.int32)
        rows = e.lm_terms(lm, ctx, nc, eos=2).cpu().numpy()
        assert np.array_equal(rows.view(np.uint32), lm.terms(ctx, nc, eos=2).view(np.uint32))
        assert e.check_flags() == 0
        out = e.beam_lm(lm, 4, 0.5, 0.5)
        assert e.check_flags() == 0
        assert out["tokens"].shape[0] == B
        for m in (lm, host, full):
            m.close()
    finally:
        e.close()
