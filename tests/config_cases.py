"""The configurations beyond the deployed one that the suite runs (test helper, not a conftest; used by
test_gpu_configs.py on the device and test_configs_host.py on the CPU).

include/casr.h accepts enc_layers 1..8, residual 0 / 1, any vocab >= 4, any max_len >= 1, any sos and
eos of the vocabulary and any temperature > 0.  The cases here are the values of each axis at which the
plans, the weight layout or the kernels take another branch; every other dimension stays at the
deployed value.  A case names a configuration, a batch (frame counts and an fbank seed) and, for the
searches whose tokens the device must share with the numpy oracle, the search: test_configs_host.py
shows for each of those that a float64 run of the same search keeps the oracle's tokens, so that the
demand does not rest on a near tie.
"""
import contextlib
import functools
from collections import namedtuple

import numpy as np

from golden_util import fbank_for
from oracle import casr_oracle as O
from casr.config import CasrConfig
from casr.weights import synthetic_state_dicts

RAGGED6 = (101, 75, 48, 9, 6, 200)   # test_gpu_accuracy.ENC_SHAPES["ragged6"]
SMALL3 = (101, 75, 48)               # test_gpu_accuracy.SMALL_FRAMES
ATOL = 2e-3                          # tokens and scores against the oracle: the file-wide tolerance


def config(V=5004, layers=4, residual=True, L=40, sos=1, eos=2, temperature=1.0):
    return CasrConfig(max_num_words=V - 4, enc_layers=layers, residual=residual, max_len=L, sos=sos, eos=eos,
                      temperature=temperature)


@functools.lru_cache(maxsize=4)
def weights(cfg, peaked):
    """synthetic_state_dicts of the config: the shapes follow enc_layers and vocab, the peaked eos bias
    sits at cfg.eos.  Read-only."""
    enc_sd, dec_sd = synthetic_state_dicts(cfg, peaked=peaked)
    for sd in (enc_sd, dec_sd):
        for v in sd.values():
            v.setflags(write=False)
    return enc_sd, dec_sd


def fbank(b, t, seed=0):
    """utterance b of a batch: golden_util.fbank_for at seed 0, another draw of the same kind otherwise"""
    return fbank_for(b + 1000 * seed, t)


# ---------------------------------------------------------------- the axes
ENCODERS = [(1, True), (2, False), (4, False), (8, True)]          # (enc_layers, residual)
VOCABS = [4, 36, 83, 5003, 5120, 5121, 7168, 7169]
BEAM_WIDTHS = [1, 4, 16]                                            # run where 2k <= V
BIG_VOCABS = [36, 5003]                                             # B = 128, k = 8: R = 1024
TOKEN_IDS = [(83, 82, 0), (83, 0, 82), (5004, 5003, 5002)]          # (V, sos, eos)
MAX_LENS = [1, 2, 3]
# the fbank draw of the max_len batch: the 48-frame utterance's first token is the eos, so a finished
# record and the unfinished fallback both occur at max_len = 1 (test_configs_host.py asserts it)
MAX_LEN_SEED = 11
TEMPERATURES = [0.7, 2.0]


# what the plan decides from the vocabulary alone (csrc/decode_plan.h; tests/host_plan/plan_check.cpp
# checks these boundaries by value)
def greedy_folds(V):
    """the fused GEMM's seven-tile column blocks over vocabulary and pad tiles fit the 64 partial blocks"""
    return ((V + 15) // 16 + 6) // 7 <= 64


def projection_partials(V):
    """the three-launch projection's five-tile column blocks fit the 64 partial blocks"""
    return ((V + 63) // 64 * 4 + 4) // 5 <= 64


# ---------------------------------------------------------------- searches compared with the oracle
Search = namedtuple("Search", "id cfg frames seed kind k")


def _searches():
    out = []
    for layers, residual in ENCODERS:
        out.append(Search(f"enc-l{layers}r{int(residual)}-greedy", config(layers=layers, residual=residual), RAGGED6, 0,
                          "greedy", 1))
    for V, sos, eos in TOKEN_IDS:
        cfg = config(V=V, sos=sos, eos=eos)
        out.append(Search(f"ids-V{V}s{sos}e{eos}-greedy", cfg, SMALL3, 0, "greedy", 1))
        for k in (4, 16):
            out.append(Search(f"ids-V{V}s{sos}e{eos}-beam{k}", cfg, SMALL3, 0, "beam", k))
    for L in MAX_LENS:
        out.append(Search(f"len-L{L}-greedy", config(L=L), SMALL3, MAX_LEN_SEED, "greedy", 1))
        out.append(Search(f"len-L{L}-beam8", config(L=L), SMALL3, MAX_LEN_SEED, "beam", 8))
    out.append(Search("temp-T2.0-beam4", config(temperature=2.0), SMALL3, 0, "beam", 4))
    return out


SEARCHES = {s.id: s for s in _searches()}


@contextlib.contextmanager
def oracle_dtype(dtype):
    """every float32 of the oracle replaced by dtype (its F32 is looked up at call time)"""
    old = O.F32
    O.F32 = dtype
    try:
        yield
    finally:
        O.F32 = old


@functools.lru_cache(maxsize=None)
def _encoded(layers, residual, frames, seed, dtype):
    enc_sd, _ = weights(config(layers=layers, residual=residual), True)
    feats = [O.features_from_fbank(fbank(b, t, seed)).astype(dtype) for b, t in enumerate(frames)]
    lens = [f.shape[0] for f in feats]
    with oracle_dtype(dtype):
        return lens, O.encoder_forward(feats, lens, {n: v.astype(dtype) for n, v in enc_sd.items()}, layers, residual)


@functools.lru_cache(maxsize=None)
def oracle_search(sid, dtype=np.float32):
    """The oracle's greedy or beam decode of one SEARCHES entry with the peaked weights, in dtype.  The
    encoder runs once per (depth, residual, batch, dtype)."""
    s = SEARCHES[sid]
    cfg = s.cfg
    lens, encoded = _encoded(cfg.enc_layers, cfg.residual, s.frames, s.seed, dtype)
    dec_sd = {n: v.astype(dtype) for n, v in weights(cfg, True)[1].items()}
    real = O.encoder_forward
    with oracle_dtype(dtype):
        O.encoder_forward = lambda *a, **kw: encoded
        try:
            kw = dict(sos=cfg.sos, eos=cfg.eos, max_len=cfg.max_len, temperature=cfg.temperature,
                      num_layers=cfg.enc_layers, residual=cfg.residual)
            if s.kind == "greedy":
                return O.greedy_decode([None] * len(lens), lens, None, dec_sd, **kw)
            return O.beam_decode([None] * len(lens), lens, None, dec_sd, s.k, pad=cfg.pad, **kw)
        finally:
            O.encoder_forward = real


# ---------------------------------------------------------------- the derived searches at V = 83, eos = 0
# casr_beam_grammar, casr_beam_lm and casr_beam_bias at (sos, eos) = (82, 0).  What the inputs must
# give, and test_configs_host.py asserts: at DERIVED_EOS_BIAS, under a random 4-gram model over the 83
# ids at weights 1.5 / 1.5, the fused search and the biased one (with and without the LM; phrases drawn
# from the fused search's records by bias_ref.draw_phrases) keep every step's best 2k + 1 vals at least
# 1e-2 apart at k = DERIVED_K, finish hypotheses before max_len, and the bias changes a choice.  At
# k = 4 the fused gap is below 1e-2, so only k = 2 is compared with the restatements, as bias_ref.GPU_K
# does at the deployed config.  At DERIVED_PLAIN_EOS_BIAS the plain beam search finishes hypotheses and
# ends after more than one step and before max_len at every width of DERIVED_IDENTITY_K: the identities
# with casr_beam run there (at the last step the grammar's horizon rule offers eos only).
DERIVED_CFG = config(V=83, sos=82, eos=0)
DERIVED_EOS_BIAS = 20.0
DERIVED_PLAIN_EOS_BIAS = 18.0
DERIVED_IDENTITY_K = (2, 4, 16)
DERIVED_LM_SEED = 61
DERIVED_PHRASE_SEED = 9
DERIVED_WEIGHTS = (1.5, 1.5)   # lm_weight, length_weight
DERIVED_K = 2


@functools.lru_cache(maxsize=None)
def derived_case():
    """dict(cfg, enc_sd, dec_sd, grams, phrases, boosts, fused, biased {with_lm: result}): the inputs
    and the numpy restatements' answers (fusion_ref.fused_beam, bias_ref.biased_beam)."""
    import bias_ref as BR
    import fusion_ref as FR
    import ngram_ref as NR
    cfg = DERIVED_CFG
    V, ids = cfg.vocab, dict(sos=cfg.sos, eos=cfg.eos, pad=cfg.pad, max_len=cfg.max_len)
    enc_sd, dec_sd = synthetic_state_dicts(cfg, peaked=True, eos_bias=DERIVED_EOS_BIAS)
    feats = [O.features_from_fbank(fbank(b, t)) for b, t in enumerate(SMALL3)]
    encoded = FR.encode(feats, [f.shape[0] for f in feats], enc_sd, dec_sd)
    grams = NR.random_model(4, V, DERIVED_LM_SEED, n_high=300)
    ref = NR.RefLM(4, V, grams)
    fused = FR.fused_beam(encoded, dec_sd, DERIVED_K, ref, *DERIVED_WEIGHTS, **ids)
    phrases, boosts = BR.draw_phrases(fused["records"], np.random.RandomState(DERIVED_PHRASE_SEED))
    biased = {w: BR.biased_beam(encoded, dec_sd, DERIVED_K, phrases, boosts, 1.0, ref if w else None,
                                DERIVED_WEIGHTS[0] if w else 0.0, DERIVED_WEIGHTS[1], **ids) for w in (True, False)}
    return dict(cfg=cfg, enc_sd=enc_sd, dec_sd=dec_sd, grams=grams, phrases=phrases, boosts=boosts, fused=fused,
                biased=biased)


@functools.lru_cache(maxsize=None)
def derived_plain_weights():
    """the derived configuration's weights at DERIVED_PLAIN_EOS_BIAS"""
    return synthetic_state_dicts(DERIVED_CFG, peaked=True, eos_bias=DERIVED_PLAIN_EOS_BIAS)


@functools.lru_cache(maxsize=None)
def derived_plain_beam(k):
    """O.beam_decode at DERIVED_PLAIN_EOS_BIAS"""
    cfg = DERIVED_CFG
    feats = [O.features_from_fbank(fbank(b, t)) for b, t in enumerate(SMALL3)]
    return O.beam_decode(feats, [f.shape[0] for f in feats], *derived_plain_weights(), k, sos=cfg.sos, eos=cfg.eos,
                         pad=cfg.pad, max_len=cfg.max_len)
