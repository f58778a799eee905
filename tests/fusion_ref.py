"""Yardstick of the fused beam (include/casr.h casr_beam_lm): a numpy restatement from the
definition, on the oracle's encoder_forward, decoder_step and _log_softmax and the reference LM
(tests/ngram_ref.py RefLM).  It shares no code with the product.

    am  = (x_v / T - lse_r) + a_r
    lm  = l == 0 ? term : g_r + term
    val = (am + lm_weight lm) + len_l,  len_l = float32(float64(length_weight) (l + 1))

every operation a float32 operation.  Top 2k of val per utterance (ties to the lower flat index, step
0 ranks beam 0 only), the oracle's record / early-stop / active-set rules on that ranking, am and lm
carried separately; the best is the first maximum of (rec_am + lm_weight rec_lm) + len_l over the
records, or over the live rows of the last step without one.

Also here: the inputs the CPU and GPU comparisons share (fusion_case), so the LM is the same object on
both sides."""
import functools

import numpy as np

import ngram_ref as R
from golden_util import fbank_for
from oracle import casr_oracle as O

F = np.float32


class TermRows:
    """terms(ctx)[v]: RefLM.term of every ASR token v after ctx (LM ids, oldest first; v == eos scores
    </s>).  A word that only has a unigram under ctx gets the m = 1 chain, vectorised (the same f32
    adds in the same order); every word some longer n-gram lists after a suffix of ctx, the eos
    token and the tokens without a unigram go through RefLM.term itself."""

    def __init__(self, ref, eos):
        self.ref, self.eos, V = ref, eos, ref.V
        self.uni = np.array([ref.grams[0].get((v,), (F(0), F(0)))[0] for v in range(V)], F)
        self.has_uni = np.array([(v,) in ref.grams[0] for v in range(V)])
        self.after = {}
        for g in ref.grams[1:]:
            for key in g:
                self.after.setdefault(key[:-1], set()).add(key[-1])
        self.cache = {}

    def __call__(self, ctx):
        ref, V = self.ref, self.ref.V
        ctx = tuple(ctx)[-(ref.order - 1):] if ref.order > 1 else ()
        row = self.cache.get(ctx)
        if row is None:
            row = self.uni.copy()
            for j in range(1, len(ctx) + 1):
                c = ctx[len(ctx) - j:]
                if c in ref.grams[j - 1]:
                    row = (row + F(ref.grams[j - 1][c][1])).astype(F)
            special = {self.eos} | set(np.nonzero(~self.has_uni)[0].tolist())
            for j in range(1, len(ctx) + 1):
                special |= {w for w in self.after.get(ctx[len(ctx) - j:], ()) if w < V}
            for v in special:
                row[v] = ref.term(ctx, ref.lm_id(ref.eos) if v == self.eos else ref.lm_id(v))
            self.cache[ctx] = row
        return row


def encode(feats, lens, enc_sd, dec_sd):
    """The part of a decode that does not depend on k or the LM."""
    lens = np.asarray(lens, np.int64)
    enc, (h, c) = O.encoder_forward(feats, lens, enc_sd)
    return enc, h, c, O.mask_for_softmax(lens), O.compute_keys(enc, dec_sd)


def fused_beam(encoded, dec_sd, k, ref_lm, lm_weight, length_weight, sos=1, eos=2, pad=0, max_len=40,
               temperature=1.0):
    """Returns dict(tokens, score (the choice's am), lm, records {b: [(tokens, am, lm)]} in (step,
    rank) order, steps, gap [B]: per utterance the smallest distance between vals adjacent in rank
    among the best 2k + 1, over all steps; gap_steps [steps, B]: the same per step)."""
    enc, h, c, mask, keys = encoded
    B = enc.shape[1]
    V = dec_sd["proj_linear.weight"].shape[0]
    rows = TermRows(ref_lm, eos)
    w = F(lm_weight)
    rep = np.repeat(np.arange(B), k)
    enc_t, mask_t, keys_t = enc[:, rep], mask[:, rep], keys[:, rep]
    h, c = h[rep], c[rep]
    ctx = np.zeros((B * k, enc.shape[2]), F)
    hist = np.full((max_len + 1, B * k), pad, np.int64)
    hist[0] = sos
    a_buf, g_buf = np.zeros(B * k, F), np.zeros(B * k, F)
    bb_off = k * np.arange(B)
    records = {b: [] for b in range(B)}
    top_fin = np.zeros(B, bool)
    gap, gap_steps = np.full(B, np.inf), []
    len_of = lambda l: F(float(F(length_weight)) * float(l + 1))
    comb = lambda am, lm, l: F(F(am + F(w * lm)) + len_of(l))
    l = 0
    for l in range(max_len):
        logit, h, c, ctx, _ = O.decoder_step(enc_t, mask_t, keys_t, hist[l], h, c, ctx, dec_sd)
        logit = (logit / F(temperature)).astype(F)
        am = (O._log_softmax(logit) + a_buf[:, None]).astype(F)
        term = np.stack([rows([ref_lm.lm_id(ref_lm.bos)] + [ref_lm.lm_id(int(t)) for t in hist[1:l + 1, r]])
                         for r in range(B * k)])
        lm = term if l == 0 else (g_buf[:, None] + term).astype(F)
        val = ((am + (w * lm).astype(F)).astype(F) + len_of(l)).astype(F)
        flat = lambda x: x.reshape(B, k * V)[:, :V] if l == 0 else x.reshape(B, k * V)
        val, am, lm = flat(val), flat(am), flat(lm)
        order = np.argsort(-val, axis=1, kind="stable")[:, :2 * k + 1]
        ranked = np.take_along_axis(val, order, axis=1).astype(np.float64)
        gap_steps.append((ranked[:, :-1] - ranked[:, 1:]).min(axis=1))
        gap = np.minimum(gap, gap_steps[-1])
        order = order[:, :2 * k]
        cand_am = np.take_along_axis(am, order, axis=1)
        cand_lm = np.take_along_axis(lm, order, axis=1)
        cand_beams, cand_tok = order // V, order % V
        for b in range(B):
            for j in range(k):
                if cand_tok[b, j] == eos:
                    src = b * k + cand_beams[b, j]
                    records[b].append((hist[1:l + 1, src].tolist(), cand_am[b, j], cand_lm[b, j], l))
        top_fin |= cand_tok[:, 0] == eos
        if top_fin.all():
            break
        key = np.arange(2 * k)[None, :] + (cand_tok == eos) * (2 * k)
        active = np.argsort(key, axis=1, kind="stable")[:, :k]
        bb = (np.take_along_axis(cand_beams, active, axis=1) + bb_off[:, None]).reshape(-1)
        h, c, ctx = h[bb], c[bb], ctx[bb]
        hist = hist[:, bb]
        hist[l + 1] = np.take_along_axis(cand_tok, active, axis=1).reshape(-1)
        a_buf = np.take_along_axis(cand_am, active, axis=1).reshape(-1).astype(F)
        g_buf = np.take_along_axis(cand_lm, active, axis=1).reshape(-1).astype(F)
    toks, score, lms = [], [], []
    for b in range(B):
        if records[b]:
            i = int(np.argmax([comb(a, q, rl) for _, a, q, rl in records[b]]))
            t, a, q, _ = records[b][i]
        else:
            j = int(np.argmax([comb(a_buf[b * k + j], g_buf[b * k + j], l) for j in range(k)]))
            t, a, q = hist[1:l + 2, b * k + j].tolist(), a_buf[b * k + j], g_buf[b * k + j]
        toks.append(t)
        score.append(F(a))
        lms.append(F(q))
    return dict(tokens=toks, score=np.array(score, F), lm=np.array(lms, F),
                records={b: [(t, a, q) for t, a, q, _ in v] for b, v in records.items()}, steps=l + 1, gap=gap,
                gap_steps=np.stack(gap_steps))


# ---------------------------------------------------------------------------- shared inputs
# Chosen on the CPU (tests/test_fusion_ref_host.py asserts it): with eos_bias 33 the search of these six
# utterances (golden_util.fbank_for's ids) stops after two steps, and at k = 2 and k = 4 every
# utterance's smallest gap between vals adjacent in rank is >= 3e-2; three of the six choices differ
# from the plain beam's.  At k = 16 the 33 best vals of a step lie closer than 1e-2 for every utterance
# tried, so k = 16 is covered by the device tests' invariants instead.
B, T = 6, 101
UTTS = (11, 13, 16, 23, 24, 25)
EOS_BIAS = 33.0
WEIGHTS = (1.5, 1.5)
LM_SEED = 500
GPU_K = (2, 4)  # the widths compared against this reference on the device (gap >= 1e-2 checked on the CPU)


def lm_grams_from_records(recs, V, seed):
    """tests/test_gpu_ngram.py _lm_from_records' recipe on {b: [(tokens, ...)]}: a 4-gram model seeded
    with half of the records' own n-grams, one in eight of their tokens without a unigram."""
    rs = np.random.RandomState(seed)
    seen, toks = set(), set()
    for v in recs.values():
        for rec in v:
            t = rec[0]
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
    return grams


@functools.lru_cache(maxsize=None)
def fusion_case():
    """The inputs of the comparisons: synthetic peaked weights (EOS_BIAS), the B = 6 utterances UTTS of
    T = 101 frames, and a 4-gram LM from the records of the oracle's plain beam at k = 4.  Returns dict(cfg,
    enc_sd, dec_sd, feats, lens, encoded, grams, plain {k: O.beam_decode's result})."""
    from casr.config import CasrConfig
    from casr.weights import synthetic_state_dicts
    cfg = CasrConfig()
    enc_sd, dec_sd = synthetic_state_dicts(cfg, peaked=True, eos_bias=EOS_BIAS)
    feats = [O.features_from_fbank(fbank_for(b, T)) for b in UTTS]
    lens = [f.shape[0] for f in feats]
    plain4 = O.beam_decode(feats, lens, enc_sd, dec_sd, 4)
    grams = lm_grams_from_records(plain4["records"], cfg.vocab, LM_SEED)
    return dict(cfg=cfg, enc_sd=enc_sd, dec_sd=dec_sd, feats=feats, lens=lens,
                encoded=encode(feats, lens, enc_sd, dec_sd), grams=grams, plain={4: plain4})


@functools.lru_cache(maxsize=None)
def fused_case(k, lm_weight=WEIGHTS[0], length_weight=WEIGHTS[1]):
    case = fusion_case()
    ref = R.RefLM(4, case["cfg"].vocab, case["grams"])
    return fused_beam(case["encoded"], case["dec_sd"], k, ref, lm_weight, length_weight)
