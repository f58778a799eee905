"""Teacher-forced scoring (casr_score / Engine.score) against the reference fixture
(tests/golden/score_golden.npz, captured by make_score_golden.py) and the CPU oracle, in both MFMA
arithmetics (the eng fixture, as test_gpu_parity.py).

Tolerances: total_logp and the greedy-form score 2e-3 (the project's tolerance for sums of up to 40
log-probabilities), alignments 1e-5 (the project's), and per token (token_logp, best_logp,
mean_logp) PTOL below: 4x the largest deviation measured over tests 1 and 2 in both arithmetics,
capped at 2e-3 (a single token cannot legitimately be worse than the 40-token sum)."""
import functools
import os

import numpy as np
import pytest
import torch

from golden_util import load_golden, fbank_for, golden_frames
from oracle import casr_oracle as O
from casr.config import CasrConfig
from casr.lib import pack_weights
from casr.results import label_smoothed_loss, score_outputs
from casr.weights import synthetic_state_dicts

pytestmark = pytest.mark.gpu

G, META = load_golden()
CFG = CasrConfig()
V, LMAX = CFG.vocab, CFG.max_len
NUTT = 8
FRAMES = golden_frames(META)[:NUTT]
SG = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_golden.npz"))

# per-token tolerance.  Measured maxima of |device - reference| over token_logp, best_logp and
# mean_logp in tests 1 and 2 (MI355X; the [score-dev] lines of a run with -s):
#                          s16x3      f32
#   fixture, plain         1.9e-06    1.9e-06
#   fixture, peaked        1.7e-05    1.6e-05
#   oracle, plain  (5 R)   2.9e-06    2.9e-06
#   oracle, peaked (5 R)   5.531e-05  5.722e-05   (both at R = 1320, token_logp)
# MEASURED is the largest of them; PTOL = min(4 x MEASURED, 2e-3) = 2.29e-4
MEASURED = 5.722e-05
PTOL = min(4 * MEASURED, 2e-3)
ALIGN_ATOL = 1e-5
SUM_ATOL = 2e-3


@pytest.fixture(scope="module", params=["s16x3", "f32"])
def eng(request):
    from casr.engine import Engine
    e = Engine(CFG, *synthetic_state_dicts(CFG, peaked=False))
    e.set_precision(request.param)
    e.requested = request.param
    assert e.precision() == request.param
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def weights(peaked):
    return synthetic_state_dicts(CFG, peaked=peaked)


@functools.lru_cache(maxsize=None)
def packed(peaked):
    return pack_weights(CFG, *weights(peaked))


def bind(eng, name):
    eng.bind(packed(name == "peaked"))


def encode(eng, frames):
    T = max(frames)
    x = np.zeros((len(frames), T, 80), np.float32)
    for b, t in enumerate(frames):
        x[b, :t] = fbank_for(b, t)
    fb = torch.from_numpy(x).to(eng.device)
    fr = torch.tensor(frames, dtype=torch.int32, device=eng.device)
    feat, flen = eng.features(fb, fr, eps=1e-6)
    eng.encode(feat, flen)


def run_score(eng, targets, tgt_len, **kw):
    out = eng.score(targets, tgt_len, alignment=True, best=True, mean=True, **kw)
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


def report(tag, eng, **devs):
    """each figure before it is asserted (a run with -s shows them; the maxima set MEASURED)"""
    print(f"[score-dev] {tag} {eng.requested} " + " ".join(f"{k}={v:.3e}" for k, v in devs.items()))


def scored(tgt_len, L):
    return np.arange(L)[None, :] < np.asarray(tgt_len)[:, None]


def maxdev(a, b, mask):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))[mask]
    return float(d.max()) if d.size else 0.0


# ------------------------------------------------------------------ 1. the reference fixture
@pytest.mark.parametrize("name", ["plain", "peaked"])
def test_matches_reference_fixture(eng, name):
    bind(eng, name)
    encode(eng, FRAMES)
    targets, n = SG[f"{name}_targets"], SG[f"{name}_tgt_len"]
    r = run_score(eng, targets, n)
    assert eng.device_flags() == 0
    m = scored(n, LMAX)
    d_tok = maxdev(r["token_logp"], SG[f"{name}_token_logp"], m)
    d_mean = maxdev(r["mean_logp"], SG[f"{name}_mean_logp"], m)
    _, score = score_outputs(r["token_logp"], n, SG[f"{name}_finished"])
    gold = META[name]["greedy"]["score"][:NUTT]
    report(f"fixture-{name}", eng, token=d_tok, mean=d_mean, score=float(np.abs(np.array(score) - gold).max()))
    assert d_tok <= PTOL and d_mean <= PTOL
    np.testing.assert_allclose(score, gold, rtol=0, atol=SUM_ATOL)
    np.testing.assert_allclose(r["total_logp"], SG[f"{name}_token_logp"].astype(np.float64).sum(1), rtol=0, atol=SUM_ATOL)
    # past tgt_len: exactly 0 (best_token -1)
    for k in ("token_logp", "best_logp", "mean_logp"):
        assert not r[k][~m].any(), k
    assert (r["best_token"][~m] == -1).all()
    # the targets are the reference's greedy argmax under the same feeding: the device's argmax
    # agrees, and its log-probability is the target's, bit for bit (the same logit, the same lse)
    assert (r["best_token"][m] == targets[m]).all()
    assert (r["best_logp"][m] == r["token_logp"][m]).all()
    # alignments of the scored steps: rows sum to 1, and the expectation sum_t t alpha_t moves by at
    # most 1e-5 T^2 / 2 when every weight moves by the alignment tolerance
    al = r["alignment"].astype(np.float64)
    for b, t in enumerate(FRAMES):
        T = t // 3
        k = int(n[b])
        np.testing.assert_allclose(al[:k, :, b].sum(1), SG[f"{name}_align_sum"][:k, b], rtol=0, atol=1e-4)
        assert not al[:, T:, b].any()
        np.testing.assert_allclose(al[:k, :T, b] @ np.arange(T), SG[f"{name}_align_expect"][:k, b], rtol=0,
                                   atol=ALIGN_ATOL * T * T / 2)


# ------------------------------------------------------------------ 2. the oracle at each projection shape
# (frames, L): R = L B rows of the batched projection in each of launch_proj's shape classes
SHAPES = {
    "R21": ([101, 75, 48], 7),      # R <= 32, a row-block tail
    "R120": ([75, 48, 60], 40),     # R <= 256 (this file's addition: the class between the issue's shapes)
    "R320": ([48] * 8, 40),         # R <= 512
    "R1320": ([60] * 33, 40),       # R > 512 (s16x3: the one-accumulator form; f32: two accumulators)
    "R2080": ([48] * 52, 40),       # R >= 2048 (dec_wide)
}


def shape_targets(frames, L):
    B = len(frames)
    t = np.random.RandomState(77).randint(3, V, size=(B, L)).astype(np.int32)
    t[0, :4] = [0, 79, 80, V - 1][:min(4, L)]  # first column, both sides of an 80-column block edge, last column
    n = np.random.RandomState(78).randint(1, L + 1, size=B).astype(np.int32)
    n[0] = L
    n[-1] = 0
    if B > 2:
        n[1] = L - 1
    return t, n


@functools.lru_cache(maxsize=None)
def oracle_score(peaked, key):
    """The oracle's teacher-forced pass (computed once per weight set and shape, shared by both
    arithmetics; read-only)."""
    frames, L = SHAPES[key]
    enc_sd, dec_sd = weights(peaked)
    targets, n = shape_targets(frames, L)
    B = len(frames)
    feats = [O.features_from_fbank(fbank_for(b, t)) for b, t in enumerate(frames)]
    lens = np.array([f.shape[0] for f in feats])
    enc, (h, c) = O.encoder_forward(feats, lens, enc_sd)
    mask = O.mask_for_softmax(lens)
    keys = O.compute_keys(enc, dec_sd)
    ctx = np.zeros((B, enc.shape[2]), np.float32)
    tok = np.full(B, CFG.sos, np.int64)
    res = dict(token_logp=np.zeros((B, L), np.float32), mean_logp=np.zeros((B, L), np.float32),
               best_logp=np.zeros((B, L), np.float32), best_token=np.full((B, L), -1, np.int64),
               gap=np.zeros((B, L), np.float32), align=np.zeros((L, enc.shape[0], B), np.float32))
    for l in range(L):
        logit, h, c, ctx, alpha = O.decoder_step(enc, mask, keys, tok, h, c, ctx, dec_sd)
        lp = O._log_softmax(logit)
        live = l < n
        rows = np.arange(B)
        res["align"][l] = alpha
        res["token_logp"][:, l] = np.where(live, lp[rows, targets[:, l]], 0)
        res["mean_logp"][:, l] = np.where(live, logit.mean(1, dtype=np.float64) - (logit[:, 0] - lp[:, 0]), 0)
        top2 = np.sort(logit, axis=1)[:, -2:]
        res["gap"][:, l] = top2[:, 1] - top2[:, 0]
        res["best_token"][:, l] = np.where(live, logit.argmax(1), -1)
        res["best_logp"][:, l] = np.where(live, lp.max(1), 0)
        tok = np.where(live, targets[:, l], CFG.eos).astype(np.int64)
    tot = np.zeros(B, np.float32)
    for b in range(B):
        for l in range(int(n[b])):
            tot[b] = np.float32(tot[b] + res["token_logp"][b, l])
    res["total_logp"] = tot
    for v in res.values():
        v.setflags(write=False)
    return targets, n, res


@pytest.mark.parametrize("key", list(SHAPES))
@pytest.mark.parametrize("name", ["plain", "peaked"])
def test_matches_oracle_at_each_projection_shape(eng, name, key):
    frames, L = SHAPES[key]
    targets, n, ref = oracle_score(name == "peaked", key)
    bind(eng, name)
    encode(eng, frames)
    r = run_score(eng, targets, n)
    assert eng.device_flags() == 0
    m = scored(n, L)
    d = {k: maxdev(r[k], ref[k], m) for k in ("token_logp", "mean_logp", "best_logp")}
    d_tot = float(np.abs(r["total_logp"].astype(np.float64) - ref["total_logp"]).max())
    d_al = float(np.abs(r["alignment"] - ref["align"]).max())
    report(f"oracle-{name}-{key}", eng, total=d_tot, align=d_al, **d)
    assert d_tot <= SUM_ATOL
    assert d_al <= ALIGN_ATOL
    assert max(d.values()) <= PTOL, d
    for k in ("token_logp", "best_logp", "mean_logp"):
        assert not r[k][~m].any(), k
    # the device's own total: its token_logp added in ascending l, in f32
    np.testing.assert_array_equal(r["total_logp"], score_outputs(r["token_logp"], n, np.zeros(len(n)))[0])
    if name == "peaked":  # plain weights give almost flat logits (46 of 2,080 positions under the gap)
        clear = m & (ref["gap"] >= 1e-3)
        assert (m & ~clear).sum() <= 0.005 * m.sum(), ((m & ~clear).sum(), m.sum())
        assert (r["best_token"][clear] == ref["best_token"][clear]).all()


# ------------------------------------------------------------------ 3. the three-launch step's arithmetic
@pytest.mark.parametrize("name", ["plain", "peaked"])
def test_same_arithmetic_as_three_launch_greedy(eng, name):
    """The step loop reuses the LSTMCell GEMM and attention launches of CASR_OPT_DEC_FOLD = 0 greedy:
    scoring greedy's own tokens reproduces its attention weights bit for bit at every step of an
    utterance's transcript (plain weights: all 40 executed steps of all utterances; peaked: an
    utterance's steps up to its eos, after which greedy goes on feeding its argmax and scoring
    feeds eos), and the sum of its token log-probabilities is greedy's accum."""
    bind(eng, name)
    eng.set_option("DEC_FOLD", 0)
    try:
        encode(eng, FRAMES)
        g = eng.greedy(alignment=True)
        n = (g["out_len"] + g["finished"].to(torch.int32)).cpu().numpy()
        r = run_score(eng, g["tokens"], n)
        assert eng.device_flags() == 0
    finally:
        eng.set_option("DEC_FOLD", 1)
    ga = g["alignment"].cpu().numpy()
    if name == "plain":
        assert n.tolist() == [LMAX] * NUTT
    for b in range(NUTT):
        k = int(n[b])
        assert k > 0
        np.testing.assert_array_equal(r["alignment"][:k, :, b], ga[:k, :, b])
    np.testing.assert_allclose(r["total_logp"], g["accum"].cpu().numpy(), rtol=0, atol=SUM_ATOL)
    m = scored(n, LMAX)
    assert (r["best_token"][m] == g["tokens"].cpu().numpy()[m]).all()


# ------------------------------------------------------------------ 4. padding is inert
def test_padding_entries_are_never_used(eng):
    bind(eng, "peaked")
    encode(eng, FRAMES)
    targets, n = SG["peaked_targets"].copy(), SG["peaked_tgt_len"]
    m = scored(n, LMAX)
    base = run_score(eng, targets, n)
    assert eng.device_flags() == 0
    for pad in (-1, V + 7):
        t = targets.copy()
        t[~m] = pad
        r = run_score(eng, t, n)
        assert eng.device_flags() == 0
        for k in ("token_logp", "total_logp", "best_token", "best_logp", "mean_logp", "alignment"):
            np.testing.assert_array_equal(r[k], base[k], err_msg=f"pad {pad}: {k}")


# ------------------------------------------------------------------ 5. the encode is untouched
def test_score_leaves_the_encode_untouched(eng):
    bind(eng, "peaked")
    targets, n = SG["peaked_targets"], SG["peaked_tgt_len"]
    encode(eng, FRAMES)
    g0 = eng.greedy(alignment=True)
    b0 = eng.beam(4)
    encode(eng, FRAMES)
    eng.score(targets, n, alignment=True, best=True, mean=True)
    g1 = eng.greedy(alignment=True)
    eng.score(targets, n)
    b1 = eng.beam(4)
    assert eng.device_flags() == 0
    for k in ("tokens", "out_len", "finished", "accum", "alignment"):
        assert torch.equal(g0[k], g1[k]), k
    for k in ("tokens", "length", "score", "steps"):
        assert torch.equal(b0[k], b1[k]), k


# ------------------------------------------------------------------ 6. Model.score_one_batch
def test_model_score_one_batch_loss_matches_oracle():
    import model as M
    from gpd import gpd
    key = "R120"
    frames, L = SHAPES[key]
    targets, n = shape_targets(frames, L)  # Model() starts from the plain synthetic weights
    n = np.maximum(n, 1)  # give the empty transcript one token: every utterance is scored
    m = M.Model()
    feats = [torch.from_numpy(O.features_from_fbank(fbank_for(b, t))).to(m.device) for b, t in enumerate(frames)]
    lens = torch.tensor([f.shape[0] for f in feats])
    text = [targets[b, :n[b]].tolist() for b in range(len(frames))]
    had = "label_smooth" in gpd
    old = gpd.get("label_smooth")
    try:
        for ls in (None, 0.1):
            if ls is None:
                gpd.pop("label_smooth", None)
            else:
                gpd["label_smooth"] = ls
            res = m.score_one_batch(m.device, feats, lens, text, word2int=False, eos=False)
            want = label_smoothed_loss(oracle_full(key)[0], oracle_full(key)[1], n, V, ls or 0.0)
            want = float(want.sum(dtype=np.float64) / n.sum())
            print(f"[score-dev] model-loss ls={ls} dev={abs(res.loss - want):.3e}")
            # every term of the loss is a per-token log-probability with weights summing to
            # (1 - ls) + ls V / (V - 1) + ls / (V - 1) <= 1 + 2 / (V - 1)
            assert abs(res.loss - want) <= PTOL * (1 + 2 / (V - 1))
            assert [len(t) for t in res.token_logp] == n.tolist()
            assert res.times["frame"].shape == (len(frames), int(n.max()))
            assert all(len(t) == int(k) for t, k in zip(res.best_text, n))
    finally:
        if had:
            gpd["label_smooth"] = old
        else:
            gpd.pop("label_smooth", None)


@functools.lru_cache(maxsize=None)
def oracle_full(key):
    """token_logp / mean_logp of the plain-weight oracle with every position scored (the feed of
    step l is targets[:, l - 1] wherever l - 1 < tgt_len, which for the Model test's whole
    transcripts means: positions below max(tgt_len, 1))."""
    frames, L = SHAPES[key]
    enc_sd, dec_sd = weights(False)
    targets, n = shape_targets(frames, L)
    n = np.maximum(n, 1)
    B = len(frames)
    feats = [O.features_from_fbank(fbank_for(b, t)) for b, t in enumerate(frames)]
    lens = np.array([f.shape[0] for f in feats])
    enc, (h, c) = O.encoder_forward(feats, lens, enc_sd)
    mask = O.mask_for_softmax(lens)
    keys = O.compute_keys(enc, dec_sd)
    ctx = np.zeros((B, enc.shape[2]), np.float32)
    tok = np.full(B, CFG.sos, np.int64)
    lpt, mlp = np.zeros((B, L), np.float32), np.zeros((B, L), np.float32)
    for l in range(L):
        logit, h, c, ctx, _ = O.decoder_step(enc, mask, keys, tok, h, c, ctx, dec_sd)
        lp = O._log_softmax(logit)
        lpt[:, l] = lp[np.arange(B), targets[:, l]]
        mlp[:, l] = logit.mean(1, dtype=np.float64) - (logit[:, 0] - lp[:, 0])
        tok = np.where(l < n, targets[:, l], CFG.eos).astype(np.int64)
    return lpt, mlp
