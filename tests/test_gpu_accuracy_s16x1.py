"""Float64 accuracy budgets for the s16x1 build (libcasr_hip_s16x1.so: every split product keeps its
hi.hi MFMA only), stage by stage, against the exact model of its own arithmetic.

s16x1 computes, at every MFMA site, sum_k f16(a_k) f16(b_k) with f32 accumulators: hi = (_Float16)x
is a round to nearest even and every f16 x f16 product is exact in f32.  The reference of a stage is
therefore not the plain float64 stage but the float64 stage with both operands of each MFMA site
rounded to f16 (tests/f64_ref.py, ``sites``; the site table there cites the kernel line of each),
and the float32 reference of the budget is the same model evaluated in numpy float32.  Against that
pair the device must sit where a float32 evaluation sits: f64_ref.budget at M_DEFAULT = 8, maximum
and rms, exact zeros (keys: exactly b_attn) outside the valid elements, clean device flags and
precision() == "s16x1" in every case.  As in test_gpu_accuracy.py each stage is fed the device's own
output of the stage before it, and the helpers are that file's.

Through a dependent chain (the recurrence, the decode steps) two float32-grade evaluations of the
model differ in the last bits of h, and some of those differences flip the f16 rounding of the next
operand: per element the device can be 2^-12 |h| from the model.  The float32 evaluation of the
model flips at the same rate, so the budget calibrates itself; its resolution through a chain is
about one mis-rounded site (test_accuracy_budget_host.py: truncation at every site, bf16 at every
site and a dropped 32-k block at any one site are rejected; bf16 at one site is above M at every site
but the embedding's; the folded paths' f32 embedding table is not told from a rounded embedding).
The chain-free keys GEMM resolves a single site.  That analysis was made on the CPU, with float32
evaluations of the model; the table below is what the device itself measured.

  encoder, keys  ENC_SHAPES ragged6, B37, Tp267; keys with both weight sets and both KEYS_ROWS forms;
                 ragged6 also under GEMM16_PERSIST 0 / 1 and GEMM16_TAIL 1
  encode_fbank   bit for bit features + encode
  score          three-launch step + batched projection: R21 (plain, peaked), R320, R1320 (the
                 one-accumulator projection), R2080 peaked
  greedy         the folded greedy step: B19, B19-ksplit0, B33, both weight sets
  beam           three-launch at B3k2, B3k5; folded at B128k8 (CELL 4), B256k4 (CELL 3, 16 rows
                 re-scored), B128k16 (CELL 2, 16 rows); which step ran is read from the LSTMCell
                 GEMM's launch count

Run with -s: per quantity one "[acc] stage shape s16x1 what max_ratio= ..." line (the budget) and one
"[acc] stage shape s16x1 what cost e_dev_max= .. e_model_max= .." line, the device's and the float64
model's distance from the UNROUNDED float64 stage (sites = None).  The second is not asserted (it is
bounded by the budget plus the model's own distance): it is what s16x1 costs.
tools/acc_lines.py turns both into profiles/accuracy/accuracy_budget_s16x1.json.

MEASURED on one MI355X (every case is in profiles/accuracy/accuracy_budget_s16x1.json): per stage and
quantity the largest ratio of the device's error to the float32 model's over the cases, maximum and
rms, the shape of the largest maximum, and the cost: the largest distance of the device, and of the
float64 model, from the unrounded float64 stage.  All ratios are below M = 8; the largest is 2.12
(the beam score at B3k2, three-launch step, peaked weights).  Every other form of the input
projection and of the keys GEMM returned the default form's bits on ragged6.

  stage    quantity     cases     max    rms  worst shape      cost: device     model
  encoder  enc             13    1.13   1.03  Tp267-plain           1.7e-03   1.8e-03
  encoder  h               13    1.53   1.09  B37-plain             9.5e-04   9.6e-04
  encoder  c               13    1.07   1.07  ragged6-plain         1.6e-03   1.6e-03
  keys     keys            16    0.60   0.53  B37-peaked            4.8e-04   4.8e-04
  score    token_logp       5    1.05   1.01  R1320-peaked          1.0e-02   9.7e-03
  score    mean_logp        5    1.30   1.23  R21-plain             6.5e-03   6.1e-03
  score    best_logp        5    1.43   1.11  R320-peaked           5.0e-03   5.4e-03
  score    alignment        5    1.08   1.06  R2080-peaked          3.2e-06   3.0e-06
  score    total_logp       5    1.85   1.91  R21-plain             1.0e-01   9.0e-02
  greedy   accum            6    1.36   1.19  B33-peaked            3.9e-02   3.7e-02
  greedy   alignment        6    0.92   0.97  B19-ksplit0-peaked    2.1e-06   1.9e-06
  beam     score            8    2.12   1.85  B3k2-peaked           6.9e-02   7.2e-02

The beam cases (maximum / rms): B3k2-peaked 2.12 / 1.85, B3k5-peaked 1.51 / 1.38, B128k8 1.09 / 1.19
plain and 1.16 / 0.95 peaked, B256k4 1.10 / 1.42 and 1.43 / 1.36, B128k16 1.20 / 0.93 and 1.19 / 1.49.

The cost depends on the weights: with the plain set a token's log-probability is 6e-5 from the
unrounded stage (a 40-step sum 2.6e-3), with the peaked set up to 1e-2 (a sum up to 1e-1).  The float32
model's own error, for scale, is set by the flips where there is a chain: encoder output 2.4e-4 to
3.2e-4 (the plain stage's float32 oracle: 1e-6), per-token log-probabilities 1e-5 plain and 6e-4 to
3.7e-3 peaked, the 40-term sums 3e-4 plain and 4e-3 to 1.5e-2 peaked; the chain-free keys 0.7e-6 to
1.4e-6, alignments 1e-7 to 4e-7.  The budget therefore resolves about one mis-rounded site through a
chain and a single site on the keys; an s16x3-grade answer (operands left exact) would also pass the
chain stages, as test_accuracy_budget_host.py records.
"""
import numpy as np
import pytest
import torch

import f64_ref as R
import test_gpu_accuracy as TA
from test_gpu_accuracy import (BEAM_CASES, CFG, ENC_SHAPES, GREEDY_CASES, LMAX, M, batch_fbank, bind, cycle_frames,
                               encode, memo, results_tm, scored, valid_tb, weights)
from test_gpu_score import SHAPES, shape_targets
from casr.results import greedy_steps
from casr.weights import synthetic_state_dicts

pytestmark = pytest.mark.gpu

F32 = np.float32
ENC_SITES = R.SITES_X1_ENCODER


@pytest.fixture(scope="module")
def eng():
    from casr.engine import Engine
    e = Engine(CFG, *synthetic_state_dicts(CFG, peaked=False), arithmetic="s16x1")
    e.requested = "s16x1"
    assert e.precision() == "s16x1"
    yield e
    e.close()


def clean(eng):
    assert eng.device_flags() == 0
    assert eng.precision() == "s16x1"


def hold(cand, m64, m32, truth, tag, valid=None, pad=0.0):
    """The cost line (device and model against the unrounded float64 stage, printed only), then the
    budget against the model (printed, then asserted)"""
    d = R.figures(cand, truth, m64, valid)
    print(f"[acc] {tag} cost e_dev_max={d['e_max']:.3e} e_dev_rms={d['e_rms']:.3e} "
          f"e_model_max={d['e_ref_max']:.3e} e_model_rms={d['e_ref_rms']:.3e}")
    return R.budget(cand, m64, m32, M, valid=valid, pad=pad, tag=tag)


# ------------------------------------------------------------------ encoder and keys
@memo
def encoder_refs(feat, lens):
    """per quantity (model in float64, model in float32, the unrounded float64 stage)"""
    enc_sd, _ = weights(False)  # the encoder's weights are the same in both sets
    feats = [feat[b, :n] for b, n in enumerate(lens)]
    m64 = R.encoder(feats, lens, enc_sd, sites=ENC_SITES)
    m32 = R.encoder(feats, lens, enc_sd, sites=ENC_SITES, dtype=F32)
    plain = TA.encoder_refs(feat, lens)
    return {what: (m64[i], m32[i], plain[what][0]) for i, what in enumerate(("enc", "h", "c"))}


@memo
def keys_refs(enc, peaked):
    _, dec_sd = weights(peaked)
    return (R.compute_keys(enc, dec_sd, sites=ENC_SITES), R.compute_keys(enc, dec_sd, sites=ENC_SITES, dtype=F32),
            R.compute_keys(enc, dec_sd))


def hold_encoder_and_keys(eng, name, key, feat, lens, tag=""):
    enc, h, c, keys = results_tm(eng)
    clean(eng)
    tag = f"{key}-{name}{tag} s16x1"
    ref = encoder_refs(feat, lens)
    valid = valid_tb(lens, enc.shape[0])[:, :, None]
    hold(enc, *ref["enc"], f"encoder {tag} enc", valid=valid)
    hold(h, *ref["h"], f"encoder {tag} h")
    hold(c, *ref["c"], f"encoder {tag} c")
    _, dec_sd = weights(name == "peaked")
    hold(keys, *keys_refs(enc, name == "peaked"), f"keys {tag} keys", valid=valid,
         pad=dec_sd["attn_mechanism.b_attn"][None, None, :])
    return enc, h, c, keys


@pytest.mark.parametrize("key", list(ENC_SHAPES))
def test_encoder_and_keys_budget(eng, key):
    """Input projection (sites enc_ih), recurrence (enc_hh), residual and the keys GEMM (keys) in
    their default forms, plain weights; the keys again with the peaked W_enc on the same encode."""
    bind(eng, "plain")
    feat, lens = encode(eng, ENC_SHAPES[key])
    enc, _, _, _ = hold_encoder_and_keys(eng, "plain", key, feat, lens)
    bind(eng, "peaked")
    encode(eng, ENC_SHAPES[key])
    enc2, _, _, keys2 = results_tm(eng)
    clean(eng)
    assert np.array_equal(enc, enc2)
    _, dec_sd = weights(True)
    hold(keys2, *keys_refs(enc2, True), f"keys {key}-peaked s16x1 keys", valid=valid_tb(lens, enc2.shape[0])[:, :, None],
         pad=dec_sd["attn_mechanism.b_attn"][None, None, :])


FORMS = {
    # option values (GEMM16_PERSIST, GEMM16_TAIL, KEYS_ROWS); the defaults are (2, 2, 1)
    "persist0": (0, 2, 1),      # the per-tile input projection
    "persist1": (1, 2, 1),      # the round-2 persistent kernel
    "tail1": (2, 1, 1),         # half tiles after the whole rounds
    "persist1-tail1": (1, 1, 1),
    "keysrows0": (2, 2, 0),     # the keys GEMM as 128 x 128 tiles
}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["plain", "peaked"])
def test_encoder_and_keys_forms_budget(eng, name, form):
    """ragged6 through the other forms of the input projection and of the keys GEMM, each held to
    the same budget (the parity sweep of test_gpu_parity.py covers s16x3 only).  Whether a form
    returns the default form's bits under s16x1 is printed."""
    persist, tail, rows = FORMS[form]
    bind(eng, name)
    feat, lens = encode(eng, ENC_SHAPES["ragged6"])
    base = results_tm(eng)
    clean(eng)
    try:
        eng.set_option("GEMM16_PERSIST", persist)
        eng.set_option("GEMM16_TAIL", tail)
        eng.set_option("KEYS_ROWS", rows)
        feat2, _ = encode(eng, ENC_SHAPES["ragged6"])
        assert np.array_equal(feat, feat2)
        got = hold_encoder_and_keys(eng, name, "ragged6", feat, lens, tag="-" + form)
    finally:
        eng.set_option("GEMM16_PERSIST", 2)
        eng.set_option("GEMM16_TAIL", 2)
        eng.set_option("KEYS_ROWS", 1)
    print(f"[acc] forms ragged6-{name}-{form} s16x1 bit-equal to the default form: "
          + " ".join(f"{w}={np.array_equal(a, b)}" for w, a, b in zip(("enc", "h", "c", "keys"), base, got)))


def test_encode_fbank_equals_features_then_encode(eng):
    bind(eng, "plain")
    frames = ENC_SHAPES["ragged6"]
    encode(eng, frames)
    want = [t.cpu() for t in eng.encoder_results()]
    fb, fr = batch_fbank(frames, eng.device)
    eng.encode_fbank(fb, fr)
    clean(eng)
    for a, b in zip(want, eng.encoder_results()):
        assert torch.equal(a, b.cpu())


# ------------------------------------------------------------------ decode stages
@memo
def forced_refs(path, peaked, enc, keys, h, c, lens, targets, tgt_len, feed_len):
    """The teacher-forced pass of one decode path's model from the device's encoder results: model
    in float64, model in float32, the unrounded float64 pass; each with the per-utterance totals
    (float32: added in ascending l, as the device's accumulators are)."""
    _, dec_sd = weights(peaked)
    args = (enc, keys, h, c, lens, targets, tgt_len, dec_sd, CFG.sos, CFG.eos, feed_len)
    sites = {"three-launch": R.SITES_X1_THREE_LAUNCH, "fold-greedy": R.SITES_X1_FOLD_GREEDY,
             "fold-beam": R.SITES_X1_FOLD_BEAM}[path]
    m64 = R.teacher_forced(*args, sites=sites)
    m32 = R.teacher_forced(*args, sites=sites, dtype=F32)
    t64 = R.teacher_forced(*args)
    m64["total"] = m64["token_logp"].sum(axis=1)
    t64["total"] = t64["token_logp"].sum(axis=1)
    tot = np.zeros(len(lens), F32)
    for l in range(targets.shape[1]):
        tot = (tot + m32["token_logp"][:, l]).astype(F32)
    m32["total"] = tot
    return m64, m32, t64


SCORE_CASES = [("R21", "plain"), ("R21", "peaked"), ("R320", "peaked"), ("R1320", "peaked"), ("R2080", "peaked")]


@pytest.mark.parametrize("key,name", SCORE_CASES, ids=[f"{k}-{n}" for k, n in SCORE_CASES])
def test_score_budget(eng, key, name):
    """The three-launch step (sites cell_emb, cell_ch; its query is the exact-f32 MFMA of
    DecLstmEpi, not a site) and the batched projection (proj), one shape per projection class; R1320
    and R2080 take the one-accumulator form, whose w_hi 2^11 is exact."""
    frames, L = SHAPES[key]
    targets, n = shape_targets(frames, L)
    bind(eng, name)
    _, lens = encode(eng, tuple(frames))
    enc, h, c, keys = results_tm(eng)
    out = eng.score(targets, n, alignment=True, best=True, mean=True)
    r = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
    clean(eng)
    m64, m32, t64 = forced_refs("three-launch", name == "peaked", enc, keys, h, c, lens, targets.astype(np.int64),
                                n.astype(np.int64), n.astype(np.int64))
    m = scored(n, L)
    tag = f"score {key}-{name} s16x1"
    for what in ("token_logp", "mean_logp", "best_logp"):
        hold(r[what], m64[what], m32[what], t64[what], f"{tag} {what}", valid=m)
    va = np.broadcast_to(valid_tb(lens, enc.shape[0])[None], r["alignment"].shape)
    hold(r["alignment"], m64["alignment"], m32["alignment"], t64["alignment"], f"{tag} alignment", valid=va)
    hold(r["total_logp"], m64["total"], m32["total"], t64["total"], f"{tag} total_logp", valid=n > 0)


@pytest.mark.parametrize("case", ["B19", "B19-ksplit0", "B33"])
@pytest.mark.parametrize("name", ["plain", "peaked"])
def test_folded_greedy_budget(eng, name, case):
    """The folded greedy step, teacher-forced on the device's own tokens: step 0 is the three-launch
    LSTMCell, from step 1 on the gates are [ctx | h] . W_ch (site cell_ch) plus the f32 per-token
    table, and the query is an f32 fma chain (SITES_X1_FOLD_GREEDY)."""
    B, opt, val, align = GREEDY_CASES[case]
    frames = cycle_frames(B)
    bind(eng, name)
    _, lens = encode(eng, frames)
    enc, h, c, keys = results_tm(eng)
    default = eng.get_option(opt) if opt else None
    try:
        if opt:
            eng.set_option(opt, val)
        assert eng.get_option("DEC_FOLD") == 1
        g = eng.greedy(alignment=align)
        flags = eng.device_flags()
    finally:
        if opt:
            eng.set_option(opt, default)
    assert flags == 0
    clean(eng)
    tokens = g["tokens"].cpu().numpy().astype(np.int64)
    out_len, fin = g["out_len"].cpu().numpy(), g["finished"].cpu().numpy().astype(bool)
    steps = greedy_steps(out_len, fin, LMAX)
    n = (out_len + fin).astype(np.int64)
    assert n.min() >= 1 and n.max() <= steps
    assert tokens[:, :steps].min() >= 0 and tokens[:, :steps].max() < CFG.vocab
    m64, m32, t64 = forced_refs("fold-greedy", name == "peaked", enc, keys, h, c, lens, tokens[:, :steps], n,
                                np.full(B, steps))
    tag = f"greedy {case}-{name} s16x1"
    hold(g["accum"].cpu().numpy(), m64["total"], m32["total"], t64["total"], f"{tag} accum")
    al = g["alignment"].cpu().numpy()[:steps]
    va = np.broadcast_to(valid_tb(lens, enc.shape[0])[None], al.shape)
    hold(al, m64["alignment"], m32["alignment"], t64["alignment"], f"{tag} alignment", valid=va)


BEAM_X1 = [("B3k2", "peaked"), ("B3k5", "peaked"), ("B128k8", "plain"), ("B128k8", "peaked"), ("B256k4", "plain"),
           ("B256k4", "peaked"), ("B128k16", "plain"), ("B128k16", "peaked")]


@pytest.mark.parametrize("case,name", BEAM_X1, ids=[f"{c}-{n}" for c, n in BEAM_X1])
def test_beam_budget(eng, case, name):
    """One beam decode; each utterance's best hypothesis is re-scored teacher-forced by the model of
    the path that ran (test_gpu_accuracy.beam_budget's conventions: a hypothesis shorter than the
    executed steps finished, so its eos is scored too).  Below 1,024 rows the three-launch step runs;
    from there on the folded beam step, whose cell forms q = h . W_hidden as an s16 MFMA from step 1
    on (SITES_X1_FOLD_BEAM).  The folded step launches the LSTMCell GEMM at step 0 only."""
    B, k, frames, big, rows = BEAM_CASES[case]
    bind(eng, name)
    _, lens = encode(eng, frames)
    enc, h, c, keys = results_tm(eng)
    eng.profile(["dec_lstm"])
    try:
        r = {n_: v.cpu().numpy() for n_, v in eng.beam(k).items()}
        n_lstm = eng.profile_read()["dec_lstm"][0]
    finally:
        eng.profile([])
    clean(eng)
    steps = int(r["steps"][0])
    assert (n_lstm == 1) if big else (n_lstm > 1)
    length = r["length"].astype(np.int64)
    finished = length < steps
    assert length.min() >= 0 and length.max() <= steps <= LMAX
    assert np.isfinite(r["score"]).all()
    for b in range(B):
        assert ((r["tokens"][b, :length[b]] >= 0) & (r["tokens"][b, :length[b]] < CFG.vocab)).all()
    n = length + finished
    assert n.min() >= 1
    targets = np.zeros((B, int(n.max())), np.int64)
    for b in range(B):
        targets[b, :length[b]] = r["tokens"][b, :length[b]]
        if finished[b]:
            targets[b, length[b]] = CFG.eos
    sel = np.arange(B) if rows is None else np.unique(np.round(np.linspace(0, B - 1, rows)).astype(np.int64))
    assert sel[0] == 0 and sel[-1] == B - 1 and len(sel) == (B if rows is None else rows)
    m64, m32, t64 = forced_refs("fold-beam" if big else "three-launch", name == "peaked",
                                np.ascontiguousarray(enc[:, sel]), np.ascontiguousarray(keys[:, sel]), h[sel], c[sel],
                                lens[sel], targets[sel], n[sel], n[sel])
    hold(r["score"][sel], m64["total"], m32["total"], t64["total"], f"beam {case}-{name} s16x1 score")
