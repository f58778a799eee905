"""The configurations include/casr.h accepts beyond the deployed one, each axis at the values where the
plans, the weight layout or the kernels take another branch (tests/config_cases.py), in both MFMA
arithmetics, held to the float64 accuracy budget of test_gpu_accuracy.py.

The method is that file's: each stage is compared with tests/f64_ref.py fed the DEVICE's own output of
the stage before it, the bound is f64_ref.budget at M = f64_ref.M_DEFAULT on the maximum and on the
rms, and the float32 numpy oracle is the yardstick.  No tolerance is new: where tokens and scores are
compared with the oracle it is the file-wide atol = 2e-3, and tests/test_configs_host.py shows on the
CPU that none of those searches rests on a near tie (a float64 run keeps the oracle's tokens).  One
engine per configuration serves both arithmetics.  Every case asserts device_flags() == 0, that the
effective precision is the requested one, and exact zeros on the padding (keys: exactly b_attn),
through budget()'s ``valid``.  A case named for a path reads the LSTMCell GEMM's launch count (the
folded step runs it at step 0 only) and, for the greedy select, the select launches (fused into the
next step where the projection writes row partials: one launch, the last step's).

  encoder      (layers, residual) in (1, 1), (2, 0), (4, 0), (8, 1) on ragged6, persistent recurrence
               and per-step: enc, h, c, keys; one greedy decode against the oracle
  vocabulary   V in 4, 36, 83, 5003, 5120, 5121, 7168, 7169: greedy folded and DEC_FOLD = 0 (teacher-
               forced on the device's own tokens), score with every optional output (V > 5120: refused,
               nothing written), beam 1, 4, 16 where 2k <= V (else refused, nothing launched), and
               B = 128, k = 8 at V = 36 and 5003 (R = 1024: the fused select with vec == false / with
               fewer tiles than 2k)
  token ids    (sos, eos) = (82, 0), (0, 82) at V = 83 and (5003, 5002) at V = 5004: greedy, beam 4, beam
               16 against the oracle, score with eos appended; at (82, 0) casr_beam_grammar under
               the universal grammar bit for bit casr_beam (and, with the LM, casr_beam_lm), zero
               weights bit for bit casr_beam, and casr_beam_lm / casr_beam_bias against fusion_ref /
               bias_ref
  max_len      1, 2, 3: greedy with alignment, beam 8, score at L = max_len, against the oracle
  temperature  0.7 and 2.0: greedy and score bit for bit the temperature-1 engine's; beam 4 at 2.0
               against the oracle

Run with -s for one "[acc] stage case arithmetic what max_ratio rms_ratio e_ref_max e_max" line per
compared quantity (tools/acc_lines.py turns them into profiles/accuracy/accuracy_budget_configs.json).

MEASURED on one MI355X (every case is in profiles/accuracy/accuracy_budget_configs.json): per
configuration axis and stage the largest ratio of the device's error to the float32 reference's over
the cases and quantities, maximum and rms, and the case of the largest maximum.  All are below M = 8;
the largest is 6.33 (f32 MFMA, the beam-1 score at V = 83: a float32 sum of 40 log-probabilities 9.9e-6
from the float64 re-score where the oracle's sum is 1.6e-6 from it).

  axis       stage    cases  s16x3 max    rms    f32 max    rms  worst case (s16x3 / f32)
  encoder    encoder     24       1.04   0.92       1.42   1.19  l8r1-per-step / l4r0-per-step
  encoder    keys         8       0.42   0.41       1.07   1.00  l2r0-per-step / l4r0-per-step
  vocabulary greedy      32       1.61   1.31       3.93   4.20  V7169-three-launch / V36-three-launch
  vocabulary score       25       2.11   1.62       2.93   2.86  V83 / V83
  vocabulary beam        24       2.24   2.57       6.33   5.41  V5121-B3k4 / V83-B3k1
  token ids  greedy       6       2.02   1.81       1.73   1.41  V83s0e82 / V83s82e0
  token ids  score       15       2.02   1.59       3.43   2.22  V83s0e82-eos / V83s82e0-eos
  token ids  beam         6       3.72   3.30       4.85   3.90  V5004s5003e5002-B3k16 / V83s0e82-B3k16
  max_len    greedy      12       1.22   1.23       1.87   1.84  L3-fold / L1-three-launch
  max_len    beam         3       0.94   0.86       1.87   1.73  L3-B3k8 / L1-B3k8
  max_len    score       15       1.31   1.28       1.87   1.98  L3 / L1

A greedy case is named by the step the plan chose: "V7169-three-launch-by-plan" ran the default options,
under which that vocabulary keeps the three-launch step, so its rows equal "V7169-three-launch".
The two R = 1024 cases (maximum / rms; s16x3, then f32): V36-B128k8 0.75 / 0.96 and 5.27 / 4.17,
V5003-B128k8 1.12 / 1.67 and 2.12 / 2.31.  No case of this file is among the suite's 30 slowest (all
below 1.2 s).
"""
import numpy as np
import pytest
import torch

import config_cases as CC
import f64_ref as R
from test_gpu_accuracy import batch_fbank, memo, results_tm, scored, valid_tb
from oracle import casr_oracle as O
from casr.lib import CasrError
from casr.results import greedy_outputs, greedy_steps

pytestmark = pytest.mark.gpu

M = R.M_DEFAULT
ARITH = ["s16x3", "f32"]
DECODE_CLASSES = ["dec_lstm", "attention", "proj", "select"]


# ------------------------------------------------------------------ engines and stage helpers
def engine_fixture(name, cfgs, ids, peaked=True):
    @pytest.fixture(scope="module", params=cfgs, ids=ids, name=name)
    def fx(request):
        from casr.engine import Engine
        e = Engine(request.param, *CC.weights(request.param, peaked))
        yield e
        e.close()
    return fx


def use(eng, arith):
    eng.set_precision(arith)
    eng.requested = arith
    assert eng.precision() == arith


def clean(eng):
    assert eng.device_flags() == 0
    assert eng.precision() == eng.requested


def encode(eng, frames, seed=0):
    fb, fr = batch_fbank(frames, eng.device, lambda b, t: CC.fbank(b, t, seed))
    feat, flen = eng.features(fb, fr, eps=1e-6)
    eng.encode(feat, flen)
    flen = flen.cpu().numpy()
    assert flen.tolist() == [t // 3 for t in frames]
    return feat.cpu().numpy(), flen


def profiled(eng, fn):
    """fn() with the decode kernel classes timed per launch: (result, {class: launches})"""
    eng.profile(DECODE_CLASSES)
    try:
        out = fn()
        prof = eng.profile_read()
    finally:
        eng.profile([])
    return out, {c: prof.get(c, (0, 0.0))[0] for c in DECODE_CLASSES}


def every_step(n, steps, L):
    """a kernel class launched at every step of the host loop: at least the executed steps, at most max_len"""
    return steps <= n <= L


def host(d):
    return {n: (v.cpu().numpy() if v is not None else None) for n, v in d.items()}


@memo
def encoder_refs(feat, lens, layers, residual):
    enc_sd, _ = CC.weights(CC.config(layers=layers, residual=bool(residual)), True)
    feats = [feat[b, :n] for b, n in enumerate(lens)]
    enc64, h64, c64 = R.encoder(feats, lens, enc_sd, layers, bool(residual))
    enc32, (h32, c32) = O.encoder_forward(feats, np.asarray(lens), enc_sd, layers, bool(residual))
    return dict(enc=(enc64, enc32), h=(h64, h32), c=(c64, c32))


@memo
def forced_refs(cfg_key, enc, keys, h, c, lens, targets, tgt_len, feed_len):
    """test_gpu_accuracy.forced_refs with the config as a parameter: the teacher-forced pass from the
    device's encoder results in float64 and in the float32 oracle, with the per-utterance totals"""
    cfg = CFG_OF[cfg_key]
    dec_sd = CC.weights(cfg, True)[1]
    args = (enc, keys, h, c, lens, targets, tgt_len, dec_sd, cfg.sos, cfg.eos, feed_len)
    t64 = R.teacher_forced(*args)
    t32 = R.oracle32_teacher_forced(O, *args)
    t64["total"] = t64["token_logp"].sum(axis=1)
    tot = np.zeros(len(lens), np.float32)
    for l in range(targets.shape[1]):
        tot = (tot + t32["token_logp"][:, l]).astype(np.float32)
    t32["total"] = tot
    return t64, t32


CFG_OF = {}


def refs_for(cfg, *args):
    CFG_OF[repr(cfg)] = cfg
    return forced_refs(repr(cfg), *args)


def greedy_budget(eng, tag, align=True):
    """One greedy decode of the last encode, the reference fed the device's own tokens at every executed
    step (test_gpu_accuracy.test_folded_greedy_budget).  Returns (host outputs, launches, steps)."""
    cfg = eng.cfg
    enc, h, c, keys = results_tm(eng)
    lens = eng._lens.cpu().numpy()
    g, launches = profiled(eng, lambda: host(eng.greedy(alignment=align)))
    clean(eng)
    B = len(lens)
    tokens = g["tokens"].astype(np.int64)
    fin = g["finished"].astype(bool)
    steps = greedy_steps(g["out_len"], fin, cfg.max_len)
    n = (g["out_len"] + fin).astype(np.int64)
    assert n.min() >= 1 and n.max() <= steps <= cfg.max_len
    assert tokens[:, :steps].min() >= 0 and tokens[:, :steps].max() < cfg.vocab
    t64, t32 = refs_for(cfg, enc, keys, h, c, lens, tokens[:, :steps], n, np.full(B, steps))
    R.budget(g["accum"], t64["total"], t32["total"], M, tag=f"greedy {tag} accum")
    if align:
        al = g["alignment"][:steps]
        va = np.broadcast_to(valid_tb(lens, enc.shape[0])[None], al.shape)
        R.budget(al, t64["alignment"], t32["alignment"], M, valid=va, tag=f"greedy {tag} alignment")
    return g, launches, steps


def score_budget(eng, targets, n, tag):
    cfg = eng.cfg
    enc, h, c, keys = results_tm(eng)
    lens = eng._lens.cpu().numpy()
    r = host(eng.score(targets, n, alignment=True, best=True, mean=True))
    clean(eng)
    n64 = np.asarray(n, np.int64)
    t64, t32 = refs_for(cfg, enc, keys, h, c, lens, np.asarray(targets, np.int64), n64, n64)
    m = scored(n, targets.shape[1])
    for what in ("token_logp", "mean_logp", "best_logp"):
        R.budget(r[what], t64[what], t32[what], M, valid=m, tag=f"score {tag} {what}")
    va = np.broadcast_to(valid_tb(lens, enc.shape[0])[None], r["alignment"].shape)
    R.budget(r["alignment"], t64["alignment"], t32["alignment"], M, valid=va, tag=f"score {tag} alignment")
    R.budget(r["total_logp"], t64["total"], t32["total"], M, valid=n64 > 0, tag=f"score {tag} total_logp")
    return r


def beam_budget(eng, k, tag, rows=None):
    """test_gpu_accuracy.beam_budget with the config as a parameter: one beam decode of the last encode,
    each utterance's best hypothesis re-scored teacher-forced (its eos appended where it finished) and
    the device's score held to the budget against the float64 re-score; with ``rows`` that many
    utterances are re-scored, and every row is checked for a scored length >= 1, tokens of the
    vocabulary and a finite score.  Temperature 1.  Returns (host outputs, lengths, launches)."""
    cfg = eng.cfg
    assert cfg.temperature == 1.0
    enc, h, c, keys = results_tm(eng)
    lens = eng._lens.cpu().numpy()
    B = len(lens)
    r, launches = profiled(eng, lambda: host(eng.beam(k)))
    clean(eng)
    steps = int(r["steps"][0])
    length = r["length"].astype(np.int64)
    finished = length < steps
    assert length.min() >= 0 and length.max() <= steps <= cfg.max_len
    assert np.isfinite(r["score"]).all()
    n = length + finished
    assert n.min() >= 1
    L = int(n.max())
    targets = np.zeros((B, L), np.int64)
    for b in range(B):
        assert ((r["tokens"][b, :length[b]] >= 0) & (r["tokens"][b, :length[b]] < cfg.vocab)).all()
        targets[b, :length[b]] = r["tokens"][b, :length[b]]
        if finished[b]:
            targets[b, length[b]] = cfg.eos
    sel = np.arange(B) if rows is None else np.unique(np.round(np.linspace(0, B - 1, rows)).astype(np.int64))
    assert sel[0] == 0 and sel[-1] == B - 1 and len(sel) == (B if rows is None else rows)
    t64, t32 = refs_for(cfg, np.ascontiguousarray(enc[:, sel]), np.ascontiguousarray(keys[:, sel]), h[sel], c[sel],
                        lens[sel], targets[sel], n[sel], n[sel])
    R.budget(r["score"][sel], t64["total"], t32["total"], M, tag=f"beam {tag} score")
    return r, length, launches


def same_as_oracle_greedy(g, ref):
    toks, score = greedy_outputs(g["tokens"], g["out_len"], g["finished"].astype(bool), g["accum"])
    assert toks == ref["tokens"]
    assert g["out_len"].tolist() == ref["text_len"].tolist()
    assert g["finished"].astype(bool).tolist() == ref["finished"].tolist()
    np.testing.assert_allclose(score, ref["score"], rtol=0, atol=CC.ATOL)
    np.testing.assert_allclose(g["accum"], ref["accum"], rtol=0, atol=CC.ATOL)
    assert np.array_equal(g["tokens"][:, :ref["steps"]], ref["all_tokens"])


def same_as_oracle_beam(r, ref):
    B = len(ref["tokens"])
    assert int(r["steps"][0]) == ref["steps"]
    assert [r["tokens"][b, :r["length"][b]].tolist() for b in range(B)] == ref["tokens"]
    np.testing.assert_allclose(r["score"], ref["score"], rtol=0, atol=CC.ATOL)


def refused(eng, status, match, fn):
    """fn() must return ``status`` with a message, launch nothing and raise no flag"""
    eng.profile(DECODE_CLASSES)
    try:
        with pytest.raises(CasrError, match=f"{status}: .*{match}"):
            fn()
        assert eng.profile_read() == {}
    finally:
        eng.profile([])
    assert eng.device_flags() == 0


# ------------------------------------------------------------------ encoder depth and residual
enc_eng = engine_fixture("enc_eng", [CC.config(layers=n, residual=r) for n, r in CC.ENCODERS],
                         [f"l{n}r{int(r)}" for n, r in CC.ENCODERS])


@pytest.mark.parametrize("persistent", [True, False], ids=["persistent", "per-step"])
@pytest.mark.parametrize("arith", ARITH)
def test_encoder_depth_and_residual(enc_eng, arith, persistent):
    """enc_layers sizes the blob layout, the bind-time images and the layer loop; residual is an argument
    of both recurrence forms (the persistent kernel and, with set_persistent(False), the per-step one).
    enc, h, c and keys against f64_ref.encoder / oracle.encoder_forward at that depth, then one greedy
    decode against the oracle's."""
    eng, cfg = enc_eng, enc_eng.cfg
    use(eng, arith)
    eng.set_persistent(persistent)
    try:
        assert eng.recurrence_mode(len(CC.RAGGED6)) == int(persistent)
        feat, lens = encode(eng, CC.RAGGED6)
        enc, h, c, keys = results_tm(eng)
        clean(eng)
        tag = f"l{cfg.enc_layers}r{int(cfg.residual)}-{'persistent' if persistent else 'per-step'} {arith}"
        ref = encoder_refs(feat, lens, cfg.enc_layers, int(cfg.residual))
        valid = valid_tb(lens, enc.shape[0])[:, :, None]
        R.budget(enc, *ref["enc"], M, valid=valid, tag=f"encoder {tag} enc")
        R.budget(h, *ref["h"], M, tag=f"encoder {tag} h")
        R.budget(c, *ref["c"], M, tag=f"encoder {tag} c")
        dec_sd = CC.weights(cfg, True)[1]
        R.budget(keys, R.compute_keys(enc, dec_sd), O.compute_keys(enc, dec_sd), M, valid=valid,
                 pad=dec_sd["attn_mechanism.b_attn"][None, None, :], tag=f"keys {tag} keys")
        g = host(eng.greedy())
        clean(eng)
        same_as_oracle_greedy(g, CC.oracle_search(f"enc-l{cfg.enc_layers}r{int(cfg.residual)}-greedy"))
    finally:
        eng.set_persistent(True)


# ------------------------------------------------------------------ vocabulary size
vocab_eng = engine_fixture("vocab_eng", [CC.config(V=V) for V in CC.VOCABS], [f"V{V}" for V in CC.VOCABS])
big_eng = engine_fixture("big_eng", [CC.config(V=V) for V in CC.BIG_VOCABS], [f"V{V}" for V in CC.BIG_VOCABS])


@pytest.mark.parametrize("fold", [1, 0], ids=["fold", "three-launch"])
@pytest.mark.parametrize("arith", ARITH)
def test_vocab_greedy(vocab_eng, arith, fold):
    """Greedy at every vocabulary, the folded step and DEC_FOLD = 0.  V = 4: one projection tile with 12
    padded columns; V < 80: less than one wave column; V % 4 != 0: the logits rows are stored and read
    element by element; V = 5120 | 5121: the three-launch projection's last vocabulary with row partials
    (the select fused into the next step) | the first with a full-row select every step; V = 7168 | 7169:
    the last vocabulary that folds | the first where greedy keeps the three-launch step."""
    eng, V = vocab_eng, vocab_eng.cfg.vocab
    use(eng, arith)
    encode(eng, CC.SMALL3)
    # the case is named by what the plan chooses: at V = 7169 the default options keep the three-launch step
    folded = bool(fold) and CC.greedy_folds(V)
    path = "fold" if folded else "three-launch" if not fold else "three-launch-by-plan"
    eng.set_option("DEC_FOLD", fold)
    try:
        g, launches, steps = greedy_budget(eng, f"V{V}-{path} {arith}")
    finally:
        eng.set_option("DEC_FOLD", 1)
    partials = folded or CC.projection_partials(V)
    L = eng.cfg.max_len
    assert L > 1  # (so that one launch and one per step differ)
    assert launches["dec_lstm"] == 1 if folded else every_step(launches["dec_lstm"], steps, L), launches
    assert launches["select"] == 1 if partials else every_step(launches["select"], steps, L), launches


def random_targets(V, B, L, seed):
    """targets of the vocabulary (its first and last id among them), lengths L, about L / 2, ..., 1"""
    t = np.random.RandomState(seed).randint(0, V, size=(B, L)).astype(np.int32)
    t[0, 0], t[1, 0] = V - 1, 0
    n = np.maximum(1, L >> np.arange(B)).astype(np.int32)
    return t, n


@pytest.mark.parametrize("arith", ARITH)
def test_vocab_score(vocab_eng, arith):
    """casr_score with every optional output; where the projection's column blocks exceed the 64 row
    partials (V > 5120) CASR_ERR_UNSUPPORTED, nothing written, nothing launched, no flag."""
    eng, V = vocab_eng, vocab_eng.cfg.vocab
    use(eng, arith)
    encode(eng, CC.SMALL3)
    B, L = len(CC.SMALL3), 12
    targets, n = random_targets(V, B, L, 40 + V)
    if CC.projection_partials(V):
        score_budget(eng, targets, n, f"V{V} {arith}")
        return
    from casr.engine import _ptr, _stream
    dev = eng.device
    t = torch.from_numpy(targets).to(dev)
    nn = torch.from_numpy(n).to(dev)
    outs = [torch.full((B, L), 7.25, device=dev), torch.full((B,), 7.25, device=dev),
            torch.full((B, L), 77, dtype=torch.int32, device=dev), torch.full((B, L), 7.25, device=dev),
            torch.full((B, L), 7.25, device=dev), torch.full((L, eng._Tp, B), 7.25, device=dev)]
    eng.profile(DECODE_CLASSES)
    try:
        rc = eng.lib.casr_score(eng.handle, _ptr(t), _ptr(nn), L, *[_ptr(o) for o in outs], _stream())
        assert eng.profile_read() == {}
    finally:
        eng.profile([])
    assert rc == 4  # CASR_ERR_UNSUPPORTED
    msg = eng.lib.casr_last_error(eng.handle).decode()
    assert "casr_score" in msg and "row partials" in msg
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == (77 if o.dtype == torch.int32 else 7.25)).all())
    assert eng.device_flags() == 0


@pytest.mark.parametrize("k", CC.BEAM_WIDTHS)
@pytest.mark.parametrize("arith", ARITH)
def test_vocab_beam(vocab_eng, arith, k):
    """Beam 1, 4 and 16 on the three-launch step (R < 1024) at every vocabulary: the select from the tile
    maxima where V % 4 == 0 and V <= 5120 (with fewer than 2k tiles at V = 4 and 36), from the whole row
    otherwise.  2k > V is CASR_ERR_ARG with nothing launched: the reference's topk raises there."""
    eng, V = vocab_eng, vocab_eng.cfg.vocab
    use(eng, arith)
    encode(eng, CC.SMALL3)
    if 2 * k > V:
        refused(eng, "CASR_ERR_ARG", f"beam width {k} .*{2 * k} candidates.* {V} tokens", lambda: eng.beam(k))
        return
    r, length, launches = beam_budget(eng, k, f"V{V}-B3k{k} {arith}")
    steps, L = int(r["steps"][0]), eng.cfg.max_len
    assert every_step(launches["dec_lstm"], steps, L) and every_step(launches["select"], steps, L), launches
    assert launches["dec_lstm"] > 1


@pytest.mark.parametrize("arith", ARITH)
def test_vocab_folded_beam(big_eng, arith):
    """B = 128, k = 8 (R = 1024) at V = 36 and V = 5003: under s16x3 the folded beam step with the select
    inside the attention kernel, with fewer 16-column tiles than 2k (V = 36: the threshold rounds run
    past the tiles that exist) and with vec == false (V = 5003: no tile-maxima path, the rows read
    element by element); under f32 the three-launch step.  16 utterances are re-scored, every row is
    held to beam_budget's sanity checks."""
    eng, V = big_eng, big_eng.cfg.vocab
    use(eng, arith)
    encode(eng, (48,) * 128)
    r, length, launches = beam_budget(eng, 8, f"V{V}-B128k8 {arith}", rows=16)
    steps, L = int(r["steps"][0]), eng.cfg.max_len
    if arith == "s16x3":  # the folded step, every select but the last inside the attention
        assert launches["dec_lstm"] == 1 and launches["select"] == 1, launches
    else:
        assert every_step(launches["dec_lstm"], steps, L) and every_step(launches["select"], steps, L), launches
        assert launches["dec_lstm"] > 1


def test_beam_width_past_vocab_is_refused_by_every_entry():
    """2k > V at V = 4, k = 4 (the pair that must never launch) and at V = 31, k = 16: casr_beam,
    casr_beam_lm, casr_beam_bias and casr_beam_grammar return CASR_ERR_ARG with a message that names k
    and the vocabulary, launch nothing, raise no flag, and leave the last beam readable."""
    import ngram_ref as NR
    from casr.bias import PhraseBias
    from casr.engine import Engine
    from casr.grammar import Grammar
    from casr.ngram import NgramLM
    for V, ok, bad in ((4, 2, 4), (31, 15, 16)):
        cfg = CC.config(V=V)
        e = Engine(cfg, *CC.weights(cfg, True))
        lm = NgramLM.from_ids(*NR.arrays_of(NR.random_model(2, V, 7, n_high=4)), {}, V)
        pb = PhraseBias([[0, 3]], {}, V, [1.0])
        uni = Grammar.universal(V, cfg.eos)
        try:
            encode(e, CC.SMALL3)
            want = host(e.beam(ok))
            recs = [x.cpu().numpy() for x in e.beam_records()]
            assert e.device_flags() == 0
            match = f"beam width {bad} .*{2 * bad} candidates.* {V} tokens"
            for call in (lambda: e.beam(bad), lambda: e.beam_lm(lm, bad, 0.5, 0.5), lambda: e.beam_bias(pb, bad),
                         lambda: e.beam_bias(pb, bad, 1.0, lm, 0.5, 0.5), lambda: e.beam_grammar(uni, bad),
                         lambda: e.beam_grammar(uni, bad, lm, 0.5, 0.5)):
                refused(e, "CASR_ERR_ARG", match, call)
            again = [x.cpu().numpy() for x in e.beam_records()]  # the refused calls spent nothing
            assert all(np.array_equal(a, b) for a, b in zip(again, recs))
            after = host(e.beam(ok))
            assert all(np.array_equal(v, after[n]) for n, v in want.items())
            assert e.device_flags() == 0
        finally:
            e.close()
            lm.close()
            pb.close()
            uni.close()


# ------------------------------------------------------------------ token ids
ids_eng = engine_fixture("ids_eng", [CC.config(V=V, sos=s, eos=e) for V, s, e in CC.TOKEN_IDS],
                         [f"V{V}s{s}e{e}" for V, s, e in CC.TOKEN_IDS])


def ids_tag(cfg):
    return f"V{cfg.vocab}s{cfg.sos}e{cfg.eos}"


@pytest.mark.parametrize("arith", ARITH)
def test_token_ids_greedy_and_score(ids_eng, arith):
    """sos reaches the step-0 embedding lookup, eos every comparison of greedy and score and the peaked
    bias; eos = V - 1 sits in the last tile beside the padding, eos = 0 in the first column.  Greedy
    against the oracle and the budget; then the device's own hypotheses with eos appended through
    casr_score: its totals are the budget's, and within 2e-3 of greedy's accum where greedy finished."""
    eng, cfg = ids_eng, ids_eng.cfg
    use(eng, arith)
    encode(eng, CC.SMALL3)
    g, launches, steps = greedy_budget(eng, f"{ids_tag(cfg)} {arith}")
    assert launches["dec_lstm"] == 1
    same_as_oracle_greedy(g, CC.oracle_search(f"ids-{ids_tag(cfg)}-greedy"))
    B = len(CC.SMALL3)
    n = np.minimum(g["out_len"] + 1, cfg.max_len).astype(np.int32)
    targets = np.full((B, int(n.max())), cfg.eos, np.int32)
    for b in range(B):
        targets[b, :g["out_len"][b]] = g["tokens"][b, :g["out_len"][b]]
    r = score_budget(eng, targets, n, f"{ids_tag(cfg)}-eos {arith}")
    fin = g["finished"].astype(bool)
    np.testing.assert_allclose(r["total_logp"][fin], g["accum"][fin], rtol=0, atol=CC.ATOL)


@pytest.mark.parametrize("k", [4, 16])
@pytest.mark.parametrize("arith", ARITH)
def test_token_ids_beam(ids_eng, arith, k):
    """eos decides the records, the early stop, the active set and the finalize of the beam search:
    tokens, lengths, step counts and scores against the oracle's, the best hypotheses to the budget."""
    eng, cfg = ids_eng, ids_eng.cfg
    use(eng, arith)
    encode(eng, CC.SMALL3)
    r, length, _ = beam_budget(eng, k, f"{ids_tag(cfg)}-B3k{k} {arith}")
    same_as_oracle_beam(r, CC.oracle_search(f"ids-{ids_tag(cfg)}-beam{k}"))


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def derived():
    """the engine, LM, phrase bias and universal grammar of config_cases.derived_case (V = 83, sos = 82,
    eos = 0)"""
    import ngram_ref as NR
    from casr.bias import PhraseBias
    from casr.engine import Engine
    from casr.grammar import Grammar
    from casr.ngram import NgramLM
    case = CC.derived_case()
    cfg, V = case["cfg"], case["cfg"].vocab
    from casr.lib import pack_weights
    packed = dict(fused=pack_weights(cfg, case["enc_sd"], case["dec_sd"]),
                  plain=pack_weights(cfg, *CC.derived_plain_weights()))
    e = Engine(cfg, packed=packed["fused"])
    lm = NgramLM.from_ids(*NR.arrays_of(case["grams"]), {}, V)
    pb = PhraseBias(case["phrases"], {}, V, [b / 256 for b in case["boosts"]])
    uni = Grammar.universal(V, cfg.eos)
    yield dict(e=e, lm=lm, pb=pb, uni=uni, case=case, packed=packed)
    e.close()
    lm.close()
    pb.close()
    uni.close()


def records_of(e):
    return [x.cpu().numpy() for x in e.beam_records()]


@pytest.mark.parametrize("k", CC.DERIVED_IDENTITY_K)
@pytest.mark.parametrize("arith", ARITH)
def test_derived_searches_identities_at_eos_0(derived, arith, k):
    """The identities test_gpu_fusion.py, test_gpu_bias.py and test_gpu_grammar.py assert at the deployed
    ids, at (sos, eos) = (82, 0) and V = 83 (vec == false), bit for bit in tokens, lengths, steps, scores
    and records.  At DERIVED_PLAIN_EOS_BIAS, where the plain search ends early after several steps:
    casr_beam_grammar under the grammar that allows everything, without an LM, is casr_beam (its eos check
    and records keyed on id 0), and so are casr_beam_lm and casr_beam_bias at zero weights.  At
    DERIVED_EOS_BIAS, with the LM: casr_beam_grammar and casr_beam_bias at zero bias weight are casr_beam_lm."""
    e, lm, pb, uni = derived["e"], derived["lm"], derived["pb"], derived["uni"]
    L = e.cfg.max_len

    def same(z, zrecs, want, wrecs, names):
        for n in ("tokens", "length", "steps"):
            assert np.array_equal(z[n], want[n]), n
        for n in names:
            assert np.array_equal(bits(z[n]), bits(want[n])), n
        assert np.array_equal(zrecs[0], wrecs[0]) and np.array_equal(bits(zrecs[1]), bits(wrecs[1]))
        assert np.array_equal(zrecs[2], wrecs[2])

    try:
        e.bind(derived["packed"]["plain"])
        use(e, arith)
        encode(e, CC.SMALL3)
        beam, recs = host(e.beam(k)), records_of(e)
        # (at the last step the horizon rule offers eos only; test_configs_host.py: the oracle's search too)
        assert 1 < int(beam["steps"][0]) < L and recs[2].any()
        z = host(e.beam_grammar(uni, k))  # no LM, length weight 0: casr_beam's
        same(z, records_of(e), beam, recs, ("score",))
        assert z["lm"] is None and z["complete"].all()
        same(host(e.beam_lm(lm, k, 0.0, 0.0)), records_of(e), beam, recs, ("score",))
        same(host(e.beam_bias(pb, k, 0.0)), records_of(e), beam, recs, ("score",))
        clean(e)
    finally:
        e.bind(derived["packed"]["fused"])
    use(e, arith)
    encode(e, CC.SMALL3)
    w = CC.DERIVED_WEIGHTS
    fused, frecs, frq = host(e.beam_lm(lm, k, *w)), records_of(e), e.beam_record_lm().cpu().numpy()
    assert int(fused["steps"][0]) < L and frecs[2].any()
    same(host(e.beam_bias(pb, k, 0.0, lm, *w)), records_of(e), fused, frecs, ("score", "lm"))
    z = host(e.beam_grammar(uni, k, lm, *w))  # with the LM: casr_beam_lm's
    same(z, records_of(e), fused, frecs, ("score", "lm"))
    assert np.array_equal(bits(e.beam_record_lm().cpu().numpy()), bits(frq))
    assert z["complete"].all()
    clean(e)


@pytest.mark.parametrize("arith", ARITH)
def test_derived_searches_equal_the_numpy_restatements_at_eos_0(derived, arith):
    """casr_beam_lm against fusion_ref.fused_beam and casr_beam_bias (with and without the LM) against
    bias_ref.biased_beam at (sos, eos) = (82, 0), k = 2, where tests/test_configs_host.py has asserted
    that the restatements' smallest gap between vals adjacent in rank is >= 1e-2: tokens, records and
    step counts equal, am and lm within 2e-3, the bias bit for bit."""
    from casr.results import records_by_utterance
    e, lm, pb, case = derived["e"], derived["lm"], derived["pb"], derived["case"]
    k, (lw, nw), B = CC.DERIVED_K, CC.DERIVED_WEIGHTS, len(CC.SMALL3)
    use(e, arith)
    encode(e, CC.SMALL3)
    want = case["fused"]
    r = host(e.beam_lm(lm, k, lw, nw))
    recs = records_by_utterance(*records_of(e))
    clean(e)
    assert int(r["steps"][0]) == want["steps"]
    for b in range(B):
        assert r["tokens"][b, :r["length"][b]].tolist() == want["tokens"][b], b
        assert abs(r["score"][b] - want["score"][b]) <= CC.ATOL and abs(r["lm"][b] - want["lm"][b]) <= CC.ATOL, b
        assert [t for t, _ in recs.get(b, [])] == [t for t, _, _ in want["records"][b]], b
    for with_lm in (True, False):
        want = case["biased"][with_lm]
        r = host(e.beam_bias(pb, k, 1.0, lm if with_lm else None, lw if with_lm else 0.0, nw))
        rt, rs, rv = records_of(e)
        rz = e.beam_record_bias().cpu().numpy()
        clean(e)
        assert int(r["steps"][0]) == want["steps"]
        for b in range(B):
            assert r["tokens"][b, :r["length"][b]].tolist() == want["tokens"][b], b
            assert abs(r["score"][b] - want["score"][b]) <= CC.ATOL, b
            assert bits(r["bias"][b]) == bits(want["bias"][b]), b
            if with_lm:
                assert abs(r["lm"][b] - want["lm"][b]) <= CC.ATOL, b
            idx = [(l, c) for l in range(e.cfg.max_len) for c in range(k) if rv[b, l, c]]
            assert [rt[b, l, c, :l].tolist() for l, c in idx] == [t for t, _, _, _ in want["records"][b]], b
            for (l, c), (_, a, _, zb) in zip(idx, want["records"][b]):
                assert abs(rs[b, l, c] - a) <= CC.ATOL and bits(rz[b, l, c]) == bits(zb), (b, l, c)


# ------------------------------------------------------------------ max_len 1, 2, 3
len_eng = engine_fixture("len_eng", [CC.config(L=L) for L in CC.MAX_LENS], [f"L{L}" for L in CC.MAX_LENS])


@pytest.mark.parametrize("fold", [1, 0], ids=["fold", "three-launch"])
@pytest.mark.parametrize("arith", ARITH)
def test_max_len_greedy(len_eng, arith, fold):
    """The folded greedy step has an LSTMCell at step 0 only and a distinct last step (the vocabulary
    tiles alone, with its own k split); at max_len = 1 the first step is the last.  Tokens, lengths,
    finished flags and scores against the oracle's; accum and every step's alignment to the budget."""
    eng, L = len_eng, len_eng.cfg.max_len
    use(eng, arith)
    encode(eng, CC.SMALL3, CC.MAX_LEN_SEED)
    eng.set_option("DEC_FOLD", fold)
    try:
        g, launches, steps = greedy_budget(eng, f"L{L}-{'fold' if fold else 'three-launch'} {arith}")
    finally:
        eng.set_option("DEC_FOLD", 1)
    assert steps == L and launches["dec_lstm"] == (1 if fold else L) and launches["select"] == 1, launches
    ref = CC.oracle_search(f"len-L{L}-greedy")
    same_as_oracle_greedy(g, ref)
    assert ref["finished"].any() and not ref["finished"].all()  # both ends, at max_len = 1 too


@pytest.mark.parametrize("arith", ARITH)
def test_max_len_beam_and_score(len_eng, arith):
    """Beam 8: the finished record of the 48-frame utterance (the empty hypothesis) and the unfinished
    fallback of the others, at max_len = 1 both in the one step.  Then casr_score at L = max_len."""
    eng, L = len_eng, len_eng.cfg.max_len
    use(eng, arith)
    encode(eng, CC.SMALL3, CC.MAX_LEN_SEED)
    r, length, launches = beam_budget(eng, 8, f"L{L}-B3k8 {arith}")
    ref = CC.oracle_search(f"len-L{L}-beam8")
    same_as_oracle_beam(r, ref)
    assert int(r["steps"][0]) == L and launches["dec_lstm"] == L
    assert len(ref["tokens"][0]) == L and ref["tokens"][2] == []  # the unfinished fallback, a finished record
    targets, n = random_targets(eng.cfg.vocab, len(CC.SMALL3), L, 90 + L)
    n[:] = L
    score_budget(eng, targets, n, f"L{L} {arith}")


# ------------------------------------------------------------------ temperature
@pytest.fixture(scope="module")
def temp_engs():
    from casr.engine import Engine
    engs = {T: Engine(CC.config(temperature=T), *CC.weights(CC.config(temperature=T), True)) for T in [1.0] + CC.TEMPERATURES}
    yield engs
    for e in engs.values():
        e.close()


@pytest.mark.parametrize("T", CC.TEMPERATURES)
@pytest.mark.parametrize("arith", ARITH)
def test_temperature_leaves_greedy_and_score_alone(temp_engs, arith, T):
    """include/casr.h: the temperature is the beam search's.  casr_greedy (folded and three-launch, with
    alignment) and casr_score (every optional output) give the temperature-1 engine's bits."""
    base, eng = temp_engs[1.0], temp_engs[T]
    targets, n = random_targets(base.cfg.vocab, len(CC.SMALL3), 12, 17)
    outs = []
    for e in (base, eng):
        use(e, arith)
        encode(e, CC.SMALL3)
        got = {}
        for fold in (1, 0):
            e.set_option("DEC_FOLD", fold)
            try:
                got.update({f"greedy{fold}.{n_}": v for n_, v in e.greedy(alignment=True).items()})
            finally:
                e.set_option("DEC_FOLD", 1)
        got.update({f"score.{n_}": v for n_, v in e.score(targets, n, alignment=True, best=True, mean=True).items()})
        clean(e)
        outs.append({n_: v.cpu() for n_, v in got.items()})
    assert outs[0].keys() == outs[1].keys()
    assert {"greedy1.alignment", "greedy0.accum", "score.mean_logp", "score.alignment"} <= outs[0].keys()
    for n_ in outs[0]:
        assert torch.equal(outs[0][n_], outs[1][n_]), n_


@pytest.mark.parametrize("arith", ARITH)
def test_temperature_2_beam(temp_engs, arith):
    """Beam 4 at temperature 2.0 (model.py:834 divides the logits first: the select reads the whole
    rows) against O.beam_decode at that temperature; 0.7 is test_gpu_select_paths.py's."""
    eng = temp_engs[2.0]
    use(eng, arith)
    encode(eng, CC.SMALL3)
    r = host(eng.beam(4))
    clean(eng)
    same_as_oracle_beam(r, CC.oracle_search("temp-T2.0-beam4"))
    base = temp_engs[1.0]
    use(base, arith)
    encode(base, CC.SMALL3)
    assert not np.array_equal(host(base.beam(4))["score"], r["score"])  # (the temperature does reach the beam)
