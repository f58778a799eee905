"""The float64 accuracy budget (tests/f64_ref.py) proved on the CPU before test_gpu_accuracy.py
points it at the device:

  1. the float64 reference is right: it agrees with the vectors captured from the reference
     implementation (tests/golden/golden.npz) and with the float32 oracle, within bounds 7 to 10
     times the deviations a float32 evaluation shows (encoder and keys 1e-5, alignments 1e-6, peaked
     token log-probabilities 1e-4);
  2. the budget admits a valid float32 implementation: the torch-CPU port passes budget(..., M) on
     every stage;
  3. the budget rejects seeded defects: six mutants of the oracle (a lost lo term on one 64-wide k
     block of one layer, one layer's input GEMM at f16, hi-only layer inputs, hi-only W_hh, an f16
     projection weight, an f16 projection input) each fail budget at the same M.  The mildest is 45
     times the float32 reference's own error, so an M that let it through would be too large.

Run with -s for the measured figures ("[acc]" lines)."""
import functools

import numpy as np
import pytest
import torch

import f64_ref as R
from golden_util import load_golden, fbank_for, golden_frames
from oracle import casr_oracle as O
from oracle import torch_port as TP
from casr.config import CasrConfig
from casr.weights import synthetic_state_dicts

G, META = load_golden()
CFG = CasrConfig()
M = R.M_DEFAULT
RAGGED = (101, 75, 48, 9, 6, 200)   # 396 encoder rows, lengths down to Tp = 2
LONG = (801,)                       # Tp = 267 dependent steps
STEPS = 20                          # teacher-forced steps of the decoder checks


@functools.lru_cache(maxsize=None)
def weights(peaked):
    return synthetic_state_dicts(CFG, peaked=peaked)


@functools.lru_cache(maxsize=None)
def port(peaked):
    return TP.TorchPort(*weights(peaked))


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def encoded(frames):
    """Features (float32 oracle), then the encoder in float64 and in the float32 oracle on those
    same features, once per batch (the encoder weights are the same in both weight sets)."""
    enc_sd, _ = weights(False)
    feats = [O.features_from_fbank(fbank_for(b, t)) for b, t in enumerate(frames)]
    lens = np.array([f.shape[0] for f in feats])
    enc32, (h32, c32) = O.encoder_forward(feats, lens, enc_sd)
    enc64, h64, c64 = R.encoder(feats, lens, enc_sd)
    valid = (np.arange(enc32.shape[0])[:, None] < lens[None, :])[:, :, None]
    frozen(enc32, h32, c32, enc64, h64, c64, *feats)
    return dict(feats=feats, lens=lens, enc32=enc32, h32=h32, c32=c32, enc64=enc64, h64=h64, c64=c64, valid=valid)


def targets_for(B, L=STEPS):
    t = np.random.RandomState(77).randint(3, CFG.vocab, size=(B, L))
    n = np.full(B, L)
    n[-1] = L // 2
    return t, n


@functools.lru_cache(maxsize=None)
def decoded(frames, peaked):
    """Keys and a teacher-forced pass of STEPS steps from the float32 oracle's encoder output, in
    float64 and in the float32 oracle."""
    e = encoded(frames)
    _, dec_sd = weights(peaked)
    keys32 = O.compute_keys(e["enc32"], dec_sd)
    keys64 = R.compute_keys(e["enc32"], dec_sd)
    t, n = targets_for(len(frames))
    args = (e["enc32"], keys32, e["h32"], e["c32"], e["lens"], t, n, dec_sd)
    tf64 = R.teacher_forced(*args)
    tf32 = R.oracle32_teacher_forced(O, *args)
    scored = np.arange(STEPS)[None, :] < n[:, None]
    return dict(keys32=keys32, keys64=keys64, tf32=tf32, tf64=tf64, args=args, scored=scored)


def maxdev(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


# ------------------------------------------------------------------ 1. the float64 reference is right
def test_f64_features_match_reference_golden():
    """|x| < 6 after CMVN; a float32 evaluation rounds the deltas, the mean, the std and the
    quotient, each within an ulp of 4 (4.8e-7): 5e-6 is the bound test_oracle_golden.py holds the
    float32 oracle to against the same vector."""
    d = maxdev(R.features(fbank_for(0, 101)), G["feat_cmvn_T101"])
    print(f"[acc] f64-vs-golden feat_cmvn_T101 {d:.3e}")
    assert d <= 5e-6
    for b, t in enumerate(RAGGED):
        fb = fbank_for(b, t)
        if t // 3 > 2:  # two rows: every column is +-1/sqrt(2) over an ill-conditioned std
            assert maxdev(R.features(fb), O.features_from_fbank(fb)) <= 5e-6
        assert maxdev(R.features(fb, eps=-1.0), O.stack_frames(O.add_delta_deltas(fb))) <= 2e-6


def test_f64_encoder_matches_reference_golden():
    e = encoded(tuple(golden_frames(META)))
    for name in ("plain", "peaked"):
        d = dict(h=maxdev(e["h64"], G[f"{name}_enc_h"]), c=maxdev(e["c64"], G[f"{name}_enc_c"]),
                 slice=maxdev(e["enc64"][::7, :, ::64], G[f"{name}_enc_slice"]))
        print(f"[acc] f64-vs-golden encoder {name} " + " ".join(f"{k}={v:.3e}" for k, v in d.items()))
        assert max(d.values()) <= 1e-5, d


@pytest.mark.parametrize("name", ["plain", "peaked"])
def test_f64_first_alignment_matches_reference_golden(name):
    e = encoded(tuple(golden_frames(META)))
    _, dec_sd = weights(name == "peaked")
    B = len(e["lens"])
    keys = R.compute_keys(e["enc64"], dec_sd)
    _, _, _, _, alpha = R.decoder_step(e["enc64"], e["lens"], keys, np.full(B, CFG.sos), e["h64"], e["c64"],
                                       np.zeros((B, CFG.enc_size)), dec_sd)
    d = maxdev(alpha, G[f"{name}_greedy_align_step0"])
    print(f"[acc] f64-vs-golden align_step0 {name} {d:.3e}")
    assert d <= 1e-6
    assert not alpha[~np.broadcast_to(e["valid"][:, :, 0], alpha.shape)].any()


@pytest.mark.parametrize("frames", [RAGGED, LONG], ids=["ragged", "Tp267"])
def test_f64_encoder_and_keys_match_f32_oracle(frames):
    e = encoded(frames)
    k = decoded(frames, False)
    d = dict(enc=maxdev(e["enc64"], e["enc32"]), h=maxdev(e["h64"], e["h32"]), c=maxdev(e["c64"], e["c32"]),
             keys=maxdev(k["keys64"], k["keys32"]))
    print(f"[acc] f64-vs-oracle Tp={e['enc32'].shape[0]} " + " ".join(f"{n}={v:.3e}" for n, v in d.items()))
    assert max(d.values()) <= 1e-5, d
    assert not e["enc64"][~np.broadcast_to(e["valid"], e["enc64"].shape)].any()


@pytest.mark.parametrize("name", ["plain", "peaked"])
def test_f64_teacher_forced_matches_f32_oracle(name):
    k = decoded(RAGGED, name == "peaked")
    d = {n: maxdev(k["tf64"][n], k["tf32"][n]) for n in ("token_logp", "mean_logp", "best_logp", "alignment")}
    print(f"[acc] f64-vs-oracle teacher-forced {name} " + " ".join(f"{n}={v:.3e}" for n, v in d.items()))
    # plain: measured 1.1e-6, and a log-probability near -8.5 has an ulp of 9.5e-7
    tol = 1e-4 if name == "peaked" else 1e-5
    assert max(d["token_logp"], d["mean_logp"], d["best_logp"]) <= tol, d
    assert d["alignment"] <= 1e-6, d
    for n in ("token_logp", "mean_logp", "best_logp"):
        assert not k["tf64"][n][~k["scored"]].any()


# ------------------------------------------------------------------ 2. a valid float32 implementation passes
@pytest.mark.parametrize("T", [6, 9, 101, 1100])
@pytest.mark.parametrize("family", ["normal", "logmel"])
def test_budget_admits_f32_features(T, family):
    """ref32 for the features is the torch port (the oracle takes its CMVN statistics in float64,
    so it is not a float32 evaluation); as a candidate the oracle must fit the budget."""
    fb = fbank_for(3, T) if family == "normal" else 4 * fbank_for(3, T) - 8
    truth = R.features(fb)
    ref = TP.features_from_fbank(fb).numpy()
    R.budget(O.features_from_fbank(fb), truth, ref, M, tag=f"host-features-{family} T{T} oracle")
    fig = R.figures(ref, truth, ref)
    assert fig["max_ratio"] == 1.0 and 0 < fig["e_ref_max"] < 2e-4


@pytest.mark.parametrize("frames", [RAGGED, LONG], ids=["ragged", "Tp267"])
def test_budget_admits_torch_port_encoder_and_keys(frames):
    e = encoded(frames)
    p = port(False)
    enc, h, c, lens = (x.numpy() for x in p.encode([f.copy() for f in e["feats"]]))
    assert lens.tolist() == e["lens"].tolist()
    tag = f"host-encoder Tp{enc.shape[0]} port"
    R.budget(enc, e["enc64"], e["enc32"], M, valid=e["valid"], tag=tag + " enc")
    R.budget(h, e["h64"], e["h32"], M, tag=tag + " h")
    R.budget(c, e["c64"], e["c32"], M, tag=tag + " c")
    k = decoded(frames, False)
    keys = (torch.tensor(e["enc32"]) @ p.w_enc + p.b_attn).numpy()
    R.budget(keys, k["keys64"], k["keys32"], M, tag=f"host-keys Tp{enc.shape[0]} port")


@pytest.mark.parametrize("name", ["plain", "peaked"])
def test_budget_admits_torch_port_decoder(name):
    k = decoded(RAGGED, name == "peaked")
    p = port(name == "peaked")
    enc, keys, h, c, lens, t, n, dec_sd = k["args"]
    mask = p.mask(torch.as_tensor(lens), enc.shape[0])
    enc_t, keys_t = torch.tensor(enc), torch.tensor(keys)  # copies: the shared references stay read-only

    @torch.no_grad()
    def step(enc_, lens_, keys_, tok, h_, c_, ctx, sd):
        out = p.step(enc_t, mask, keys_t, torch.as_tensor(tok), torch.tensor(h_), torch.tensor(c_), torch.tensor(ctx))
        logit, h2, c2, ctx2 = (x.numpy() for x in out)
        return logit, h2, c2, ctx2, 0.0  # the port's step returns no attention weights

    lsm = lambda x: (torch.from_numpy(x) - torch.logsumexp(torch.from_numpy(x), 1, keepdim=True)).numpy()
    got = R._teacher_forced(step, lsm, np.float32, enc, keys, h, c, lens, t, n, dec_sd, CFG.sos, CFG.eos, None)
    for what in ("token_logp", "mean_logp", "best_logp"):
        R.budget(got[what], k["tf64"][what], k["tf32"][what], M, valid=k["scored"],
                 tag=f"host-decoder {name} port {what}")


# ------------------------------------------------------------------ 3. seeded defects fail
def f16(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def _layer_mutant(change):
    """O._bilstm_layer with change(layer index, x, weights) -> (x, weights) applied to what the layer
    contracts; the residual outside still adds the unchanged input."""
    plain = O._bilstm_layer
    seen = []

    def layer(x, lens, *w):
        i = len(seen)
        seen.append(i)
        x2, w2 = change(i, x, list(w))
        return plain(x2, lens, *w2)
    return layer


def lo_lost_on_one_k_block(i, x, w):
    if i == 3:
        x = x.copy()
        x[..., :64] = f16(x[..., :64])
    return x, w


def one_layer_input_gemm_f16(i, x, w):
    if i == 3:
        x, w[0], w[4] = f16(x), f16(w[0]), f16(w[4])   # x, W_ih, W_ih reverse
    return x, w


def inputs_hi_only(i, x, w):
    return f16(x), w


def whh_hi_only(i, x, w):
    w[1], w[5] = f16(w[1]), f16(w[5])
    return x, w


@pytest.mark.parametrize("change", [lo_lost_on_one_k_block, one_layer_input_gemm_f16, inputs_hi_only, whh_hi_only],
                         ids=lambda f: f.__name__)
def test_budget_rejects_encoder_mutants(monkeypatch, change):
    e = encoded(RAGGED)
    monkeypatch.setattr(O, "_bilstm_layer", _layer_mutant(change))
    enc, (h, c) = O.encoder_forward(e["feats"], e["lens"], weights(False)[0])
    monkeypatch.undo()
    fig = R.figures(enc, e["enc64"], e["enc32"], e["valid"])
    print(f"[acc] mutant {change.__name__} enc max_ratio={fig['max_ratio']:.1f} rms_ratio={fig['rms_ratio']:.1f} "
          f"e_max={fig['e_max']:.3e}")
    assert fig["max_ratio"] > M and fig["rms_ratio"] > M
    with pytest.raises(AssertionError):
        R.budget(enc, e["enc64"], e["enc32"], M, valid=e["valid"])
    # the sanity of the instrument: the unmutated oracle is its own reference
    enc0, _ = O.encoder_forward(e["feats"], e["lens"], weights(False)[0])
    assert np.array_equal(enc0, e["enc32"])


def _proj_input_f16_step(plain):
    def step(enc, mask, keys, token, h, c, ctx_prev, dec_sd):
        logit, h2, c2, ctx, alpha = plain(enc, mask, keys, token, h, c, ctx_prev, dec_sd)
        x = f16(np.concatenate([h2, ctx], axis=1))
        logit = (x @ dec_sd["proj_linear.weight"].T + dec_sd["proj_linear.bias"]).astype(np.float32)
        return logit, h2, c2, ctx, alpha
    return step


@pytest.mark.parametrize("name", ["plain", "peaked"])
@pytest.mark.parametrize("mutant", ["proj_weight_f16", "proj_input_f16"])
def test_budget_rejects_decoder_mutants(monkeypatch, name, mutant):
    k = decoded(RAGGED, name == "peaked")
    args = list(k["args"])
    if mutant == "proj_weight_f16":
        args[-1] = dict(args[-1], **{"proj_linear.weight": f16(args[-1]["proj_linear.weight"])})
    else:
        monkeypatch.setattr(O, "decoder_step", _proj_input_f16_step(O.decoder_step))
    got = R.oracle32_teacher_forced(O, *args)
    monkeypatch.undo()
    for what in ("token_logp", "mean_logp", "best_logp"):
        fig = R.figures(got[what], k["tf64"][what], k["tf32"][what], k["scored"])
        print(f"[acc] mutant {mutant} {name} {what} max_ratio={fig['max_ratio']:.1f} "
              f"rms_ratio={fig['rms_ratio']:.1f} e_max={fig['e_max']:.3e}")
        if what == "mean_logp":
            # the mean over the V columns averages a per-column rounding defect away (with the plain
            # weights its ratio stays at 1.0): the per-token figures are the ones that must catch it
            continue
        assert fig["max_ratio"] > M and fig["rms_ratio"] > M
        with pytest.raises(AssertionError):
            R.budget(got[what], k["tf64"][what], k["tf32"][what], M, valid=k["scored"])
