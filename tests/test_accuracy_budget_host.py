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

The log-mel front end has the same three sections (f64_ref.log_mel, two figures per comparison:
the log output and the linear domain, f64_ref.log_mel_budget): the golden wav0_logmel, two admitted
float32 evaluations (the oracle, and the device's radix-4 operation order in numpy float32), and
six defects of the window, the filterbank and the floor in the float32 port.  The mildest that the
budget rejects is the window rounded from double instead of evaluated in float32: 17.7 times the
float32 error, on one frame of wav0.

  4. the s16x1 model (f64_ref ``sites``: the float64 stage with both operands of each MFMA site rounded
     to f16; tests/test_gpu_accuracy_s16x1.py points it at the s16x1 build).  sites = None returns what
     the functions returned before, bit for bit.  Candidates are compared with (model in float64, model
     in float32) at the same M.  Admitted: the model in float32 with every site's contraction in four
     k chunks, and on the keys torch's matmul on pre-rounded operands.  Through a chain two float32
     evaluations differ by rounding flips of the next operand, at the same rate as the float32 model
     against the float64 one, so the ratios stay near 1:

       stage (chunked k order)                     max    rms
       encoder enc / h / c, ragged (Tp 66)        1.18 / 0.91 / 0.92   1.02 / 0.98 / 0.99
       encoder enc / h / c, Tp 267                0.80 / 1.54 / 1.24   1.00 / 1.10 / 1.06
       keys, chunked / torch on pre-rounded       0.34 / 1.37          0.64 / 1.77
       decoder, three paths x two weight sets     at most 1.98 (token_logp, fold-beam, peaked)

     Rejected (float32 model with the defect; maximum / rms on the encoder output, ragged): operands
     truncated toward zero at every site 13.3 / 15.7, bf16 at every site 40 / 40, the last 32-k block
     dropped from the input projection 2,980 / 3,290 and from the recurrence 3,080 / 3,220; on the
     chain-free keys truncation 903 / 2,185, bf16 2,620 / 5,950, the dropped block 295,000; the decoder
     defects are listed at test_x1_budget_rejects_decoder_defects.  Recorded without an assertion
     (test_x1_single_site_bf16_and_folded_embedding_recorded): bf16 at one site is above M at every
     site (enc_ih 43, enc_hh 24, cell_ch 15 to 36, proj 20 to 43 on token_logp, the beam query 20 on
     the alignment) but the embedding's (4.5 three-launch, 1.0 to 2.9 at the folded paths' step 0);
     a folded model with the embedding rounded after all measures 1.2 to 2.9, so the budget does NOT
     tell the folded path's f32 embedding table from the three-launch step's rounded embedding; the
     unrounded float32 stage (an s16x3-grade answer) measures 6.5 / 5.2 on the encoder output, inside
     the band, and 306 / 735 on the keys.

Run with -s for the measured figures ("[acc]" lines)."""
import functools

import numpy as np
import pytest
import torch

import f64_ref as R
from golden_util import load_golden, fbank_for, golden_frames, wav_family, WAV_FAMILIES
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


# ---- the log-mel front end (the references of test_gpu_accuracy.test_log_mel_budget)
FB = np.ascontiguousarray(G["fb_matrix"])     # the reference's own filterbank
WINDOW = torch.hann_window(400).numpy()       # data.py:381-382
LOGMEL_N = 4000                               # 22 frames per signal
EPS32 = float(np.finfo(np.float32).eps)


def silence_wav(n=LOGMEL_N, seed=31):
    """noise with samples 1000..2600 exactly zero: six frames whose mel power is exactly 0"""
    x = wav_family("noise", n, seed)
    x[1000:2600] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def logmel_case(kind):
    """One signal, its float64 log-mel and mel power, and the float32 port's log-mel"""
    wav = G["wav0"] if kind == "wav0" else silence_wav() if kind == "silence" else \
        wav_family(kind, LOGMEL_N, 40 + len(kind))
    truth, mel = R.log_mel(wav, FB, WINDOW)
    ref = TP.log_mel(wav, fb=FB).numpy()
    return frozen(np.asarray(wav), truth, mel, ref)


LOGMEL_KINDS = WAV_FAMILIES + ("tone", "silence", "wav0")


def test_f64_log_mel_matches_reference_golden():
    """The reference's own log-mel of wav0 (its float32 torch.stft chain, tests/golden/make_golden.py)
    against f64_ref.log_mel with the reference's filterbank and window: measured 1.06e-4 at the
    maximum and 3.63e-6 rms over the 147 x 80 values, and oracle.torch_port.log_mel on the same
    input the same two figures (the same torch operators: bit for bit the golden here).  The bound
    is no guessed tolerance: the golden is a float32 evaluation, so it is held to the budget itself,
    M times the port's error on both figures, maximum and rms (another build of torch may take
    another FFT code path; the device-order model below stays within 3.3 of the port)."""
    wav, truth, mel, ref = logmel_case("wav0")
    gold = G["wav0_logmel"]
    assert truth.shape == gold.shape == ref.shape == (R.log_mel_frames(wav.shape[0]), 80)
    fig = R.figures(gold, truth, ref)
    print(f"[acc] f64-vs-golden wav0_logmel max={fig['e_max']:.3e} rms={fig['e_rms']:.3e} "
          f"port max={fig['e_ref_max']:.3e} rms={fig['e_ref_rms']:.3e}")
    R.log_mel_budget(gold, truth, mel, ref, M)
    assert 0 < fig["e_ref_max"] < 1e-3 and fig["e_ref_rms"] < 1e-4   # the port is a float32 evaluation, no more
    # the mel power is the unfloored one, and the float64 oracle-free chain has no zero here
    assert (mel > 0).all() and np.array_equal(truth, np.log(mel))


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


def _rev4(k):
    return ((k & 3) << 6) | (((k >> 2) & 3) << 4) | (((k >> 4) & 3) << 2) | ((k >> 6) & 3)


def device_model_log_mel(wav, fb=FB, window=None, preemphasis=0.97):
    """The device's algorithm (csrc/frontend.hip) in numpy float32 / complex64, another operation
    order than torch.stft's: the 512-point real transform as a 256-point complex radix-4
    decimation-in-frequency transform of z[m] = y[2m] + i y[2m+1], four stages with float32
    twiddles (rounded once from double), the even/odd split with float32 W512, the mel product
    accumulated in bin order.  A model of the operation order only: numpy rounds every product
    where the device fuses some."""
    f32, c64 = np.float32, np.complex64
    x = np.asarray(wav, f32)
    y = x[1:] - f32(preemphasis) * x[:-1]
    w = np.zeros(512, f32)
    w[56:456] = O.hann_window() if window is None else window   # the device's table, up to the last bit of cosf
    L = 1 + (y.shape[0] - 512) // 160
    fr = y[np.arange(L)[:, None] * 160 + np.arange(512)[None, :]] * w[None, :]
    a = (fr[:, 0::2] + 1j * fr[:, 1::2]).astype(c64)                       # [L, 256]
    w256 = np.exp(-2j * np.pi * np.arange(256) / 256).astype(c64)
    w512 = np.exp(-2j * np.pi * np.arange(257) / 512).astype(c64)
    mi = lambda z: (z.imag - 1j * z.real).astype(c64)                      # -i z, exact
    for S in (64, 16, 4, 1):
        g = a.reshape(L, 256 // (4 * S), 4, S)                            # position = group 4S + r S + j
        t0, t1, t2, t3 = g[:, :, 0] + g[:, :, 2], g[:, :, 0] - g[:, :, 2], g[:, :, 1] + g[:, :, 3], g[:, :, 1] - g[:, :, 3]
        out = [t0 + t2, t1 + mi(t3), t0 - t2, t1 - mi(t3)]
        if S > 1:
            j = np.arange(S)
            for q in (1, 2, 3):
                out[q] = (out[q] * w256[((64 // S) * j * q) & 255][None, None, :]).astype(c64)
        a = np.stack(out, axis=2).astype(c64).reshape(L, 256)
    q = np.arange(257)
    z1, z2 = a[:, _rev4(q & 255)], np.conj(a[:, _rev4((256 - q) & 255)])  # X[k] sits at position rev4(k)
    e, o = (f32(0.5) * (z1 + z2)).astype(c64), mi((f32(0.5) * (z1 - z2)).astype(c64))
    X = (e + (o * w512[None, :]).astype(c64)).astype(c64)
    power = (X.real * X.real + X.imag * X.imag).astype(f32)
    mel = np.zeros((L, fb.shape[1]), f32)
    for k in range(257):
        mel = (mel + power[:, k:k + 1] * fb[k][None, :]).astype(f32)
    mel[mel == 0] = np.finfo(f32).eps
    return np.log(mel).astype(f32)


@pytest.mark.parametrize("kind", LOGMEL_KINDS)
def test_budget_admits_f32_log_mel(kind):
    """Two float32-grade evaluations other than the port fit the budget on both figures, on every
    signal family, the golden wav0 and a signal with a silent stretch: the numpy oracle (its FFT is
    float64, the rest float32) and the device's algorithm in numpy float32.  Measured: the oracle at
    most 1.7 times the port's error on the log figure and 3.0 on the linear one, the device-order
    model 3.3 and 3.0 (the 3.0 is wav0's all-leakage frame, through one bit of 12 window values:
    test_budget_rejects_window_rounded_from_double); everything else is below 1.8."""
    wav, truth, mel, ref = logmel_case(kind)
    R.log_mel_budget(O.log_mel(wav, fb=FB), truth, mel, ref, M, tag=f"host-logmel {kind} oracle")
    model = device_model_log_mel(wav)
    R.log_mel_budget(model, truth, mel, ref, M, tag=f"host-logmel {kind} device-model")
    if kind == "silence":   # both floors: the float64 mel power is exactly 0 on the silent frames
        dead = (mel == 0).all(axis=1)
        assert dead.sum() >= 5 and np.all(model[dead] == np.float32(np.log(np.float32(EPS32))))


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


# ---- log-mel mutants, each applied to the float32 port
def window_off_centre():
    w = np.zeros(512, np.float32)
    w[57:457] = WINDOW                       # torch.stft centres the 400 points at 56
    return dict(window=w)


def window_symmetric():
    return dict(window=torch.hann_window(400, periodic=False).numpy())


def filter_last_bin_dropped():
    fb = FB.copy()
    for m in range(fb.shape[1]):
        fb[np.nonzero(fb[:, m])[0][-1], m] = 0
    return dict(fb=fb)


def filterbank_true_bin_frequencies():
    """create_fb_matrix with the bins' true frequencies linspace(0, 8000, 257) instead of the
    reference's linspace(f_min, f_max, n_stft) (data.py:43)"""
    mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)
    f_pts = 700.0 * (10.0 ** (np.linspace(mel(80.0), mel(7600.0), 82) / 2595.0) - 1.0)
    slopes = f_pts[None, :] - np.linspace(0.0, 8000.0, 257)[:, None]
    d = np.diff(f_pts)
    return dict(fb=np.maximum(0.0, np.minimum(-slopes[:, :-2] / d[:-1], slopes[:, 2:] / d[1:])).astype(np.float32))


def window_rounded_from_double():
    """0.5 - 0.5 cos(2 pi j / 400) in double, rounded once: up to 2.4e-7 from torch's float32
    evaluation"""
    return dict(window=(0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(400) / 400)).astype(np.float32))


LOGMEL_MUTANTS = [window_off_centre, window_symmetric, filter_last_bin_dropped, filterbank_true_bin_frequencies]


def _mutant_figures(mutant, kind):
    wav, truth, mel, ref = logmel_case(kind)
    got = TP.log_mel(wav, **dict(dict(fb=FB), **mutant())).numpy()
    log = R.figures(got, truth, ref)
    lin = R.figures(R.mel_linear(got, mel), R.mel_linear(None, mel), R.mel_linear(ref, mel))
    print(f"[acc] mutant {mutant.__name__} {kind} log max_ratio={log['max_ratio']:.1f} rms_ratio={log['rms_ratio']:.1f} "
          f"lin max_ratio={lin['max_ratio']:.1f} rms_ratio={lin['rms_ratio']:.1f}")
    return got, truth, mel, ref, log, lin


@pytest.mark.parametrize("kind", WAV_FAMILIES + ("tone",))
@pytest.mark.parametrize("mutant", LOGMEL_MUTANTS, ids=lambda f: f.__name__)
def test_budget_rejects_log_mel_mutants(mutant, kind):
    """Four defects of the operation's constants, each in the float32 port.  On the five broadband
    families both figures reject each of them, maximum and rms; the mildest measured is the
    symmetric window on the DC signal, 3,105 times the float32 error (log, maximum), every other
    figure is above 4,100.  On the tone the log figure is set by the leakage bins, where the float32
    reference itself is off by 0.15, so only the linear figure is asserted there: 56,000 and more
    for the symmetric window and the two filterbank defects (the log figure measured 9.5, 172 and 25
    on them).  The window one sample off centre is not asserted on the tone: a time shift of a
    stationary tone changes its power only through the leakage between its two mirror components,
    and the float32 port with that window measured 15.7 (log) and 7.4 / 9.3 (linear, maximum / rms)
    against a reference error of 6e-8, on either side of M.  That is what the budget can resolve."""
    got, truth, mel, ref, log, lin = _mutant_figures(mutant, kind)
    if kind == "tone" and mutant is window_off_centre:
        return
    assert lin["max_ratio"] > M and lin["rms_ratio"] > M
    if kind != "tone":
        assert log["max_ratio"] > M and log["rms_ratio"] > M
    with pytest.raises(AssertionError):
        R.log_mel_budget(got, truth, mel, ref, M)


def test_budget_rejects_window_rounded_from_double():
    """The mildest defect the budget resolves: the window rounded once from double differs from torch's float32 evaluation in 320 of 400 values, by
    2.4e-7 at most.  Frame 31 of the golden wav0 lies in a stretch near DC, whose energy is below the
    first filter: every mel band of that frame holds only window leakage, and follows the window's
    last bits.  Measured on the linear figure: 17.7 times the float32 error at the maximum (4.1 rms),
    6.9e-6 of the frame's scale; the log figure stays at 1.2.  With the window evaluated as torch
    does but the correctly rounded cosine (oracle.casr_oracle.hann_window; 12 values differ from
    this torch's by one bit; the device's table is the same up to the last bit of libm's cosf) the
    same figure is 3.0."""
    got, truth, mel, ref, log, lin = _mutant_figures(window_rounded_from_double, "wav0")
    assert lin["max_ratio"] > M
    with pytest.raises(AssertionError):
        R.log_mel_budget(got, truth, mel, ref, M)
    near = TP.log_mel(logmel_case("wav0")[0], fb=FB, window=O.hann_window()).numpy()
    R.log_mel_budget(near, truth, mel, ref, M)
    assert np.abs(O.hann_window() - WINDOW).max() <= 2.0 ** -24


def test_budget_rejects_log_mel_without_floor():
    """Without the floor the silent frames are log(0) = -inf: the budget refuses a candidate that
    is not finite on a valid element.  On a signal with no exactly-zero mel power the floor does
    nothing, and its absence cannot be seen."""
    wav, truth, mel, ref = logmel_case("silence")
    got = TP.log_mel(wav, fb=FB, floor=False).numpy()
    assert np.isneginf(got[(mel == 0)]).all() and (mel == 0).any()
    with pytest.raises(AssertionError, match="not finite"):
        R.log_mel_budget(got, truth, mel, ref, M)
    assert np.array_equal(TP.log_mel(logmel_case("noise")[0], fb=FB, floor=False).numpy(), logmel_case("noise")[3])


# ------------------------------------------------------------------ the oracle tokens of the small beam widths
SMALL_FRAMES = (101, 75, 48)   # test_gpu_accuracy.SMALL_FRAMES


@functools.lru_cache(maxsize=None)
def _small_width_encoded(dtype):
    enc_sd, _ = weights(True)
    feats = [O.features_from_fbank(fbank_for(b, t)).astype(dtype) for b, t in enumerate(SMALL_FRAMES)]
    lens = [f.shape[0] for f in feats]
    return lens, O.encoder_forward(feats, lens, {n: v.astype(dtype) for n, v in enc_sd.items()})


def _small_width_beam(monkeypatch, k, dtype):
    """O.beam_decode with every float32 of the oracle replaced by dtype (its F32 is looked up at
    call time); the encoder runs once per dtype"""
    monkeypatch.setattr(O, "F32", dtype)
    lens, encoded_ = _small_width_encoded(dtype)
    monkeypatch.setattr(O, "encoder_forward", lambda *a, **kw: encoded_)
    dec_sd = {n: v.astype(dtype) for n, v in weights(True)[1].items()}
    r = O.beam_decode([None] * len(lens), lens, None, dec_sd, k)
    monkeypatch.undo()
    return r


@pytest.mark.parametrize("k", [1, 2, 3, 5, 7, 12])
def test_small_width_beam_tokens_rest_on_no_near_tie(monkeypatch, k):
    """test_gpu_accuracy.test_small_width_beam_budget asks the device for the oracle's tokens at
    widths 1, 2, 3, 5, 7 and 12.  That is a fair demand only where the float32 oracle's own choice
    does not rest on a near tie of two candidates: a float64 run of the same search must keep the
    same tokens.  It does at every width (scores within 6e-5 of each other), so the fbank seeds are
    golden_util.fbank_for's and golden_util.near_tie_beam_check is not needed."""
    r32 = _small_width_beam(monkeypatch, k, np.float32)
    r64 = _small_width_beam(monkeypatch, k, np.float64)
    assert r32["tokens"] == r64["tokens"]
    assert r32["steps"] == r64["steps"]
    np.testing.assert_allclose(r32["score"], r64["score"], rtol=0, atol=2e-4)


def test_library_filterbank_is_the_reference_matrix():
    """casr.lib.mel_filterbank (csrc/frontend.hip mel_filterbank, the table casr_log_mel applies)
    equals the matrix torch builds for the reference, bit for bit.  A weight is a difference of two
    frequencies near 7,000 Hz over a band width of 30 to 250 Hz, so one last bit of a mel point moves
    it by 1e-5: a linspace of two roundings (product, then sum, where torch's is one fused
    multiply-add) changes 11 of the 82 mel points, and libm's log10f(1 + 80 / 700) is one bit above
    the correctly rounded value torch returns.  With either, 98 of the 504 nonzero weights differ by
    up to 8.4e-6 and a band's sum by 4.7e-6 of it, which the linear figure rejects everywhere, at
    10.6 to 26.6 times the float32 error (the log figure admits it, at most 2.2).  Should another
    libm's powf move a mel point, the matrix must still pass the budget on both figures."""
    from casr.lib import mel_filterbank
    lib_fb = mel_filterbank()
    assert np.array_equal(lib_fb, FB)
    for kind in WAV_FAMILIES + ("tone",):
        wav, truth, mel, ref = logmel_case(kind)
        R.log_mel_budget(TP.log_mel(wav, fb=lib_fb).numpy(), truth, mel, ref, M)


# ------------------------------------------------------------------ 4. the s16x1 model (f64_ref sites)
ENC_SITES = R.SITES_X1_ENCODER
X1_PATHS = {"three-launch": R.SITES_X1_THREE_LAUNCH, "fold-greedy": R.SITES_X1_FOLD_GREEDY,
            "fold-beam": R.SITES_X1_FOLD_BEAM}
TF_WHAT = ("token_logp", "mean_logp", "best_logp", "alignment")


# ---- the float64 functions as they stood before f64_ref took ``sites``: the bit-for-bit reference
def _plain_lstm_scan(gx, w_hh, b_hh, reverse):
    T, H = gx.shape[0], w_hh.shape[1]
    h, c, y = np.zeros(H), np.zeros(H), np.zeros((T, H))
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        g = gx[t] + (w_hh @ h + b_hh)
        i, f, o = R._sigm(g[:H]), R._sigm(g[H:2 * H]), R._sigm(g[3 * H:])
        c = f * c + i * np.tanh(g[2 * H:3 * H])
        h = o * np.tanh(c)
        y[t] = h
    return y, h, c


def _plain_encoder(feats, lens, enc_sd, num_layers=4):
    lens = [int(n) for n in lens]
    B = len(feats)
    w = {k: R._f64(v) for k, v in enc_sd.items()}
    H = w["rnn.rnn.0.weight_hh_l0"].shape[1]
    enc, hN, cN = np.zeros((max(lens), B, 2 * H)), np.zeros((B, 2 * H)), np.zeros((B, 2 * H))
    for b in range(B):
        x = R._f64(feats[b])[:lens[b]]
        for i in range(num_layers):
            y = np.zeros((lens[b], 2 * H))
            for d, suf in enumerate(("", "_reverse")):
                p = f"rnn.rnn.{i}."
                gx = x @ w[p + "weight_ih_l0" + suf].T + w[p + "bias_ih_l0" + suf]
                y[:, d * H:(d + 1) * H], hN[b, d * H:(d + 1) * H], cN[b, d * H:(d + 1) * H] = _plain_lstm_scan(
                    gx, w[p + "weight_hh_l0" + suf], w[p + "bias_hh_l0" + suf], reverse=(d == 1))
            x = x + y if i > 0 else y
        enc[:lens[b], b] = x
    return enc, hN, cN


def _plain_decoder_step(enc, lens, keys, token, h, c, ctx_prev, dec_sd):
    w, f = dec_sd, R._f64
    enc, keys, h, c, ctx_prev = f(enc), f(keys), f(h), f(c), f(ctx_prev)
    T, Hd = enc.shape[0], h.shape[1]
    x = np.concatenate([f(w["embedding.weight"])[np.asarray(token)], ctx_prev], axis=1)
    g = (x @ f(w["cell.cell.0.weight_ih"]).T + f(w["cell.cell.0.bias_ih"])
         + h @ f(w["cell.cell.0.weight_hh"]).T + f(w["cell.cell.0.bias_hh"]))
    i, fg, o = R._sigm(g[:, :Hd]), R._sigm(g[:, Hd:2 * Hd]), R._sigm(g[:, 3 * Hd:])
    c2 = fg * c + i * np.tanh(g[:, 2 * Hd:3 * Hd])
    h2 = o * np.tanh(c2)
    q = h2 @ f(w["attn_mechanism.W_hidden"])
    e = np.tanh(keys + q[None]) @ f(w["attn_mechanism.v"])
    e = np.where(np.arange(T)[:, None] < np.asarray(lens)[None, :], e, -np.inf)
    p = np.exp(e - e.max(axis=0, keepdims=True))
    alpha = p / p.sum(axis=0, keepdims=True)
    ctx = np.einsum("tr,trc->rc", alpha, enc)
    logit = np.concatenate([h2, ctx], axis=1) @ f(w["proj_linear.weight"]).T + f(w["proj_linear.bias"])
    return logit, h2, c2, ctx, alpha


def _plain_log_softmax(logit):
    logit = R._f64(logit)
    m = logit.max(axis=-1, keepdims=True)
    return logit - (m + np.log(np.exp(logit - m).sum(axis=-1, keepdims=True)))


@pytest.mark.parametrize("name", ["plain", "peaked"])
def test_sites_none_is_the_plain_float64_reference(name):
    """f64_ref's encoder, compute_keys, decoder_step and teacher_forced with sites = None (the
    default) return what they returned before they took ``sites`` and ``dtype``, bit for bit: the
    functions above are that code, kept here unchanged."""
    e = encoded(RAGGED)
    enc_sd, dec_sd = weights(name == "peaked")
    for got, want in zip(R.encoder(e["feats"], e["lens"], enc_sd), _plain_encoder(e["feats"], e["lens"], enc_sd)):
        assert got.dtype == np.float64 and np.array_equal(got, want)
    assert np.array_equal(e["enc64"], _plain_encoder(e["feats"], e["lens"], enc_sd)[0])
    f = R._f64
    assert np.array_equal(R.compute_keys(e["enc32"], dec_sd),
                          f(e["enc32"]) @ f(dec_sd["attn_mechanism.W_enc"]) + f(dec_sd["attn_mechanism.b_attn"]))
    k = decoded(RAGGED, name == "peaked")
    enc, keys, h, c, lens, t, n, _ = k["args"]
    want = R._teacher_forced(_plain_decoder_step, _plain_log_softmax, np.float64, f(enc), f(keys), f(h), f(c), lens,
                             t, n, dec_sd, CFG.sos, CFG.eos, None)
    got = R.teacher_forced(*k["args"], sites=None)
    for what in TF_WHAT:
        assert got[what].dtype == np.float64
        assert np.array_equal(got[what], want[what]) and np.array_equal(got[what], k["tf64"][what]), what
    B = len(lens)
    one = (enc, lens, keys, np.full(B, CFG.sos), h, c, np.zeros((B, CFG.enc_size)), dec_sd)
    for got1, want1 in zip(R.decoder_step(*one), _plain_decoder_step(*one)):
        assert np.array_equal(got1, want1)


# ---- a second float32 evaluation of the model: the contraction in four k chunks
def chunked_mm(a, b, chunks=4):
    edges = np.linspace(0, a.shape[-1], chunks + 1).astype(int)
    out = None
    for lo, hi in zip(edges[:-1], edges[1:]):
        part = a[..., lo:hi] @ b[lo:hi]
        out = part if out is None else out + part
    return out


class k_order:
    """with k_order(mm): f64_ref's site products run through mm"""

    def __init__(self, mm):
        self.mm = mm

    def __enter__(self):
        self.old, R._mm = R._mm, self.mm

    def __exit__(self, *exc):
        R._mm = self.old


@functools.lru_cache(maxsize=None)
def x1_encoded(frames):
    """The s16x1 model of the encoder on the float32 oracle's features, in float64 and in float32"""
    e = encoded(frames)
    enc_sd, _ = weights(False)
    m64 = R.encoder(e["feats"], e["lens"], enc_sd, sites=ENC_SITES)
    m32 = R.encoder(e["feats"], e["lens"], enc_sd, sites=ENC_SITES, dtype=np.float32)
    assert all(a.dtype == np.float32 for a in m32)
    frozen(*m64, *m32)
    return m64, m32


@functools.lru_cache(maxsize=None)
def x1_keys(frames):
    e = encoded(frames)
    _, dec_sd = weights(False)
    return frozen(R.compute_keys(e["enc32"], dec_sd, sites=ENC_SITES),
                  R.compute_keys(e["enc32"], dec_sd, sites=ENC_SITES, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def x1_decoded(peaked, path):
    """The s16x1 model of one decode path, teacher-forced as decoded(): float64 and float32"""
    args = decoded(RAGGED, peaked)["args"]
    m64 = R.teacher_forced(*args, sites=X1_PATHS[path])
    m32 = R.teacher_forced(*args, sites=X1_PATHS[path], dtype=np.float32)
    assert all(m32[w].dtype == np.float32 for w in TF_WHAT)
    return m64, m32


def x1_figures(tag, cand, m64, m32, valid=None):
    fig = R.figures(cand, m64, m32, valid)
    print(f"[acc] x1-host {tag} max_ratio={fig['max_ratio']:.2f} rms_ratio={fig['rms_ratio']:.2f} "
          f"e_ref_max={fig['e_ref_max']:.3e} e_max={fig['e_max']:.3e}")
    return fig


def rejected(cand, m64, m32, valid=None):
    try:
        R.budget(cand, m64, m32, M, valid=valid)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("frames", [RAGGED, LONG], ids=["ragged", "Tp267"])
def test_x1_budget_admits_second_f32_encoder_and_keys(frames):
    """The model in float32 with the contraction of every site in four k chunks, against (model in
    float64, model in plain float32), at M_DEFAULT.  Through the recurrence the two float32
    evaluations differ in the last bits of h, and some of those differences flip an f16 rounding
    of the next step's operand; both do so at the same rate against the float64 model, so the
    ratio stays near 1.  The keys have no chain: there a second candidate, torch's matmul on the
    pre-rounded operands, reaches the stage's only site."""
    e = encoded(frames)
    enc_sd, dec_sd = weights(False)
    m64, m32 = x1_encoded(frames)
    with k_order(chunked_mm):
        cand = R.encoder(e["feats"], e["lens"], enc_sd, sites=ENC_SITES, dtype=np.float32)
        keys_c = R.compute_keys(e["enc32"], dec_sd, sites=ENC_SITES, dtype=np.float32)
    tag = f"encoder Tp{m64[0].shape[0]} chunked"
    for what, c, a, b, v in zip(("enc", "h", "c"), cand, m64, m32, (e["valid"], None, None)):
        x1_figures(f"{tag} {what}", c, a, b, v)
        R.budget(c, a, b, M, valid=v)
    k64, k32 = x1_keys(frames)
    x1_figures(f"keys Tp{m64[0].shape[0]} chunked", keys_c, k64, k32)
    R.budget(keys_c, k64, k32, M)
    keys_t = (torch.tensor(f16(e["enc32"])) @ torch.tensor(f16(dec_sd["attn_mechanism.W_enc"]))
              + torch.tensor(dec_sd["attn_mechanism.b_attn"])).numpy()
    x1_figures(f"keys Tp{m64[0].shape[0]} torch-prerounded", keys_t, k64, k32)
    R.budget(keys_t, k64, k32, M)
    # the model is not the plain stage: its distance from the unrounded float64 truth is the cost
    cost = R.figures(m64[0], e["enc64"], e["enc32"], e["valid"])
    print(f"[acc] x1-host encoder Tp{m64[0].shape[0]} model-vs-unrounded e_max={cost['e_max']:.3e}")
    assert cost["max_ratio"] > M


@pytest.mark.parametrize("path", list(X1_PATHS))
@pytest.mark.parametrize("name", ["plain", "peaked"])
def test_x1_budget_admits_second_f32_decoder(name, path):
    """Each decode path's model, teacher-forced over STEPS steps with both weight sets: the float32
    evaluation in four k chunks fits M_DEFAULT on every quantity.  (oracle.torch_port on pre-rounded
    weights is no candidate here: it cannot round the activations between its operators, so it
    reaches no site of the decoder.)"""
    args = decoded(RAGGED, name == "peaked")["args"]
    scored = decoded(RAGGED, name == "peaked")["scored"]
    m64, m32 = x1_decoded(name == "peaked", path)
    with k_order(chunked_mm):
        cand = R.teacher_forced(*args, sites=X1_PATHS[path], dtype=np.float32)
    for what in TF_WHAT:
        v = None if what == "alignment" else scored
        x1_figures(f"decoder {path} {name} chunked {what}", cand[what], m64[what], m32[what], v)
        R.budget(cand[what], m64[what], m32[what], M, valid=v)


# ---- seeded defects, each in the float32 evaluation of the model (f64_ref._op takes a dict site -> fn)
def rn16(x, weight=False):
    return R.round_f16(x)


def rz16(x, weight=False):
    """to f16, toward zero"""
    x = np.asarray(x, np.float64)
    h = x.astype(np.float16)
    return np.where(np.abs(h.astype(np.float64)) > np.abs(x), np.nextafter(h, np.float16(0)), h)


def bf16(x, weight=False):
    """to bfloat16 (8 significant bits), nearest even"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def drop32(x, weight=False):
    """the last 32-deep k block of the product missing (the activation's last 32 columns)"""
    h = R.round_f16(x).copy()
    if not weight:
        h[..., -32:] = 0
    return h


def scale_twice(x, weight=False):
    """the one-accumulator form's 2^11 on w_hi (decoder.hip:338) applied a second time"""
    h = R.round_f16(x).astype(np.float32)
    return h * np.float32(2048.0) if weight else h


def seeded(sites, fn, only=None):
    """sites as a dict: fn at every site, or at the sites whose plain name is ``only`` (rn16 elsewhere)"""
    return {s: (fn if only is None or s.partition("@")[0] == only else rn16) for s in sites}


ENC_DEFECTS = {"rz-all": (rz16, None), "bf16-all": (bf16, None), "drop32-enc_ih": (drop32, "enc_ih"),
               "drop32-enc_hh": (drop32, "enc_hh")}


@pytest.mark.parametrize("defect", list(ENC_DEFECTS))
def test_x1_budget_rejects_encoder_defects(defect):
    fn, only = ENC_DEFECTS[defect]
    e = encoded(RAGGED)
    m64, m32 = x1_encoded(RAGGED)
    cand = R.encoder(e["feats"], e["lens"], weights(False)[0], sites=seeded(ENC_SITES, fn, only), dtype=np.float32)
    x1_figures(f"defect encoder {defect} enc", cand[0], m64[0], m32[0], e["valid"])
    assert rejected(cand[0], m64[0], m32[0], e["valid"])


@pytest.mark.parametrize("defect", [rz16, bf16, drop32], ids=lambda f: f.__name__)
def test_x1_budget_rejects_keys_defects(defect):
    """The keys have no dependent chain, so no rounding flips: a single mis-rounded site is resolved"""
    e = encoded(RAGGED)
    k64, k32 = x1_keys(RAGGED)
    cand = R.compute_keys(e["enc32"], weights(False)[1], sites={"keys": defect}, dtype=np.float32)
    x1_figures(f"defect keys {defect.__name__}", cand, k64, k32)
    assert rejected(cand, k64, k32)
    # the instrument: the same call with the model's own rounding is the reference itself
    assert np.array_equal(R.compute_keys(e["enc32"], weights(False)[1], sites={"keys": rn16}, dtype=np.float32), k32)


DEC_DEFECTS = {"rz-all": (rz16, None), "bf16-all": (bf16, None), "drop32-cell": (drop32, "cell_ch"),
               "drop32-proj": (drop32, "proj"), "drop32-query": (drop32, "query"), "scale-twice": (scale_twice, "proj")}


def _decoder_defect_figures(name, path, tag, sites):
    k = decoded(RAGGED, name == "peaked")
    m64, m32 = x1_decoded(name == "peaked", path)
    cand = R.teacher_forced(*k["args"], sites=sites, dtype=np.float32)
    out = {}
    for what in TF_WHAT:
        v = None if what == "alignment" else k["scored"]
        x1_figures(f"defect decoder {path} {name} {tag} {what}", cand[what], m64[what], m32[what], v)
        out[what] = rejected(cand[what], m64[what], m32[what], v)
    return out


@pytest.mark.parametrize("defect", list(DEC_DEFECTS))
@pytest.mark.parametrize("path", list(X1_PATHS))
@pytest.mark.parametrize("name", ["plain", "peaked"])
def test_x1_budget_rejects_decoder_defects(name, path, defect):
    """Rejected: the budget fails on a quantity the GPU test holds to it.  Measured (maximum ratio on
    token_logp, plain / peaked weights, the smallest over the three paths): truncation at every site
    19 / 23, bf16 at every site 37 / 21, a dropped 32-k block of the cell 3,700 / 2,600 and of the
    projection 2,600 / 1,500, the 2^11 applied twice 4e7; the dropped block of the beam query 48 / 43
    on token_logp and 1,262 on the alignment."""
    fn, only = DEC_DEFECTS[defect]
    if only == "query" and path != "fold-beam":
        return  # the beam cell's query MFMA is that path's site alone
    rej = _decoder_defect_figures(name, path, defect, seeded(X1_PATHS[path], fn, only))
    # the query moves the attention weights first; every other defect must show in the token's log-probability
    assert rej["alignment" if only == "query" else "token_logp"], rej


def test_x1_single_site_bf16_and_folded_embedding_recorded():
    """Recorded, not asserted (the figures are in the module docstring): bf16 at one site of a chain
    sits inside the band the flips leave (the issue's stand-in: 5.7), and a folded model with the
    embedding rounded after all (= the three-launch model from step 1 on) shows whether the budget
    tells the two paths apart."""
    e = encoded(RAGGED)
    m64, m32 = x1_encoded(RAGGED)
    # operands left exact (an s16x3-grade answer): inside the band through a chain, far outside on the keys
    x1_figures("recorded encoder unrounded enc", e["enc32"], m64[0], m32[0], e["valid"])
    x1_figures("recorded keys unrounded", decoded(RAGGED, False)["keys32"], *x1_keys(RAGGED))
    for site in ("enc_ih", "enc_hh"):
        cand = R.encoder(e["feats"], e["lens"], weights(False)[0], sites=seeded(ENC_SITES, bf16, site), dtype=np.float32)
        fig = x1_figures(f"recorded encoder bf16-{site} enc", cand[0], m64[0], m32[0], e["valid"])
        assert np.isfinite(fig["max_ratio"])
    for name in ("plain", "peaked"):
        for path in X1_PATHS:
            for site in sorted({s.partition("@")[0] for s in X1_PATHS[path]}):
                _decoder_defect_figures(name, path, f"recorded-bf16-{site}", seeded(X1_PATHS[path], bf16, site))
        for path in ("fold-greedy", "fold-beam"):
            sites = {s.replace("cell_emb@0", "cell_emb") for s in X1_PATHS[path]}
            _decoder_defect_figures(name, path, "recorded-embedding-rounded", frozenset(sites))
