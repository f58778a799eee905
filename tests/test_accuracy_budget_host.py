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
