"""Float64 accuracy budgets for every device stage, in both MFMA arithmetics (the eng fixture).

Each stage is compared, over all of its valid elements, with the float64 reference of that one
stage (tests/f64_ref.py) fed the DEVICE's own float32 output of the stage before it, so a bound
speaks about one kernel group and not about accumulated drift:

  logmel         eng.log_mel: both kernel forms of the wav -> log-mel
                 front end, two figures (log, linear domain)             <- the samples
  features       eng.features (one-pass kernels; two-pass at T > 1024)   <- the fbank
  encoder        eng.encode: input GEMM, recurrence, residual, splits    <- device feat
  keys           the keys GEMM of the same encode                        <- device enc
  score          eng.score: three-launch step + batched projection       <- device enc, keys, h, c
  greedy         eng.greedy: the folded step, teacher-forced on the
                 device's own tokens (accum, alignment)                  <- device enc, keys, h, c
  beam           eng.beam(k), each utterance's best hypothesis re-scored
                 (eos appended where it finished): the three-launch step
                 at k = 1, 2, 3, 5, 7, 12 (every attention instantiation
                 and select width), the folded step at R = 1024 and 2048
                 (k = 4, 8, 16), under f32 the wide blocks at R = 2048   <- device enc, keys, h, c

The bound is f64_ref.budget at M = 8 on the maximum and on the rms error: the device may be 8 times
as far from the float64 truth as the float32 numpy oracle is on the same stage inputs (for the
features and the log-mel, oracle.torch_port: the oracle takes its CMVN statistics and its FFT in
float64).  M is derived in f64_ref.M_DEFAULT from float32 evaluations, not from the device, and
test_accuracy_budget_host.py shows that it admits the torch-CPU port and rejects the seeded defects.
Elements outside the valid ones must be exactly 0 (keys: exactly b_attn).  Every case also asserts
the device flags and that the effective precision is the requested one.

Run with -s for one "[acc] stage shape arithmetic what max_ratio rms_ratio e_ref_max e_max" line
per compared quantity (tools/acc_lines.py turns them into profiles/accuracy/accuracy_budget.json).

MEASURED on one MI355X (every case is in profiles/accuracy/accuracy_budget.json): per stage and
quantity the largest ratio of the device's error to the float32 reference's over the cases
(shapes, weight sets, options), maximum and rms, and the shape of the largest maximum.  All are
below M = 8; the largest is 3.55 (f32 MFMA, mean_logp at R = 1320, peaked).  The s16x3 ratios are at
or below the exact-f32 path's everywhere but two 40-term float32 sums, both inside such a sum's
rounding: the greedy accum's maximum (1.42 against 1.26) and the beam score (3.05 against 2.50, at
B256k8-peaked; its rms is 2.42 against 2.47).  The log-mel kernels use no MFMA: both columns hold
the same figures.

  stage    quantity     cases  s16x3 max    rms    f32 max    rms  worst shape (s16x3 / f32)
  logmel   log             10       1.61   1.79       1.61   1.79  tone-wave / tone-wave
  logmel   lin             10       2.96   1.17       2.96   1.17  wav0-wave / wav0-wave
  features feat            16       1.35   1.45       1.35   1.45  logmel-T9-cmvn / logmel-T9-cmvn
  encoder  enc              6       1.02   0.85       1.76   1.17  B37-peaked / ragged6-peaked
  encoder  h                6       0.93   0.85       1.12   1.13  ragged6-peaked / ragged6-peaked
  encoder  c                6       0.96   0.87       1.19   1.14  ragged6-peaked / ragged6-peaked
  keys     keys             6       0.86   0.58       1.49   1.43  B37-peaked / B37-peaked
  score    token_logp      10       1.96   1.47       2.48   2.25  R120-plain / R1320-peaked
  score    mean_logp       10       1.63   1.58       3.55   2.51  R320-plain / R1320-peaked
  score    best_logp       10       1.80   1.66       3.09   2.64  R2080-plain / R1320-peaked
  score    alignment       10       1.88   1.42       1.89   1.44  R2080-peaked / R320-peaked
  score    total_logp      10       1.60   1.88       1.81   2.01  R21-plain / R21-peaked
  greedy   accum           10       1.42   1.26       1.26   1.42  B19-direct-plain / B33-peaked
  greedy   alignment        8       1.40   1.23       1.58   1.24  B19-peaked / B19-plain
  beam     score           14       3.05   2.42       2.50   2.47  B256k8-peaked / B256k8-peaked

The beam cases one by one (maximum / rms; s16x3, then f32):

  B128k8-plain   0.75 / 0.98   0.84 / 1.02      B3k1-peaked    0.30 / 0.28   1.27 / 1.47
  B128k8-peaked  1.96 / 1.74   2.44 / 2.13      B3k2-peaked    2.55 / 2.23   1.77 / 2.45
  B256k4-plain   0.65 / 1.04   1.00 / 0.95      B3k3-peaked    0.71 / 0.78   1.65 / 2.31
  B256k4-peaked  1.42 / 1.34   1.24 / 1.26      B3k5-peaked    0.40 / 0.42   0.55 / 0.72
  B256k8-plain   1.17 / 1.27   1.10 / 1.01      B3k7-peaked    0.40 / 0.42   0.55 / 0.72
  B256k8-peaked  3.05 / 2.42   2.50 / 2.47      B3k12-peaked   0.72 / 0.71   0.80 / 1.07
  B128k16-plain  1.10 / 1.25   0.97 / 0.95
  B128k16-peaked 1.51 / 2.09   1.73 / 2.41

The log-mel cases (both forms give the same bits; log / lin, maximum): ragged9 0.88 / 0.89, wav0
1.55 / 2.96, tone 1.61 / 1.00, silence 0.62 / 1.00, shortrow 0.52 / 0.81.

(The encoder's weights, and so its rows, are the same in the plain and the peaked set.)  The
float32 reference's own maximum error, for scale: log-mel 2e-5 to 1.3e-4 in the log domain (0.19
on the tone's leakage bins) and 6e-8 to 7e-7 of the frame's scale in the linear one, features 3e-7
to 3e-6 (1e-5 to 1e-4 at Tp = 2), encoder output 1.0e-6 to 1.5e-6, keys 0.7e-6 to 1.3e-6, per-token
log-probabilities 0.7e-6 to 1.4e-6 plain and 4e-6 to 1.7e-5 peaked, alignments 2e-8 to 4e-8, the
40-term sums (total_logp, accum, beam score) 4e-6 to 1.8e-4.
"""
import functools
import hashlib

import numpy as np
import pytest
import torch

import f64_ref as R
from golden_util import fbank_for, load_golden, wav_family, WAV_FAMILIES
from test_gpu_score import SHAPES, shape_targets
from oracle import casr_oracle as O
from oracle import torch_port as TP
from casr.config import CasrConfig
from casr.lib import pack_weights
from casr.results import greedy_steps
from casr.weights import synthetic_state_dicts

pytestmark = pytest.mark.gpu

CFG = CasrConfig()
LMAX = CFG.max_len
M = R.M_DEFAULT


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
    assert eng.precision() == eng.requested


def cycle_frames(B):
    """B lengths cycling over 60 .. 120 frames (Tp 20 .. 40)"""
    return tuple(60 + (7 * b) % 61 for b in range(B))


ENC_SHAPES = {
    "ragged6": (101, 75, 48, 9, 6, 200),   # 396 GEMM rows: a full 256-row tile and a tail; Tp down to 2
    "B37": cycle_frames(37),               # > 4 row tiles; two 32-row and three 16-row recurrence blocks
    "Tp267": (801, 400, 12),               # 267 dependent steps: growth with the step count
}


def batch_fbank(frames, dev, fbank=fbank_for):
    x = np.zeros((len(frames), max(frames), 80), np.float32)
    for b, t in enumerate(frames):
        x[b, :t] = fbank(b, t)
    return torch.from_numpy(x).to(dev), torch.tensor(frames, dtype=torch.int32, device=dev)


def encode(eng, frames):
    """features + encode; returns the device's feat [B, Tp, D] and its lengths on the host"""
    fb, fr = batch_fbank(frames, eng.device)
    feat, flen = eng.features(fb, fr, eps=1e-6)
    eng.encode(feat, flen)
    flen = flen.cpu().numpy()
    assert flen.tolist() == [t // 3 for t in frames]
    return feat.cpu().numpy(), flen


def results_tm(eng):
    """The encode's results in the reference's time-major layouts: enc [Tp, B, C], h, c [B, C],
    keys [Tp, B, A]."""
    enc, h, c, keys = (x.cpu().numpy() for x in eng.encoder_results())
    return np.ascontiguousarray(enc.transpose(1, 0, 2)), h, c, np.ascontiguousarray(keys.transpose(2, 0, 1))


def memo(fn):
    """References are computed once per distinct stage input and shared by the two arithmetics
    wherever the device hands both the same bits (the key is a digest of the inputs); read-only."""
    cache = {}

    def wrapped(*args):
        h = hashlib.sha1()
        for a in args:
            h.update(np.ascontiguousarray(a).tobytes() if isinstance(a, np.ndarray) else repr(a).encode())
        k = h.digest()
        if k not in cache:
            out = fn(*args)
            for v in (out.values() if isinstance(out, dict) else out):
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            cache[k] = out
        return cache[k]
    return wrapped


def valid_tb(lens, T):
    return np.arange(T)[:, None] < np.asarray(lens)[None, :]


# ------------------------------------------------------------------ log-mel front end
GOLD = load_golden()[0]
FB = np.ascontiguousarray(GOLD["fb_matrix"])   # the reference's own filterbank
WINDOW = torch.hann_window(400).numpy()        # data.py:381-382
RAGGED_N = (513, 672, 673, 993, 1153, 1793, 1953, 5473, 5633)
RAGGED_FRAMES = [1, 1, 2, 4, 5, 9, 10, 32, 33]


def silence_wav():
    x = wav_family("noise", 4000, 31)
    x[1000:2600] = 0.0
    return x


LOGMEL_CASES = {
    # frame counts on each side of the 16-lane form's 4 frames per quad, the wave form's 8 frames per
    # wave and both forms' 32 frames per block; 513 samples is the shortest signal with a frame, 672
    # the longest with one; the signal family changes with the row
    "ragged9": lambda: [wav_family(WAV_FAMILIES[b % 5], n, 60 + b) for b, n in enumerate(RAGGED_N)],
    "wav0": lambda: [np.asarray(GOLD["wav0"])],
    "tone": lambda: [wav_family("tone", 2000, 0)],
    "silence": lambda: [silence_wav()],
    # a row below one frame inside a batch that has frames: flag 64, frames 0, a row of zeros
    "shortrow": lambda: [wav_family("speech", 2000, 5), wav_family("speech", 400, 6)],
}


@functools.lru_cache(maxsize=None)
def logmel_refs(case):
    """Per utterance with a frame: (float64 log-mel, float64 mel power, float32 reference), read-only,
    with the reference's constants (its filterbank from the golden file, torch's window).  The
    float32 reference is oracle.torch_port.log_mel; for wav0 the reference's own wav0_logmel."""
    out = []
    for w in LOGMEL_CASES[case]():
        if R.log_mel_frames(w.shape[0]) == 0:
            out.append(None)
            continue
        truth, mel = R.log_mel(w, FB, WINDOW)
        ref = np.asarray(GOLD["wav0_logmel"]) if case == "wav0" else TP.log_mel(w, fb=FB).numpy()
        for a in (truth, mel, ref):
            a.setflags(write=False)
        out.append((truth, mel, ref))
    return out


@pytest.mark.parametrize("form", [1, 0], ids=["q16", "wave"])
@pytest.mark.parametrize("case", list(LOGMEL_CASES))
def test_log_mel_budget(eng, case, form):
    """Both kernels of csrc/frontend.hip (LOGMEL_Q16 = 1: 16 lanes per frame; 0: a wave per frame)
    against f64_ref.log_mel, on two figures at M = 8 (f64_ref.log_mel_budget): the log output, and
    the linear domain exp(out) over the frame's largest float64 mel power.  The output does not
    depend on the MFMA arithmetic; the fixture's two engines both run it.  Samples past n_samples[b]
    are NaN: a valid frame that read one would not be finite.  Every case asserts exact zeros on the
    padding rows (3 past the longest utterance, t_max = frames(n_max) + 3), exact frame counts, and
    the device flags.
      tone      1 kHz: the float32 reference itself is off by 0.19 in the log domain, in the bins
                that hold only leakage, so only the linear figure binds here
      silence   samples 1000..2600 exactly zero: the float64 mel power of the frames inside is
                exactly 0, and both floors apply (log FLT_EPSILON on either side)
      wav0      frame 31 lies in a stretch near DC and holds only window leakage: it sets the linear
                figure (2.96) through the last bit of 12 window values, and measured 17.7 with the
                window table rounded from double
    The filterbank and the window are data of the operation: the truth uses the reference's own
    (the golden file's fb_matrix, torch.hann_window).  Three constants and functions of
    csrc/frontend.hip follow the reference to the last bit because this figure resolves them:
      filterbank  equal to the reference's matrix bit for bit (test_capi_host.py); with a linspace of
                  two roundings and libm's log10f 98 weights differed by up to 8.4e-6, and the linear
                  figure measured 10.5 to 12.2 on every case but wav0
      log         rounded from double; the device's logf is up to 1.75 float32 steps off near 475, the
                  tone's peak band, where the reference lands 0.06 from the exact value: 15.3 on the
                  tone's linear figure, and 2.26 instead of 0.89 on ragged9
      window      evaluated in float32 as torch does (wav0 above)"""
    wavs = LOGMEL_CASES[case]()
    ns = [w.shape[0] for w in wavs]
    B, n_max = len(ns), max(ns)
    want = [R.log_mel_frames(n) for n in ns]
    if case == "ragged9":
        assert want == RAGGED_FRAMES
    t_max = max(want) + 3
    x = np.full((B, n_max), np.nan, np.float32)
    for b, w in enumerate(wavs):
        x[b, :ns[b]] = w
    try:
        eng.set_option("LOGMEL_Q16", form)
        fb, frames = eng.log_mel(torch.from_numpy(x).to(eng.device), torch.tensor(ns, dtype=torch.int32), t_max=t_max)
        flags = eng.device_flags()
    finally:
        eng.set_option("LOGMEL_Q16", 1)
    assert flags == (64 if min(want) == 0 else 0)
    fb, frames = fb.cpu().numpy(), frames.cpu().numpy()
    assert fb.shape == (B, t_max, 80)
    assert frames.tolist() == want == [1 + (n - 513) // 160 if n >= 513 else 0 for n in ns]
    valid = (np.arange(t_max)[None, :] < np.asarray(want)[:, None])[:, :, None]
    truth, mel, ref = (np.zeros(fb.shape) for _ in range(3))
    for b, r in enumerate(logmel_refs(case)):
        if r is not None:
            assert r[0].shape == (want[b], 80)
            truth[b, :want[b]], mel[b, :want[b]], ref[b, :want[b]] = r
    if case == "silence":
        dead = (mel[0, :want[0]] == 0).all(axis=1)
        assert dead.sum() >= 5 and (mel[0, :want[0]][~dead] > 0).all()
    # (budget asserts the exact zeros of every element outside valid: padding rows, the short row)
    R.log_mel_budget(fb, truth, mel, ref, M, valid=valid,
                     tag=f"logmel {case}-{'q16' if form else 'wave'} {eng.requested}")


@pytest.mark.parametrize("form", [1, 0], ids=["q16", "wave"])
def test_log_mel_batch_below_one_frame(eng, form):
    """n_max = 400 < 513: no row of wav holds the 513 samples of one frame (the 16-lane kernel
    loads that many for a frame that is not live), so neither kernel runs: frames 0, zeros, flag 64."""
    wav = torch.from_numpy(np.stack([wav_family("speech", 400, 70 + b) for b in range(3)])).to(eng.device)
    try:
        eng.set_option("LOGMEL_Q16", form)
        fb, frames = eng.log_mel(wav, [400, 400, 17])
        flags = eng.device_flags()
    finally:
        eng.set_option("LOGMEL_Q16", 1)
    assert flags == 64
    assert frames.cpu().tolist() == [0, 0, 0]
    assert fb.shape == (3, 1, 80) and not fb.cpu().numpy().any()
    assert eng.device_flags() == 0


# ------------------------------------------------------------------ features
def logmel_like(b, t):
    """a log-mel-like input: mean -8, spread 4 (fbank_for alone has zero mean)"""
    return (4 * fbank_for(b, t) - 8).astype(np.float32)


@memo
def features_refs(family, frames, eps):
    fbank = fbank_for if family == "normal" else logmel_like
    truth, ref = [], []
    for b, t in enumerate(frames):
        fb = fbank(b, t)
        truth.append(R.features(fb, eps))
        # eps < 0 (no CMVN): the port has no such form; the oracle's stacking is float32 throughout
        ref.append(TP.features_from_fbank(fb, eps).numpy() if eps >= 0 else O.stack_frames(O.add_delta_deltas(fb)))
    return truth, ref


@pytest.mark.parametrize("eps", [1e-6, -1.0], ids=["cmvn", "raw"])
@pytest.mark.parametrize("family", ["normal", "logmel"])
@pytest.mark.parametrize("T", [6, 9, 101, 1100])
def test_features_budget(eng, T, family, eps):
    """T = 6 and 9 give Tp = 2 and 3 rows (at Tp = 2 with the offset the float32 reference itself is
    about 1e-5 or more from float64: an ill-conditioned std, which a bound relative to the reference
    follows); 1100 > 1024 runs the two-pass kernels.  The second utterance is one row shorter."""
    frames = (T, T - 3) if T > 6 else (T, T)
    fb, fr = batch_fbank(frames, eng.device, fbank_for if family == "normal" else logmel_like)
    feat, flen = eng.features(fb, fr, eps=eps)
    assert eng.device_flags() == 0
    assert eng.precision() == eng.requested
    feat, flen = feat.cpu().numpy(), flen.cpu().numpy()
    assert flen.tolist() == [t // 3 for t in frames]
    truth, ref = features_refs(family, frames, eps)
    Tp = feat.shape[1]

    def padded(rows):
        out = np.zeros(feat.shape, np.float64)
        for b, r in enumerate(rows):
            out[b, :len(r)] = r
        return out
    valid = valid_tb(flen, Tp).T[:, :, None]
    R.budget(feat, padded(truth), padded(ref), M, valid=valid,
             tag=f"features {family}-T{T}-{'cmvn' if eps >= 0 else 'raw'} {eng.requested} feat")


# ------------------------------------------------------------------ encoder and keys
@memo
def encoder_refs(feat, lens):
    enc_sd, _ = weights(False)  # the encoder's weights are the same in both sets
    feats = [feat[b, :n] for b, n in enumerate(lens)]
    enc64, h64, c64 = R.encoder(feats, lens, enc_sd)
    enc32, (h32, c32) = O.encoder_forward(feats, np.asarray(lens), enc_sd)
    return dict(enc=(enc64, enc32), h=(h64, h32), c=(c64, c32))


@memo
def keys_refs(enc, peaked):
    _, dec_sd = weights(peaked)
    return R.compute_keys(enc, dec_sd), O.compute_keys(enc, dec_sd)


@pytest.mark.parametrize("key", list(ENC_SHAPES))
@pytest.mark.parametrize("name", ["plain", "peaked"])
def test_encoder_and_keys_budget(eng, name, key):
    frames = ENC_SHAPES[key]
    bind(eng, name)
    feat, lens = encode(eng, frames)
    enc, h, c, keys = results_tm(eng)
    assert eng.device_flags() == 0
    assert eng.precision() == eng.requested
    ref = encoder_refs(feat, lens)
    valid = valid_tb(lens, enc.shape[0])[:, :, None]
    tag = f"{key}-{name} {eng.requested}"
    R.budget(enc, *ref["enc"], M, valid=valid, tag=f"encoder {tag} enc")
    R.budget(h, *ref["h"], M, tag=f"encoder {tag} h")
    R.budget(c, *ref["c"], M, tag=f"encoder {tag} c")
    # the keys GEMM alone, on the device's own encoder output; padding slots hold exactly b_attn
    _, dec_sd = weights(name == "peaked")
    R.budget(keys, *keys_refs(enc, name == "peaked"), M, valid=valid,
             pad=dec_sd["attn_mechanism.b_attn"][None, None, :], tag=f"keys {tag} keys")


# ------------------------------------------------------------------ decode stages
@memo
def forced_refs(peaked, enc, keys, h, c, lens, targets, tgt_len, feed_len):
    """The teacher-forced pass from the device's encoder results, in float64 and in the float32
    oracle, with the per-utterance totals (float32: added in ascending l, as the reference's and the
    device's accumulators are)."""
    _, dec_sd = weights(peaked)
    args = (enc, keys, h, c, lens, targets, tgt_len, dec_sd, CFG.sos, CFG.eos, feed_len)
    t64 = R.teacher_forced(*args)
    t32 = R.oracle32_teacher_forced(O, *args)
    t64["total"] = t64["token_logp"].sum(axis=1)
    tot = np.zeros(len(lens), np.float32)
    for l in range(targets.shape[1]):
        tot = (tot + t32["token_logp"][:, l]).astype(np.float32)
    t32["total"] = tot
    return t64, t32


def scored(tgt_len, L):
    return np.arange(L)[None, :] < np.asarray(tgt_len)[:, None]


@pytest.mark.parametrize("key", list(SHAPES))
@pytest.mark.parametrize("name", ["plain", "peaked"])
def test_score_budget(eng, name, key):
    """The three-launch decode step and the batched projection, one shape per projection class."""
    frames, L = SHAPES[key]
    targets, n = shape_targets(frames, L)
    bind(eng, name)
    _, lens = encode(eng, tuple(frames))
    enc, h, c, keys = results_tm(eng)
    out = eng.score(targets, n, alignment=True, best=True, mean=True)
    r = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
    assert eng.device_flags() == 0
    assert eng.precision() == eng.requested
    t64, t32 = forced_refs(name == "peaked", enc, keys, h, c, lens, targets.astype(np.int64), n.astype(np.int64),
                           n.astype(np.int64))
    m = scored(n, L)
    tag = f"score {key}-{name} {eng.requested}"
    for what in ("token_logp", "mean_logp", "best_logp"):
        R.budget(r[what], t64[what], t32[what], M, valid=m, tag=f"{tag} {what}")
    # every step's attention weights (steps past tgt_len feed eos, in the references too)
    va = np.broadcast_to(valid_tb(lens, enc.shape[0])[None], r["alignment"].shape)
    R.budget(r["alignment"], t64["alignment"], t32["alignment"], M, valid=va, tag=f"{tag} alignment")
    R.budget(r["total_logp"], t64["total"], t32["total"], M, valid=n > 0, tag=f"{tag} total_logp")


GREEDY_CASES = {
    # (B, option, value, alignment)
    "B19": (19, None, None, True),                    # R <= 32: the k-split folded GEMM (the default)
    "B19-ksplit0": (19, "DEC_KSPLIT", 0, True),       # one workgroup per output block
    "B33": (33, None, None, True),                    # R > 32
    "B19-direct": (19, "ATTN_DIRECT", 1, True),       # direct tanh scores instead of the split exponential
    "B19-attnsplit": (19, "ATTN_SPLIT", 1, False),    # time steps split over blocks: no alignment output
}


@pytest.mark.parametrize("case", list(GREEDY_CASES))
@pytest.mark.parametrize("name", ["plain", "peaked"])
def test_folded_greedy_budget(eng, name, case):
    """The folded greedy step: the reference is fed the device's own tokens at every executed step
    (greedy goes on feeding its argmax after an utterance's eos), and scores them up to and
    including the eos: the sum is greedy's accum (model.py:567-576)."""
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
    assert eng.precision() == eng.requested
    tokens = g["tokens"].cpu().numpy().astype(np.int64)
    out_len, fin = g["out_len"].cpu().numpy(), g["finished"].cpu().numpy().astype(bool)
    steps = greedy_steps(out_len, fin, LMAX)
    n = (out_len + fin).astype(np.int64)
    assert n.min() >= 1 and n.max() <= steps
    assert tokens[:, :steps].min() >= 0 and tokens[:, :steps].max() < CFG.vocab
    t64, t32 = forced_refs(name == "peaked", enc, keys, h, c, lens, tokens[:, :steps], n, np.full(B, steps))
    tag = f"greedy {case}-{name} {eng.requested}"
    R.budget(g["accum"].cpu().numpy(), t64["total"], t32["total"], M, tag=f"{tag} accum")
    if align:
        al = g["alignment"].cpu().numpy()[:steps]
        va = np.broadcast_to(valid_tb(lens, enc.shape[0])[None], al.shape)
        R.budget(al, t64["alignment"], t32["alignment"], M, valid=va, tag=f"{tag} alignment")


SMALL_FRAMES = (101, 75, 48)
BEAM_CASES = {
    # (B, k, frames, R >= 1024: the folded step under s16x3, rows held to the budget and the oracle)
    "B128k8": (128, 8, (48,) * 128, True, None),        # one-accumulator fused GEMM, 4 rows per attention block
    # small widths: the three-launch step in both arithmetics (R < 1024)
    "B3k1": (3, 1, SMALL_FRAMES, False, None),           # attention_kernel<1>, select width 4
    "B3k2": (3, 2, SMALL_FRAMES, False, None),           # attention_kernel<2>, select width 4
    "B3k3": (3, 3, SMALL_FRAMES, False, None),           # 3 live rows of a 4-row attention block, select width 8
    "B3k5": (3, 5, SMALL_FRAMES, False, None),           # two 4-row blocks, the second with 1 live row; width 16
    "B3k7": (3, 7, SMALL_FRAMES, False, None),           # ... with 3 live rows
    "B3k12": (3, 12, SMALL_FRAMES, False, None),         # three 4-row blocks, select width 32
    # R >= 1024: folded under s16x3, three-launch under f32 (R >= 2048: its wide LSTMCell and
    # projection blocks, 16 query slots)
    "B256k4": (256, 4, (48,) * 256, True, 16),           # one 4-row attention block per utterance
    "B256k8": (256, 8, (48,) * 256, True, 16),           # R = 2048, one 8-row block per utterance
    "B128k16": (128, 16, (48,) * 128, True, 16),         # R = 2048, four 4-row blocks, select width 32
}


@functools.lru_cache(maxsize=None)
def small_width_oracle(k):
    """O.beam_decode on the small-width batch, peaked weights.  Its tokens rest on no near tie of two
    float32 candidates: a float64 run of the same search keeps the same tokens at every width
    (test_accuracy_budget_host.test_small_width_beam_tokens_rest_on_no_near_tie), so no fbank seed
    had to change."""
    feats = [O.features_from_fbank(fbank_for(b, t)) for b, t in enumerate(SMALL_FRAMES)]
    return O.beam_decode(feats, [f.shape[0] for f in feats], *weights(True), k)


@functools.lru_cache(maxsize=None)
def oracle_beam_rows(rows, frames, k, peaked):
    feats = [O.features_from_fbank(fbank_for(b, t)) for b, t in zip(rows, frames)]
    return O.beam_decode(feats, [f.shape[0] for f in feats], *weights(peaked), k)


def beam_budget(eng, name, case):
    """One beam decode: each utterance's best hypothesis is re-scored teacher-forced (the convention
    of golden_util.teacher_forced_score; a hypothesis shorter than the executed steps finished, so
    its eos is scored too: a record of step l holds l tokens, the unfinished fallback holds all of
    them, model.py:708-733, :961-972) and the device's score is held to the budget against the
    float64 re-score.  With ``rows`` the references run on that many utterances (0, B - 1 and the
    rest evenly between); every row, re-scored or not, is checked for a scored length >= 1, tokens
    of the vocabulary and a finite score.  Which step ran is read from the LSTMCell GEMM's launch count:
    the folded step runs it at step 0 only."""
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
    assert eng.device_flags() == 0
    assert eng.precision() == eng.requested
    steps = int(r["steps"][0])
    # the folded step runs the LSTMCell GEMM at step 0 only (s16x3); f32 keeps the three-launch step
    assert (n_lstm == 1) if (big and eng.requested == "s16x3") else (n_lstm > 1)
    length = r["length"].astype(np.int64)
    finished = length < steps
    # every row, re-scored or not: at least one scored position, tokens of the vocabulary, a finite
    # score.  Where only 16 rows are re-scored, with the plain weights, every length is >= 1; with
    # the peaked weights the best hypothesis of some 48-frame utterances is the empty one (eos at
    # step 0, length 0, one scored position), in the oracle's beam search too, as asserted below
    assert length.min() >= (1 if name == "plain" and rows is not None else 0) and length.max() <= steps <= LMAX
    empty = tuple(int(b) for b in np.nonzero(length == 0)[0][:2])
    if empty:  # the first two empty hypotheses are the oracle's too, with its score
        ref = oracle_beam_rows(empty, tuple(frames[b] for b in empty), k, name == "peaked")
        assert ref["tokens"] == [[]] * len(empty)
        np.testing.assert_allclose(r["score"][list(empty)], ref["score"], rtol=0, atol=2e-3)
    assert (length + finished).min() >= 1
    assert np.isfinite(r["score"]).all()
    for b in range(B):
        assert ((r["tokens"][b, :length[b]] >= 0) & (r["tokens"][b, :length[b]] < CFG.vocab)).all()
    L = int((length + finished).max())
    targets = np.zeros((B, L), np.int64)
    for b in range(B):
        targets[b, :length[b]] = r["tokens"][b, :length[b]]
        if finished[b]:
            targets[b, length[b]] = CFG.eos
    n = length + finished
    assert n.min() >= 1
    sel = np.arange(B) if rows is None else np.unique(np.round(np.linspace(0, B - 1, rows)).astype(np.int64))
    assert sel[0] == 0 and sel[-1] == B - 1 and len(sel) == (B if rows is None else rows)
    t64, t32 = forced_refs(name == "peaked", np.ascontiguousarray(enc[:, sel]), np.ascontiguousarray(keys[:, sel]),
                           h[sel], c[sel], lens[sel], targets[sel], n[sel], n[sel])
    R.budget(r["score"][sel], t64["total"], t32["total"], M, tag=f"beam {case}-{name} {eng.requested} score")
    return r, length


@pytest.mark.parametrize("name", ["plain", "peaked"])
def test_folded_beam_budget(eng, name):
    """Beam 8 at B = 128: R = 1024 decode rows, where s16x3 runs the folded beam step with the
    one-accumulator fused GEMM (the whole sum scaled by 2^11).  All 128 utterances are re-scored
    (beam_budget)."""
    beam_budget(eng, name, "B128k8")


@pytest.mark.parametrize("k", [1, 2, 3, 5, 7, 12])
def test_small_width_beam_budget(eng, k):
    """The widths no other GPU test runs, each through its own attention instantiation, partial
    attention blocks and select width (BEAM_CASES), on the three-launch step that every beam decode
    below 1,024 rows takes in both arithmetics.  On top of the budget: tokens and lengths equal the
    oracle's beam search, scores within the file-wide 2e-3 of it."""
    r, length = beam_budget(eng, "peaked", f"B3k{k}")
    ref = small_width_oracle(k)
    assert [r["tokens"][b, :length[b]].tolist() for b in range(len(SMALL_FRAMES))] == ref["tokens"]
    np.testing.assert_allclose(r["score"], ref["score"], rtol=0, atol=2e-3)


@pytest.mark.parametrize("case", ["B256k4", "B256k8", "B128k16"])
@pytest.mark.parametrize("name", ["plain", "peaked"])
def test_fold_and_wide_beam_budget(eng, name, case):
    """R = 1024 with one 4-row attention block per utterance, and R = 2048 at k = 8 and k = 16: the
    folded step under s16x3; under f32 the three-launch step, at R = 2048 with its wide blocks.  16
    utterances are held to the budget, the whole batch to the sanity checks of beam_budget."""
    beam_budget(eng, name, case)
