"""Float64 accuracy budgets for every device stage, in both MFMA arithmetics (the eng fixture).

Each stage is compared, over all of its valid elements, with the float64 reference of that one
stage (tests/f64_ref.py) fed the DEVICE's own float32 output of the stage before it, so a bound
speaks about one kernel group and not about accumulated drift:

  features       eng.features (one-pass kernels; two-pass at T > 1024)   <- the fbank
  encoder        eng.encode: input GEMM, recurrence, residual, splits    <- device feat
  keys           the keys GEMM of the same encode                        <- device enc
  score          eng.score: three-launch step + batched projection       <- device enc, keys, h, c
  greedy         eng.greedy: the folded step, teacher-forced on the
                 device's own tokens (accum, alignment)                  <- device enc, keys, h, c
  beam           eng.beam(8) at R = 1024: the folded beam step, each
                 utterance's best hypothesis re-scored (eos appended
                 where it finished)                                      <- device enc, keys, h, c

The bound is f64_ref.budget at M = 8 on the maximum and on the rms error: the device may be 8 times
as far from the float64 truth as the float32 numpy oracle is on the same stage inputs (for the
features, oracle.torch_port: the oracle takes its CMVN statistics in float64).  M is derived in
f64_ref.M_DEFAULT from float32 evaluations, not from the device, and test_accuracy_budget_host.py
shows that it admits the torch-CPU port and rejects six seeded defects.  Elements outside the valid
ones must be exactly 0 (keys: exactly b_attn).  Every case also asserts device_flags() == 0 and
that the effective precision is the requested one.

Run with -s for one "[acc] stage shape arithmetic what max_ratio rms_ratio e_ref_max e_max" line
per compared quantity (tools/acc_lines.py turns them into profiles/accuracy/accuracy_budget.json).

MEASURED on one MI355X (every case is in profiles/accuracy/accuracy_budget.json): per stage and
quantity the largest ratio of the device's error to the float32 reference's over the cases
(shapes, weight sets, options), maximum and rms, and the shape of the largest maximum.  All are
below M = 8; the largest is 3.55 (f32 MFMA, mean_logp at R = 1320, peaked), and the s16x3 ratios
are at or below the exact-f32 path's everywhere but the greedy accum's maximum (1.42 against
1.26, both inside the rounding of a 40-term float32 sum).

  stage    quantity     cases  s16x3 max    rms    f32 max    rms  worst shape (s16x3 / f32)
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
  beam     score            2       1.96   1.74       2.44   2.13  B128k8-peaked / B128k8-peaked

(The encoder's weights, and so its rows, are the same in the plain and the peaked set.)  The
float32 reference's own maximum error, for scale: features 3e-7 to 3e-6 (1e-5 to 1e-4 at Tp = 2),
encoder output 1.0e-6 to 1.5e-6, keys 0.7e-6 to 1.3e-6, per-token log-probabilities 0.7e-6 to
1.4e-6 plain and 4e-6 to 1.7e-5 peaked, alignments 2e-8 to 4e-8, the 40-term sums (total_logp,
accum, beam score) 4e-6 to 1.8e-4.
"""
import functools
import hashlib

import numpy as np
import pytest
import torch

import f64_ref as R
from golden_util import fbank_for
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


@pytest.mark.parametrize("name", ["plain", "peaked"])
def test_folded_beam_budget(eng, name):
    """Beam 8 at B = 128: R = 1024 decode rows, where s16x3 runs the folded beam step with the
    one-accumulator fused GEMM (the whole sum scaled by 2^11).  Each utterance's best hypothesis is
    re-scored teacher-forced (the convention of golden_util.teacher_forced_score; a hypothesis
    shorter than the executed steps finished, so its eos is scored too: a record of step l holds l
    tokens, the unfinished fallback holds all of them, model.py:708-733, :961-972)."""
    B, k = 128, 8
    frames = (48,) * B
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
    assert (n_lstm == 1) if eng.requested == "s16x3" else (n_lstm > 1)
    length = r["length"].astype(np.int64)
    finished = length < steps
    L = int((length + finished).max())
    targets = np.zeros((B, L), np.int64)
    for b in range(B):
        targets[b, :length[b]] = r["tokens"][b, :length[b]]
        if finished[b]:
            targets[b, length[b]] = CFG.eos
    n = length + finished
    assert n.min() >= 1
    t64, t32 = forced_refs(name == "peaked", enc, keys, h, c, lens, targets, n, n)
    R.budget(r["score"], t64["total"], t32["total"], M, tag=f"beam B128k8-{name} {eng.requested} score")
