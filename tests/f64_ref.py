"""Float64 reference of every stage, and the accuracy budget built on it (test helper, not a
conftest; used by test_accuracy_budget_host.py and test_gpu_accuracy.py).

A plain numpy float64 restatement of the reference's inference path, written from the reference
lines each function cites, independently of oracle/casr_oracle.py (it imports nothing from it, so
it also cross-checks the oracle).  Every function takes its inputs as given and casts them to
float64: a stage can be fed the float32 output that the device (or the oracle) produced for the
stage before it, and then answers "what is this stage, evaluated exactly, on these inputs".  The
float32 weights are inputs like any other.

Layouts are the reference's (time-major): enc [T, B, 2H], keys [T, B, A], alignment [L, T, B].

budget() compares a candidate with this truth, in multiples of the error that a plain float32
evaluation of the same stage on the same inputs (the numpy oracle) makes against it.
log_mel_budget() does so on two figures of the front end's output: as it is, and in the linear
domain relative to each frame's scale (mel_linear), where the float32 reference is the torch port.
"""
import numpy as np

F64 = np.float64


def _f64(x):
    return np.asarray(x, dtype=F64)


# --------------------------------------------------------------------------------------
# front end
# --------------------------------------------------------------------------------------
FLT_EPSILON = F64(np.finfo(np.float32).eps)


def log_mel(wav, fb, window, preemphasis=0.97, n_fft=512, hop=160):
    """wav [n] -> (log-mel [L, n_mels], mel power [L, n_mels]), L = 1 + (n - 1 - n_fft) // hop
    (get_log_mel, data.py:167-224, inference: no dither, no augmentation).  Three float32 constants
    are data of the operation and are only widened: the pre-emphasis coefficient as numpy's
    float32 product rounds it (data.py:201-202), the window (torch.hann_window(400), periodic,
    data.py:381-382; torch.stft centres it in the n_fft points) and the filterbank fb [n_fft // 2 + 1,
    n_mels] (create_fb_matrix, data.py:21-57).  Then, in float64: y[m] = x[m+1] - pre x[m]; frames
    y[hop f + j] w[j], j < n_fft, no centring (data.py:205-209); |rfft|^2 (data.py:220-221); the
    product with fb (data.py:222); mel == 0 -> FLT_EPSILON and log (data.py:223-224).  The mel
    power is returned as computed, before the floor."""
    x = _f64(np.asarray(wav, np.float32))
    y = x[1:] - F64(np.float32(preemphasis)) * x[:-1]
    win = _f64(np.asarray(window, np.float32))
    lpad = (n_fft - win.shape[0]) // 2
    w = np.zeros(n_fft)
    w[lpad:lpad + win.shape[0]] = win
    assert y.shape[0] >= n_fft, "shorter than one frame (torch.stft raises, data.py:204)"
    L = 1 + (y.shape[0] - n_fft) // hop
    frames = y[np.arange(L)[:, None] * hop + np.arange(n_fft)[None, :]] * w[None, :]
    spec = np.fft.rfft(frames, axis=1)
    assert spec.dtype == np.complex128
    mel = (spec.real ** 2 + spec.imag ** 2) @ _f64(np.asarray(fb, np.float32))
    return np.log(np.where(mel == 0, FLT_EPSILON, mel)), mel


def log_mel_frames(n, n_fft=512, hop=160):
    """frames of n samples: the pre-emphasised signal has n - 1"""
    return 1 + (n - 1 - n_fft) // hop if n - 1 >= n_fft else 0


# --------------------------------------------------------------------------------------
# features
# --------------------------------------------------------------------------------------
def delta_taps():
    """The identity, delta and delta-delta 9-tap filters of add_delta_deltas (data.py:129-150).
    The reference builds them once as float32 constants (integer taps divided by their float32 L2
    norm, data.py:146-148): those constants are data of the operation, so they are formed the same
    way and only then widened."""
    d = np.array([2, 1, 0, -1, -2], np.float32)
    dd = np.convolve(d, d).astype(np.float32)                 # 4 4 1 -4 -10 -4 1 4 4
    taps = np.zeros((3, 9), np.float32)
    taps[0, 4] = 1
    taps[1, 2:7] = d
    taps[2] = dd
    taps = taps / np.sqrt((taps * taps).sum(axis=1, keepdims=True, dtype=np.float32))
    return _f64(taps.astype(np.float32))


def features(fbank, eps=1e-6):
    """fbank [T, n_mels] -> encoder input [T // 3, 9 n_mels]: deltas and delta-deltas by
    cross-correlation over time with 4 zero frames either side (data.py:151-164), three
    consecutive frames stacked channel-major, out[j, c 3M + r M + m] = F[c, 3 j + r, m]
    (data.py:242-249), then per-dimension (x - mean_t) / (std_t + eps) with the unbiased std
    (main.py:37).  eps < 0: the stacked features without CMVN (what get_log_mel returns)."""
    x = _f64(fbank)
    T, M = x.shape
    taps = delta_taps()
    padded = np.concatenate([np.zeros((4, M)), x, np.zeros((4, M))], axis=0)
    chan = np.zeros((3, T, M))
    for c in range(3):
        for k in range(9):
            chan[c] += taps[c, k] * padded[k:k + T]
    Tp = T // 3
    out = np.zeros((Tp, 9 * M))
    for j in range(Tp):
        for c in range(3):
            for r in range(3):
                out[j, c * 3 * M + r * M:c * 3 * M + (r + 1) * M] = chan[c, 3 * j + r]
    if eps < 0:
        return out
    mean = out.mean(axis=0)
    var = ((out - mean) ** 2).sum(axis=0) / (Tp - 1) if Tp > 1 else np.full(9 * M, np.nan)
    return (out - mean) / (np.sqrt(var) + F64(np.float32(eps)))


# --------------------------------------------------------------------------------------
# encoder
# --------------------------------------------------------------------------------------
def _sigm(x):
    return 1.0 / (1.0 + np.exp(-x))


def _lstm_scan(gx, w_hh, b_hh, reverse):
    """One direction of an nn.LSTM layer over one sequence.  gx [T, 4H] = x W_ih^T + b_ih; gate
    order i, f, g, o; c' = f c + i g, h' = o tanh(c').  Returns (y [T, H] in time order, h, c)."""
    T = gx.shape[0]
    H = w_hh.shape[1]
    h = np.zeros(H)
    c = np.zeros(H)
    y = np.zeros((T, H))
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        g = gx[t] + (w_hh @ h + b_hh)
        i, f, o = _sigm(g[:H]), _sigm(g[H:2 * H]), _sigm(g[3 * H:])
        c = f * c + i * np.tanh(g[2 * H:3 * H])
        h = o * np.tanh(c)
        y[t] = h
    return y, h, c


def encoder(feats, lens, enc_sd, num_layers=4, residual=True):
    """RNNEncoder.forward (encoder.py:36-81) over RNN_RES.forward (util.py:1223-1324): packed
    bidirectional single-layer LSTMs (each utterance runs over exactly its own length, the
    backward direction from its own last frame), the layer input added to the layer output from
    the second layer on (util.py:1284-1291), final state = the last layer's [fw || bw]
    (encoder.py:67-72).  feats: B arrays [>= lens[b], D].  One utterance at a time, which is what
    packing means.  Returns (enc [Tmax, B, 2H] zero past each length, h [B, 2H], c [B, 2H])."""
    lens = [int(n) for n in lens]
    B = len(feats)
    w = {k: _f64(v) for k, v in enc_sd.items()}
    H = w["rnn.rnn.0.weight_hh_l0"].shape[1]
    enc = np.zeros((max(lens), B, 2 * H))
    hN = np.zeros((B, 2 * H))
    cN = np.zeros((B, 2 * H))
    for b in range(B):
        x = _f64(feats[b])[:lens[b]]
        for i in range(num_layers):
            y = np.zeros((lens[b], 2 * H))
            for d, suf in enumerate(("", "_reverse")):
                p = f"rnn.rnn.{i}."
                gx = x @ w[p + "weight_ih_l0" + suf].T + w[p + "bias_ih_l0" + suf]
                y[:, d * H:(d + 1) * H], hN[b, d * H:(d + 1) * H], cN[b, d * H:(d + 1) * H] = _lstm_scan(
                    gx, w[p + "weight_hh_l0" + suf], w[p + "bias_hh_l0" + suf], reverse=(d == 1))
            x = x + y if (residual and i > 0) else y
        enc[:lens[b], b] = x
    return enc, hN, cN


# --------------------------------------------------------------------------------------
# decoder
# --------------------------------------------------------------------------------------
def compute_keys(enc, dec_sd):
    """BauAttn.compute_key_value (attention.py:67-78): keys = enc W_enc + b_attn at every time slot
    (a zero padding row gives exactly b_attn); the values are enc itself (map_enc False)."""
    return _f64(enc) @ _f64(dec_sd["attn_mechanism.W_enc"]) + _f64(dec_sd["attn_mechanism.b_attn"])


def log_softmax(logit):
    logit = _f64(logit)
    m = logit.max(axis=-1, keepdims=True)
    return logit - (m + np.log(np.exp(logit - m).sum(axis=-1, keepdims=True)))


def decoder_step(enc, lens, keys, token, h, c, ctx_prev, dec_sd):
    """RNNDecoder.forward (decoder.py:94-137), one step for R rows: input feeding x = [embed(token)
    || previous context], the LSTMCell (util.py:1650-1661), Bahdanau attention e_t = v . tanh(key_t
    + h W_hidden) with -inf added past each length before the softmax over time (attention.py:91-95,
    util.py:131-142), context = sum_t alpha_t enc_t, logit = proj([h || context]).
    enc [T, R, C], keys [T, R, A], lens [R].  Returns (logit [R, V], h, c, ctx, alpha [T, R])."""
    w = dec_sd
    enc, keys, h, c, ctx_prev = _f64(enc), _f64(keys), _f64(h), _f64(c), _f64(ctx_prev)
    T, R, _ = enc.shape
    Hd = h.shape[1]
    x = np.concatenate([_f64(w["embedding.weight"])[np.asarray(token)], ctx_prev], axis=1)
    g = (x @ _f64(w["cell.cell.0.weight_ih"]).T + _f64(w["cell.cell.0.bias_ih"])
         + h @ _f64(w["cell.cell.0.weight_hh"]).T + _f64(w["cell.cell.0.bias_hh"]))
    i, f, o = _sigm(g[:, :Hd]), _sigm(g[:, Hd:2 * Hd]), _sigm(g[:, 3 * Hd:])
    c2 = f * c + i * np.tanh(g[:, 2 * Hd:3 * Hd])
    h2 = o * np.tanh(c2)
    q = h2 @ _f64(w["attn_mechanism.W_hidden"])
    e = np.tanh(keys + q[None]) @ _f64(w["attn_mechanism.v"])             # [T, R]
    live = np.arange(T)[:, None] < np.asarray(lens)[None, :]
    e = np.where(live, e, -np.inf)
    p = np.exp(e - e.max(axis=0, keepdims=True))
    alpha = p / p.sum(axis=0, keepdims=True)
    ctx = np.einsum("tr,trc->rc", alpha, enc)
    logit = np.concatenate([h2, ctx], axis=1) @ _f64(w["proj_linear.weight"]).T + _f64(w["proj_linear.bias"])
    return logit, h2, c2, ctx, alpha


def _teacher_forced(step, lsm, dtype, enc, keys, h, c, lens, targets, tgt_len, dec_sd, sos, eos, feed_len):
    targets = np.asarray(targets, np.int64)
    tgt_len = np.asarray(tgt_len, np.int64)
    feed_len = tgt_len if feed_len is None else np.asarray(feed_len, np.int64)
    B, L = targets.shape
    rows = np.arange(B)
    out = dict(token_logp=np.zeros((B, L), dtype), mean_logp=np.zeros((B, L), dtype),
               best_logp=np.zeros((B, L), dtype), alignment=np.zeros((L, enc.shape[0], B), dtype))
    ctx = np.zeros((B, enc.shape[2]), dtype)
    tok = np.full(B, sos, np.int64)
    for l in range(L):
        logit, h, c, ctx, alpha = step(enc, lens, keys, tok, h, c, ctx, dec_sd)
        lp = lsm(logit)
        live = l < tgt_len
        out["alignment"][l] = alpha
        out["token_logp"][:, l] = np.where(live, lp[rows, targets[:, l]], 0)
        # (sum_v logit_v) / V - logsumexp = the mean of the log-softmax row
        out["mean_logp"][:, l] = np.where(live, lp.mean(axis=1, dtype=F64), 0)
        out["best_logp"][:, l] = np.where(live, lp.max(axis=1), 0)
        tok = np.where(l < feed_len, targets[:, l], eos)
    return out


def teacher_forced(enc, keys, h, c, lens, targets, tgt_len, dec_sd, sos=1, eos=2, feed_len=None):
    """The decoder fed a given transcript (model.py:405-469): step l feeds sos (l = 0) or
    targets[b, l - 1], and scores targets[b, l].  Positions l >= tgt_len[b] are not scored (their
    token_logp / mean_logp / best_logp are 0); steps past feed_len[b] (default tgt_len) feed eos.
    Returns dict(token_logp, mean_logp, best_logp [B, L], alignment [L, T, B]), float64.
    mean_logp = (sum_v logit_v) / V - logsumexp, the label-smoothing term (util.py:265-279)."""
    return _teacher_forced(decoder_step, log_softmax, F64, _f64(enc), _f64(keys), _f64(h), _f64(c), lens,
                           targets, tgt_len, dec_sd, sos, eos, feed_len)


def oracle32_teacher_forced(O, enc, keys, h, c, lens, targets, tgt_len, dec_sd, sos=1, eos=2, feed_len=None):
    """The same pass through the float32 numpy oracle O (its decoder_step and _log_softmax, looked
    up at call time): budget()'s ref32 for the decode stages."""
    mask = O.mask_for_softmax(np.asarray(lens), enc.shape[0])

    def step(enc, lens, keys, tok, h, c, ctx, sd):
        return O.decoder_step(enc, mask, keys, tok, h, c, ctx, sd)

    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return _teacher_forced(step, O._log_softmax, np.float32, f32(enc), f32(keys), f32(h), f32(c), lens,
                           targets, tgt_len, dec_sd, sos, eos, feed_len)


# --------------------------------------------------------------------------------------
# the budget
# --------------------------------------------------------------------------------------
M_DEFAULT = 8
"""The margin, on both the maximum and the rms error, for every stage and both arithmetics: a
candidate may be M times as far from the float64 truth as the float32 numpy oracle is on the same
stage inputs.  It is measured against that reference error, never against the device.  Two
independent valid float32 evaluations (numpy / BLAS and torch CPU) differ by at most 2.2x from each
other here; a strict k-order float32 chain is 3x the s16x3 error in the project's own dot-product
probe (DESIGN 3.0: 2.6e-7 against 8.8e-8); DESIGN 3.3 states 3e-7 for the fast tanh against about
6e-8 for libm, 5x.  Eight covers the largest of these, and test_accuracy_budget_host.py shows that
it rejects every seeded defect (the mildest sits at 45x)."""


def figures(candidate, truth64, ref32, valid=None):
    """Errors of candidate and ref32 against truth64 over the valid elements: dict(max_ratio,
    rms_ratio, e_ref_max, e_ref_rms, e_max, e_rms).  A ratio is 0 when the candidate's error is 0,
    inf when only the reference's is."""
    cand, truth, ref = _f64(candidate), _f64(truth64), _f64(ref32)
    assert cand.shape == truth.shape == ref.shape, (cand.shape, truth.shape, ref.shape)
    valid = np.ones(cand.shape, bool) if valid is None else np.broadcast_to(np.asarray(valid, bool), cand.shape)
    assert valid.any(), "no valid element"
    ec = np.abs(cand - truth)[valid]
    er = np.abs(ref - truth)[valid]
    assert np.isfinite(truth[valid]).all() and np.isfinite(er).all(), "the reference is not finite"
    assert np.isfinite(ec).all(), "the candidate is not finite on valid elements"
    e_max, e_rms = float(ec.max()), float(np.sqrt((ec * ec).mean()))
    r_max, r_rms = float(er.max()), float(np.sqrt((er * er).mean()))
    ratio = lambda a, b: 0.0 if a == 0 else (a / b if b > 0 else float("inf"))
    return dict(max_ratio=ratio(e_max, r_max), rms_ratio=ratio(e_rms, r_rms), e_ref_max=r_max, e_ref_rms=r_rms,
                e_max=e_max, e_rms=e_rms)


def budget(candidate, truth64, ref32, M=M_DEFAULT, valid=None, pad=0.0, tag=None, extra=0.0):
    """Assert max |candidate - truth64| <= M max |ref32 - truth64| (+ extra), and the same for the
    rms, over the valid (unpadded, scored) elements; every other element of candidate must equal
    pad exactly (0; for keys b_attn, broadcast to candidate's shape).  ``extra`` is an absolute
    term for a documented design choice, derived analytically at the call site, never measured.
    With ``tag`` the figures are printed as an "[acc]" line before anything is asserted.
    Returns the figures."""
    fig = figures(candidate, truth64, ref32, valid)
    if tag is not None:
        print(f"[acc] {tag} max_ratio={fig['max_ratio']:.3f} rms_ratio={fig['rms_ratio']:.3f} "
              f"e_ref_max={fig['e_ref_max']:.3e} e_max={fig['e_max']:.3e}")
    cand = np.asarray(candidate)
    if valid is not None:
        v = np.broadcast_to(np.asarray(valid, bool), cand.shape)
        want = np.broadcast_to(np.asarray(pad, cand.dtype), cand.shape)
        assert np.array_equal(cand[~v], want[~v]), f"{tag}: padding elements differ from the pad value"
    assert fig["e_max"] <= M * fig["e_ref_max"] + extra, (tag, "max", fig)
    assert fig["e_rms"] <= M * fig["e_ref_rms"] + extra, (tag, "rms", fig)
    return fig


def mel_linear(out, mel64, valid=None):
    """A log-mel output in the linear domain: exp(out) divided, frame by frame, by that frame's
    largest float64 mel power (after the floor).  mel64: the float64 mel power of the same shape;
    with out = None, the float64 truth itself.  Elements outside ``valid`` are 0.  An error of this
    figure is relative to the frame's scale, so a bin that holds only another bin's leakage (where a
    float32 transform is off by 0.2 in the log domain) cannot set it."""
    floored = np.where(_f64(mel64) == 0, FLT_EPSILON, _f64(mel64))
    v = np.ones(floored.shape, bool) if valid is None else np.broadcast_to(np.asarray(valid, bool), floored.shape)
    scale = np.where(v, floored, 0).max(axis=-1, keepdims=True)
    lin = floored if out is None else np.exp(np.where(v, _f64(out), 0))
    return np.where(v, lin / np.where(scale > 0, scale, 1), 0)


def log_mel_budget(candidate, truth_log, truth_mel, ref32, M=M_DEFAULT, valid=None, tag=None):
    """budget() on two figures of a log-mel output, both at the same M: ``log``, the output as it
    is (padding rows exactly 0), and ``lin``, mel_linear() of candidate and ref32 against the
    float64 mel power.  Returns (figures of log, figures of lin)."""
    log = budget(candidate, truth_log, ref32, M, valid=valid, tag=None if tag is None else tag + " log")
    lin = budget(mel_linear(candidate, truth_mel, valid), mel_linear(None, truth_mel, valid),
                 mel_linear(ref32, truth_mel, valid), M, valid=valid, tag=None if tag is None else tag + " lin")
    return log, lin
