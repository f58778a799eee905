"""Float64 reference of every stage, and the accuracy budget built on it (test helper, not a
conftest; used by test_accuracy_budget_host.py, test_gpu_accuracy.py and test_gpu_accuracy_s16x1.py).

A plain numpy float64 restatement of the reference's inference path, written from the reference
lines each function cites, independently of oracle/casr_oracle.py (it imports nothing from it, so
it also cross-checks the oracle).  Every function takes its inputs as given and casts them to
float64: a stage can be fed the float32 output that the device (or the oracle) produced for the
stage before it, and then answers "what is this stage, evaluated exactly, on these inputs".  The
float32 weights are inputs like any other.

Layouts are the reference's (time-major): enc [T, B, 2H], keys [T, B, A], alignment [L, T, B].

With ``sites`` the encoder, the keys and the decoder functions evaluate the exact model of the s16x1
arithmetic instead (SITES below): both operands of each named product rounded to f16, everything
else as before; with ``dtype=np.float32`` the float32 evaluation of the same model.

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


# The s16x1 arithmetic (the build with CASR_S16_ONE, csrc/casr_common.h:68-85) has an exact model: an
# MFMA site keeps the hi.hi product of its split operands only, hi = (_Float16)x rounded to nearest
# even (split16_word, casr_common.h:38-43), every f16 x f16 product is exact in f32 and the
# accumulators are f32.  So a site computes sum_k f16(a_k) f16(b_k), and the model of a stage is the
# stage with both operands of each such product rounded to f16.  The sites, each read from the kernel:
#   enc_ih    encoder input projection, every layer (gemm16.hip:119, :279, :579, :798, :951; the cross
#             MFMAs behind kS16Cross are compiled out): A is the row image of the layer input, written
#             by features.hip:333 (layer 0) and by the recurrence from the residual sum y = h + x
#             (recurrence.hip:354-361) for the layers after it; W_ih's image is the host's
#             (casr_capi.hip:81-118).  The residual itself adds the unrounded f32 input.
#   enc_hh    the recurrent product, persistent and per-step kernels alike: the hand-off granule of h
#             is its split word (recurrence.hip:53-61), W_hh the host image.
#   keys      enc (encoder.hip:371, :639) and W_enc.
#   cell_emb  the embedding columns of the LSTMCell GEMM of the three-launch step: the A row is
#             [emb16 | ctx16 | h16] (decoder.hip:131, :649 emb16, :680) against dec_w16.
#   cell_ch   its [ctx | h] columns (the state row's split words: attention.hip:850-867 ctx,
#             decoder.hip:773 / attention.hip:311, :417 h, decoder.hip:1173 at step 0).  The folded
#             step's GEMM contracts the same [ctx16 | h16] with the same dec_w16 k blocks
#             (fold_image_kernel, decoder.hip:1074-1083); its embedding part is the f32 table
#             emb_gates (fold_emb_gates_kernel, decoder.hip:1089-1115: an fmaf chain on the f32
#             images), which is not rounded.
#   proj      [h | ctx] and W_p (ProjA, decoder.hip:800-808, proj_w16).  The one-accumulator form
#             multiplies a_hi by w_hi 2^11 (decoder.hip:338-341), exact in f16 while |w| < 16: the same
#             values.
#   query     q = h W_hidden as an s16 MFMA: the folded beam step only (attention.hip:422-434, B
#             operand fold_wq16_kernel, decoder.hip:1120-1130).  The three-launch step forms q from the
#             f32 h tile and f32 W_hidden with the exact-f32 MFMA (DecLstmEpi::run, decoder.hip:781-790)
#             and the folded greedy step with an fmaf chain (attention.hip:316-331): neither is rounded.
# Never rounded: biases, the cell nonlinearities, scores / softmax / context (VALU f32), log-softmax,
# the sums over steps.  A decode's step 0 is the three-launch LSTMCell and attention on every path
# (run_greedy_fold, decoder.hip:1781: decode_step(.., proj = false)); the folded forms start at
# step 1.  A name with "@0" holds at step 0 only, with "@1+" from step 1 on (teacher_forced).
SITES_X1_ENCODER = frozenset({"enc_ih", "enc_hh", "keys"})
SITES_X1_THREE_LAUNCH = frozenset({"cell_emb", "cell_ch", "proj"})
SITES_X1_FOLD_GREEDY = frozenset({"cell_emb@0", "cell_ch", "proj"})
SITES_X1_FOLD_BEAM = frozenset({"cell_emb@0", "cell_ch", "proj", "query@1+"})
SITE_NAMES = frozenset({"enc_ih", "enc_hh", "keys", "cell_emb", "cell_ch", "proj", "query"})


def round_f16(x):
    """the s16x1 operand rounding: to f16, nearest even (split16_word's hi half)"""
    return np.asarray(x).astype(np.float16)


def _op(x, site, sites, dtype, weight=False):
    """x as an operand of the product ``site``: through f16 if the site is named, widened to dtype.
    The contracted index is x's last axis for an activation.  ``sites`` is a set of names, or (the
    host tests' seeded defects) a dict name -> fn(x, weight) that stands in for the rounding."""
    if sites is not None and site in sites:
        x = sites[site](x, weight) if isinstance(sites, dict) else round_f16(x)
    return np.asarray(x, dtype=dtype)


def _mm(a, b):
    """every product that is an MFMA site on the device (the host tests swap in another k order)"""
    return a @ b


def step_sites(sites, l):
    """The plain site names that hold at decode step l ("@0": step 0 only, "@1+": from step 1 on);
    a dict keeps its values"""
    if sites is None:
        return None
    out = {}
    for s in sites:
        name, _, when = s.partition("@")
        assert name in SITE_NAMES and when in ("", "0", "1+"), s
        if when == "" or (when == "0") == (l == 0):
            out[name] = sites[s] if isinstance(sites, dict) else None
    return out if isinstance(sites, dict) else frozenset(out)


def _lstm_scan(gx, w_hh, b_hh, reverse, sites=None, dtype=F64):
    """One direction of an nn.LSTM layer over one sequence.  gx [T, 4H] = x W_ih^T + b_ih; gate
    order i, f, g, o; c' = f c + i g, h' = o tanh(c').  Returns (y [T, H] in time order, h, c).
    Site enc_hh: h and W_hh of the recurrent product (the state h itself stays unrounded)."""
    T = gx.shape[0]
    H = w_hh.shape[1]
    w_hh = _op(w_hh, "enc_hh", sites, dtype, True)
    h = np.zeros(H, dtype)
    c = np.zeros(H, dtype)
    y = np.zeros((T, H), dtype)
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        g = gx[t] + (_mm(w_hh, _op(h, "enc_hh", sites, dtype)) + b_hh)
        i, f, o = _sigm(g[:H]), _sigm(g[H:2 * H]), _sigm(g[3 * H:])
        c = f * c + i * np.tanh(g[2 * H:3 * H])
        h = o * np.tanh(c)
        y[t] = h
    return y, h, c


def encoder(feats, lens, enc_sd, num_layers=4, residual=True, sites=None, dtype=F64):
    """RNNEncoder.forward (encoder.py:36-81) over RNN_RES.forward (util.py:1223-1324): packed
    bidirectional single-layer LSTMs (each utterance runs over exactly its own length, the
    backward direction from its own last frame), the layer input added to the layer output from
    the second layer on (util.py:1284-1291), final state = the last layer's [fw || bw]
    (encoder.py:67-72).  feats: B arrays [>= lens[b], D].  One utterance at a time, which is what
    packing means.  Returns (enc [Tmax, B, 2H] zero past each length, h [B, 2H], c [B, 2H]).
    Sites enc_ih (the layer input, for layers >= 1 the residual sum, and W_ih) and enc_hh; the
    residual adds the unrounded input."""
    lens = [int(n) for n in lens]
    B = len(feats)
    w = {k: np.asarray(v, dtype=dtype) for k, v in enc_sd.items()}
    H = w["rnn.rnn.0.weight_hh_l0"].shape[1]
    enc = np.zeros((max(lens), B, 2 * H), dtype)
    hN = np.zeros((B, 2 * H), dtype)
    cN = np.zeros((B, 2 * H), dtype)
    w_ih = {k: _op(v, "enc_ih", sites, dtype, True) for k, v in w.items() if "weight_ih" in k}
    for b in range(B):
        x = np.asarray(feats[b], dtype=dtype)[:lens[b]]
        for i in range(num_layers):
            y = np.zeros((lens[b], 2 * H), dtype)
            xin = _op(x, "enc_ih", sites, dtype)
            for d, suf in enumerate(("", "_reverse")):
                p = f"rnn.rnn.{i}."
                gx = _mm(xin, w_ih[p + "weight_ih_l0" + suf].T) + w[p + "bias_ih_l0" + suf]
                y[:, d * H:(d + 1) * H], hN[b, d * H:(d + 1) * H], cN[b, d * H:(d + 1) * H] = _lstm_scan(
                    gx, w[p + "weight_hh_l0" + suf], w[p + "bias_hh_l0" + suf], reverse=(d == 1), sites=sites,
                    dtype=dtype)
            x = x + y if (residual and i > 0) else y
        enc[:lens[b], b] = x
    return enc, hN, cN


# --------------------------------------------------------------------------------------
# decoder
# --------------------------------------------------------------------------------------
def compute_keys(enc, dec_sd, sites=None, dtype=F64):
    """BauAttn.compute_key_value (attention.py:67-78): keys = enc W_enc + b_attn at every time slot
    (a zero padding row gives exactly b_attn); the values are enc itself (map_enc False).
    Site keys: enc and W_enc."""
    return (_mm(_op(enc, "keys", sites, dtype), _op(dec_sd["attn_mechanism.W_enc"], "keys", sites, dtype, True))
            + np.asarray(dec_sd["attn_mechanism.b_attn"], dtype=dtype))


def log_softmax(logit, dtype=F64):
    logit = np.asarray(logit, dtype=dtype)
    m = logit.max(axis=-1, keepdims=True)
    return logit - (m + np.log(np.exp(logit - m).sum(axis=-1, keepdims=True)))


class _Prepared(dict):
    """the decoder's weights as decoder_step contracts them under one set of sites and one dtype"""


def prepare_decoder(dec_sd, sites=None, dtype=F64):
    """The weight operands of decoder_step, rounded once where their site is named (the same values
    decoder_step forms from the plain state dict)."""
    if isinstance(dec_sd, _Prepared):
        return dec_sd
    E = dec_sd["embedding.weight"].shape[1]
    w_ih = np.asarray(dec_sd["cell.cell.0.weight_ih"], dtype=dtype)
    if sites is not None and ("cell_emb" in sites or "cell_ch" in sites):
        w_ih = np.concatenate([_op(w_ih[:, :E], "cell_emb", sites, dtype, True),
                               _op(w_ih[:, E:], "cell_ch", sites, dtype, True)], axis=1)
    f = lambda name: np.asarray(dec_sd[name], dtype=dtype)
    return _Prepared(
        sites=sites, dtype=dtype, emb=f("embedding.weight"), w_ih=w_ih, b_ih=f("cell.cell.0.bias_ih"),
        w_hh=_op(dec_sd["cell.cell.0.weight_hh"], "cell_ch", sites, dtype, True), b_hh=f("cell.cell.0.bias_hh"),
        w_hidden=_op(dec_sd["attn_mechanism.W_hidden"], "query", sites, dtype, True), v=f("attn_mechanism.v"),
        w_p=_op(dec_sd["proj_linear.weight"], "proj", sites, dtype, True), b_p=f("proj_linear.bias"))


def decoder_step(enc, lens, keys, token, h, c, ctx_prev, dec_sd, sites=None, dtype=F64):
    """RNNDecoder.forward (decoder.py:94-137), one step for R rows: input feeding x = [embed(token)
    || previous context], the LSTMCell (util.py:1650-1661), Bahdanau attention e_t = v . tanh(key_t
    + h W_hidden) with -inf added past each length before the softmax over time (attention.py:91-95,
    util.py:131-142), context = sum_t alpha_t enc_t, logit = proj([h || context]).
    enc [T, R, C], keys [T, R, A], lens [R].  Returns (logit [R, V], h, c, ctx, alpha [T, R]).
    Sites (plain names, see SITES above): cell_emb, cell_ch, query, proj.  dec_sd may be the result
    of prepare_decoder (its sites and dtype then hold)."""
    w = prepare_decoder(dec_sd, sites, dtype)
    sites, dtype = w["sites"], w["dtype"]
    cast = lambda a: np.asarray(a, dtype=dtype)
    enc, keys, h, c, ctx_prev = cast(enc), cast(keys), cast(h), cast(c), cast(ctx_prev)
    T, R, _ = enc.shape
    Hd = h.shape[1]
    x = np.concatenate([_op(w["emb"][np.asarray(token)], "cell_emb", sites, dtype),
                        _op(ctx_prev, "cell_ch", sites, dtype)], axis=1)
    g = (_mm(x, w["w_ih"].T) + w["b_ih"]
         + _mm(_op(h, "cell_ch", sites, dtype), w["w_hh"].T) + w["b_hh"])
    i, f, o = _sigm(g[:, :Hd]), _sigm(g[:, Hd:2 * Hd]), _sigm(g[:, 3 * Hd:])
    c2 = f * c + i * np.tanh(g[:, 2 * Hd:3 * Hd])
    h2 = o * np.tanh(c2)
    q = _mm(_op(h2, "query", sites, dtype), w["w_hidden"])
    e = np.tanh(keys + q[None]) @ w["v"]                                  # [T, R]
    live = np.arange(T)[:, None] < np.asarray(lens)[None, :]
    e = np.where(live, e, -np.inf)
    p = np.exp(e - e.max(axis=0, keepdims=True))
    alpha = p / p.sum(axis=0, keepdims=True)
    ctx = np.einsum("tr,trc->rc", alpha, enc)
    logit = _mm(_op(np.concatenate([h2, ctx], axis=1), "proj", sites, dtype), w["w_p"].T) + w["b_p"]
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


def teacher_forced(enc, keys, h, c, lens, targets, tgt_len, dec_sd, sos=1, eos=2, feed_len=None, sites=None,
                   dtype=F64):
    """The decoder fed a given transcript (model.py:405-469): step l feeds sos (l = 0) or
    targets[b, l - 1], and scores targets[b, l].  Positions l >= tgt_len[b] are not scored (their
    token_logp / mean_logp / best_logp are 0); steps past feed_len[b] (default tgt_len) feed eos.
    Returns dict(token_logp, mean_logp, best_logp [B, L], alignment [L, T, B]), of dtype.
    mean_logp = (sum_v logit_v) / V - logsumexp, the label-smoothing term (util.py:265-279).
    sites: one of the SITES_X1_* decode paths (names with "@0" / "@1+" hold at those steps only)."""
    prepared = [prepare_decoder(dec_sd, step_sites(sites, l), dtype) for l in (0, 1)]
    at = iter(range(np.asarray(targets).shape[1]))

    def step(enc, lens, keys, tok, h, c, ctx, sd):
        return decoder_step(enc, lens, keys, tok, h, c, ctx, prepared[min(next(at), 1)])

    cast = lambda a: np.asarray(a, dtype=dtype)
    return _teacher_forced(step, lambda x: log_softmax(x, dtype), dtype, cast(enc), cast(keys), cast(h), cast(c),
                           lens, targets, tgt_len, dec_sd, sos, eos, feed_len)


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
