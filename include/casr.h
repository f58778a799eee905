/*
 * casr.h — C ABI of the MI355X (gfx950) inference path for the shawnthu/chinese-asr
 * attention seq2seq model: fbank features -> 4-layer BiLSTM encoder -> Bahdanau
 * attention -> LSTM decoder -> greedy / beam-search decode loop.
 *
 * The reference has no FFI: its boundary is the Python method surface of `Model`
 * (model.py:18-987) and `main.py` (main.py:27-102).  Each entry point below names the
 * reference function it replaces; the Python host layer (chinese-asr_amd/model.py,
 * main.py, data.py) binds them with ctypes and keeps the reference signatures.
 *
 * Conventions
 *   - every function returns CASR_OK (0) or an error code; casr_last_error() explains;
 *   - all tensor arguments are DEVICE pointers owned by the caller, float32 / int32,
 *     C-contiguous, unless a comment says "host";
 *   - `stream` is a hipStream_t passed as void*; no call synchronises the host except
 *     where noted (the beam/greedy calls return after enqueueing);
 *   - one handle per device; a handle is not thread-safe; workspaces are owned by the
 *     handle and grow on demand (first call at a new size allocates).
 *
 * The stream contract (tests/test_gpu_streams.py holds every entry that takes a `stream` to it, on a
 * caller's own non-blocking stream; tests/stream_cases.py has the cases)
 *   - Order.  A call's device work, whatever it launches, copies or replays and on whichever stream of
 *     its own (the graph replays run on the handle's private streams, fenced by events both ways), is
 *     ordered after everything already enqueued on `stream`, and its results are visible to everything
 *     enqueued on `stream` afterwards.  So inputs may still be in the making on `stream` when the call
 *     is issued, outputs may be consumed on `stream` without a host synchronisation in between, and an
 *     input buffer may be overwritten on `stream` right after the call.  The legacy null stream is a
 *     valid `stream`.
 *   - Host synchronisation.  Three entries wait for `stream`: casr_lm_estimate and casr_lm_prune
 *     (synchronous: they return with the result on the host) and casr_device_flags (it returns the
 *     words).  Every other entry returns after enqueueing once it is warm.
 *   - First use.  The first call at a new size, rate, precision or graph mode may allocate or free a
 *     workspace, capture a graph, or build and upload a table or a weight image (the f32 folded image
 *     and the guard words on the null stream, which the call then waits for; a resample table from
 *     pageable host memory on `stream`).  Any of these may wait for the device, `stream` included; none
 *     changes the order above, and a guard bit raised by a handle's very first call is not lost.  A
 *     repeated call at a size, rate and mode already seen does none of it.
 *   - One handle, one stream at a time.  A handle's workspaces, its encode and beam state, its guard
 *     words and the events that fence its graph replays are shared by all its calls and are not
 *     versioned per stream: calls on one handle must be issued on one stream, or be ordered by the
 *     caller (the second stream waits for an event recorded on the first after the earlier call).
 *     Nothing orders two calls of one handle on two unordered streams.  For work in flight side by side
 *     use one handle per stream (casr.pipeline.StreamPipeline); handles share nothing but what is
 *     immutable: the packed weight blob and the casr_lm, casr_bias and casr_grammar objects, which any
 *     number of handles may read on any streams at once.
 */
#ifndef CASR_H
#define CASR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CASR_API_VERSION 3
#define CASR_MAX_LAYERS 8

enum {
  CASR_OK = 0,
  CASR_ERR_ARG = 1,         /* bad argument / shape */
  CASR_ERR_HIP = 2,         /* HIP runtime error */
  CASR_ERR_STATE = 3,       /* call order (e.g. decode before encode, no weights) */
  CASR_ERR_UNSUPPORTED = 4  /* configuration this build does not implement */
};

typedef struct casr_handle casr_handle;

/* Frozen `gpd` values (gpd.py:13-125), bound at import time in the reference
 * (encoder.py:17-24, decoder.py:11-16, attention.py:21).
 * Six dimensions are fixed by the build (n_mels, feat_dim, enc_hidden, dec_hidden, embed_dim, attn_size:
 * any other value is CASR_ERR_UNSUPPORTED).  The rest is open: enc_layers 1..CASR_MAX_LAYERS, residual 0 / 1,
 * vocab >= 4 (not a multiple of 4 too), max_len >= 1, sos and eos any ids of the vocabulary,
 * temperature > 0; outside these CASR_ERR_ARG.  The suite holds each of them to the float64 accuracy
 * budget at the values where the plans or the kernels branch (tests/test_gpu_configs.py).  Two calls depend on the vocabulary: casr_score needs vocab <= 5120
 * (CASR_ERR_UNSUPPORTED beyond), and a beam width k needs 2k <= vocab (casr_beam). */
typedef struct casr_config {
  int32_t n_mels;      /* 80   gpd['n_mels'] */
  int32_t feat_dim;    /* 720  encoder.py:19 (n_mels * 3 * 3) */
  int32_t enc_hidden;  /* 256  gpd['encoder_hidden_size'] */
  int32_t enc_layers;  /* 4    gpd['encoder_num_layers'] */
  int32_t residual;    /* 1    gpd['residual'] (util.py:1284) */
  int32_t dec_hidden;  /* 512  gpd['decoder_hidden_size'] (must be 2*enc_hidden) */
  int32_t embed_dim;   /* 256  gpd['embed_dim'] */
  int32_t attn_size;   /* 128  gpd['attn_size'] */
  int32_t vocab;       /* 5004 decoder.py:12 real_vcb_sz */
  int32_t max_len;     /* 40   gpd['max_len'] */
  int32_t sos;         /* 1 */
  int32_t eos;         /* 2 */
  float temperature;   /* gpd['temperature'], model.py:834 (beam only: casr_greedy and casr_score give the
                          same bits at every temperature) */
} casr_config;

/* HOST pointers to the reference state-dict tensors, in their reference layouts
 * (Model.save, model.py:347-355).  [l][0] = forward, [l][1] = `_reverse`. */
typedef struct casr_weights_host {
  const float* enc_w_ih[CASR_MAX_LAYERS][2]; /* rnn.rnn.{l}.weight_ih_l0{,_reverse} [4H][Din] */
  const float* enc_w_hh[CASR_MAX_LAYERS][2]; /* rnn.rnn.{l}.weight_hh_l0{,_reverse} [4H][H]   */
  const float* enc_b_ih[CASR_MAX_LAYERS][2]; /* rnn.rnn.{l}.bias_ih_l0{,_reverse}   [4H]      */
  const float* enc_b_hh[CASR_MAX_LAYERS][2]; /* rnn.rnn.{l}.bias_hh_l0{,_reverse}   [4H]      */
  const float* embedding;      /* embedding.weight       [V][E]           decoder.py:30 */
  const float* dec_w_ih;       /* cell.cell.0.weight_ih  [4Hd][E+C]       util.py:1629  */
  const float* dec_w_hh;       /* cell.cell.0.weight_hh  [4Hd][Hd]                      */
  const float* dec_b_ih;       /* cell.cell.0.bias_ih    [4Hd]                          */
  const float* dec_b_hh;       /* cell.cell.0.bias_hh    [4Hd]                          */
  const float* proj_w;         /* proj_linear.weight     [V][Hd+C]        decoder.py:50 */
  const float* proj_b;         /* proj_linear.bias       [V]                            */
  const float* attn_w_enc;     /* attn_mechanism.W_enc   [C][A]           attention.py:28 */
  const float* attn_b;         /* attn_mechanism.b_attn  [A]                            */
  const float* attn_w_hidden;  /* attn_mechanism.W_hidden [Hd][A]                       */
  const float* attn_v;         /* attn_mechanism.v       [A]                            */
} casr_weights_host;

int casr_api_version(void);

/* Packed weight blob (kernel layouts: gate-interleaved LSTM rows, MFMA-fragment-major
 * decoder matrices, transposed attention key matrix).  Replaces Model.load's
 * load_state_dict (model.py:357-370): pack once on the host, upload / broadcast the
 * blob (RCCL over xGMI for multi-GPU), then bind it on each device. */
size_t casr_packed_weights_floats(const casr_config* cfg);
int casr_pack_weights(const casr_config* cfg, const casr_weights_host* w, float* packed_host);

int casr_create(const casr_config* cfg, int device, casr_handle** out);
/* Bind a device copy of the packed blob (not copied; must outlive its use).  The blob must hold
 * casr_packed_weights_floats(cfg) floats: the library checks the layout stamp casr_pack_weights
 * writes (magic + size) and refuses (CASR_ERR_ARG) a blob packed by another layout. */
int casr_bind_weights(casr_handle* h, const float* packed_device);
void casr_destroy(casr_handle* h);
const char* casr_last_error(const casr_handle* h); /* h may be NULL: last global error */

/* Feature post-processing of a batch of log-mel / fbank frames (data.py:226-249 +
 * main.py:37 CMVN): 9-tap delta / delta-delta (add_delta_deltas, data.py:129-164),
 * 3-frame stacking to feat_dim, per-utterance per-dimension (x-mean)/(std_unbiased+eps).
 *   fbank    [B][T][n_mels]    frames [B] (valid frames per utterance, <= T)
 *   feat     [B][Tp][feat_dim] with Tp = T/3; rows past frames[b]/3 are zero
 *   feat_len [B] = frames[b]/3
 * eps < 0 skips CMVN (the stacked features get_log_mel itself returns). */
int casr_features(casr_handle* h, const float* fbank, const int32_t* frames, int B, int T,
                  float eps, float* feat, int32_t* feat_len, void* stream);

/* wav -> log-mel (get_log_mel data.py:167-224, inference: no dither / augmentation):
 * pre-emphasis (data.py:201-202), |STFT|^2 with n_fft 512, hop 160, periodic hann(400)
 * centred, center=False (data.py:205-221), mel filterbank (MelScale, create_fb_matrix
 * data.py:21-106, incl. the linspace(80, 7600, 257) bin quirk), eps floor and log
 * (data.py:223-224).
 *   wav       [B][n_max] float32 samples (soundfile float32 scale), n_samples [B] int32
 *   fbank     [B][t_max][80] log-mel, rows past frames[b] zero
 *   frames    [B] = 1 + (n_samples[b] - 1 - 512) / 160  (0 and device flag 64 when
 *             n_samples[b] < 513, where torch.stft raises, data.py:204)
 * t_max must be >= casr_log_mel_frames(n_max).  Any n_max > 0 is accepted: below 513 no row
 * holds a frame, wav is not read, every frames[b] is 0, fbank is all zeros and flag 64 is set.
 * preemphasis must be > 0 (the reference's value is 0.97): at preemphasis <= 0 the reference
 * skips the filter and keeps all n samples (data.py:201-202), which is another operation (no
 * one-sample shift, 1 + (n - 512) / 160 frames) and is not implemented; CASR_ERR_ARG, nothing
 * is launched or written. */
int casr_log_mel(casr_handle* h, const float* wav, const int32_t* n_samples, int B, int n_max, int t_max,
                 float preemphasis, float* fbank, int32_t* frames, void* stream);

/* Frames casr_log_mel produces for an utterance of n samples (0 if n < 513).  Host only. */
int casr_log_mel_frames(int n_samples);

/* The mel filterbank [n_stft][n_mels] casr_log_mel uses (create_fb_matrix, data.py:21-57,
 * float32).  Equal bit for bit to the matrix torch builds for the reference: linspace's
 * start + step i is one fused rounding and log10 the correctly rounded one, as torch's are
 * (a weight follows the last bit of the mel points).  Host only, no device needed. */
int casr_mel_filterbank(int n_stft, float f_min, float f_max, int n_mels, float* fb_host);

/* Any-rate, any-channel-count PCM -> the 16 kHz mono samples casr_log_mel takes: the reference's
 * convert_audio (main.py:19-24: ffmpeg -sample_fmt s16 -ar 16000 -ac 1, then sox --norm=-1) on the
 * device.  The operation is DEFINED BY THE FORMULAS BELOW, not by those tools' output: parity with
 * swresample or sox bit for bit is not claimed (their filters differ, and sox dithers at random by
 * default).  Per utterance, n frames of ch interleaved float32 channels at the integer rate
 * `rate_in` go through four stages in order:
 *  (a) downmix   x[i] = (sum_c pcm[i][c]) (1/ch): an f32 sum in ascending channel order, times 1/ch
 *                rounded to f32 (stereo: ffmpeg's 0.5 / 0.5).  ch in 1..8.
 *  (b) resample  polyphase windowed sinc.  g = gcd(16000, rate), L = 16000/g, M = rate/g;
 *                c = 0.94 min(1, L/M), hw = 32/c, K = ceil(hw): 2K taps per phase.  Output m:
 *                pos = m M (64-bit), base = pos div L, p = pos mod L,
 *                  y[m] = sum_{j=-K+1..K} tab[p][j] x[base + j],  x = 0 outside [0, n),
 *                one f32 fma chain in ascending j.  tab[p][j] = h_j / sum_j h_j (unit DC gain in
 *                every phase) with u = p/L - j, sinc(t) = sin(pi t)/(pi t) and
 *                  h(u) = c sinc(c u) I0(9 sqrt(1 - (u/hw)^2)) / I0(9) for |u| < hw, else 0,
 *                computed in float64 on the host and rounded to f32 once.  n_out = ceil(n L / M).
 *                rate_in = 16000 is an exact pass-through of (a): no filter, equal bit for bit.
 *                Measured in float64 on 0.5 s tones: error against the analytic 16 kHz
 *                tone <= -95 dB at 1, 3 and 6 kHz (-45 dB at 7 kHz, inside the 0.94 roll-off),
 *                aliases and images <= -90 dB.
 *  (c) quantise  (quantize != 0)  q = clamp(rint(y 32768), -32768, 32767), ties to even, NaN -> 0:
 *                ffmpeg's -sample_fmt s16 without dither; the value passed on is q (wav = q/32768).
 *                quantize = 0 skips the stage and y passes on.
 *  (d) normalise (norm_db < 0; a value >= 0 switches the stage off)  peak = max_m |v_m| over the
 *                utterance's n_out values.  quantize: g = float32(32768 10^(norm_db/20)) /
 *                float32(peak_int), ONE correctly rounded f32 division; out_int =
 *                clamp(rintf(float32(q) g)) (the product rounded to f32 on its own) and wav =
 *                out_int/32768.  quantize = 0: wav = y g with g = float32(10^(norm_db/20)) / peak
 *                (a NaN sample takes no part in the peak).  peak = 0 (silence, n = 0): g = 1.
 *                The peak is an integer maximum (of |q|, or of the bit pattern of |y|): no float
 *                atomics, results do not depend on scheduling.
 *   pcm   [B][n_max_in][channels] float32, n_in [B] int32 (frames per utterance)
 *   wav   [B][m_max] float32: exactly zero past n_out[b];  n_out [B] int32;  gain [B] g (1 with
 *         stage (d) off), or NULL
 * All five are device pointers; one rate_in and one channel count per call.  m_max must be >=
 * casr_resample_frames(n_max_in, rate_in).  Returns after enqueueing, no host synchronisation: wav
 * and n_out feed casr_log_mel directly.  Rows of pcm past n_in[b] are never read as data; an n_in[b]
 * outside [0, n_max_in] is clamped and raises guard bit 64.  An utterance's output depends only on
 * its own samples, n_in[b], the rate and the flags: not on B, n_max_in, m_max or its neighbours.
 * The handle keeps the table of each rate it has seen (host and device; built and uploaded,
 * stream-ordered, at the first call at that rate; six rates, the oldest evicted).  Not among the
 * timed kernel classes.
 * CASR_ERR_ARG: a NULL handle, pcm, n_in, wav or n_out, B (at most 65,535), n_max_in or m_max <= 0,
 * channels outside 1..8, or m_max too short; CASR_ERR_UNSUPPORTED: rate_in outside [4000, 384000] or
 * a table L x 2K of more than 65,536 floats (e.g. 44,101 Hz; casr_last_error has the numbers).
 * Nothing is launched or written on an error. */
int casr_convert_audio(casr_handle* h, const float* pcm, const int32_t* n_in, int B, int n_max_in,
                       int channels, int rate_in, int m_max, int quantize, float norm_db,
                       float* wav, int32_t* n_out, float* gain, void* stream);

/* The resampler's design for a rate, host only, no device needed: L, M and the taps per phase (2K);
 * the f32 table [L][taps] (tab[p][j] at column j + K - 1); and n_out = ceil(n_in L / M) (-1 on a rate
 * the other two refuse, or when the count does not fit an int).  CASR_ERR_UNSUPPORTED as above,
 * CASR_ERR_ARG for a NULL output. */
int casr_resample_plan(int rate_in, int32_t* L, int32_t* M, int32_t* taps);
int casr_resample_filter(int rate_in, float* table_host);
int casr_resample_frames(int n_in, int rate_in);

/* Long recordings: cut the log-mel of a recording at its pauses into segments of at most max_frames
 * frames, which are then transcribed one by one (main.transcribe).  The reference does no segmentation
 * (its main.py takes one utterance), so, like casr_convert_audio, the operation is DEFINED BY THE
 * FORMULAS BELOW; tests/segment_ref.py restates them in numpy.  After stage (a) everything is an
 * integer: the host entry, the device and the restatement agree exactly.  Per recording, on rows
 * [0, n) of fbank, n = frames[b]:
 *  (a) level     p_j = fb[t][j] + fb[t][16 + j] + .. (ascending, f32 adds) for j = 0..15, then the fixed
 *                halving tree p_j += p_{j+8} (j < 8), then += p_{j+4}, p_{j+2}, p_{j+1};
 *                E[t] = p_0 float32(1 / n_mels) (one f32 product, never fused with the next add);
 *                q[t] = clamp(floor((E[t] + 24f) 8f), 0, 511), NaN -> 0: bins of 1/8 neper over
 *                [-24, 40).  n_mels must be a multiple of 16.
 *  (b) threshold hist = the histogram of q[0..n).  P(pct) = the smallest v with
 *                sum_{u <= v} hist[u] >= max(1, (n pct + 99) div 100) (64-bit); lo = P(pct_lo),
 *                hi = P(pct_hi); thr = lo + max(rise_min, ((hi - lo) rel_q8 + 128) >> 8), saturating at
 *                INT32_MAX; thr = 0 at n = 0.  A0[t] = q[t] >= thr.
 *  (c) filters   over maximal runs inside [0, n).  A1: every active run of A0 shorter than min_speech is
 *                cleared.  A2: on A1, every inactive run shorter than min_pause with an active frame on
 *                both sides is set (leading and trailing quiet is never filled).  The islands are the
 *                maximal active runs [a, b) of A2, each widened to [max(0, a - pad), min(n, b + pad));
 *                min_pause > 2 pad keeps widened islands apart.
 *  (d) split     per island [s, e) in order: while e - s > max_frames, the cut c in
 *                [s + min_frames, min(s + max_frames, e - min_frames)] that minimises q[c-1] + q[c], the
 *                LARGEST such c on a tie; the piece [s, c) is emitted and s = c; finally [s, e).
 *  (e) merge     greedy from the left over the pieces: a segment starts at piece i and absorbs piece j
 *                while start_j - end <= max_gap and end_j - start_i <= max_frames (the pauses in between
 *                stay inside the segment).
 * Output per recording: (start, len) per segment, ascending, disjoint, 1 <= len <= max_frames, inside
 * [0, n).  n = 0, or no active frame, gives no segment.
 * A parameter set is valid iff min_speech >= 1, pad >= 0, min_pause > 2 pad, min_frames >= 1,
 * 2 min_frames <= max_frames, max_gap >= 0, 0 <= pct_lo <= pct_hi <= 100, 0 <= rel_q8 <= 256 and
 * rise_min >= 0; anything else is CASR_ERR_ARG and nothing is launched or written. */
typedef struct casr_segment_params {
  int32_t max_frames;  /* 800  longest segment, in frames */
  int32_t min_frames;  /* 200  shortest piece a split may leave */
  int32_t min_pause;   /* 20   shortest quiet run that counts as a pause */
  int32_t min_speech;  /* 5    shortest active run that is kept */
  int32_t pad;         /* 8    frames added on each side of a speech island */
  int32_t max_gap;     /* 100  largest gap across which pieces are merged */
  int32_t pct_lo;      /* 10   percentile that gives the noise floor */
  int32_t pct_hi;      /* 95   percentile that gives the speech level */
  int32_t rel_q8;      /* 90   rise above the floor, as a fraction of hi - lo in units of 1/256 */
  int32_t rise_min;    /* 12   smallest rise above the floor, in bins */
} casr_segment_params;

/* The defaults above.  CASR_ERR_ARG for NULL.  Host only. */
int casr_segment_default_params(casr_segment_params* p);

/* An upper bound of a recording's segment count at T frames: (T + min_pause) / (min_speech + min_pause)
 * + T / min_frames (islands lie at least min_speech active and min_pause quiet frames apart, and every
 * split piece but an island's last holds at least min_frames).  -1 on invalid parameters, T < 0 or a
 * bound that does not fit an int.  Host only. */
int casr_segment_bound(int T, const casr_segment_params* p);

/* Stages (a) to (e) on the host: every pointer a HOST pointer, no GPU needed.
 *   fbank [B][T][n_mels], frames [B]
 *   seg_start, seg_len [B][s_max]; n_seg [B]; thr [B] or NULL
 * n_seg[b] is the TRUE count even when it exceeds s_max: only the first s_max entries of a row are
 * written and the rest of it is left untouched, so the caller compares.
 * CASR_ERR_ARG: a NULL required pointer (seg_start and seg_len may be NULL at s_max = 0), B or T < 0,
 * s_max < 0, invalid parameters, a frames[b] outside [0, T]; CASR_ERR_UNSUPPORTED: n_mels not a positive
 * multiple of 16. */
int casr_segment_host(const float* fbank, const int32_t* frames, int B, int T, int n_mels,
                      const casr_segment_params* p, int s_max, int32_t* seg_start, int32_t* seg_len,
                      int32_t* n_seg, int32_t* thr);

/* The same on the device, on the fbank and frames casr_log_mel wrote (n_mels is the handle's): every
 * pointer a DEVICE pointer, outputs as above with the same s_max rule.  Returns after enqueueing; needs
 * no weights and no encode.  A frames[b] outside [0, T] is clamped and raises guard bit 64; rows of fbank
 * past frames[b] are never read as data.  A recording's segments depend only on its own frames and the
 * parameters: not on B, T, s_max or its neighbours.
 * Two launches (csrc/segment.hip): the level kernel, 16 lanes per frame, writes q as uint16 into a
 * handle-owned workspace (2 B T bytes, grows on demand) and adds a per-workgroup LDS histogram to
 * [B][512] words with integer atomics (cleared per call; no float atomics: the result does not depend
 * on scheduling); the decision kernel, one workgroup per recording, streams q in tiles of 2,048 frames,
 * compacts each tile's active runs with ballots and feeds them to the run filters, the split and the
 * merge of csrc/segment_plan.h, the text casr_segment_host compiles too.  Not among the timed kernel
 * classes, never replayed as a hipGraph.
 * CASR_ERR_ARG: a NULL handle or required pointer, B outside [1, 65535], T < 1, s_max < 0 or invalid
 * parameters; CASR_ERR_UNSUPPORTED: the handle's n_mels not a multiple of 16. */
int casr_segment(casr_handle* h, const float* fbank, const int32_t* frames, int B, int T,
                 const casr_segment_params* p, int s_max, int32_t* seg_start, int32_t* seg_len,
                 int32_t* n_seg, int32_t* thr, void* stream);

/* Copy S segments of fbank [B][T][n_mels] into the padded batch casr_features and casr_encode_fbank
 * take: out [S][t_seg][n_mels], segment s = rows [seg_start[s], seg_start[s] + seg_len[s]) of recording
 * seg_src[s]; rows past the length are exactly zero; frames_out [S] = the length.  All device pointers
 * (seg_src, seg_start, seg_len [S] int32); fbank and out 16-byte aligned (dwordx4 loads and stores).
 * A seg_src[s] outside [0, B), or a range leaving [0, T) or longer than t_seg, is clamped and raises
 * guard bit 64.  Returns after enqueueing; not among the timed kernel classes.
 * CASR_ERR_ARG: a NULL argument, B, T, S or t_seg < 1, or a misaligned fbank or out. */
int casr_gather_segments(casr_handle* h, const float* fbank, int B, int T, const int32_t* seg_src,
                         const int32_t* seg_start, const int32_t* seg_len, int S, int t_seg, float* out,
                         int32_t* frames_out, void* stream);

/* The list-of-tensors boundary of Model.eval_one_batch_* (model.py:514-516): gather B
 * device rows [lens[b]][feat_dim] (utt_ptrs is a DEVICE array of B device pointers) into
 * the padded batch-major [B][Tp][feat_dim] layout. */
int casr_gather_utterances(casr_handle* h, const float* const* utt_ptrs, const int32_t* lens,
                           int B, int Tp, float* feat, void* stream);

/* RNNEncoder.forward (encoder.py:36-81, RNN_RES util.py:1223-1324) + BauAttn
 * .compute_key_value (attention.py:67-78).  feat [B][Tp][feat_dim], lens [B] (<= Tp).
 * Results stay in the handle for the following casr_greedy / casr_beam. */
int casr_encode(casr_handle* h, const float* feat, const int32_t* lens, int B, int Tp, void* stream);

/* casr_features + casr_encode in one call, from fbank [B][T][n_mels] (frames [B]): the parse()
 * chain main.py:36-53 (stacking, deltas, CMVN with eps, then RNNEncoder.forward).  The features
 * stay inside the handle: in s16x3 arithmetic the feature kernel writes the encoder's layer-0
 * split-f16 row image directly, so the f32 features never reach HBM (results equal the two-call
 * sequence bit for bit).  feat_len [B] = frames[b]/3 is also written when not NULL. */
int casr_encode_fbank(casr_handle* h, const float* fbank, const int32_t* frames, int B, int T, float eps,
                      int32_t* feat_len, void* stream);

/* Copy of the encoder results (tests / EncoderOutput): enc [B][Tp][2H] (zeros past len),
 * h_final / c_final [B][2H] (last layer [fw || bw]), keys [B][A][Tp] (any may be NULL). */
int casr_encoder_results(casr_handle* h, float* enc, float* h_final, float* c_final, float* keys,
                         void* stream);

/* Model.eval_one_batch_with_greedy decode loop (model.py:527-580) on the last encode.
 *   tokens   [B][max_len] argmax token of every executed step
 *   out_len  [B] final_lens (tokens before the first EOS, model.py:573)
 *   finished [B] 0/1, accum [B] accumulated logp (model.py:567-576)
 *   align    NULL or [max_len][Tp][B] attention weights per step (model.py:553)
 * Score = accum / (out_len + finished) is formed by the host (model.py:593).
 * Spends the last beam: its readers return CASR_ERR_STATE afterwards (casr_beam_records). */
int casr_greedy(casr_handle* h, int32_t* tokens, int32_t* out_len, uint8_t* finished, float* accum,
                float* align, void* stream);

/* Model.eval_one_batch_with_beam search loop (model.py:660-931) + first-max finalize
 * (model.py:765 / :961-972) for bmsz = k (1..16) on the last encode.
 *   best_tokens [B][max_len], best_len [B], best_score [B], steps [1] loop steps executed.
 * With length_weight the unfinished fallback adds length_weight*(l+1) (model.py:964).
 * Every step keeps 2k candidates per utterance (torch.topk over the vocabulary, model.py:863, which
 * raises for more than it holds): 2k > vocab is CASR_ERR_ARG, here and in casr_beam_lm, casr_beam_bias
 * and casr_beam_grammar, before anything is launched or any earlier result is spent. */
int casr_beam(casr_handle* h, int k, float lm_weight, float length_weight, int32_t* best_tokens,
              int32_t* best_len, float* best_score, int32_t* steps, void* stream);

/* Every finished hypothesis of the last casr_beam, for second-pass rescoring on the host
 * (parse_finished_tensors, model.py:708-765):
 *   rec_tokens [B][max_len][k][max_len] (record at step l has l tokens), rec_score
 *   [B][max_len][k], rec_valid [B][max_len][k] (0/1); order = (step, candidate rank).
 * The readers of a beam (this call, casr_beam_rescore, casr_beam_mbr, casr_beam_mbr_distances,
 * casr_beam_nbest, casr_beam_confusion, casr_beam_record_lm, casr_beam_record_bias) read the tree and the
 * records the last beam entry left in the handle's decode workspaces and leave them as they are, so any
 * number of them may follow one beam in any order.  A casr_encode, casr_encode_fbank, casr_greedy or
 * casr_score reuses those workspaces and spends the beam: every reader then returns CASR_ERR_STATE
 * until the next casr_beam, casr_beam_lm or casr_beam_bias.  A beam entry that is refused (a bad k, a
 * NULL output) leaves the last beam readable. */
int casr_beam_records(casr_handle* h, int32_t* rec_tokens, float* rec_score, uint8_t* rec_valid,
                      void* stream);

/* Teacher-forced pass over the last encode (model.py:405-469: steps with compute_logit=False, one
 * batched projection, util.py:265-279 for the loss terms).  Step l feeds sos (l = 0) or
 * targets[b][l-1], and scores targets[b][l].
 *   targets    [B][L] int32 (device), tgt_len [B] (0..L) scored positions per utterance; the caller
 *              appends eos itself where it wants it scored.  1 <= L <= max_len.
 *   token_logp [B][L]  log-softmax value of targets[b][l]; exactly 0 for l >= tgt_len[b]
 *   total_logp [B]     sum over l < tgt_len[b], added in ascending l (deterministic, no float atomics)
 *   best_token [B][L], best_logp [B][L]  NULL or: first-index argmax of the step's logits and its
 *              log-prob (each may be NULL on its own); -1 and 0 for l >= tgt_len[b]
 *   mean_logp  [B][L]  NULL or: (sum_v logit_v)/V - logsumexp  (the label-smoothing term); 0 for
 *              l >= tgt_len[b]
 *   align      NULL or [L][Tp][B] attention weights per step (the greedy alignment layout)
 * Entries of targets at l >= tgt_len[b] are never used as data: any value, negative included, gives
 * the same outputs and raises no guard bit (steps past an utterance's scored positions feed eos).
 * An id outside [0, V) at l < tgt_len[b] is clamped to 0 and reported as guard bit 1, as everywhere
 * else.  The steps are the three-launch decode step's LSTMCell GEMM and attention (the arithmetic of
 * greedy decoding with CASR_OPT_DEC_FOLD = 0), in the handle's current precision; the projection is
 * one GEMM over the L B rows of every step, which stores no logits.  Workspace (handle-owned, grows
 * on demand): (L + 1) B state rows of 10 KB plus 1 KB of row partials per scored row (118 MB at
 * B = 256, L = 40).  Never replayed as a hipGraph; the timed classes CASR_K_DEC_LSTM, _ATTENTION,
 * _PROJ and _SELECT cover its launches.  Returns after enqueueing; does not disturb the encode: a
 * greedy or beam decode after it gives the bits it gives without it.  It spends the last beam
 * (casr_beam_records), as casr_greedy does.
 * CASR_ERR_STATE before an encode or before weights are bound; CASR_ERR_ARG for a NULL handle,
 * targets, tgt_len, token_logp or total_logp, or L out of range; CASR_ERR_UNSUPPORTED when the
 * vocabulary needs more than 64 projection column blocks (V > 5120). */
int casr_score(casr_handle* h, const int32_t* targets, const int32_t* tgt_len, int L,
               float* token_logp, float* total_logp, int32_t* best_token, float* best_logp,
               float* mean_logp, float* align, void* stream);

/* A backoff n-gram language model (ARPA, the text format KenLM reads) for sentence scoring and for the
 * second pass of Model.eval_one_batch_with_beam (parse_finished_tensors, model.py:749-763; main.py:79-85)
 * on the device.  The operation is DEFINED BY THE FORMULAS BELOW: the textbook ARPA backoff query, which
 * is what KenLM evaluates.  Agreement with KenLM to float rounding is expected but NOT PINNED (KenLM is
 * not available to test against); parity bit for bit is not claimed.
 *   Model     order N in 1..4.  LM ids: 0 .. V - 1 the ASR token ids (V = cfg.vocab), V = <s>,
 *             V + 1 = </s>, V + 2 = <unk>.  Each n-gram of each order has prob (log10, f32) and backoff
 *             (f32; 0 where none is given; the top order has none).  An id with no unigram scores and
 *             matches as <unk>: it is redirected to V + 2 in every lookup, context positions included
 *             (the n-grams themselves are stored as given).  Without a <unk> unigram, <unk> is
 *             (prob -100, backoff 0), KenLM's default.
 *   Word      ctx = the up to N - 1 LM ids before w (starting with <s> under bos).  m = the largest
 *             order whose n-gram (ctx[-(m-1):], w) is in the model (the unigram always is); p = prob_m;
 *             then for j = m, m + 1, .., len(ctx) in that order: where ctx[-j:] is in the model as a
 *             j-gram, p = p + backoff(ctx[-j:]).  Every operation an f32 add, in that order.
 *   Sentence  q = (..((t_1 + t_2) + t_3).. + t_n) + t_eos: t_i the term of word i, t_eos that of </s>
 *             after the last words; f32 adds, ascending, t_1 taken as is.  bos = 0 starts from an empty
 *             context instead of <s>.
 * casr_lm_create builds the tables from HOST arrays, per order n = 1..order: count[n-1] n-grams,
 * ids[n-1] [count][n] int32 LM ids, prob[n-1] [count], backoff[n-1] [count] (NULL: zeros; the top
 * order's is not read).  Unigrams are a direct array [V + 3]; orders 2..4 open-addressing tables with
 * linear probing of 16-byte entries {uint64 key, f32 prob, f32 backoff}, capacity the power of two
 * >= 2 count; the key packs id + 1 of each word into a 16-bit field (exact, never 0; 0 = empty) and the
 * slot is the splitmix64 finaliser of the key, masked (csrc/ngram_table.h).  device >= 0 also uploads
 * the tables to that device (synchronously); device = -1 makes a host-only object: nothing is uploaded
 * and no GPU is needed.  The object is immutable: any number of handles on its device may share it,
 * from any thread.  It must outlive the work enqueued with it.
 * CASR_ERR_UNSUPPORTED: order > 4, or V + 3 > 65535.  CASR_ERR_ARG: order < 1, a NULL array, a duplicate
 * n-gram, an id outside [0, V + 3), a non-finite value (casr_last_error(NULL) says which). */
typedef struct casr_lm casr_lm;
int casr_lm_create(int device, int order, int vocab, const int64_t* count, const int32_t* const* ids,
                   const float* const* prob, const float* const* backoff, casr_lm** out);
void casr_lm_destroy(casr_lm* lm);

/* Sentence scores q [n] of tokens [n][L] (LM ids; lens [n] words each, 0..L).  An id outside
 * [0, V + 3) scores as <unk>.
 * casr_lm_score_host: every pointer a HOST pointer, any LM object, no GPU; CASR_ERR_ARG for a NULL
 * argument or a length outside [0, L].
 * casr_lm_score: every pointer a DEVICE pointer; one work item per (sentence, position) computes the
 * terms, then one per sentence adds them in ascending order: the host's bits.  An id outside
 * [0, V + 3), or a length outside [0, L] (clamped), raises guard bit 1.  L >= 1.  Returns after
 * enqueueing.  CASR_ERR_ARG: a NULL argument, an LM that is host-only or on another device, or whose
 * vocab is not the handle's.  Needs no weights and no encode.  Nothing is launched or written on an
 * error. */
int casr_lm_score_host(const casr_lm* lm, const int32_t* tokens, const int32_t* lens, int n, int L, int bos,
                       float* q);
int casr_lm_score(casr_handle* h, const casr_lm* lm, const int32_t* tokens, const int32_t* lens, int n, int L,
                  int bos, float* q, void* stream);

/* The second pass (model.py:749-763) over the finished hypotheses of the last casr_beam, on the
 * device, from the beam tree the handle still holds: no record is expanded and nothing is copied to the
 * host.  Per utterance, over its valid records in (step, rank) order, with l the record's length, q its
 * sentence score under bos and rec_score its first-pass score:
 *     comb = (double(rec_score) + lm_weight double(q)) + length_weight double(l),
 * each operation one IEEE double operation (never contracted), as the host path evaluates it on Python
 * floats.  The choice is the first maximum; if a comb is NaN the first NaN (np.argmax's rule).  An
 * utterance with no record keeps casr_beam's unfinished fallback (its own weights), bit for bit.
 *   best_tokens [B][max_len] (-1 past the length), best_len [B], best_score [B] = the chosen record's
 *   rec_score (not comb, as the host path returns)
 *   best_lm  NULL or [B]: q of the choice, 0 where the utterance has no record
 *   rec_lm   NULL or [B][max_len][k]: q of every valid record, 0 elsewhere
 * A word's term depends only on its at most 3 predecessors, so it is computed once per beam-tree node
 * (at most steps x k per utterance) and summed down the tree in f32, ascending: the sentence sum's
 * bits.  One workgroup per utterance; no float atomics; the handle's beam state is only read, so a
 * later casr_beam_records, or a second rescore, gives the same bits.  A token id outside [0, V) scores
 * as <unk> (guard bit 1); a back-pointer outside [0, k) is clamped (guard bit 16).  Never replayed as a
 * hipGraph and not among the timed kernel classes.  Returns after enqueueing.
 * CASR_ERR_STATE before casr_beam; CASR_ERR_ARG: a NULL handle, LM or required output, an LM that is
 * host-only or on another device, or whose vocab is not the handle's; CASR_ERR_UNSUPPORTED: a max_len x
 * k whose tree does not fit the LDS (64 KB: 16 max_len k + 3 KB).  Nothing is launched or written on an
 * error. */
int casr_beam_rescore(casr_handle* h, const casr_lm* lm, double lm_weight, double length_weight,
                      int32_t* best_tokens, int32_t* best_len, float* best_score, float* best_lm,
                      float* rec_lm, void* stream);

/* The term of EVERY ASR token under one context, per row: terms[i][v], v in [0, V), is the Word term
 * above of w(v) after row i's context, where w(v) = </s> for v == eos_token (pass -1 for none) and v
 * itself otherwise (redirected to <unk> without a unigram, as everywhere).  ctx [n][3]: the up to
 * three LM ids before, NEAREST FIRST, of which the first nc[i] (0 .. N - 1) are read.  An id outside
 * [0, V + 3) scores as <unk>, an nc outside [0, N - 1] is clamped; both raise guard bit 1.
 * The result is the per-word query's, bit for bit, but a row costs V sequential reads plus its
 * context's successors instead of V hash queries: casr_lm_create also builds, per order n = 2..N,
 * successor lists (csrc/ngram_succ.h): the n-grams that start with an (n - 1)-word context stored as
 * {int32 w, f32 prob}, contiguous per context and ascending in w; the context is located through a
 * direct array [V + 3] of {offset, count} at n = 2 and through an open-addressing table {uint64 key,
 * uint32 offset, uint32 count} at n = 3, 4 (the key packing, slot function and linear probing of the
 * n-gram tables; independent of them, since a context with successors need not itself be an n-gram).
 * N-grams with a word that has no unigram are left out (no redirected query reaches them).  A row:
 * (1) the context's up to three backoffs, looked up once; (2) the dense chain ((uni[w].prob + bo_1) +
 * bo_2) + bo_3 over the backoffs that exist (the m = 1 case); (3) the successors of orders 2, 3, 4 in
 * that order, each overwriting with prob_m plus the backoffs of orders >= m, so the highest order
 * wins; (4) <unk> (every token without a unigram) and </s> by one ordinary query each.
 * casr_lm_terms_host: HOST pointers, any LM object, no GPU.  casr_lm_terms: DEVICE pointers, one
 * workgroup per row, which assembles the row in LDS and writes it once; returns after enqueueing.
 * CASR_ERR_ARG: a NULL argument, n < 0, an LM that is host-only or on another device, or whose vocab
 * is not the handle's.  CASR_ERR_UNSUPPORTED: a row past the LDS it is assembled in (4 V bytes > 64 KB:
 * V > 16,384).  Nothing is launched or written on an error. */
int casr_lm_terms_host(const casr_lm* lm, const int32_t* ctx, const int32_t* nc, int n, int eos_token,
                       float* terms);
int casr_lm_terms(casr_handle* h, const casr_lm* lm, const int32_t* ctx, const int32_t* nc, int n, int eos_token,
                  float* terms, void* stream);

/* Beam search with the n-gram LM fused into the first pass (shallow fusion; the ranking the reference's
 * beam was designed for, model.py:843-857): the LM decides which hypotheses stay in the beam, not only
 * which finished one wins.  Every beam row carries two f32 sums: a, the acoustic log-probabilities
 * (exactly what casr_beam carries as its score), and g, the LM terms.  At step l, row r ranks
 * candidate v by
 *     am  = (x_v / T - lse_r) + a_r         casr_beam's value, the same bits
 *     lm  = l == 0 ? term : g_r + term      term = the Word term of v after r's up to N - 1 tokens
 *                                           before (<s> before step 0); v == eos scores </s>
 *     val = (am + lm_weight lm) + len_l     len_l = (float)((double)length_weight (double)(l + 1))
 * each operation an f32 operation rounded on its own (never contracted).  Top 2k of val per utterance,
 * ties to the lower flat index, step 0 ranking beam 0 only; the record, early-stop and active-set
 * bookkeeping is casr_beam's, on that ranking.  The chosen candidates pass on am and lm, not val: a
 * finished record stores am (casr_beam_records returns it) and lm (casr_beam_record_lm: rec_lm
 * [B][max_len][k], 0 where there is no valid record), so a record's lm is its Sentence score under bos,
 * the same adds in the same order.  The best hypothesis is the first maximum over an utterance's valid
 * records, in (step, rank) order, of (rec_score + lm_weight rec_lm) + len_l (l the record's step);
 * without a record, the first maximum over the k live rows of the same expression at the last executed
 * step.  best_score is the choice's am, best_lm its lm.  With both weights 0 every output equals
 * casr_beam's bit for bit.
 * A row's context is read off the beam tree on the device.  The decode steps are those casr_beam runs
 * at the same shape; the select is always a launch of its own (CASR_OPT_FUSE_SELECT does not apply)
 * that reads the whole logits row and the row's terms, which casr_lm_terms' kernel wrote to a handle-
 * owned workspace of R V floats just before (41 MB at R = 2,048).  It counts under CASR_K_SELECT.
 * Never replayed as a hipGraph; no float atomics; results do not depend on scheduling.  A token id
 * outside [0, V) in the tree scores as <unk> (guard bit 1), a back-pointer outside [0, k) is clamped
 * (guard bit 16).  Returns after enqueueing.
 * CASR_ERR_STATE before an encode or before weights are bound; CASR_ERR_ARG: a NULL handle, LM or
 * output, an LM that is host-only or on another device, or whose vocab is not the handle's, k outside
 * 1..16; CASR_ERR_UNSUPPORTED: V > 16,384 (a term row is assembled in 64 KB of LDS, 4 V bytes).  After
 * it, casr_beam_rescore returns CASR_ERR_STATE (its fallback assumes casr_beam's scores) until the next
 * casr_beam; casr_beam_record_lm returns CASR_ERR_STATE unless the last beam was a casr_beam_lm. */
int casr_beam_lm(casr_handle* h, const casr_lm* lm, int k, float lm_weight, float length_weight,
                 int32_t* best_tokens, int32_t* best_len, float* best_score, float* best_lm, int32_t* steps,
                 void* stream);
int casr_beam_record_lm(casr_handle* h, float* rec_lm, void* stream);

/* Estimating the n-gram LM from a token corpus: an interpolated modified-Kneser-Ney model of order N in
 * 1..4, the estimator lmplz implements.  As with casr_lm_*, the operation is DEFINED BY THE FORMULAS
 * BELOW, not by another tool's output; parity with lmplz is expected to float rounding and NOT PINNED.
 *   Input     tokens [total] int32 LM ids, offsets [n + 1] int64 ascending from 0 to total; sentence i is
 *             tokens[offsets[i] : offsets[i + 1]] and may be empty.  Ids 0 .. V - 1 and V + 2 = <unk>
 *             (counted as a word) may occur; <s> = V and </s> = V + 1 may not, they are the padding:
 *             every sentence is counted as <s> w_1 .. w_l </s>.  P = total + n positions.
 *   Counts    c_n(g), n = 1..N: the windows of n consecutive ids of the padded sentences equal to g.
 *   Adjusted  a_N = c_N; for n < N, a_n(g) = c_n(g) where g starts with <s>, else the number of
 *             distinct v with c_{n+1}(v g) > 0.  The unigram <s> takes no part in what follows.
 *   Discounts t_{n,k} = the n-grams with a_n = k (k = 1..4); Y = t1 / (t1 + 2 t2); D_n(k) = k -
 *             (((k + 1) Y) t_{k+1}) / t_k for k = 1, 2, 3.  Where t1..t4 are not all positive or some
 *             D_n(k) is not in (0, k], order n FALLS BACK to D_n = (0.5, 1, 1.5).  D(a) = D(min(a, 3)).
 *   Context   for an (n - 1)-gram c (the empty one for n = 1): S_n(c) = sum_w a_n(c w), N_k(c) = the w
 *             with min(a_n(c w), 3) = k; gamma_n(c) = ((D_n(1) N_1 + D_n(2) N_2) + D_n(3) N_3) / S_n(c).
 *   p         u = (a - D(a)) / S.  p_1(w) = u + gamma_1() / |W| with |W| the unigram types other than
 *             <s> and <unk>, plus 1; <unk> always has a unigram (u = 0 where it was never seen).
 *             p_n(w | c) = u + gamma_n(c) p_{n-1}(w | c without its first word).  All float64, every
 *             operation one IEEE operation in the order written, nothing contracted to an fma.
 *   Stored    prob = f32(log10 p); backoff of an n-gram g, n < N: f32(log10 gamma_{n+1}(g)) where
 *             something follows g in the corpus, else 0; the unigram <s> has prob -99.  Orders 2..N hold
 *             exactly the distinct windows.  An ASR id the corpus never holds gets no unigram:
 *             casr_lm_create's redirect to <unk> applies.
 * Both entries run one text (csrc/lm_estimate_plan.h); the log10 and the rounding to f32 happen on the
 * host for both, in casr_lm_estimate_arrays, so their float64 p and gamma agree bit for bit.
 * casr_lm_estimate_host: HOST pointers, no GPU; within an order the n-grams are in ascending key order
 * (= ascending id tuples).  CASR_ERR_ARG: order outside 1..4, n < 1, vocab < 1, a NULL argument, offsets
 * that do not ascend from 0, an id that is neither in [0, V) nor V + 2.  CASR_ERR_UNSUPPORTED: V + 3 >
 * 65,535, P > 2^28 (counts are 32 bits wide).
 * casr_lm_estimate: DEVICE pointers, V = the handle's vocab; needs no weights and no encode; synchronous
 * (it returns with the result on the host); the order within an order is unspecified.  Counting tables
 * of the power of two >= 2 P slots per order live in a workspace the handle keeps
 * (casr_lm_estimate_workspace_bytes); every probe loop is bounded by the capacity.  A bad id is counted
 * as <unk>, and offsets are clamped (sentence i = [clamp(offsets[i], 0, total), clamp(offsets[i + 1],
 * that start, total))); both raise guard bit 1.  Offsets that overlap so far that a table proves full
 * are refused with CASR_ERR_ARG.  Otherwise errors as the host entry, checked before anything is
 * launched (total is read from offsets[n] first).
 * casr_lm_estimate_combine: whether the count kernel combines equal keys in LDS before the global
 * atomic (default 1; the same result either way; process-wide, for measurements).  Returns the
 * previous value. */
typedef struct casr_lm_est casr_lm_est;
int casr_lm_estimate_host(int order, int vocab, const int32_t* tokens, const int64_t* offsets, int64_t n,
                          casr_lm_est** est);
int casr_lm_estimate(casr_handle* h, int order, const int32_t* tokens, const int64_t* offsets, int64_t n,
                     void* stream, casr_lm_est** est);
int casr_lm_estimate_combine(int on);
/* count [4]: n-grams per order (0 above N); discount [4][3]: D_n(1..3); fallback [4]: 1 where the order
 * fell back; n_types: |W|; positions: P.  Any output may be NULL. */
int casr_lm_estimate_info(const casr_lm_est* est, int64_t* count, double* discount, int32_t* fallback,
                          int64_t* n_types, int64_t* positions);
/* Order n's arrays, HOST outputs, any of them NULL: ids [count][n], prob and backoff [count] (what
 * casr_lm_create takes), adjusted [count] (a_n; c_1 for the unigram <s>), p_f64 [count] (0 for the
 * unigram <s>) and gamma_f64 [count] (gamma_{n+1} of the n-gram as a context; 0 where it is none).
 * casr_lm_estimate_counts: the raw counts c_n [count].  casr_lm_estimate_timing: milliseconds of the
 * device entry's stages (count, extend, stats, prob, compact, copy, 0, all); zeros from the host entry.
 * CASR_ERR_ARG: a NULL object, n outside 1..N. */
int casr_lm_estimate_arrays(const casr_lm_est* est, int n, int32_t* ids, float* prob, float* backoff,
                            int64_t* adjusted, double* p_f64, double* gamma_f64);
int casr_lm_estimate_counts(const casr_lm_est* est, int n, int64_t* raw);
int casr_lm_estimate_timing(const casr_lm_est* est, double* ms);
void casr_lm_estimate_destroy(casr_lm_est* est);
/* Bytes of casr_lm_estimate's counting tables for P positions (the plan; no GPU): -1 for an order
 * outside 1..4 or P outside [1, 2^28].  The dense result arrays (32 bytes per n-gram) come on top. */
int64_t casr_lm_estimate_workspace_bytes(int order, int64_t positions);

/* Making an n-gram LM smaller: relative-entropy pruning (Stolcke 1998; SRILM's -prune) of ANY backoff
 * model a casr_lm holds, an estimate of ours or a third party's ARPA file.  As with casr_lm_* the
 * operation is DEFINED BY THE FORMULAS BELOW, not by another tool's output.
 *   Linear    every stored value goes through P = exp10(prob), B = exp10(backoff) in float64 (lmp_exp10
 *             below).  An n-gram without a backoff has B = 1, and so has an absent context.
 *   Query     Q(w | c) is the "Word" rule above in the linear domain: m = the largest order whose n-gram
 *             (c[-(m-1):], w) is present; start from P_m; for j = m .. len(c) multiply by B(c[-j:])
 *             where that j-gram is present.  Float64 multiplications in that order.
 *   Part      an n-gram holding a word without a unigram passes through untouched: it is in no sum, is
 *             never removed, and its backoff stays as given.  Unigrams are never removed.
 *   ph        for a context h = h_1 .. h_{n-1}: ph(h) = the product over i, ascending from 1, of
 *             Q(h_i | h_1 .. h_{i-1}); where h_i = <s> the factor is P_1(</s>) (the model stores -99 for
 *             <s>; every sentence has one of each, so their marginals are equal).
 *   sum       sum(x_0 .. x_{m-1}) has one association: 64 partials s_l = x_l + x_{l+64} + .. ascending,
 *             then for d = 32, 16, 8, 4, 2, 1: s_l = s_l + s_{l+d} for l < d; the result is s_0 (0 for an
 *             empty list).  A wave computes exactly this; the host loops it.
 *   Context   for n = 2..N and every context h with order-n successors v (ascending v):
 *             num = 1 - sum P_n(h v), den = 1 - sum Q(v | h') with h' = h without its oldest word,
 *             a = B(h) as stored.
 *   Decision  for the n-gram (h, w): p = P_n(h w), q = Q(w | h'), a' = (num + p) / (den + q),
 *             dH = -ph ( (p ((L(q) + L(a')) - L(p))) + (num (L(a') - L(a))) ), L the natural log
 *             (lmp_log), every operation one IEEE operation as bracketed, nothing contracted.  Where p,
 *             q, a, num + p and den + q are not all positive and finite, dH = +inf.  With tau =
 *             L(1 + theta) the n-gram is REMOVABLE iff dH < tau (SRILM's exp(dH) - 1 < theta).
 *   Kept      orders n = N down to 2: an n-gram that is the prefix of a kept (n + 1)-gram is PROTECTED
 *             and stays (the result is prefix-closed); every other removable n-gram goes.  All decisions
 *             read the model as given; only protection couples the orders.
 *   Backoffs  if nothing was removed the output equals the input bit for bit.  Otherwise, for n = 2..N
 *             ascending, every kept (n - 1)-gram h that takes part gets B'(h) = num' / den': the sums as
 *             above over its KEPT successors (each successor keeps its place l in h's list; a removed
 *             one adds nothing), Q evaluated in the pruned model (present = kept) with the backoffs
 *             already renewed below.  B' = 1 where h has no kept successor.  Where num', den' or their
 *             quotient is not positive and finite the context is DEGENERATE: B' = 0, stored as -99.
 *   Stored    kept probs are the input's f32 bits; a renewed backoff is f32(log10 B'), 0 at the top
 *             order; the log10 and the rounding happen on the host for both entries.
 *   lmp_exp10, lmp_log: written out in csrc/lm_prune_plan.h from IEEE + - * / alone (integer range
 *             reduction, a fixed polynomial in Horner form), because two libms do not agree in the last
 *             bit: absolute error <= 1e-12 max(1, |ln x|) and relative error <= 1e-12 over [-99, 0],
 *             four orders below what f32 storage can express.
 * Both entries run one text (csrc/lm_prune_plan.h) and agree bit for bit on dH, the kept flags, B' and the
 * stored values.  casr_lm_prune_host: any LM object, no GPU; within an order the n-grams come out in
 * ascending key order.  casr_lm_prune: the LM's device copy must serve the handle (casr_lm_score's
 * rules); needs no weights and no encode; synchronous; the order within an order is unspecified; the
 * workspace (casr_lm_prune_workspace_bytes) stays with the handle.  Stages: linearise (one work item per
 * slot), decide (orders N..2, one wave per context: the two sums, then one lane per n-gram), renew
 * (orders 2..N, one wave per context), compact (one cursor add per wave).  Every probe loop is bounded
 * by the capacity; no float atomics; nothing depends on scheduling.
 * CASR_ERR_ARG: theta negative or not finite, a NULL argument; for the device entry also an LM that is
 * host-only, on another device or of another vocabulary.  Nothing is launched or written on an error. */
typedef struct casr_lm_pruned casr_lm_pruned;
int casr_lm_prune_host(const casr_lm* lm, double theta, casr_lm_pruned** out);
int casr_lm_prune(casr_handle* h, const casr_lm* lm, double theta, void* stream, casr_lm_pruned** out);
/* count_in, count_out, n_protected [4]: n-grams per order before and after, and those kept only because
 * they were protected (0 above N); n_degenerate: the degenerate contexts; tau.  Any output may be NULL. */
int casr_lm_prune_info(const casr_lm_pruned* p, int64_t* count_in, int64_t* count_out, int64_t* n_protected,
                       int64_t* n_degenerate, double* tau);
/* The KEPT n-grams of order n, HOST outputs, any NULL: ids [count_out][n], prob and backoff (what
 * casr_lm_create takes), backoff_f64 (B'; exp10 of the stored backoff where it was not renewed).
 * casr_lm_prune_decisions: EVERY n-gram of order n of the input: ids [count_in][n], delta (dH; NaN for
 * an n-gram that takes no part, unigrams included), kept.  casr_lm_prune_timing: milliseconds of the
 * device entry's stages (linearise, decide, renew, compact, copy, 0, 0, all); zeros from the host entry.
 * CASR_ERR_ARG: a NULL object, n outside 1..N. */
int casr_lm_prune_arrays(const casr_lm_pruned* p, int n, int32_t* ids, float* prob, float* backoff,
                         double* backoff_f64);
int casr_lm_prune_decisions(const casr_lm_pruned* p, int n, int32_t* ids, double* delta, uint8_t* kept);
int casr_lm_prune_timing(const casr_lm_pruned* p, double* ms);
void casr_lm_prune_destroy(casr_lm_pruned* p);
/* Bytes of casr_lm_prune's workspace for this LM (the plan; no GPU): -1 for NULL. */
int64_t casr_lm_prune_workspace_bytes(const casr_lm* lm);

/* Hotword (contextual) biasing: the caller lists phrases (names, product terms, addresses) and the beam
 * search favours hypotheses that spell them WHILE it searches.  An n-gram LM cannot do this: the words
 * that need the help are the ones its training text never saw.  The reference has no such pass; like
 * the n-gram LM and the edit distance, the operation is DEFINED BY THE FORMULAS BELOW.  All bias
 * arithmetic is int32, so the incremental device form, the host entries and a brute-force restatement
 * (tests/bias_ref.py) agree exactly, in any order of evaluation.
 *   Phrases   P >= 0 phrases; phrase p is a token sequence p[0..n_p), 1 <= n_p <= CASR_BIAS_MAX_LEN, ids
 *             in [0, V), with an int32 boost b_p in [1, 4096] in units of 1/256 nat PER TOKEN.
 *   Sequence  y[0..l) of plain int32 symbols; an id outside [0, V) matches nothing.
 *   full(y)   the sum over every phrase p and every j with y[j - n_p .. j) == p of n_p b_p.  EVERY
 *             occurrence of EVERY phrase counts, overlapping and nested ones included: listing both
 *             北京 and 北京大学 boosts the longer one by both.
 *   tail(y)   the maximum of m b_p over phrases p and 1 <= m < n_p, m <= l, with y[l - m .. l) ==
 *             p[0..m); 0 when there is none.  The credit of a match in progress; it is withdrawn when the
 *             match fails (the next step's tail no longer holds it).
 *   bias_open(y) = (float)(full(y) + tail(y)) / 256, bias_closed(y) = (float)full(y) / 256: a finished
 *             hypothesis keeps no partial credit.  The conversion is correctly rounded, the division exact.
 * Boosts <= 4096 and lengths <= 16 keep every sum below 2^31 for sequences of up to 512 tokens (a
 * position adds at most 4096 (1 + 2 + ... + 16) = 557,056; 512 of them 2.9e8).
 * casr_bias_create builds, on the host, an Aho-Corasick automaton over the phrases (csrc/bias_plan.h):
 * per node its fail link and depth, out_sum (the sum of n_p b_p over the phrases ending at the node or on
 * its fail chain), tail (the maximum over the node and its fail chain of depth x the largest b_p among
 * the phrases passing properly through) and its children ascending in token; the root's children are
 * dense arrays [V].  State 0 is the root.  tokens holds the phrases back to back, lens [n_phrases],
 * boost [n_phrases], all HOST arrays.  device >= 0 also uploads the automaton to that device
 * (synchronously); device = -1 makes a host-only object.  The object is immutable: any number of handles
 * on its device may share it, from any thread.  It must outlive the work enqueued with it.
 * CASR_ERR_ARG: a NULL array, a length, id or boost out of range, a duplicate phrase
 * (casr_last_error(NULL) says which); CASR_ERR_UNSUPPORTED: more than 2^20 tokens in total. */
#define CASR_BIAS_MAX_LEN 16
typedef struct casr_bias casr_bias;
int casr_bias_create(int device, int vocab, int n_phrases, const int32_t* tokens, const int32_t* lens,
                     const int32_t* boost, casr_bias** out);
void casr_bias_destroy(casr_bias* bias);

/* full [n], tail [n] and the final automaton state [n] (each may be NULL) of the sentences tokens
 * [n][L] with lens [n].
 * casr_bias_score_host: HOST pointers, any object, no GPU, any L >= 0; CASR_ERR_ARG for a NULL argument
 * or a length outside [0, L].
 * casr_bias_score: DEVICE pointers, one work item per sentence; a length outside [0, L] is clamped and
 * raises guard bit 1; 1 <= L <= 512, else CASR_ERR_UNSUPPORTED.  Needs no weights and no encode. */
int casr_bias_score_host(const casr_bias* bias, const int32_t* tokens, const int32_t* lens, int n, int L,
                         int32_t* full, int32_t* tail, int32_t* state);
int casr_bias_score(casr_handle* h, const casr_bias* bias, const int32_t* tokens, const int32_t* lens, int n,
                    int L, int32_t* full, int32_t* tail, int32_t* state, void* stream);

/* The dense rows of automaton states (the analogue of casr_lm_terms): for state [n], gain [n][V] int32,
 * gain[i][v] = out_sum(d) + tail(d) with d = delta(state[i], v) (what candidate v adds to the row's full
 * under bias_open), and next [n][V] (NULL or the d themselves).  delta(s, v) is the first node on s,
 * fail(s), ... (root excluded) that has child v, else the root's child; the chain has at most 16 nodes.
 * casr_bias_rows_host: HOST pointers; a state outside the automaton is CASR_ERR_ARG.
 * casr_bias_rows: DEVICE pointers, one workgroup per row: the row is assembled in LDS from the root's
 * dense arrays, the chain's children are scattered over it from the node nearest the root to the state
 * itself with a barrier between nodes, so the deepest wins, and the row is written once, coalesced.  A
 * state outside the automaton is clamped to the root and raises guard bit 1.  CASR_ERR_UNSUPPORTED: a row
 * past the LDS it is assembled in (8 V bytes > 64 KB).  CASR_ERR_ARG: a NULL argument, n < 0, an object
 * that is host-only or on another device, or whose vocab is not the handle's. */
int casr_bias_rows_host(const casr_bias* bias, const int32_t* state, int n, int32_t* gain, int32_t* next);
int casr_bias_rows(casr_handle* h, const casr_bias* bias, const int32_t* state, int n, int32_t* gain,
                   int32_t* next, void* stream);

/* Beam search with the phrase bias, and optionally the n-gram LM, in the first pass.  am, lm, len_l, the
 * top 2k, the tie rule, ranking beam 0 only at step 0, and the record, early-stop and active-set
 * bookkeeping are exactly casr_beam_lm's.  At step l, row r with tokens y_r ranks candidate v by
 *     bias = v == eos ? bias_closed(y_r) : bias_open(y_r . v)
 *     val  = ((am + lm_weight lm) + bias_weight bias) + len_l
 * each operation an f32 operation rounded on its own; with lm == NULL the lm_weight lm term is left out.
 * A row carries the integer pair (s_r, C_r), its automaton state and C_r = full(y_r): the candidate's
 * integer is C_r + gain(s_r, v) (C_r for eos), and the successor carries (delta, C_r + out_sum(delta)).
 * The chosen candidates pass on am, lm and the integer state, not val.  A record stores am, lm and
 * rec_bias = bias_closed of its tokens (casr_beam_record_bias: rec_bias [B][max_len][k] float, 0 where
 * there is no valid record).  The best hypothesis is the first maximum of the same expression over the
 * valid records in (step, rank) order; without a record, over the k live rows of the last executed step,
 * which use bias_open.  best_score is the choice's am, best_lm (NULL without an LM, else optional) its lm,
 * best_bias its bias.  With bias_weight = 0, or P = 0, every output equals casr_beam_lm's bit for bit (an
 * added +0 changes no bits that are carried); with lm == NULL as well and length_weight = 0, casr_beam's.
 * Per step the dense gain rows of the rows' states go through a handle-owned workspace of R V int32
 * (casr_bias_rows' kernel), read by the select beside the logits and the optional term rows; the
 * select's bookkeeping lanes recompute delta and out_sum of the chosen candidates from the automaton (at
 * most 32 walks per utterance).  It counts under CASR_K_SELECT.  Never replayed as a hipGraph; no float
 * atomics; results do not depend on scheduling.  Returns after enqueueing.
 * Errors and state as casr_beam_lm: CASR_ERR_STATE before an encode or before weights are bound;
 * CASR_ERR_ARG: a NULL handle, bias or required output, a bias or LM that is host-only, on another
 * device or of another vocab, k outside 1..16; CASR_ERR_UNSUPPORTED: V > 8,192 (the gain row with its
 * states is assembled in 64 KB of LDS).  After it casr_beam_rescore and casr_beam_mbr return
 * CASR_ERR_STATE until the next casr_beam; casr_beam_records works; casr_beam_record_lm works only if an
 * LM was given; casr_beam_record_bias returns CASR_ERR_STATE unless the last beam was a casr_beam_bias. */
int casr_beam_bias(casr_handle* h, const casr_bias* bias, const casr_lm* lm_or_null, int k, float bias_weight,
                   float lm_weight, float length_weight, int32_t* best_tokens, int32_t* best_len,
                   float* best_score, float* best_lm_or_null, float* best_bias, int32_t* steps, void* stream);
int casr_beam_record_bias(casr_handle* h, float* rec_bias, void* stream);

/* Grammar-constrained decoding: every answer is a sentence of a grammar the caller gives (a voice menu, a
 * digit string, a closed list of names).  An n-gram LM and hotwords only move scores; a grammar decides
 * which hypotheses exist.  The reference has no such pass; the operation is DEFINED BY THE RULES BELOW
 * (csrc/grammar_plan.h is their one text for the kernels and the host; tests/grammar_ref.py restates them).
 *   Grammar   a deterministic finite acceptor over token ids: states 0 .. S - 1, per state s the arcs
 *             (token, next) in arc_tok / arc_next [arc_off[s], arc_off[s + 1]), strictly ascending in
 *             token, and is_final [S] (0 / 1).  Sentences start in state 0 (casr_beam_grammar: in start[b]).
 *             eos_token is never an arc label: a hypothesis may end exactly in a final state.
 *   dist[s]   the fewest tokens from s to a final state, by backward breadth-first search.
 * casr_grammar_create checks the arrays (all HOST) and computes dist.  device >= 0 also uploads the grammar
 * to that device (synchronously); device = -1 makes a host-only object.  The object is immutable: any
 * number of handles on its device may share it, from any thread.  It must outlive the work enqueued with it.
 * CASR_ERR_ARG (casr_last_error(NULL) names the state or arc): a NULL array, vocab or n_states < 1, eos
 * outside [0, vocab), arc_off not ascending from 0, a token outside [0, vocab) or equal to eos_token, tokens
 * not strictly ascending within a state, a next outside [0, S), no final state, a state from which no final
 * state can be reached (the caller trims those out; casr/grammar.py does).  CASR_ERR_UNSUPPORTED: more
 * than 2^20 states or 2^24 arcs.
 * casr_grammar_info: n_states, n_arcs and dist [S] (HOST; each may be NULL). */
typedef struct casr_grammar casr_grammar;
int casr_grammar_create(int device, int vocab, int eos_token, int n_states, const int64_t* arc_off,
                        const int32_t* arc_tok, const int32_t* arc_next, const uint8_t* is_final, casr_grammar** out);
void casr_grammar_destroy(casr_grammar* g);
int casr_grammar_info(const casr_grammar* g, int32_t* n_states, int64_t* n_arcs, int32_t* dist_host_or_null);

/* Words of a mask row: GW = 4 ceil(vocab / 128) uint32 (160 at vocab 5,004), so rows are 16-byte aligned.
 * Bit v & 31 of word v >> 5 is token v; bits at and past vocab are 0.  0 for vocab < 1. */
int casr_grammar_mask_words(int vocab);

/* The walk of the sentences tokens [n][L] with lens [n] from state 0; each output may be NULL:
 *   consumed [n]  the tokens walked before the first one without an arc, or the length
 *   state    [n]  the state after those tokens
 *   accepted [n]  consumed == len and is_final[state]
 * An id outside [0, V) has no arc.
 * casr_grammar_accept_host: HOST pointers, any object, no GPU, any L >= 0; CASR_ERR_ARG for a NULL argument
 * or a length outside [0, L].
 * casr_grammar_accept: DEVICE pointers, one thread per sentence; a length outside [0, L] is clamped and
 * raises guard bit 1; 1 <= L <= 512, else CASR_ERR_UNSUPPORTED.  Needs no weights and no encode.
 * CASR_ERR_ARG: a NULL argument, n < 0, a grammar that is host-only or on another device, or whose vocab or
 * eos is not the handle's. */
int casr_grammar_accept_host(const casr_grammar* g, const int32_t* tokens, const int32_t* lens, int n, int L,
                             int32_t* consumed, int32_t* state, uint8_t* accepted);
int casr_grammar_accept(casr_handle* h, const casr_grammar* g, const int32_t* tokens, const int32_t* lens, int n,
                        int L, int32_t* consumed, int32_t* state, uint8_t* accepted, void* stream);

/* The mask rows of grammar states: for state [n] and budget [n], mask [n][GW] uint32.  Bit v != eos of row
 * i is set iff there is an arc (state[i], v, d) with dist[d] <= budget[i]: the token is allowed and a
 * final state stays within budget[i] further tokens.  Bit eos is set iff is_final[state[i]], whatever the
 * budget.  State -1 (a dead beam row) gives an all-zero row.
 * casr_grammar_rows_host: HOST pointers; any other state outside [0, S) is CASR_ERR_ARG.
 * casr_grammar_rows: DEVICE pointers, one wave per row, four rows per workgroup: the wave zeroes its GW
 * words in LDS, its lanes stride the state's arcs and OR their bits in, and the row is written once,
 * coalesced.  A state other than -1 outside [0, S) gives an all-zero row and raises guard bit 1.
 * Errors as casr_grammar_accept; CASR_ERR_UNSUPPORTED: four rows past 64 KB of LDS (V > 131,072). */
int casr_grammar_rows_host(const casr_grammar* g, const int32_t* state, const int32_t* budget, int n,
                           uint32_t* mask);
int casr_grammar_rows(casr_handle* h, const casr_grammar* g, const int32_t* state, const int32_t* budget, int n,
                      uint32_t* mask, void* stream);

/* Beam search over the sentences of a grammar, optionally with the n-gram LM in the first pass.  am, lm,
 * val = (am + lm_weight lm) + len_l (without an LM the lm_weight lm term is left out), the tie rule,
 * ranking beam 0 only at step 0, and len_l are casr_beam_lm's, bit for bit; lse is over the whole logits
 * row (no renormalisation over the allowed set: am stays the acoustic log-probability).
 * Row r carries a grammar state s_r: start[b] at step 0 (start: DEVICE [B], NULL: all 0), -1 for a dead
 * row.  At step l, with L = max_len, the CANDIDATES of an utterance are
 *     (r, v != eos)  with an arc (s_r, v, d) and dist[d] <= L - 2 - l     (the horizon rule)
 *     (r, eos)       with s_r final
 * and dead rows offer nothing.  A pair that is not a candidate is never ranked, whatever its value.  The
 * utterance's list is the top 2k of its candidates by val and may be shorter, or empty.  Records: the eos
 * candidates among the first k ranks.  Active rows: the non-eos candidates in rank order, at most k, each
 * carrying its arc's next state; the slots they leave are dead rows (token eos, back-pointer 0, score 0,
 * state -1), so every word of the tree stays in range for its readers.  An utterance counts as finished
 * for the early stop when rank 0 is eos or its list is empty.
 * The horizon rule keeps every live row able to finish by the last step: at step L - 1 only eos is
 * offered, so an utterance whose start state has dist <= L - 1 always ends with a record, and its output
 * is always a sentence of the grammar.
 * The best hypothesis is casr_beam_lm's final choice (the first maximum over the valid records in (step,
 * rank) order of (rec_score + lm_weight rec_lm) + len_l); without a record, the same over the LIVE rows of
 * the last executed step; complete [B] is 1 iff the choice is a record.  An utterance with no candidate at
 * all (its start state has dist > L - 1, or lies outside [0, S), which also raises guard bit 1) gives
 * best_len 0, best_score 0 and complete 0.  best_score is the choice's am, best_lm (NULL without an LM,
 * else optional) its lm.  With a grammar that allows every token everywhere, every record of a step
 * < L - 1 and, where the search ends before step L - 1, every output equals casr_beam_lm's bit for bit
 * (without an LM and with length_weight 0: casr_beam's).
 * Per step the mask rows of the rows' states under the budget L - 2 - l go through a handle-owned
 * workspace of R GW words (casr_grammar_rows' kernel): one bit per token, read by the select beside the
 * logits and the optional term rows; the bookkeeping lanes look up the chosen candidates' next states (at
 * most 32 binary searches per utterance).  An empty slot raises guard bit 8 only where the utterance had
 * more candidates than were ranked (a NaN row).  It counts under CASR_K_SELECT.  Never replayed as a
 * hipGraph; no float atomics; results do not depend on scheduling.  Returns after enqueueing.
 * Errors as casr_beam_bias: CASR_ERR_STATE before an encode or before weights are bound; CASR_ERR_ARG: a
 * NULL handle, grammar or required output, a grammar or LM that is host-only, on another device or of
 * another vocab, a grammar whose eos is not the handle's, k outside 1..16.  After it casr_beam_rescore,
 * casr_beam_mbr, casr_beam_nbest and casr_beam_confusion return CASR_ERR_STATE until the next casr_beam
 * (they assume a tree without dead rows); casr_beam_records works; casr_beam_record_lm works only if an
 * LM was given. */
int casr_beam_grammar(casr_handle* h, const casr_grammar* g, const casr_lm* lm_or_null,
                      const int32_t* start_or_null /* DEVICE [B], NULL: all 0 */, int k,
                      float lm_weight, float length_weight, int32_t* best_tokens, int32_t* best_len,
                      float* best_score, float* best_lm_or_null, uint8_t* complete, int32_t* steps,
                      void* stream);

/* Edit distance, its operation counts, and a minimum-Bayes-risk (MBR) choice among the finished
 * hypotheses of a beam.  The reference computes a WER per utterance with python-Levenshtein
 * (util.py:237-262) and has no MBR; like the n-gram LM, the operation is DEFINED BY THE FORMULAS BELOW.
 * casr/results.py's edit_distance and edit_ops are the same formulas in Python (the tests' reference).
 *   Distance  symbols are int32, equal when all 32 bits are equal (negative values are ordinary
 *             symbols).  For a[0..m) and b[0..n): D[i][0] = i, D[0][j] = j, D[i][j] = D[i-1][j-1] where
 *             a[i-1] == b[j-1], else 1 + min(D[i-1][j-1], D[i-1][j], D[i][j-1]); dist = D[m][n].
 *   Ops       (insert, delete, replace) of the script turning a into b, by the backtrace from (m, n): at
 *             (i, j) the first rule that applies: i, j > 0 and a match: diagonal; i, j > 0 and D[i][j] ==
 *             D[i-1][j-1] + 1: replace; i > 0 and D[i][j] == D[i-1][j] + 1: delete; else insert.  The sum
 *             is dist.  How it splits is this tie order's; parity with python-Levenshtein's split is not
 *             pinned.  The rule a cell takes is known when it is filled: two bits per cell are kept, no D.
 *   MBR       per utterance over its valid records r_0 .. r_{n-1} in (step, rank) order; l_i the token
 *             count (eos not among the tokens), s_i rec_score, q_i the LM sentence score (0 without
 *             rec_lm):
 *               c_i    = (double(s_i) + lm_weight double(q_i)) + length_weight double(l_i)   the comb of
 *                        casr_beam_rescore, the same uncontracted double operations
 *               c_max  = the largest c_i that is no NaN (NaN when there is none)
 *               w_i    = exp(scale (c_i - c_max))   double; difference and product rounded on their own
 *               risk_i = sum_j w_j double(dist(r_i, r_j))   ascending j from 0, each product rounded
 *                        before its add
 *             The choice is the first record under the total order: a risk that is no NaN beats a NaN,
 *             then the smaller risk, then the lower index.  scale = 0 gives the medoid; a large scale
 *             gives the maximum of c wherever it is unique.  exp is the platform's (host libm, device
 *             ocml): a risk may differ in its last bits between host and device, nothing else does.
 * The two *_host entries take HOST pointers and need no GPU; the others DEVICE pointers.  All return
 * after enqueueing; nothing is launched or written on an error; none is replayed as a hipGraph or
 * counted among the timed kernel classes.
 *   a [n][La], a_len [n], b [n][Lb], b_len [n] int32; dist [n] int32; ops NULL or [n][3] int32.
 * casr_edit_distance_host: any La, Lb >= 0 and n >= 0.  CASR_ERR_ARG: a NULL required argument (a or b
 * may be NULL at La or Lb = 0), or a length outside [0, L].
 * casr_edit_distance: 1 <= La, Lb <= CASR_EDIT_MAX_LEN, else CASR_ERR_UNSUPPORTED; a length outside
 * [0, L] is clamped and raises guard bit 1.  Needs no weights and no encode.  One wave per pair
 * (csrc/edit.hip): lane = column, sweeping the anti-diagonals of a strip of 64 columns with one
 * cross-lane move each; a strip's last column reaches the next through LDS; with ops the direction bits
 * (up to 64 KB) stay in LDS and one lane walks them back. */
#define CASR_EDIT_MAX_LEN 512
int casr_edit_distance_host(const int32_t* a, const int32_t* a_len, int La, const int32_t* b,
                            const int32_t* b_len, int Lb, int n, int32_t* dist, int32_t* ops);
int casr_edit_distance(casr_handle* h, const int32_t* a, const int32_t* a_len, int La, const int32_t* b,
                       const int32_t* b_len, int Lb, int n, int32_t* dist, int32_t* ops, void* stream);

/* The edit script of long pairs: distance, counts and WHICH symbol of b each symbol of a became.
 * Distance, cell rule and backtrace are the ones above; what is new is the length of the rows and the
 * two maps:
 *   b_of_a NULL or [n][La]  b_of_a[i] = j where the backtrace takes a diagonal step (match or replace)
 *                           through cell (i, j), 0-based; -1 for a deleted a[i] and at or past a_len
 *   a_of_b NULL or [n][Lb]  a_of_b[j] = i at the same steps; -1 for an inserted b[j] and at or past b_len
 *   dist [n]; ops NULL or [n][3] as above.  All results are integers; the host and the device entry
 *   agree exactly, and with casr_edit_distance on dist and ops.
 * casr_edit_align_host: any La, Lb >= 0 and no GPU; errors as casr_edit_distance_host.
 * casr_edit_align_tiles_host: the same results computed in the order the device takes (tile by tile,
 * launch by launch, through the same hand-off arrays; csrc/edit_align_plan.h): a check of that order
 * that needs no GPU.
 * casr_edit_align: 1 <= La, Lb <= CASR_EDIT_ALIGN_MAX_LEN, else CASR_ERR_UNSUPPORTED; lengths may be 0;
 * a length outside [0, L] is clamped and raises guard bit 1.  The table is cut into tiles of 64
 * columns by 128 rows, one wave per tile, one ordinary launch per anti-diagonal of tiles, the pairs
 * of a call side by side (csrc/edit_align.hip); the direction bits (2 per cell of n La x Lb tables
 * rounded up to whole tiles: 256 MB for one pair at the limit) go to a workspace the handle owns and
 * grows on demand.  A call whose bits would pass 1 GiB returns CASR_ERR_UNSUPPORTED before anything is
 * allocated or launched.  Needs no weights and no encode, spends no beam and disturbs no encode;
 * returns after enqueueing (growing the workspace waits for the device first); never replayed as a
 * hipGraph.
 * casr_edit_align_plan: what the device entry would do with a call, without a GPU: out[0] = 1 if it is
 * taken, 0 if refused; [1] tile rows, [2] tile columns of a pair; [3] sweep launches; [4] direction-bit
 * bytes; [5] workspace bytes; grid (NULL or [out[3]]) the workgroups of every sweep launch.
 * casr_edit_align_workspace_bytes: bytes of that workspace the handle holds now (-1: NULL handle). */
#define CASR_EDIT_ALIGN_MAX_LEN 32768
int casr_edit_align_host(const int32_t* a, const int32_t* a_len, int La, const int32_t* b,
                         const int32_t* b_len, int Lb, int n, int32_t* dist, int32_t* ops,
                         int32_t* b_of_a, int32_t* a_of_b);
int casr_edit_align_tiles_host(const int32_t* a, const int32_t* a_len, int La, const int32_t* b,
                               const int32_t* b_len, int Lb, int n, int32_t* dist, int32_t* ops,
                               int32_t* b_of_a, int32_t* a_of_b);
int casr_edit_align(casr_handle* h, const int32_t* a, const int32_t* a_len, int La, const int32_t* b,
                    const int32_t* b_len, int Lb, int n, int32_t* dist, int32_t* ops, int32_t* b_of_a,
                    int32_t* a_of_b, void* stream);
int casr_edit_align_plan(int La, int Lb, int n, int with_bits, int64_t* out /* [6] */, int64_t* grid);
int64_t casr_edit_align_workspace_bytes(const casr_handle* h);

/* MBR on the host, on the expanded arrays casr_beam_records writes (rec_lm NULL or [B][max_len][k]):
 *   best_index [B]  the flat index step k + rank of the choice, -1 without a record
 *   rec_risk   NULL or [B][max_len][k] double, 0 where there is no valid record
 * CASR_ERR_ARG: a NULL required argument, B < 0, max_len or k < 1, or a scale that is negative or not
 * finite. */
int casr_mbr_host(const int32_t* rec_tokens, const float* rec_score, const uint8_t* rec_valid,
                  const float* rec_lm, int B, int max_len, int k, double scale, double lm_weight,
                  double length_weight, int32_t* best_index, double* rec_risk);

/* MBR over the finished hypotheses of the last casr_beam, on the device, from the beam tree the handle
 * still holds (no record is expanded).  rec_lm is NULL or the device array casr_beam_rescore wrote.
 *   best_tokens [B][max_len] (-1 past the length), best_len [B], best_score [B] = the choice's rec_score
 *   best_index  NULL or [B] as above; best_risk NULL or [B] double (0 without a record); rec_risk NULL
 *   or [B][max_len][k] double
 * An utterance with no record keeps the unfinished fallback of casr_beam, bit for bit, as the rescore
 * does.  Three launches: the records' list and weights (one workgroup per utterance); every distance of
 * j < i once, as a byte, into a handle-owned workspace of B (max_len k)^2 bytes that grows on demand
 * (128 workgroups of one wave per utterance; CASR_OPT_MBR_MAP picks the mapping); then per record the
 * ascending sum and per utterance the winner by the total order above.  No float atomics: the result
 * does not depend on scheduling or on the reduction tree.  The handle's beam state is only read: a later
 * casr_beam_records, rescore or second MBR call gives the same bits.  A back-pointer outside [0, k) is
 * clamped (guard bit 16); a token id outside [0, V) is an ordinary symbol and raises guard bit 1.
 * CASR_ERR_STATE before casr_beam, and after casr_beam_lm until the next casr_beam (the limit of
 * casr_beam_rescore: the fallback assumes the scores of casr_beam); CASR_ERR_ARG: a NULL handle,
 * best_tokens, best_len or best_score, or a scale that is negative or not finite;
 * CASR_ERR_UNSUPPORTED: max_len > 255 (distances are bytes) or a tree past 64 KB of LDS.
 * casr_beam_mbr_distances copies the distances of the last casr_beam_mbr as a full symmetric matrix:
 * dist [B][max_len k][max_len k] bytes over the positions in (step, rank) order of an utterance's valid
 * records (0 on the diagonal and past the count), n_rec NULL or [B] the counts.  CASR_ERR_STATE unless
 * the last beam call was followed by a casr_beam_mbr. */
int casr_beam_mbr(casr_handle* h, double scale, const float* rec_lm, double lm_weight, double length_weight,
                  int32_t* best_tokens, int32_t* best_len, float* best_score, int32_t* best_index,
                  double* best_risk, double* rec_risk, void* stream);
int casr_beam_mbr_distances(casr_handle* h, uint8_t* dist, int32_t* n_rec, void* stream);

/* N-best lists and per-character alternatives (a confusion network, "sausage") over the finished
 * hypotheses of a beam.  The reference has no counterpart; like the MBR choice the operation is DEFINED
 * BY THE FORMULAS BELOW (tests/confusion_ref.py restates them in Python).  An utterance has the valid
 * records r_0 .. r_{n-1} in (step, rank) order, l_i tokens each, and c_i, c_max and w_i as under MBR above
 * (mbr_comb, mbr_weight: the same uncontracted double operations).
 *   N-best    the records under the total order: a c that is no NaN before a NaN, then the larger c, then
 *             the lower flat index.  nbest_index [B][N] the flat index step k + rank, -1 past the record
 *             count; nbest_tokens [B][N][max_len], -1 past each length (ids as casr_beam_records gives
 *             them); nbest_len [B][N]; nbest_comb [B][N] double, 0 where there is no record.  N in
 *             1..CASR_NBEST_MAX_N.  No exp: host and device agree bit for bit.
 *   Units     u_i = (int64) floor(w_i 2^32), 0 for a NaN w_i; the record at c_max has 2^32.  U = sum u_i
 *             (below 2^44 at max_len 255, k 16).  Everything after this is integer arithmetic: no result
 *             depends on a reduction order.  exp is the platform's: a device unit may differ from the
 *             host's by at most 1, nothing else does.  A unit handed in is clamped into [0, 2^32].
 *   Votes     the pivot a is one valid record of m tokens: S = 2m + 1 slots, odd slot 2i + 1 pivot
 *             position i, even slot 2g the gap before position g (2m: after the end).  For every record
 *             b = r_j the backtrace (Ops above: the same cell rule, the same tie order) of the script
 *             turning a into b votes: a diagonal or replace at (i, j) b[j-1] at slot 2i - 1; a delete at row
 *             i EPS at slot 2i - 1; an insert of b[j-1] at row i that token at slot 2i, of several inserts
 *             into one gap the smallest j; every slot the walk does not touch EPS.  Each record casts one
 *             vote per slot; the pivot votes its tokens at the odd slots and EPS at the gaps.  A token id
 *             outside [0, V) is 0 before anything else, the alignment included (device: guard bit 1).
 *   Slots     mass[s][t] = sum of u_j over the records voting t at slot s; over all t it is U.  Per slot
 *             the M entries (1..CASR_CN_MAX_M) with mass > 0 by larger mass, then smaller token
 *             (CASR_CN_EPS = -1 first); unused entries (CASR_CN_NONE, 0).
 *   n_slots [B] 2m + 1, 0 without a pivot; slot_token [B][2 max_len + 1][M] int32 and slot_mass of the same
 *   shape int64; pivot_mass [B][max_len] int64 the mass of the pivot's own token at its slot (0 past m);
 *   total [B] int64 = U; rec_unit [B][max_len][k] int64, 0 where there is no record.  pivot [B] flat
 *   indices: -1, or the index of no valid record, gives n_slots 0 and NONE / 0 rows (total is still U).
 * The three *_host entries take HOST pointers, the expanded arrays of casr_beam_records (rec_lm NULL or
 * [B][max_len][k]) and need no GPU; total may be NULL in casr_posterior_units_host; casr_confusion_host
 * takes rec_unit as an INPUT.  CASR_ERR_ARG: a NULL required argument, B < 0, max_len or k < 1, vocab < 1,
 * M or N out of range, a scale that is negative or not finite.
 * casr_confusion: the same operation on DEVICE arrays, any B >= 1, max_len <= 255, k <= 16, vocab <=
 * 32767 whose masses fit the LDS (8 (vocab + 1) + 4 max_len k <= 160 KB), else CASR_ERR_UNSUPPORTED.  Needs
 * no weights and no encode.
 * casr_beam_nbest and casr_beam_confusion read the beam tree the handle still holds after casr_beam: no
 * record is expanded in memory, the beam state is only read.  rec_lm NULL or the device array
 * casr_beam_rescore wrote.  pivot NULL: the top of the N-best order; rec_unit NULL or an output.  A
 * back-pointer outside [0, k) is clamped (guard bit 16).  Kernels (csrc/confusion.hip): prepare, one
 * workgroup per utterance (the list, c, u, the ranks by an all-pairs compare, the pivot); align, a lane per
 * record rolling a byte column of D in LDS against the pivot, its 2-bit directions in LDS, walked back
 * into int16 votes, slot-major, in a handle-owned workspace [B][2 max_len + 1][max_len k]; reduce, one wave
 * per slot with an LDS histogram of int64 masses under integer atomics and M rounds of arg-max over the
 * touched bins.  No float atomics.  Errors as casr_beam_mbr: CASR_ERR_STATE before casr_beam and after
 * casr_beam_lm or casr_beam_bias until the next casr_beam; CASR_ERR_ARG: a NULL handle or required output,
 * M or N out of range, a scale that is negative or not finite; CASR_ERR_UNSUPPORTED: max_len > 255 and,
 * for casr_beam_confusion alone, the vocab or LDS limit above.  Nothing is launched or written on an error; none is replayed as a hipGraph or counted among
 * the timed kernel classes. */
#define CASR_CN_EPS (-1)
#define CASR_CN_NONE (-2)
#define CASR_CN_MAX_M 8
#define CASR_NBEST_MAX_N 64
int casr_posterior_units_host(const float* rec_score, const uint8_t* rec_valid, const float* rec_lm, int B,
                              int max_len, int k, double scale, double lm_weight, double length_weight,
                              int64_t* rec_unit, int64_t* total);
int casr_nbest_host(const int32_t* rec_tokens, const float* rec_score, const uint8_t* rec_valid,
                    const float* rec_lm, int B, int max_len, int k, int N, double lm_weight, double length_weight,
                    int32_t* nbest_index, int32_t* nbest_tokens, int32_t* nbest_len, double* nbest_comb);
int casr_confusion_host(const int32_t* rec_tokens, const uint8_t* rec_valid, const int64_t* rec_unit,
                        const int32_t* pivot, int B, int max_len, int k, int vocab, int M, int32_t* n_slots,
                        int32_t* slot_token, int64_t* slot_mass, int64_t* pivot_mass, int64_t* total);
int casr_confusion(casr_handle* h, const int32_t* rec_tokens, const uint8_t* rec_valid, const int64_t* rec_unit,
                   const int32_t* pivot, int B, int max_len, int k, int vocab, int M, int32_t* n_slots,
                   int32_t* slot_token, int64_t* slot_mass, int64_t* pivot_mass, int64_t* total, void* stream);
int casr_beam_nbest(casr_handle* h, int N, const float* rec_lm, double lm_weight, double length_weight,
                    int32_t* nbest_index, int32_t* nbest_tokens, int32_t* nbest_len, double* nbest_comb,
                    void* stream);
int casr_beam_confusion(casr_handle* h, int M, double scale, const float* rec_lm, double lm_weight,
                        double length_weight, const int32_t* pivot, int32_t* n_slots, int32_t* slot_token,
                        int64_t* slot_mass, int64_t* pivot_mass, int64_t* total, int64_t* rec_unit, void* stream);

/* Character timestamps: the best monotone path through the attention weights of a decode (the align
 * that casr_greedy and casr_score write), per token its first, last and peak encoder frame.  The
 * reference has no counterpart; like the edit distance the operation is DEFINED BY THE FORMULAS BELOW,
 * in integers after the first, so the host entry and the kernel agree bit for bit and nothing depends
 * on scheduling (no float atomics, no libm).
 *   Inputs    align [L][Tp][B] f32; per utterance b: T = enc_len[b] frames and n = tgt_len[b] scored
 *             positions (the closing eos among them when it was scored).  x = align[l][t][b].
 *   Weight    q[l][t] = -3072 where !(x > 0) (zero, negative, NaN), else
 *             clamp((int32)(bits(x) >> 16) - (127 << 7), -3072, 0), bits the f32's pattern: a
 *             piecewise-linear log2 in 1/128 octave with the floor 2^-24; x >= 1 gives 0.
 *   Path      cells (l, t), 0 <= l < n, 0 <= t < T, from (0, 0) to (n - 1, T - 1); a cell is entered by
 *             the diagonal (l - 1, t - 1), by staying (l, t - 1) or vertically (l - 1, t).
 *             D[0][0] = q[0][0]; D[l][t] = q[l][t] + max over the predecessors that exist; on equal
 *             values the diagonal, then the vertical, then the stay.  int32: |D| <= 3072 (L + Tp).
 *             The vertical move is what makes T < n well defined (tokens then share frames).
 *   Backtrack from (n - 1, T - 1) through the moves the cells took: first[b][l] and last[b][l] the
 *             smallest and largest t of token l's cells, peak[b][l] the smallest t in [first, last]
 *             with the largest q[l][t]; path_score[b] = D[n - 1][T - 1].
 *   Edges     n = 0 or T = 0: every output of the utterance -1 and path_score 0; positions l >= n get
 *             -1.  A tgt_len outside [0, L] or an enc_len outside [0, Tp] is clamped (the device entry
 *             raises guard bit 1; the host entry has no guard word and clamps silently).  Values of
 *             align at t >= T or l >= n are never read as data.
 *   first, last, peak [B][L] int32; path_score NULL or [B] int32.
 * casr_align_path_host: every pointer a HOST pointer; no GPU, no handle, any Tp (64-bit sums: the same
 * values wherever 3072 (L + Tp) fits an int32).
 * casr_align_path: every pointer a DEVICE pointer; needs no weights and no encode; returns after
 * enqueueing; not among the timed kernel classes and never replayed as a hipGraph.  One launch
 * (csrc/align.hip): a workgroup takes 4 adjacent utterances (16 contiguous bytes of a cell; 16 utterances,
 * the whole 64-byte run, measured 0.143 against 0.126 ms at B = 256: DESIGN.md 3.9), one wave each; per row it loads
 * the [T][4] tile, quantises and transposes it into LDS as int16, and each
 * wave scans its row in chunks of 64 frames with a prefix sum and a prefix maximum across lanes (the
 * stay move is a scan along t: with E the best of diagonal and vertical and P the row's prefix sum of
 * q, D[l][t] = P[t] + max_{s <= t} (E[s] - P[s - 1]); integers make both scans associative).  Two D
 * rows and the 2-bit moves of all L x Tp cells stay in LDS (no workspace in memory): 16 Tp/64 bytes per
 * row, 3.3 KB per utterance at L = 41, Tp = 266; one lane walks them back.  Where the utterances of a
 * workgroup do not fit the 160 KB of a CU it takes half as many, down to 1 (CASR_OPT_ALIGN_GROUP asks
 * for 1, 2, 4, 8 or 16).
 * CASR_ALIGN_MAX_TP: at L = 512 and one utterance per workgroup the move bits (128 Tp bytes), the D
 * rows (8 Tp) and the tiles (4 Tp) fit 160 KB up to Tp = 1152; 1024 is the power of two below it (30.7 s
 * of audio).  The int32 bound is far: 3072 (512 + 2 x 1024) = 7.9 million, against the sentinel 2^30.
 * CASR_ERR_ARG: a NULL required pointer (or handle), B < 1, Tp < 1, L outside [1, 512];
 * CASR_ERR_UNSUPPORTED (device entry): Tp > CASR_ALIGN_MAX_TP.  Nothing is launched or written on an
 * error. */
#define CASR_ALIGN_MAX_TP 1024
int casr_align_path_host(const float* align, const int32_t* enc_len, const int32_t* tgt_len, int B, int Tp,
                         int L, int32_t* first, int32_t* last, int32_t* peak, int32_t* path_score);
int casr_align_path(casr_handle* h, const float* align, const int32_t* enc_len, const int32_t* tgt_len, int B,
                    int Tp, int L, int32_t* first, int32_t* last, int32_t* peak, int32_t* path_score,
                    void* stream);

/* Guard bits raised by the device since the previous casr_device_flags call (read and clear;
 * they accumulate over every encode / decode / log-mel call in between, so one read after a
 * series of calls vouches for all of them; 0 = clean): a data-dependent index out of range (1 token, 2 predecessor row, 4 NaN logit
 * row, 8 beam candidate, 16 back-pointer) is clamped and reported here instead of faulting
 * the device; 32 = a bounded hand-off wait of the persistent recurrence expired (results of
 * that casr_encode are invalid); 64 = casr_log_mel got an utterance shorter than 513
 * samples or longer than n_max, or casr_convert_audio one with n_in outside [0, n_max_in], or casr_segment a
 * frames[b] outside [0, T], or casr_gather_segments a segment outside its fbank or longer than t_seg; 128 = s16x3 arithmetic met a finite activation beyond the f16
 * range (|x| >= 65520: a layer input split by the encoder), so the split images and every
 * result after them are wrong: re-run the batch with casr_set_precision(CASR_PREC_F32) (the
 * Python Model does this itself, chinese-asr_amd/casr/engine.py run_checked).
 * Synchronises `stream`. */
int casr_device_flags(casr_handle* h, int32_t* flags_host, void* stream);

/* Encoder recurrence strategy.  Default (enable = 1): one persistent launch per layer runs all
 * Tp steps, workgroups keep W_hh and c in registers and exchange h through tagged
 * write-through granules; used when its grid (16 x ceil(B/32) x 2 workgroups of 512 threads)
 * fits the device's resident capacity, else the per-step launches below.  0 = per-step
 * launches always.  Both give bitwise identical results. */
int casr_set_persistent(casr_handle* h, int enable);

/* Arithmetic of the MFMA contractions (encoder input projection and recurrence; decoder LSTM
 * cell and projection).  Both compute in f32 on f32 data and keep f32 accumulators:
 *   CASR_PREC_F32    v_mfma_f32_16x16x4_f32, exact f32 products in k order;
 *   CASR_PREC_S16X3  every f32 operand split as hi + 2^-11 lo (two f16), three f16 MFMAs per
 *                    product (hi.hi + 2^-11 (hi.lo + lo.hi)) on the 16x-faster f16 pipes; 22
 *                    significant operand bits.  Measured per stage against float64
 *                    (tests/test_gpu_accuracy.py, profiles/accuracy/accuracy_budget.json): at most
 *                    3.1 times the float32 oracle's own error (the beam score at R = 2048, k = 8;
 *                    2.6 everywhere else), and at or below the F32 path's (at most 3.6 times) at
 *                    every stage but two 40-term f32 sums, both within such a sum's rounding: the
 *                    greedy accum (1.42 against 1.26 times) and the beam score (3.05 against 2.50).
 *   CASR_PREC_S16X1  (round 6, an opt-in perf arithmetic, never the headline: BASELINE config 2's
 *                    "bf16 perf mode") the hi.hi MFMA of every split product only:
 *                    one f16 MFMA instead of three, f32 accumulators: a site computes exactly
 *                    sum_k f16(a_k) f16(b_k), operands rounded to nearest even.  Against the float64
 *                    evaluation of that model the device sits where a float32 evaluation of it
 *                    sits, at every stage (at most 2.2 times its error; tests/test_gpu_accuracy_s16x1.py,
 *                    profiles/accuracy/accuracy_budget_s16x1.json).  What the rounding costs,
 *                    measured per stage on its own inputs as the largest distance from the
 *                    unrounded float64 stage: encoder output 1.7e-3 (rms 2e-4), keys 4.8e-4, a
 *                    token's log-probability 6e-5 with flat and up to 1e-2 with peaked output
 *                    distributions, attention weights 3e-6, a 40-step score 3e-3 and up to 1e-1.
 *                    The sites differ by decode path: the three-launch step (casr_score, beam
 *                    below 1,024 rows, every decode's step 0) rounds the embedding and [ctx | h]
 *                    of the LSTMCell and keeps its query h . W_hidden an exact-f32 MFMA; the folded
 *                    step rounds [ctx | h] only and takes the embedding's gate part from an f32
 *                    table, and its query is an f32 fma chain under greedy and an s16 MFMA (h and
 *                    W_hidden rounded) under beam.  Token ids are NOT identical to the
 *                    reference's; bench.py reports its token agreement.  It is a separate build of this library,
 *                    libcasr_hip_s16x1.so (casr/build.py variant "s16x1", -DCASR_S16_ONE=1), whose
 *                    s16 mode is S16X1: each build accepts F32 and its own s16 mode, and answers
 *                    the other s16 mode with CASR_ERR_UNSUPPORTED.
 * Default: the build's s16 mode.  A blob whose MFMA weights do not fit the split (non-finite,
 * |w| >= 2^14, or an encoder W_ih entry >= 16) runs F32 whatever is set; casr_get_precision
 * reports the effective mode. */
enum { CASR_PREC_F32 = 0, CASR_PREC_S16X3 = 1, CASR_PREC_S16X1 = 2 };
int casr_set_precision(casr_handle* h, int precision);
int casr_get_precision(const casr_handle* h); /* effective mode, -1 on a NULL handle */

/* Which recurrence casr_encode would use for batch B: 1 persistent, 0 per-step, -1 bad args.
 * Does not change the calling thread's current HIP device. */
int casr_recurrence_mode(const casr_handle* h, int B);

/* Tuning options of one handle.  The defaults are the measured fastest variants;
 * every value of every option gives the same results bit for bit (tests/test_gpu_parity.py sweeps
 * them), so an option only ever changes speed.  Options are read at each call, and every decode path
 * decision derived from them is part of the key of a captured decode hipGraph, so changing one
 * between calls takes effect at the next call.
 *   CASR_OPT_FUSE_SELECT     1 (default): the select of step l runs inside a kernel of step l + 1:
 *                            greedy, the LSTMCell (three-launch step) or the attention (folded
 *                            step); beam 4 or 8 with one attention block per utterance, or beam 8
 *                            with two (4 rows per block: both run the select, the first writes the
 *                            bookkeeping) (folded step), the attention.  0: every select a launch
 *                            of its own
 *   CASR_OPT_REC_LAYOUT      persistent recurrence workgroup shape: 0 auto (default: 16 rows x 16
 *                            units when that grid fits one workgroup per CU, else 32 x 16), 1 32x16,
 *                            2 16x32, 3 16x16
 *   CASR_OPT_REC_STORE_PLAIN 1: hand-off words stored L2-kept when the workgroup's whole hand-off
 *                            group runs on its XCD (checked per launch; default); 0: write-through
 *   CASR_OPT_REC_SLEEP       pacing of the recurrence's first poll per step, x 64 clocks; -1
 *                            (default, round 6): 0 for grids of 64 workgroups or more, 1 below
 *                            (B <= 16); measured: 0 is 2-3 % faster at B = 32 and 128, 1 is 1.6 %
 *                            faster at B = 1
 *   CASR_OPT_REC_POLL_GAP    second poll of a pass issued this many x 64 clocks after the first
 *                            (1..8, default 2)
 *   CASR_OPT_REC_COOP        2 (default, round 6): the persistent recurrence is an ordinary launch
 *                            after the occupancy check, ordered after the previous persistent launch
 *                            of this process on the same device (a process-wide event per device), so
 *                            two persistent grids of batches in flight never share the chip; 1: a
 *                            cooperative launch, so a grid that cannot be co-resident fails at launch
 *                            (the encode then falls back to the per-step recurrence) instead of
 *                            spinning into the hand-off timeout (about 25 us more per launch);
 *                            0: ordinary launch, unordered
 *   CASR_OPT_GEMM16_PERSIST  s16x3 input-projection kernel: 2 persistent ping-pong form (default: two
 *                            wave groups one barrier apart, 16-deep stages on a ring of four); 1
 *                            persistent, 32-deep stages on two buffers; 0 one workgroup per tile
 *   CASR_OPT_GEMM16_TAIL     2 (default): the persistent kernel takes whole rounds of tiles and the
 *                            rows after them go to one round of (32 RT) x 128 tiles; 1: to one
 *                            launch of 128 x 256 half tiles; 0: partial last round
 *   CASR_OPT_LOGMEL_Q16      1: casr_log_mel runs 16 lanes per frame, 16 FFT points per lane, one
 *                            stage exchange per frame (default, round 5); 0: one wave per frame, three
 *                            stage exchanges (round 4).  The same butterflies in the same order
 *   CASR_OPT_ATTN_KPB        beam rows per attention block at k > 2: 0 auto (8 at B >= 256 and
 *                            k >= 8, else 4), 4 or 8
 *   CASR_OPT_KEYS_ROWS       1: the s16x3 keys GEMM keeps W_enc in registers and streams 16-row
 *                            items of the encoder output through LDS, one workgroup per CU (default,
 *                            round 5); 0: 128 x 128 tiles (gemm_nt_kernel).  The same MFMAs in the
 *                            same order
 *   CASR_OPT_X16_KM          1: the s16 images of the encoder's layer inputs (and of W_ih) are laid
 *                            out 16-k-block major, so the input GEMM's 16-deep stages read whole
 *                            cache lines (default, round 5; in effect with GEMM16_PERSIST = 2,
 *                            GEMM16_TAIL != 1 and KEYS_ROWS = 1, the forms that read it); 0: row
 *                            images.  The same words in another order: the same bits
 *   CASR_OPT_GEMM16_LEAN     1: the ping-pong input projection (GEMM16_PERSIST = 2 on 16-k-major
 *                            images) advances its DMA sources by a stride per stage and waits on
 *                            constant vmcnt counts in its steady state (round 6); 0: 64-bit stage
 *                            addresses and the runtime wait ladder.  The same MFMAs in the same order
 *   CASR_OPT_MBR_MAP         how casr_beam_mbr maps an utterance's pairs of records to lanes: 1 one wave
 *                            per pair (the anti-diagonal sweep casr_edit_distance runs); 2 one lane per
 *                            pair (a record's tokens uniform across the wave, each lane rolling a row
 *                            of D against a record of its own); 0 (default) the plan's choice
 *                            (csrc/edit_plan.h).  The same distances
 *   CASR_OPT_ALIGN_GROUP     utterances (waves) per workgroup of casr_align_path: 1, 2, 4, 8 or 16; 0
 *                            (default) the plan's choice (csrc/align_plan.h).  Either
 *                            is halved until the workgroup's LDS fits a CU.  The same paths
 * Three options select numerics variants instead (the same token ids, floating-point results within
 * the stated tolerances, not bit for bit; tests/test_gpu_parity.py compares each pair):
 *   CASR_OPT_DEC_KSPLIT      1: the greedy folded GEMM at R <= 32 decode rows (BASELINE config 2)
 *                            splits its k range over 4 workgroups per 32 x 112 output block (252
 *                            workgroups instead of 63; the 4 sums added in a fixed order by the last
 *                            to arrive) (default, round 5); 0: one workgroup per output block.  The
 *                            same products summed in another fixed order: tokens identical, scores
 *                            within 1e-4 of the unsplit form (test_greedy_ksplit_small_batch)
 *   CASR_OPT_ATTN_DIRECT     0: attention scores in the split exponential form 1 - 2 / (1 + e^{2k}
 *                            e^{2q}) (default; one transcendental per term); 1: the
 *                            direct tanh(k + q) form the split form falls back to per block
 *   CASR_OPT_DEC_FOLD        1: greedy decode in two launches per step (default; under f32 the
 *                            fused GEMM runs the exact-f32 MFMAs on an f32 fused image): the
 *                            projection GEMM also computes the next step's LSTM gate
 *                            pre-activations from the same [ctx | h] rows, the embedding part of
 *                            the gates is a per-token table built at bind, and the LSTM cell and
 *                            the attention query run inside the attention kernel;
 *                            0: three launches per step (LSTMCell GEMM, attention, projection).
 *                            Replaces decoder.py:104-114 + attention.py:92 + decoder.py:129-135 per
 *                            step with the same arithmetic regrouped (gates = [ctx | h] W_ch^T +
 *                            (emb W_emb^T + b), q by f32 fma chains).  It is also the default beam
 *                            step at R = B k >= 1024 decode rows when the attention takes 4 or 8 beam
 *                            rows per block and every projection and decoder LSTM weight is below 16
 *                            in magnitude (blob info words 4 and 5): there the fused GEMM runs the
 *                            one-accumulator s16x3 form (the whole sum scaled by 2^11) and the beam
 *                            attention kernel applies the cell (CELL 2).  Same token ids as the
 *                            three-launch step; scores within 2e-3, alignments within 1e-5
 *                            (tests/test_gpu_parity.py test_decode_fold_vs_three_launches,
 *                            test_beam_fold_vs_three_launches).  Not used by casr_beam at k = 1.
 * Two numerics choices are compile-time, not options (both on in the shipped build; the oracle
 * tests pin the tokens with them, both arithmetics):
 *   CASR_FAST_PART_EXP       (decoder.hip) the projection epilogue's per-block Σexp(x - max) partials
 *                            use v_exp_f32 of (x - max) log2(e) instead of libm expf: each row's
 *                            log-sum-exp, so the greedy accum and every beam score, moves in the
 *                            last bits (within the 2e-3 score tolerance), and at a near tie of two
 *                            beam candidates their rank can differ from an expf build's
 *   CASR_LOGITS_NT           (decoder.hip) beam logits stored with the non-temporal hint: speed only
 *   CASR_OPT_ATTN_SPLIT      0 (default): one attention block per utterance.  1 (round 6, measured and
 *                            not adopted): the folded greedy attention at R <= 64
 *                            decode rows (BASELINE config 2) splits each utterance's time steps over 8
 *                            (R <= 32) or 4 blocks, whose softmax maxima, sums and unnormalised
 *                            contexts the last block merges in split order (the same token ids; scores
 *                            within 1e-4 of the unsplit form, test_greedy_split_attention_small_batch);
 *                            2..8: that many ranges at every R <= 64.  Not with an alignment output
 *                            (it needs the whole row)
 * One option exists for tests only:
 *   CASR_OPT_REC_COOP_REFUSE 0 (default): off; n in 1..8: casr_encode treats the cooperative launch
 *                            of encoder layer n - 1 as refused (hipErrorCooperativeLaunchTooLarge,
 *                            without launching), so the mid-encode fallback to the per-step
 *                            recurrence (that layer and every later one) can be checked bit for bit
 *                            against all-persistent and all-per-step encodes
 * And one for measurement only (speed, never bits):
 *   CASR_OPT_DIAG_COLD       0 (default): off; a mask of kernel classes (bit CASR_K_*): before every
 *                            launch of such a class, a flush kernel reads a 1 GiB handle-owned buffer
 *                            (evicting every L2 and the 256 MiB Infinity Cache), outside the class's
 *                            timing events, so the class's time is that of cold operands: warm minus
 *                            cold shows how much of its traffic the Infinity Cache serves
 *                            (the GPU exposes no Infinity-Cache counter) */
enum {
  CASR_OPT_FUSE_SELECT = 0,
  CASR_OPT_REC_LAYOUT = 1,
  CASR_OPT_REC_STORE_PLAIN = 2,
  CASR_OPT_REC_SLEEP = 3,
  CASR_OPT_REC_POLL_GAP = 4,
  CASR_OPT_REC_COOP = 5,
  CASR_OPT_GEMM16_PERSIST = 6,
  CASR_OPT_GEMM16_TAIL = 7,
  CASR_OPT_ATTN_KPB = 8,
  CASR_OPT_ATTN_DIRECT = 9,
  CASR_OPT_DEC_FOLD = 10,
  CASR_OPT_REC_COOP_REFUSE = 11,
  CASR_OPT_DIAG_COLD = 12,
  CASR_OPT_LOGMEL_Q16 = 13,
  CASR_OPT_KEYS_ROWS = 14,
  CASR_OPT_X16_KM = 15,
  CASR_OPT_DEC_KSPLIT = 16,
  CASR_OPT_GEMM16_LEAN = 17,
  CASR_OPT_ATTN_SPLIT = 18,
  CASR_OPT_MBR_MAP = 19,
  CASR_OPT_ALIGN_GROUP = 20,
  CASR_OPT_COUNT = 21
};
int casr_set_option(casr_handle* h, int option, int value);
int casr_get_option(const casr_handle* h, int option, int32_t* value_host);

/* hipGraph replay of the launch-bound loops: bit CASR_GRAPHS_DECODE = the whole decode loop,
 * bit CASR_GRAPHS_RECURRENCE = each layer's Tp steps of the per-step recurrence fallback; each
 * loop is captured once per shape on a private stream and replayed on `stream`, else its kernels
 * launch eagerly on `stream` (same results, bit for bit).  Default CASR_GRAPHS_RECURRENCE: the
 * decode loop launches eagerly, measured 0.1 ms faster per greedy batch and 0.17 ms per beam
 * batch than its replay (round 3; the host enqueues ~160 launches well ahead of the device). */
enum { CASR_GRAPHS_DECODE = 1, CASR_GRAPHS_RECURRENCE = 2 };
int casr_set_graphs(casr_handle* h, int mode);

/* Launch timing per kernel class with HIP event pairs recorded on the launch stream around
 * every launch of the enabled classes (bench.py's roofline figures).  Enabling resets
 * the counters; reading synchronises on the recorded events. */
enum {
  CASR_K_FEATURES = 0,   /* stack + CMVN */
  CASR_K_INPUT_PROJ = 1, /* encoder input-projection GEMM (per layer) */
  CASR_K_REC_STEP = 2,   /* one BiLSTM time step (both directions) */
  CASR_K_KEYS = 3,       /* attention key GEMM */
  CASR_K_DEC_LSTM = 4,   /* decoder LSTM cell GEMM */
  CASR_K_ATTENTION = 5,  /* additive attention + context */
  CASR_K_PROJ = 6,       /* output projection GEMM */
  CASR_K_SELECT = 7,     /* greedy argmax / beam top-2k + bookkeeping */
  CASR_K_COUNT = 8
};
int casr_profile_enable(casr_handle* h, uint32_t class_mask);
int casr_profile_read(casr_handle* h, int kernel_class, int32_t* launches, double* total_ms);

#ifdef __cplusplus
}
#endif
#endif /* CASR_H */
