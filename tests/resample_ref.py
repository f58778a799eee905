"""numpy restatement of casr_convert_audio (include/casr.h), written from its formulas, not from the
HIP code: downmix, polyphase Kaiser-windowed-sinc resampling to 16 kHz, s16 quantisation, peak
normalisation.  ``convert(..., dtype=np.float64)`` is the reference (float64 samples, float64 table,
float64 sums); ``dtype=np.float32`` with the table rounded to float32 is the yardstick whose own
distance from the reference sets the device's budget (tests/test_gpu_convert.py)."""
import math

import numpy as np

RATE_OUT = 16000
RATES = (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 96000)


def plan(rate):
    """(L, M, K, c, hw): g = gcd(16000, rate), L = 16000 / g, M = rate / g, c = 0.94 min(1, L / M),
    hw = 32 / c, K = ceil(hw); every phase has 2 K taps."""
    g = math.gcd(RATE_OUT, int(rate))
    L, M = RATE_OUT // g, int(rate) // g
    c = 0.94 * min(1.0, L / M)
    hw = 32.0 / c
    return L, M, int(math.ceil(hw)), c, hw


def frames(n, rate):
    L, M = plan(rate)[:2]
    return -((-int(n) * L) // M)  # ceil(n L / M), exact in Python integers


def bessel_i0(x):
    """I0 by its power series sum_k ((x / 2)^k / k!)^2 (all terms positive), float64."""
    x = np.asarray(x, np.float64)
    q = 0.25 * x * x
    term = np.ones_like(x)
    total = np.ones_like(x)
    for k in range(1, 200):
        term = term * q / (k * k)
        total = total + term
    return total


_TABLES = {}


def table(rate):
    """float64 [L, 2 K]: tab[p][j + K - 1] = h_j / sum_j h_j, h(u) = c sinc(c u) I0(9 sqrt(1 - (u / hw)^2))
    / I0(9) for |u| < hw else 0, u = p / L - j, j = -K + 1 .. K."""
    if rate not in _TABLES:
        L, M, K, c, hw = plan(rate)
        j = np.arange(-K + 1, K + 1, dtype=np.float64)
        u = np.arange(L, dtype=np.float64)[:, None] / L - j[None, :]
        inside = np.abs(u) < hw
        w = np.sqrt(np.clip(1.0 - (u / hw) ** 2, 0.0, None))
        h = c * np.sinc(c * u) * bessel_i0(9.0 * w) / bessel_i0(9.0)  # np.sinc(t) = sin(pi t) / (pi t)
        h = np.where(inside, h, 0.0)
        _TABLES[rate] = h / h.sum(axis=1, keepdims=True)
    return _TABLES[rate]


def downmix(pcm, dtype):
    """[n, ch] -> [n]: the sum of the channels in ascending order, times 1 / ch, in dtype."""
    pcm = np.asarray(pcm)
    if pcm.ndim == 1:
        pcm = pcm[:, None]
    ch = pcm.shape[1]
    s = pcm[:, 0].astype(dtype)
    for c in range(1, ch):
        s = s + pcm[:, c].astype(dtype)
    return s * (dtype(1) / dtype(ch))


def resample(x, rate, dtype):
    """Stage (b) on mono samples x [n] in dtype: y[m] = sum_j tab[p][j] x[base + j], ascending j."""
    x = np.asarray(x, dtype)
    if rate == RATE_OUT:
        return x.copy()
    L, M, K, _, _ = plan(rate)
    n = len(x)
    n_out = frames(n, rate)
    tab = table(rate).astype(dtype)
    m = np.arange(n_out, dtype=np.int64)
    pos = m * M
    base, p = pos // L, pos % L
    xp = np.concatenate([np.zeros(K, dtype), x, np.zeros(K + 1, dtype)])  # x = 0 outside [0, n)
    y = np.zeros(n_out, dtype)
    for i in range(2 * K):  # j = i - K + 1: index base + j + K in the padded signal
        y = y + tab[p, i] * xp[base + i + 1]
    return y


def quantise(y):
    """Stage (c): clamp(rint(y 32768), -32768, 32767), ties to even; NaN -> 0.  Same dtype as y."""
    y = np.asarray(y)
    q = np.clip(np.rint(y * y.dtype.type(32768)), -32768, 32767)
    return np.where(np.isnan(y), y.dtype.type(0), q)


def normalise_q(q, norm_db):
    """Stage (d) on quantised values q (integral floats), in float32 as the header states it:
    g = float32(32768 10^(norm_db / 20)) / float32(peak), out = clamp(rint(float32(q) g)) / 32768.
    Returns (out float32, g float32)."""
    q = np.asarray(q, np.float32)
    peak = np.float32(np.abs(q).max()) if q.size else np.float32(0)
    if norm_db >= 0 or peak == 0:
        return q / np.float32(32768), np.float32(1)
    g = np.float32(32768.0 * 10.0 ** (float(norm_db) / 20.0)) / peak
    out = np.clip(np.rint(q * g), -32768, 32767).astype(np.float32)
    return out / np.float32(32768), g


def normalise_y(y, norm_db):
    """Stage (d) without quantisation, float32: out = y g, g = float32(10^(norm_db / 20)) / peak."""
    y = np.asarray(y, np.float32)
    peak = np.float32(np.abs(y).max()) if y.size else np.float32(0)
    if norm_db >= 0 or peak == 0:
        return y.copy(), np.float32(1)
    g = np.float32(10.0 ** (float(norm_db) / 20.0)) / peak
    return y * g, g


def convert(pcm, rate, dtype=np.float64, quantize=False, norm_db=0.0):
    """All four stages on one utterance pcm [n, ch] (or [n]); stages (a) to (c) in dtype, (d) in
    float32.  Returns (wav, gain)."""
    y = resample(downmix(pcm, dtype), rate, dtype)
    if quantize:
        return normalise_q(quantise(y), norm_db)
    if norm_db < 0:
        return normalise_y(y, norm_db)
    return y, np.float32(1)


# ---------------------------------------------------------------- tone measurements
def tone(freq, rate, n, phase=0.3):
    return np.sin(2.0 * np.pi * freq * np.arange(n) / rate + phase)


def db(num, den):
    return 20.0 * np.log10(max(float(num), 1e-300) / float(den))


def rms(v):
    return float(np.sqrt(np.mean(np.square(np.asarray(v, np.float64)))))


def tone_error_db(y, freq, skip=400, phase=0.3):
    """rms of (y - the analytic 16 kHz tone) over the tone's rms, edges skipped, in dB."""
    want = tone(freq, RATE_OUT, len(y), phase)
    return db(rms((np.asarray(y, np.float64) - want)[skip:-skip]), rms(want[skip:-skip]))


def residual_db(y, skip=400):
    """rms of y over the rms of a unit-amplitude tone (an input the filter should remove), in dB."""
    return db(rms(np.asarray(y, np.float64)[skip:-skip]), math.sqrt(0.5))


def component_db(y, freq, skip=400):
    """Amplitude of the frequency `freq` in y (least-squares fit of sin and cos), relative to 1, in dB."""
    y = np.asarray(y, np.float64)[skip:-skip]
    t = 2.0 * np.pi * freq * np.arange(len(y)) / RATE_OUT
    A = np.stack([np.sin(t), np.cos(t)], axis=1)
    coef = np.linalg.lstsq(A, y, rcond=None)[0]
    return db(np.hypot(coef[0], coef[1]), 1.0)
