"""numpy restatement of casr_segment's formulas (include/casr.h): the level of each frame (a), and the
executable statement of the threshold, the run filters, the split and the merge (b)-(e) on the integer
levels q.  After (a) everything is an integer, so the library's host entry and the device must agree
with it exactly."""
from dataclasses import dataclass, replace  # noqa: F401  (replace: for the tests' parameter variants)

import numpy as np

N_BINS = 512


@dataclass(frozen=True)
class P:
    max_frames: int = 800
    min_frames: int = 200
    min_pause: int = 20
    min_speech: int = 5
    pad: int = 8
    max_gap: int = 100
    pct_lo: int = 10
    pct_hi: int = 95
    rel_q8: int = 90
    rise_min: int = 12


SMALL = P(max_frames=64, min_frames=16, min_pause=6, min_speech=3, pad=2, max_gap=10)


def valid(p):
    return (p.min_speech >= 1 and p.pad >= 0 and p.min_pause > 2 * p.pad and p.min_frames >= 1
            and 2 * p.min_frames <= p.max_frames and p.max_gap >= 0 and 0 <= p.pct_lo <= p.pct_hi <= 100
            and 0 <= p.rel_q8 <= 256 and p.rise_min >= 0)


def bound(T, p):
    return (T + p.min_pause) // (p.min_speech + p.min_pause) + T // p.min_frames


# ---------------------------------------------------------------- (a)
def levels(fb):
    """fb [n, n_mels] float32 (n_mels a multiple of 16) -> q [n] int64: 16 partial sums in ascending
    order, the halving tree, E = p_0 float32(1 / n_mels), q = clamp(floor((E + 24) 8), 0, 511), NaN -> 0."""
    fb = np.asarray(fb, np.float32)
    n, m = fb.shape
    assert m % 16 == 0 and m > 0
    with np.errstate(all="ignore"):
        p = fb[:, 0:16].copy()
        for k in range(16, m, 16):
            p = p + fb[:, k:k + 16]
        for h in (8, 4, 2, 1):
            p = p[:, :h] + p[:, h:2 * h]
        e = p[:, 0] * (np.float32(1.0) / np.float32(m))
        x = (e + np.float32(24.0)) * np.float32(8.0)
        assert x.dtype == np.float32
        q = np.where(np.isnan(x), np.float32(0), np.clip(np.floor(x), 0, N_BINS - 1))
    return q.astype(np.int64)


# ---------------------------------------------------------------- (b)-(e)
def pctl(hist, n, pct):
    """P(pct): the smallest v with sum_{u <= v} hist[u] >= max(1, (n pct + 99) div 100)."""
    need = max(1, (int(n) * int(pct) + 99) // 100)
    return int(np.searchsorted(np.cumsum(hist.astype(np.int64)), need))


def runs(a):
    """Maximal runs of a boolean array: (value, start, end)."""
    n = len(a)
    if n == 0:
        return []
    edge = np.flatnonzero(a[1:] != a[:-1]) + 1
    starts = np.concatenate(([0], edge))
    ends = np.concatenate((edge, [n]))
    return [(bool(a[s]), int(s), int(e)) for s, e in zip(starts, ends)]


def threshold(q, P):
    n = len(q)
    if n == 0:
        return 0
    hist = np.bincount(q, minlength=N_BINS)
    lo, hi = pctl(hist, n, P.pct_lo), pctl(hist, n, P.pct_hi)
    return lo + max(P.rise_min, ((hi - lo) * P.rel_q8 + 128) >> 8)


def segment(q, P, detail=None):
    """q [n] integer levels -> [(start, len)].  detail: a dict that receives the intermediate stages
    (thr, a0, a1, a2, islands, pieces, cuts), for tests that assert what a case exercises."""
    q = np.asarray(q, np.int64)
    n = len(q)
    thr = threshold(q, P)
    a = (q >= thr).copy()
    a0 = a.copy()
    for v, s, e in runs(a):            # maximal runs (value, start, end)
        if v and e - s < P.min_speech:
            a[s:e] = False
    a1 = a.copy()
    for v, s, e in runs(a):
        if not v and s > 0 and e < n and e - s < P.min_pause:
            a[s:e] = True
    isl = [(max(0, s - P.pad), min(n, e + P.pad)) for v, s, e in runs(a) if v]
    pieces, cuts = [], []
    for s, e in isl:
        while e - s > P.max_frames:
            cs = np.arange(s + P.min_frames, min(s + P.max_frames, e - P.min_frames) + 1)
            cost = q[cs - 1] + q[cs]
            c = int(cs[len(cs) - 1 - np.argmin(cost[::-1])])
            cuts.append((c, int((cost == cost.min()).sum())))
            pieces.append((s, c))
            s = c
        pieces.append((s, e))
    segs, i = [], 0
    stops = []  # why each segment stopped absorbing: "gap", "len" or "end"
    while i < len(pieces):
        s, e = pieces[i]
        j = i + 1
        while j < len(pieces) and pieces[j][0] - e <= P.max_gap and pieces[j][1] - s <= P.max_frames:
            e = pieces[j][1]
            j += 1
        stops.append("end" if j == len(pieces) else ("gap" if pieces[j][0] - e > P.max_gap else "len"))
        segs.append((s, e - s))
        i = j
    if detail is not None:
        detail.update(thr=thr, a0=a0, a1=a1, a2=a, islands=isl, pieces=pieces, cuts=cuts, stops=stops)
    return segs


def segment_fbank(fb, n, P, detail=None):
    """Rows [0, n) of fb [T, n_mels] -> (thr, [(start, len)])."""
    q = levels(np.asarray(fb, np.float32)[:n])
    return threshold(q, P), segment(q, P, detail)


# ---------------------------------------------------------------- test inputs
def fbank_from_levels(level, seed, n_mels=80, noise=0.4):
    """A log-mel-like array whose frame t has mean level about level[t] (nepers): the level plus seeded
    noise, spread over the bins with a fixed tilt, so that stage (a) adds unequal numbers."""
    rs = np.random.RandomState(seed)
    level = np.asarray(level, np.float64)
    tilt = np.linspace(-1.5, 1.5, n_mels)
    fb = level[:, None] + tilt[None, :] + noise * rs.standard_normal((len(level), n_mels))
    return fb.astype(np.float32)


def random_levels(n, seed, quiet=-9.0, loud=-2.0, mean_on=40, mean_off=12):
    """A level sequence of alternating loud and quiet stretches with geometric lengths (short ones are
    common: runs of 1, 2, 3 frames and pauses of a few), plus a slow drift."""
    rs = np.random.RandomState(seed)
    out = np.empty(n, np.float64)
    t, on = 0, bool(rs.randint(2))
    while t < n:
        m = 1 + rs.geometric(1.0 / (mean_on if on else mean_off))
        if rs.rand() < 0.1:
            m *= 6
        out[t:t + m] = (loud if on else quiet) + 0.5 * rs.standard_normal()
        t += m
        on = not on
    return out + 0.3 * np.sin(np.arange(n) / 97.0)


def synthetic_recording(seed=7, rate=16000):
    """The 35 s synthetic signal: harmonic bursts of 2.5, 1.2, 3.0, 12.0, 0.8, 4.0, 0.03 and 5 s after
    gaps of 0.5, 0.3, 1.5, 0.15, 2.5, 0.6, 0.6 and 0.4 s, noise of 8e-4 rms, peak 0.89.  Each burst is a
    glide of 12 harmonics under a 4 Hz syllable envelope with dips, like speech."""
    bursts = (2.5, 1.2, 3.0, 12.0, 0.8, 4.0, 0.03, 5.0)
    gaps = (0.5, 0.3, 1.5, 0.15, 2.5, 0.6, 0.6, 0.4)
    rs = np.random.RandomState(seed)
    parts = []
    for g, d in zip(gaps, bursts):
        parts.append(np.zeros(int(round(g * rate))))
        m = int(round(d * rate))
        t = np.arange(m) / rate
        f0 = 110.0 + 40.0 * rs.rand() + 25.0 * np.sin(2 * np.pi * (0.3 + 0.4 * rs.rand()) * t)
        ph = 2 * np.pi * np.cumsum(f0) / rate
        x = sum(np.sin(k * ph + rs.rand() * 6.28) / k for k in range(1, 13))
        env = 0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t + rs.rand() * 6.28)
        ramp = np.minimum(1.0, np.minimum(np.arange(m), np.arange(m)[::-1]) / (0.01 * rate))
        parts.append(x * env * ramp)
    parts.append(np.zeros(int(round(0.5 * rate))))
    x = np.concatenate(parts)
    x = x / np.abs(x).max() * 0.89
    x = x + 8e-4 * rs.standard_normal(len(x))
    return x.astype(np.float32)
