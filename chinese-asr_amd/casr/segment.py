"""Segmentation of long recordings at their pauses (include/casr.h casr_segment): the parameter set,
the host entry point, and the timed result of main.transcribe.

The operation is defined by the formulas in include/casr.h; ``segment_host`` runs them on the CPU
(casr_segment_host, no GPU needed), ``Engine.segment`` on the device, with exactly the same result."""
import ctypes
from dataclasses import dataclass, fields

import numpy as np

from . import lib as _lib

FRAME_S = 0.01  # one log-mel frame: hop 160 at 16 kHz


class SegmentParamsC(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "max_frames", "min_frames", "min_pause", "min_speech", "pad", "max_gap", "pct_lo", "pct_hi",
        "rel_q8", "rise_min")]


@dataclass(frozen=True)
class SegmentParams:
    """casr_segment_params (include/casr.h), all int32."""
    max_frames: int = 800   # longest segment, in frames
    min_frames: int = 200   # shortest piece a split may leave
    min_pause: int = 20     # shortest quiet run that counts as a pause
    min_speech: int = 5     # shortest active run that is kept
    pad: int = 8            # frames added on each side of a speech island
    max_gap: int = 100      # largest gap across which pieces are merged
    pct_lo: int = 10        # percentile that gives the noise floor
    pct_hi: int = 95        # percentile that gives the speech level
    rel_q8: int = 90        # rise above the floor, as a fraction of hi - lo in units of 1/256
    rise_min: int = 12      # smallest rise above the floor, in bins

    def valid(self):
        return (self.min_speech >= 1 and self.pad >= 0 and self.min_pause > 2 * self.pad and self.min_frames >= 1
                and 2 * self.min_frames <= self.max_frames and self.max_gap >= 0
                and 0 <= self.pct_lo <= self.pct_hi <= 100 and 0 <= self.rel_q8 <= 256 and self.rise_min >= 0)

    def validate(self):
        """Raises ValueError on a set the library refuses (CASR_ERR_ARG)."""
        for f in fields(self):
            v = getattr(self, f.name)
            if int(v) != v or not -2 ** 31 <= v < 2 ** 31:
                raise ValueError(f"SegmentParams.{f.name} = {v!r} is not an int32")
        if not self.valid():
            raise ValueError(f"invalid {self}: need min_speech >= 1, pad >= 0, min_pause > 2 pad, min_frames >= 1, "
                             "2 min_frames <= max_frames, max_gap >= 0, 0 <= pct_lo <= pct_hi <= 100, "
                             "0 <= rel_q8 <= 256, rise_min >= 0")
        return self

    def struct(self):
        return SegmentParamsC(*(int(getattr(self, f.name)) for f in fields(self)))

    @classmethod
    def library_defaults(cls):
        """casr_segment_default_params, read from the library."""
        c = SegmentParamsC()
        _lib.check(_lib.load().casr_segment_default_params(ctypes.byref(c)))
        return cls(*(int(getattr(c, n)) for n, _ in SegmentParamsC._fields_))


def segment_bound(T, params=None):
    """An upper bound of one recording's segment count at T frames (casr_segment_bound)."""
    c = (params or SegmentParams()).validate().struct()
    n = int(_lib.load().casr_segment_bound(int(T), ctypes.byref(c)))
    if n < 0:
        raise _lib.CasrError(f"casr_segment_bound({T}): bad arguments, or the bound does not fit an int")
    return n


def segment_host(fbank, frames, params=None, s_max=None):
    """casr_segment_host: fbank [B, T, n_mels] float32 and frames [B] on the host -> numpy
    (seg_start [B, s_max], seg_len [B, s_max], n_seg [B], thr [B]).  Entries past n_seg[b], and past
    s_max, keep -1; n_seg is the true count.  s_max defaults to the bound.  Needs no GPU."""
    lib = _lib.load()
    params = params or SegmentParams()
    fbank = np.ascontiguousarray(fbank, np.float32)
    frames = np.ascontiguousarray(frames, np.int32)
    B, T, n_mels = fbank.shape
    c = params.struct()
    if s_max is None:
        s_max = max(int(lib.casr_segment_bound(T, ctypes.byref(c))), 0)
    start = np.full((B, s_max), -1, np.int32)
    length = np.full((B, s_max), -1, np.int32)
    n_seg = np.zeros(B, np.int32)
    thr = np.zeros(B, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _lib.check(lib.casr_segment_host(p(fbank), p(frames), B, T, n_mels, ctypes.byref(c), int(s_max), p(start),
                                     p(length), p(n_seg), p(thr)), lib=lib)
    return start, length, n_seg, thr


@dataclass
class Segment:
    """One transcribed segment of a recording: times in seconds (frame x 0.01)."""
    start_s: float
    end_s: float
    text: str
    score: float
    truncated: bool  # the decode used all max_len steps without an EOS: lower max_frames
    chars: list = None  # transcribe(timestamps=True): [(char, start_s, end_s, confidence)] in recording time
    interpolated: bool = False  # align_long: the span could not be scored; its times are evenly spaced


def frame_time(frame):
    return int(frame) * FRAME_S
