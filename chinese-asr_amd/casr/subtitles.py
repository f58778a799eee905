"""Subtitle cues from timed segments (main.transcribe(..., timestamps=True)), host only.

A segment is anything with ``start_s``, ``end_s``, ``text`` and ``chars`` (casr.segment.Segment);
``chars`` is None or a list of (char, start_s, end_s, confidence), one per character of ``text``."""
from collections import namedtuple

Cue = namedtuple('Cue', ('start_s', 'end_s', 'text'))


def _over(chars, max_chars, max_s):
    return len(chars) > max_chars or chars[-1][2] - chars[0][1] > max_s


def _split(chars, max_chars, max_s):
    """A cue over either limit is cut at the largest gap between a character's end_s and the next
    start_s; of equal gaps (the spans of a monotone path tile the audio: most gaps are equal) the one
    nearest the middle, then the earlier.  Gaps are compared to the microsecond."""
    if len(chars) < 2 or not _over(chars, max_chars, max_s):
        return [chars]
    mid = (len(chars) - 2) / 2.0
    cut = max(range(len(chars) - 1), key=lambda i: (round(chars[i + 1][1] - chars[i][2], 6), -abs(i - mid), -i))
    return _split(chars[:cut + 1], max_chars, max_s) + _split(chars[cut + 1:], max_chars, max_s)


def cues(segments, max_chars=20, max_s=6.0):
    """Segments -> [Cue(start_s, end_s, text)]: one cue per segment with text, split while it holds
    more than ``max_chars`` characters or lasts longer than ``max_s`` seconds.  A segment without
    ``chars`` cannot be split and gives one cue with the segment's own times."""
    out = []
    for s in segments:
        if not s.text:
            continue
        chars = getattr(s, 'chars', None)
        if not chars:
            out.append(Cue(float(s.start_s), float(s.end_s), s.text))
            continue
        for part in _split(list(chars), int(max_chars), float(max_s)):
            out.append(Cue(float(part[0][1]), float(part[-1][2]), ''.join(c[0] for c in part)))
    return out


def _clock(t, sep):
    ms = max(int(round(float(t) * 1000.0)), 0)
    return "%02d:%02d:%02d%s%03d" % (ms // 3600000, ms // 60000 % 60, ms // 1000 % 60, sep, ms % 1000)


def to_srt(cue_list):
    """SubRip text: numbered cues, HH:MM:SS,mmm --> HH:MM:SS,mmm; '' for no cue."""
    return ''.join("%d\n%s --> %s\n%s\n\n" % (i + 1, _clock(c.start_s, ','), _clock(c.end_s, ','), c.text)
                   for i, c in enumerate(cue_list))


def to_vtt(cue_list):
    """WebVTT text: the header, then HH:MM:SS.mmm --> HH:MM:SS.mmm cues."""
    return "WEBVTT\n\n" + ''.join("%s --> %s\n%s\n\n" % (_clock(c.start_s, '.'), _clock(c.end_s, '.'), c.text)
                                  for c in cue_list)
