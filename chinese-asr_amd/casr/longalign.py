"""Lightly supervised alignment of a long recording to its known transcript (main.align_long): the
host-side policy around casr_edit_align.  Host only; nothing here touches the GPU.

The policy:
  * Text to ids (``text_ids``).  A character that is a key of ``word2int`` is aligned and scored.  Every
    other character (punctuation, spaces, Latin letters a Chinese vocabulary lacks) takes no part in the
    alignment.  It is put back into the output right after the aligned character before it, with that
    character's end time as both of its times and None as its confidence; characters before the first
    aligned one go in front of it, at its segment's start.
  * The recording is decoded, and the decoded characters of all its segments, in order, are aligned
    against the transcript's ids as ONE pair (hypothesis = a, transcript = b): casr_edit_align's
    ``a_of_b`` says which hypothesis position each transcript position became, -1 for an insertion.
  * Spans (``assign_spans``).  Every segment gets one half-open span of transcript positions; the spans
    are monotone and cover the transcript.  A position aligned to hypothesis position i belongs to the
    segment that holds i.  A run of inserted positions whose two aligned neighbours lie in one segment
    belongs to it; a run across a boundary, and a run after the last aligned position, goes to the
    earlier segment (the one of the aligned position before it); a run before the first aligned
    position goes to the first segment that has a hypothesis (the first segment when none has).
  * A span is force-aligned inside its segment with its closing eos (casr_score, casr_align_path), the
    pass transcribe(timestamps=True) runs over a decode: a recording aligned to its own transcription
    gets transcribe's times bit for bit.  casr_score has max_len positions, so a span of up to
    max_len - 1 tokens is scored with its eos.  A span of exactly max_len tokens is scored without
    it, which is how transcribe times a decode that ran to max_len.  A longer span, or a span in a
    segment too short to encode, cannot be scored in one pass: its segment comes back
    ``interpolated``, its characters evenly spaced across the segment with None confidences
    (``interpolate``).
  * The distance and the (insert, delete, replace) counts of hypothesis against transcript are
    reported per recording: the character error count, the honest signal of how far to trust the times.
"""


class AlignedRecording(list):
    """The list of casr.segment.Segment of one recording, with the alignment's report: ``dist`` and
    ``ops`` = (insert, delete, replace) of the decoded characters against the transcript's aligned
    characters, ``hyp_len`` and ``ref_len`` their counts."""

    def __init__(self, segments=(), dist=0, ops=(0, 0, 0), hyp_len=0, ref_len=0):
        super().__init__(segments)
        self.dist, self.ops, self.hyp_len, self.ref_len = int(dist), tuple(int(x) for x in ops), hyp_len, ref_len


def text_ids(text, word2int):
    """(ids, pos): the ids of the characters of ``text`` that ``word2int`` knows, and their positions in
    ``text``."""
    ids, pos = [], []
    for p, ch in enumerate(text):
        i = word2int.get(ch)
        if i is not None:
            ids.append(int(i))
            pos.append(p)
    return ids, pos


HYP_UNKNOWN = -2  # a decoded character no transcript id equals (part of a word of several characters)


def hyp_ids(text, word2int):
    """The decoded characters as ids; a character word2int lacks is a symbol that matches nothing."""
    return [int(word2int.get(ch, HYP_UNKNOWN)) for ch in text]


def assign_spans(seg_tok_counts, a_of_b):
    """One half-open span (lo, hi) of transcript positions per segment.  ``seg_tok_counts``: hypothesis
    positions per segment, in order; ``a_of_b`` [n]: the hypothesis position of every transcript position,
    -1 for an insertion (casr_edit_align's map, increasing over its entries >= 0).  The module's
    docstring has the rules."""
    counts = [int(c) for c in seg_tok_counts]
    S, n = len(counts), len(a_of_b)
    if S == 0:
        if n:
            raise ValueError("assign_spans: a transcript but no segment")
        return []
    ends, t = [], 0
    for c in counts:
        t += c
        ends.append(t)
    first_hyp = next((s for s, c in enumerate(counts) if c > 0), 0)
    seg_of, s, cur = [], 0, first_hyp  # cur: the segment of the last aligned position (or of a leading run)
    for j in range(n):
        i = int(a_of_b[j])
        if i >= 0:
            if i >= t:
                raise ValueError(f"assign_spans: a_of_b[{j}] = {i} past the {t} hypothesis positions")
            while ends[s] <= i:
                s += 1
            cur = s
        seg_of.append(cur)
    # an inserted run belongs to the earlier segment: the one of the aligned position before it, which
    # is the later neighbour's too when both lie in one segment
    spans, lo = [], 0
    for s in range(S):
        hi = lo
        while hi < n and seg_of[hi] <= s:
            hi += 1
        spans.append((lo, hi))
        lo = hi
    return spans


def span_text(text, pos, spans):
    """The transcript's text per span, its unaligned characters put back: a span's text runs from its
    first aligned character up to the next span's; what precedes the first aligned character goes to the
    span that holds it (to the first span when nothing is aligned)."""
    n = len(pos)
    out, lead = [], False
    for lo, hi in spans:
        if n == 0:
            out.append('' if lead else text)
            lead = True
            continue
        if lo == hi:
            out.append('')
            continue
        begin = 0 if lo == 0 else pos[lo]
        end = len(text) if hi == n else pos[hi]
        out.append(text[begin:end])
    return out


def span_chars(text, pos, lo, hi, timed, start_s):
    """[(char, start_s, end_s, confidence)] of one span's text (span_text's), one per character:
    ``timed`` [(start_s, end_s, confidence)] per aligned character of the span, in recording time."""
    n = len(pos)
    if lo == hi:
        return []
    out = []
    if lo == 0:
        out += [(ch, start_s, start_s, None) for ch in text[:pos[0]]]
    for j in range(lo, hi):
        s, e, c = timed[j - lo]
        out.append((text[pos[j]], s, e, c))
        nxt = len(text) if j + 1 == n else pos[j + 1]
        out += [(ch, e, e, None) for ch in text[pos[j] + 1:nxt]]
    return out


def interpolate(count, start_s, end_s):
    """``count`` characters evenly spaced across [start_s, end_s]: [(start_s, end_s, None)]."""
    w = (end_s - start_s) / count if count else 0.0
    return [(start_s + w * k, start_s + w * (k + 1), None) for k in range(count)]
