"""main.align_long, ASR.align and ASR.subtitles(text=...) on the device: two synthetic recordings of
different lengths (bursts with pauses, the signal tests/test_gpu_segment.py cuts), synthetic weights and
a vocabulary of one character per id.  With a recording's own transcription as its text the result is
transcribe(timestamps=True)'s, bit for bit; with an edited one the spans are casr.longalign's on the
host entry's maps."""
import struct
import types

import numpy as np
import pytest

import segment_ref as SR
from casr import lib as L
from casr import longalign as LA
from casr.config import CasrConfig
from casr.segment import SegmentParams
from casr.weights import synthetic_state_dicts

pytestmark = pytest.mark.gpu

CFG = CasrConfig()
OUTSIDE = "，。 A!"  # none of them is in the vocabulary below
# Segments of 3 s at the most, so that the 20 s hold about nine of them.  The synthetic weights decode a
# segment either to nothing or to max_len = 40 characters without an eos (at this eos bias some of
# each): transcribe times such a decode by scoring its 40 tokens, and so must align_long; a span with
# room for its eos arises where the transcript is edited (test_edited_transcription)
PARAMS = SegmentParams(max_frames=300, min_frames=100)
EOS_BIAS = 15.5


def _write_wav16(path, x, rate=16000):
    data = np.clip(np.rint(x * 32768.0), -32768, 32767).astype("<i2").tobytes()
    hdr = struct.pack("<HHIIHH", 1, 1, rate, rate * 2, 2, 16)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<I", 16) + hdr)
        f.write(b"data" + struct.pack("<I", len(data)) + data)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The recordings (13 s: four bursts; 7.5 s: three of them), the model, the vocabulary and, computed once and
    left unchanged, transcribe(timestamps=True) of both."""
    import main as MN
    import model as M
    d = tmp_path_factory.mktemp("longalign")
    x = SR.synthetic_recording(7)
    paths = [str(d / "a.wav"), str(d / "b.wav")]
    _write_wav16(paths[0], x[:13 * 16000])
    _write_wav16(paths[1], x[:int(7.5 * 16000)])
    m = M.Model()
    m.load_state_dicts(*synthetic_state_dicts(CFG, peaked=True, eos_bias=EOS_BIAS))
    i2w = {i: chr(0x4E00 + i) for i in range(CFG.vocab)}
    ab = types.SimpleNamespace(int2word=i2w, word2int={w: i for i, w in i2w.items()})
    base = MN.transcribe(paths, m, ab, params=PARAMS, timestamps=True)
    assert len(base[0]) >= 3 and len(base[1]) >= 2 and all(any(s.text for s in r) for r in base)
    return types.SimpleNamespace(MN=MN, paths=paths, m=m, ab=ab, base=base)


def _host_spans(w, got, texts, base=None):
    """casr.longalign's spans and texts on the host entry's map of decode against transcript."""
    out, base = [], base or w.base
    for k, text in enumerate(texts):
        hyp = [i for s in base[k] for i in LA.hyp_ids(s.text, w.ab.word2int)]
        ids, pos = LA.text_ids(text, w.ab.word2int)
        r = L.edit_align_host(np.array([hyp or [0]], np.int32), [len(hyp)], np.array([ids or [0]], np.int32), [len(ids)])
        assert got[k].dist == r["dist"][0] and got[k].ops == tuple(r["ops"][0].tolist())
        assert (got[k].hyp_len, got[k].ref_len) == (len(hyp), len(ids))
        spans = LA.assign_spans([len(s.text) for s in base[k]], r["a_of_b"][0, :len(ids)])
        out.append((spans, LA.span_text(text, pos, spans), ids, pos))
    return out


def test_own_transcription_gives_transcribe_s_chars(world):
    w = world
    texts = [''.join(s.text for s in rec) for rec in w.base]
    got = w.MN.align_long(w.paths, texts, w.m, w.ab, params=PARAMS)
    _host_spans(w, got, texts)
    for k in range(2):
        assert got[k].dist == 0 and got[k].ops == (0, 0, 0) and len(got[k]) == len(w.base[k])
        for g, b in zip(got[k], w.base[k]):
            assert (g.start_s, g.end_s, g.text) == (b.start_s, b.end_s, b.text)
            assert not g.interpolated
            assert g.chars == (b.chars or [])  # characters, times and confidences, bit for bit


def _edited(text, rs, vocab_chars):
    """Deletions, replacements, insertions and characters outside the vocabulary, spread over the text."""
    out = []
    for i, ch in enumerate(text):
        r = i % 11
        if r in (3, 7):
            continue                                    # a deletion
        out.append(vocab_chars[rs.randint(len(vocab_chars))] if r == 6 else ch)  # a replacement
        if r == 8:
            out.append(vocab_chars[rs.randint(len(vocab_chars))])  # an insertion
        if r in (1, 9):
            out.append(OUTSIDE[(i // 11) % len(OUTSIDE)])
    return OUTSIDE[0] + ''.join(out)


def test_edited_transcription(world):
    w = world
    rs = np.random.RandomState(3)
    vocab_chars = [w.ab.int2word[i] for i in range(10, 200)]
    # batches of three segments: the decode of these batches is the hypothesis, and the second pass
    # takes the same batches
    base = w.MN.transcribe(w.paths, w.m, w.ab, params=PARAMS, batch_size=3)
    texts = [_edited(''.join(s.text for s in rec), rs, vocab_chars) for rec in base]
    got = w.MN.align_long(w.paths, texts, w.m, w.ab, params=PARAMS, batch_size=3)
    host = _host_spans(w, got, texts, base)
    assert sum(not s.interpolated and len(s.chars) > 5 for rec in got for s in rec) >= 2
    for k in range(2):
        spans, parts, ids, pos = host[k]
        assert got[k].dist > 0
        assert [s.text for s in got[k]] == parts and ''.join(parts) == texts[k]
        for g, b, (lo, hi) in zip(got[k], base[k], spans):
            assert (g.start_s, g.end_s) == (b.start_s, b.end_s)
            assert ''.join(c[0] for c in g.chars) == g.text
            aligned = [c for c in g.chars if c[0] in w.ab.word2int]
            assert [w.ab.word2int[c[0]] for c in aligned] == ids[lo:hi]
            if g.interpolated:
                assert hi - lo > CFG.max_len - 1
                continue
            # (an encoder frame is 30 ms, three of the segment's frames: the last one may end up to
            # 20 ms past the segment's last 10 ms frame)
            last = g.start_s
            for c in aligned:
                assert g.start_s <= c[1] <= c[2] < g.end_s + 0.03 - 1e-9 and c[1] >= last and c[3] is not None
                last = c[1]
            prev_end = g.start_s
            for c in g.chars:  # a character outside the vocabulary sits at the end of the one before it
                if c[0] in w.ab.word2int:
                    prev_end = c[2]
                else:
                    assert (c[1], c[2], c[3]) == (prev_end, prev_end, None)


def test_overlong_span_is_interpolated(world):
    w = world
    k, si = 0, max(range(len(w.base[0])), key=lambda i: len(w.base[0][i].text))
    extra = ''.join(w.ab.int2word[300 + i] for i in range(CFG.max_len + 5))
    texts = [''.join(s.text for s in rec) for rec in w.base]
    before = ''.join(s.text for s in w.base[k][:si])
    seg = w.base[k][si].text
    assert len(seg) >= 2
    texts[k] = before + seg[:1] + extra + seg[1:] + texts[k][len(before) + len(seg):]
    got = w.MN.align_long(w.paths, texts, w.m, w.ab, params=PARAMS)
    g = got[k][si]
    assert g.interpolated and len(g.text) >= len(seg) + len(extra) - 1 and ''.join(s.text for s in got[k]) == texts[k]
    n = len(g.chars)
    assert n == len(g.text) and all(c[3] is None for c in g.chars)
    width = (g.end_s - g.start_s) / n
    for i, c in enumerate(g.chars):
        assert c[1] == g.start_s + width * i and c[2] == g.start_s + width * (i + 1)
    # the other recording is untouched by it
    for gg, b in zip(got[1], w.base[1]):
        assert not gg.interpolated and gg.chars == (b.chars or [])


def test_asr_align_and_subtitles_with_text(world):
    w = world
    asr = object.__new__(w.MN.ASR)  # the methods' state without a checkpoint file
    asr.model, asr.audio_base, asr.lm_model, asr.bw = w.m, w.ab, None, None
    asr.fusion, asr.bias, asr.bias_weight, asr.grammar = False, None, 1.0, None
    alone = w.MN.transcribe([w.paths[1]], w.m, w.ab, params=PARAMS, timestamps=True)[0]  # (a batch of its own segments only)
    own = ''.join(s.text for s in alone)
    text = own[:3] + "，" + own[3:] + "。"
    rec = asr.align(w.paths[1], text, params=PARAMS)
    assert ''.join(s.text for s in rec) == text and rec.dist == 0
    srt = asr.subtitles(w.paths[1], text=text, params=PARAMS)
    lines = srt.strip().split("\n")
    assert ''.join(lines[i] for i in range(2, len(lines), 4)) == text and "-->" in lines[1]
    vtt = asr.subtitles(w.paths[1], fmt="vtt", text=text, params=PARAMS)
    assert vtt.startswith("WEBVTT") and ''.join(x for x in vtt.split("\n")[2:] if x and "-->" not in x) == text
    # without a text it does what it did
    from casr import subtitles
    assert asr.subtitles(w.paths[1], params=PARAMS) == subtitles.to_srt(subtitles.cues(alone))
