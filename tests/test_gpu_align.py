"""The monotone attention path on the device (casr_align_path / Engine.align_path, csrc/align.hip) and
the character timestamps built on it (Model.eval_one_batch_*'s ``timestamps``, main.transcribe).

The kernel is integer after its first stage, so it must equal the host entry (casr_align_path_host,
which tests/test_align_host.py holds to the numpy restatement) bit for bit: on every generator of
tests/align_ref.py, at the shapes where the mapping can break (a chunk-carry boundary at 64 / 65 / 129
frames, a short last utterance group, T < n, single cells, and the shapes at which the plan takes
fewer utterances per workgroup)."""
import ctypes
import struct
import types

import numpy as np
import pytest
import torch

import align_ref as R
from golden_util import fbank_for
from casr import lib as L
from casr.config import CasrConfig
from casr.weights import synthetic_state_dicts

pytestmark = pytest.mark.gpu

CFG = CasrConfig()
KEYS = ("first", "last", "peak", "path_score")
# the issue's shapes, then two of this file's at which the plan halves the utterances of a workgroup
# (csrc/align_plan.h: their LDS must fit a CU): (20, 100, 300) takes 8 where 16 are asked for, and
# (3, 512, 1024), the largest the entry accepts, 1 whatever is asked
SHAPES = [(1, 1, 1), (1, 3, 2), (17, 7, 63), (16, 40, 64), (33, 41, 65), (5, 40, 129), (65, 12, 266),
          (20, 100, 300), (3, 512, 1024)]


@pytest.fixture(scope="module")
def eng():
    from casr.engine import Engine
    e = Engine(CFG)  # no weights: the path needs none
    yield e
    e.close()


def device(eng, a, enc, tgt):
    r = eng.align_path(torch.from_numpy(np.ascontiguousarray(a)), enc, tgt)
    return {k: v.cpu().numpy() for k, v in r.items()}


def same(got, want, tag=""):
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (tag, k)


# ---------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-L%d-Tp%d" % s)
def test_equals_the_host_entry(eng, shape):
    B, Lx, Tp = shape
    eng.device_flags()
    for g, gen in enumerate(R.GENERATORS):
        a, enc, tgt = R.seeded_case(4 * (B + Lx + Tp) + g, B, Lx, Tp)
        assert R.GENERATORS[(4 * (B + Lx + Tp) + g) % 4] is gen
        got = device(eng, a, enc, tgt)
        same(got, L.align_path_host(a, enc, tgt), gen.__name__)
        R.check_invariants(a, enc, tgt, got)
    # every utterance at full length (the last chunk and the last row of the buffers)
    a = R.softmax_rows(np.random.RandomState(B), B, Lx, Tp)
    full_t, full_n = np.full(B, Tp, np.int32), np.full(B, Lx, np.int32)
    same(device(eng, a, full_t, full_n), L.align_path_host(a, full_t, full_n), "full")
    if Tp > 1:
        a, enc, tgt, first, last = R.planted(np.random.RandomState(B + 1), B, Lx, Tp)
        got = device(eng, a, enc, tgt)
        assert np.array_equal(got["first"], first) and np.array_equal(got["last"], last)
        assert np.array_equal(got["path_score"], -128 * enc)
    assert eng.device_flags() == 0


def test_independent_of_batch_and_neighbours(eng):
    """The same utterance at b = 0 and at b = 16 of a larger batch, and alone: equal rows."""
    Lx, Tp = 41, 65
    a, enc, tgt = R.seeded_case(12, 33, Lx, Tp)
    enc[0], tgt[0] = 65, 41
    a[:, :, 16], enc[16], tgt[16] = a[:, :, 0], enc[0], tgt[0]
    big = device(eng, a, enc, tgt)
    alone = device(eng, a[:, :, :1], enc[:1], tgt[:1])
    for k in KEYS:
        assert np.array_equal(big[k][0], big[k][16]) and np.array_equal(big[k][0], alone[k][0]), k
    same(big, L.align_path_host(a, enc, tgt))


def test_every_group_size_gives_the_same_bits(eng):
    a, enc, tgt = R.seeded_case(5, 33, 41, 65)
    want = L.align_path_host(a, enc, tgt)
    try:
        for g in (1, 2, 4, 8, 16):
            eng.set_option("ALIGN_GROUP", g)
            same(device(eng, a, enc, tgt), want, g)
        with pytest.raises(L.CasrError):
            eng.set_option("ALIGN_GROUP", 3)
        # 16 asked for where only 8 fit a CU's LDS, and where only 1 does
        for seed, shape in ((6, (20, 100, 300)), (7, (3, 512, 1024))):
            a, enc, tgt = R.seeded_case(seed, *shape)
            eng.set_option("ALIGN_GROUP", 16)
            same(device(eng, a, enc, tgt), L.align_path_host(a, enc, tgt), shape)
    finally:
        eng.set_option("ALIGN_GROUP", 0)


def test_clamps_raise_the_guard_bit_and_nothing_past_a_length_is_read(eng):
    a, enc, tgt = R.seeded_case(7, 19, 9, 70)
    eng.device_flags()
    same(device(eng, a, enc, tgt), L.align_path_host(a, enc, tgt))
    assert eng.device_flags() == 0
    for b, (e, t) in ((3, (None, 9 + 3)), (17, (-1, None)), (0, (70 + 1, -2))):
        enc2, tgt2 = enc.copy(), tgt.copy()
        if e is not None:
            enc2[b] = e
        if t is not None:
            tgt2[b] = t
        got = device(eng, a, enc2, tgt2)
        assert eng.device_flags() == 1
        same(got, L.align_path_host(a, np.clip(enc2, 0, 70), np.clip(tgt2, 0, 9)), b)
    want = L.align_path_host(a, enc, tgt)
    p = a.copy()
    for b in range(19):
        p[:, enc[b]:, b] = np.nan
        p[tgt[b]:, :, b] = np.nan
    same(device(eng, p, enc, tgt), want)
    assert eng.device_flags() == 0


def test_unsupported_tp_writes_nothing(eng):
    Tp = L.ALIGN_MAX_TP + 1
    dev = eng.device
    a = torch.full((1, Tp, 1), 0.5, device=dev)
    one = torch.ones(1, dtype=torch.int32, device=dev)
    out = [torch.full((1, 1), 77, dtype=torch.int32, device=dev) for _ in range(4)]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = eng.lib.casr_align_path(eng.handle, ptr(a), ptr(one), ptr(one), 1, Tp, 1, *[ptr(o) for o in out], None)
    assert L.STATUS[rc] == "CASR_ERR_UNSUPPORTED"
    rc = eng.lib.casr_align_path(eng.handle, ptr(a), ptr(one), ptr(one), 1, 4, 513, *[ptr(o) for o in out], None)
    assert L.STATUS[rc] == "CASR_ERR_ARG"
    torch.cuda.synchronize()
    assert all(int(o[0, 0]) == 77 for o in out)
    with pytest.raises(L.CasrError, match="CASR_ERR_UNSUPPORTED"):
        eng.align_path(a, one, one)


def test_repeat_calls_give_equal_bits(eng):
    a, enc, tgt = R.seeded_case(0, 65, 12, 266)
    x, y = device(eng, a, enc, tgt), device(eng, a, enc, tgt)
    same(x, y)


# ---------------------------------------------------------------------------- 2. end to end
FRAMES = [120, 96, 75, 120, 48]  # B = 5, T = 120 log-mel frames (40 encoder frames)
I2W = {i: chr(0x4E00 + i) for i in range(CFG.vocab)}  # tokens <-> characters, one to one


@pytest.fixture(scope="module")
def model():
    import model as M
    m = M.Model()
    m.load_state_dicts(*synthetic_state_dicts(CFG, peaked=True))
    yield m
    m.engine.close()


def batch(m):
    x = np.zeros((len(FRAMES), max(FRAMES), 80), np.float32)
    for b, t in enumerate(FRAMES):
        x[b, :t] = fbank_for(b, t)
    feat, flen = m.engine.features(torch.from_numpy(x).to(m.device),
                                   torch.tensor(FRAMES, dtype=torch.int32, device=m.device), eps=1e-6)
    return feat, flen.cpu()


def check_timing(res, flen):
    assert res.timing is not None and len(res.timing) == len(FRAMES)
    for b, (text, spans) in enumerate(zip(res.pred_text, res.timing)):
        assert len(spans) == len(text), b
        end = int(flen[b]) * 0.03 + 1e-9
        starts = [s[0] for s in spans]
        assert starts == sorted(starts)
        for start, stop, peak, conf in spans:
            assert 0.0 <= start <= peak < stop <= end and 0.0 < conf <= 1.0


@pytest.mark.parametrize("prec", ["s16x3", "f32"])
def test_greedy_timestamps(model, prec):
    from casr.results import token_spans
    m = model
    m.engine.set_precision(prec)
    # the three-launch step: the arithmetic the scoring pass shares with greedy bit for bit
    # (tests/test_gpu_score.py test_same_arithmetic_as_three_launch_greedy)
    m.engine.set_option("DEC_FOLD", 0)
    try:
        feat, flen = batch(m)
        plain = m.eval_one_batch_with_greedy(m.device, feat, flen, I2W)
        assert plain.timing is None
        timed = m.eval_one_batch_with_greedy(m.device, feat, flen, I2W, timestamps=True)
        assert timed.pred_text == plain.pred_text and timed.score == plain.score
        assert any(len(t) for t in timed.pred_text)
        check_timing(timed, flen)
        # the path through greedy's own attention (the bits the scoring pass reproduces) gives the same spans
        n = timed.text_len.cpu().numpy()
        tgt_len = np.minimum(n + 1, CFG.max_len).astype(np.int32)
        align = torch.zeros(CFG.max_len, feat.shape[1], len(FRAMES), device=m.device)
        align[:len(timed.alignment)] = torch.stack(list(timed.alignment))
        r = {k: v.cpu().numpy() for k, v in m.engine.align_path(align, flen, tgt_len).items()}
        assert m.engine.device_flags() == 0
        same(r, L.align_path_host(align.cpu().numpy(), flen.numpy(), tgt_len))
        spans = token_spans(r["first"], r["last"], r["peak"], np.zeros((len(FRAMES), CFG.max_len)), tgt_len, n_tokens=n)
        for b in range(len(FRAMES)):
            assert [s[:3] for s in spans[b]] == [s[:3] for s in timed.timing[b]], b
        # the default (folded) greedy step: the same text, and times of the same form
        m.engine.set_option("DEC_FOLD", 1)
        fold = m.eval_one_batch_with_greedy(m.device, feat, flen, I2W, timestamps=True)
        assert fold.pred_text == m.eval_one_batch_with_greedy(m.device, feat, flen, I2W).pred_text
        check_timing(fold, flen)
    finally:
        m.engine.set_option("DEC_FOLD", 1)
        m.engine.set_precision("s16x3")


@pytest.mark.parametrize("prec", ["s16x3", "f32"])
def test_beam_timestamps(model, prec):
    m = model
    m.engine.set_precision(prec)
    try:
        feat, flen = batch(m)
        kw = dict(second_pass=False, lm_model=None, lm_weight=0.0, length_weight=0.0)
        plain = m.eval_one_batch_with_beam(m.device, 4, feat, flen, None, I2W, **kw)
        assert plain.timing is None and m.beam_unfinished is None
        want_cut = ~m.engine.beam_records()[2].flatten(1).bool().any(1).cpu()
        timed = m.eval_one_batch_with_beam(m.device, 4, feat, flen, None, I2W, timestamps=True, **kw)
        assert timed.pred_text == plain.pred_text and timed.score == plain.score
        assert torch.equal(m.beam_unfinished.cpu(), want_cut)
        check_timing(timed, flen)
    finally:
        m.engine.set_precision("s16x3")


class _StubLM:
    """a host scorer (KenLM's interface): the host second pass, which no device mode can read"""

    def score(self, sentence, bos=True):
        return -0.3 * len(sentence.split())


def test_timestamps_whatever_chose_the_tokens(model):
    """The host second pass (scored once the host has chosen) and the MBR choice (scored inside the
    guarded decode): the same text and score as without timestamps, and timing for that text."""
    m = model
    feat, flen = batch(m)
    for kw in (dict(second_pass=True, lm_model=_StubLM(), lm_weight=1.5, length_weight=1.5),
               dict(second_pass=False, lm_model=None, lm_weight=0.0, length_weight=1.5, mbr=0.5)):
        plain = m.eval_one_batch_with_beam(m.device, 4, feat, flen, None, I2W, **kw)
        timed = m.eval_one_batch_with_beam(m.device, 4, feat, flen, None, I2W, timestamps=True, **kw)
        assert timed.pred_text == plain.pred_text and timed.score == plain.score and plain.timing is None
        assert m.beam_unfinished is not None and m.beam_unfinished.shape == (len(FRAMES),)
        check_timing(timed, flen)


def _write_wav16(path, x, rate=16000):
    data = np.clip(np.rint(x * 32768.0), -32768, 32767).astype("<i2").tobytes()
    hdr = struct.pack("<HHIIHH", 1, 1, rate, rate * 2, 2, 16)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<I", 16) + hdr)
        f.write(b"data" + struct.pack("<I", len(data)) + data)


def test_transcribe_fills_chars_inside_each_segment(model, tmp_path):
    """Two 2.5 s bursts of modulated noise 2 s apart: the segments, texts and scores of transcribe are
    those without timestamps, and every character lies inside its segment."""
    import main as MN
    from casr import subtitles
    rs = np.random.RandomState(5)
    t = np.arange(int(2.5 * 16000)) / 16000.0
    burst = lambda: 0.3 * rs.standard_normal(t.size) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t))  # noqa: E731
    quiet = lambda s: 1e-4 * rs.standard_normal(int(s * 16000))  # noqa: E731
    path = str(tmp_path / "two.wav")
    _write_wav16(path, np.concatenate([quiet(0.5), burst(), quiet(2.0), burst(), quiet(0.5)]).astype(np.float32))
    ab = types.SimpleNamespace(int2word=I2W)
    plain = MN.transcribe([path], model, ab)[0]
    timed = MN.transcribe([path], model, ab, timestamps=True)[0]
    assert len(plain) == 2 and all(s.chars is None for s in plain)
    assert [(s.start_s, s.end_s, s.text, s.score, s.truncated) for s in timed] == \
        [(s.start_s, s.end_s, s.text, s.score, s.truncated) for s in plain]
    assert any(s.text for s in timed)
    for s in timed:
        assert len(s.chars) == len(s.text)
        assert [c[0] for c in s.chars] == list(s.text)
        for _, start, stop, conf in s.chars:
            assert s.start_s <= start < stop <= s.end_s + 1e-9 and 0.0 < conf <= 1.0
    beam = MN.transcribe([path], model, ab, bw=4, timestamps=True)[0]
    base = MN.transcribe([path], model, ab, bw=4)[0]
    assert [(s.text, s.score, s.truncated) for s in beam] == [(s.text, s.score, s.truncated) for s in base]
    assert all(len(s.chars) == len(s.text) for s in beam)
    srt = subtitles.to_srt(subtitles.cues(timed))
    assert srt.count("-->") >= sum(1 for s in timed if s.text)
