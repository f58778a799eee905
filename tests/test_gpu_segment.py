"""casr_segment and casr_gather_segments on the device (include/casr.h: long recordings cut at their
pauses) against the host entry casr_segment_host and the numpy restatement (tests/segment_ref.py):
after stage (a) everything is an integer, so thr, the counts, the starts and the lengths agree EXACTLY.

Shapes: T = 5,000 is 2.4 tiles of the decision kernel's 2,048 frames and 19.5 of the level kernel's 256
(several tiles, ending inside one); rows of n = (5,000, about 60 % of it, 1, 0); the small parameters
(max_frames 64), so a row holds about a hundred segments and runs, islands and segments cross every tile
boundary.  Rows past frames[b] hold NaN: they are never read as data."""
import ctypes
import functools
import struct
import types

import numpy as np
import pytest
import torch

import segment_ref as R
from casr import lib as L
from casr.config import CasrConfig
from casr.segment import SegmentParams, segment_bound, segment_host
from casr.weights import synthetic_state_dicts

pytestmark = pytest.mark.gpu

CFG = CasrConfig()
SMALL = R.SMALL
T0 = 5000


@pytest.fixture(scope="module")
def eng():
    from casr.engine import Engine
    e = Engine(CFG)  # front end only: no weights
    yield e
    e.close()


def params_of(p):
    return SegmentParams(**{k: getattr(p, k) for k in p.__dataclass_fields__})


def batch_of(rows, T):
    """rows: fbank arrays [n_b, 80] -> (fbank [B, T, 80] with NaN past each n_b, frames [B])."""
    fb = np.full((len(rows), T, 80), np.nan, np.float32)
    for b, r in enumerate(rows):
        fb[b, :len(r)] = r
    return fb, np.array([len(r) for r in rows], np.int32)


@functools.lru_cache(maxsize=None)
def seeded(seed):
    """B = 4 rows of n = (5000, about 60 %, 1, 0) and the reference's results (computed once, shared)."""
    ns = (T0, int(0.6 * T0) | 1, 1, 0)
    rows = [R.fbank_from_levels(R.random_levels(n, 10 * seed + b), 10 * seed + b) for b, n in enumerate(ns)]
    fb, frames = batch_of(rows, T0)
    ref = [R.segment_fbank(r, len(r), SMALL) for r in rows]
    fb.setflags(write=False)
    return fb, frames, ref


def run(eng, fb, frames, p, s_max=None):
    out = eng.segment(torch.tensor(np.asarray(fb)), torch.tensor(np.asarray(frames), dtype=torch.int32),
                      params_of(p), s_max)
    return tuple(x.cpu().numpy() for x in out)


def listed(start, length, n_seg, b):
    return list(zip(start[b, :n_seg[b]].tolist(), length[b, :n_seg[b]].tolist()))


def check(eng, fb, frames, p, ref=None):
    """device == host entry == reference, and a clean guard word."""
    start, length, n_seg, thr = run(eng, fb, frames, p)
    assert eng.device_flags() == 0
    hs, hl, hn, ht = segment_host(fb, frames, params_of(p))
    assert np.array_equal(thr, ht) and np.array_equal(n_seg, hn)
    assert np.array_equal(start, hs) and np.array_equal(length, hl)  # the -1 past each count included
    for b in range(len(frames)):
        rt, segs = ref[b] if ref is not None else R.segment_fbank(fb[b], int(frames[b]), p)
        assert thr[b] == rt and listed(start, length, n_seg, b) == segs, b
    return start, length, n_seg, thr


# ---------------------------------------------------------------- 1. exact agreement
@pytest.mark.parametrize("seed", range(12))
def test_device_equals_host_and_reference(eng, seed):
    fb, frames, ref = seeded(seed)
    first = check(eng, fb, frames, SMALL, ref)
    assert first[2][0] > 50 and first[2][2] == 0 and first[2][3] == 0
    again = run(eng, fb, frames, SMALL)  # the histogram workspace is cleared per call: the same bits
    assert all(np.array_equal(a, b) for a, b in zip(first, again)) and eng.device_flags() == 0


def test_run_boundaries_on_tile_edges(eng):
    """Active and quiet stretches of 64 frames whose boundaries sit at every multiple of 64 (so of 256,
    1,024 and 2,048 too) - 1, + 0 and + 1; a row whose stretches are 1,024 long; all four in one batch."""
    t = np.arange(T0)
    rows = [R.fbank_from_levels(np.where(((t - d) // 64) % 2 == 0, -2.0, -9.0), 40 + d) for d in (-1, 0, 1)]
    rows.append(R.fbank_from_levels(np.where(((t + 1) // 1024) % 2 == 0, -2.0 + 0.5 * np.sin(t / 9.0), -9.0), 44))
    fb, frames = batch_of(rows, T0)
    d = {}
    R.segment_fbank(rows[1], T0, SMALL, d)
    a0 = d["a0"]
    edges = np.flatnonzero(a0[1:] != a0[:-1]) + 1
    assert set(range(64, T0, 64)) <= set(edges.tolist())  # the reference sees a boundary on every multiple
    start, length, n_seg, _ = check(eng, fb, frames, SMALL)
    assert n_seg.min() > 2


def test_one_island_spans_the_row(eng):
    """Two quiet frames at each end and pct_lo = 0: one island, widened to [0, n), cut about n / 64 times."""
    p = R.replace(SMALL, pct_lo=0)
    lv = np.full(T0, -2.0) + 0.6 * np.sin(np.arange(T0) / 7.0)
    lv[:2] = lv[-2:] = -9.0
    row = R.fbank_from_levels(lv, 50, noise=0.2)
    d = {}
    R.segment_fbank(row, T0, p, d)
    assert d["islands"] == [(0, T0)] and len(d["cuts"]) >= T0 // 64
    fb, frames = batch_of([row], T0)
    check(eng, fb, frames, p)


def test_default_parameters(eng):
    T = 12000
    rows = [R.fbank_from_levels(R.random_levels(n, 60 + b, mean_on=300, mean_off=60), 60 + b)
            for b, n in enumerate((T, 7001))]
    fb, frames = batch_of(rows, T)
    d = {}
    R.segment_fbank(rows[0], T, R.P(), d)
    assert len(d["cuts"]) >= 1 and len(d["pieces"]) > 8
    check(eng, fb, frames, R.P())


def test_tie_takes_the_largest_cut(eng):
    """A constant level: every cut of the window costs the same; the lanes' reduction must pick the largest."""
    lv = np.concatenate([np.full(30, -9.0), np.full(700, -2.0), np.full(300, -9.0)])
    row = R.fbank_from_levels(lv, 70, noise=0.0)
    d = {}
    R.segment_fbank(row, len(row), SMALL, d)
    assert all(ties > 1 for _, ties in d["cuts"]) and len(d["cuts"]) >= 10
    fb, frames = batch_of([row], len(row))
    check(eng, fb, frames, SMALL)


# ---------------------------------------------------------------- 2. independence
def test_independent_of_batch_and_padding(eng):
    fb, frames, ref = seeded(0)
    n = int(frames[1])
    alone = run(eng, fb[1:2, :n], [n], SMALL)
    rows = [fb[0, :700], fb[3, :0], fb[1, :n], fb[0, :2000]]
    big, fr = batch_of(rows, T0 + 1500)
    inside = run(eng, big, fr, SMALL, s_max=alone[0].shape[1] + 11)
    assert eng.device_flags() == 0
    assert alone[2][0] == inside[2][2] == len(ref[1][1]) and alone[3][0] == inside[3][2] == ref[1][0]
    assert listed(*alone[:3], 0) == listed(*inside[:3], 2) == ref[1][1]


def test_s_max_smaller_than_count(eng):
    fb, frames, ref = seeded(1)
    start, length, n_seg, _ = run(eng, fb, frames, SMALL, s_max=7)
    assert eng.device_flags() == 0
    assert n_seg.tolist() == [len(r[1]) for r in ref] and n_seg[0] > 7
    for b in range(4):
        w = min(7, int(n_seg[b]))
        assert list(zip(start[b, :w].tolist(), length[b, :w].tolist())) == ref[b][1][:w]
        assert (start[b, w:] == -1).all() and (length[b, w:] == -1).all()
    assert run(eng, fb, frames, SMALL, s_max=0)[2].tolist() == n_seg.tolist()


# ---------------------------------------------------------------- 3. guards and errors
def test_frames_out_of_range_are_clamped(eng):
    fb, frames, ref = seeded(2)
    full = np.array(fb)
    full[np.isnan(full)] = -9.0  # every row readable to T
    want = run(eng, full, [T0, T0, 0, 0], SMALL)
    assert eng.device_flags() == 0
    got = run(eng, full, [T0, T0 + 5, -1, 0], SMALL)
    assert eng.device_flags() & 64
    assert all(np.array_equal(a, b) for a, b in zip(want, got))
    assert eng.device_flags() == 0  # read and clear


def test_argument_errors(eng):
    fb = torch.zeros(1, 64, 80, device=eng.device)
    fr = torch.tensor([64], dtype=torch.int32, device=eng.device)
    with pytest.raises(ValueError):
        eng.segment(fb, fr, SegmentParams(min_pause=16))  # not > 2 pad
    out = torch.zeros(4, dtype=torch.int32, device=eng.device)
    c = SegmentParams(min_frames=500).struct()  # 2 min_frames > max_frames
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = eng.lib.casr_segment(eng.handle, p(fb), p(fr), 1, 64, ctypes.byref(c), 4, p(out), p(out), p(out), None, None)
    assert rc == 1 and b"invalid parameters" in eng.lib.casr_last_error(eng.handle)
    c = SegmentParams().struct()
    assert eng.lib.casr_segment(eng.handle, p(fb), p(fr), 0, 64, ctypes.byref(c), 4, p(out), p(out), p(out), None, None) == 1
    assert eng.lib.casr_segment(eng.handle, p(fb), None, 1, 64, ctypes.byref(c), 4, p(out), p(out), p(out), None, None) == 1
    assert eng.lib.casr_gather_segments(eng.handle, p(fb), 1, 64, p(out), p(out), p(out), 0, 8, p(fb), p(out), None) == 1
    assert eng.lib.casr_gather_segments(eng.handle, ctypes.c_void_p(fb.data_ptr() + 4), 1, 63, p(out), p(out), p(out), 1, 8,
                                        p(fb), p(out), None) == 1
    torch.cuda.synchronize()
    assert eng.device_flags() == 0 and out.tolist() == [0, 0, 0, 0]  # nothing was launched or written


# ---------------------------------------------------------------- 4. gather
def test_gather_segments(eng):
    rs = np.random.RandomState(3)
    B, T = 3, 700
    fb = rs.standard_normal((B, T, 80)).astype(np.float32)
    src = [2, 0, 1, 1, 0, 2]
    start = [0, 13, 699, 640, 300, 1]
    length = [64, 1, 1, 60, 37, 9]  # a segment ending at T (640 + 60), one of one frame at T - 1
    t_seg = 70
    out, fo = eng.gather_segments(torch.from_numpy(fb), src, start, length, t_seg=t_seg)
    out, fo = out.cpu().numpy(), fo.cpu().numpy()
    assert eng.device_flags() == 0 and fo.tolist() == length and out.shape == (6, t_seg, 80)
    for s in range(6):
        want = np.zeros((t_seg, 80), np.float32)
        want[:length[s]] = fb[src[s], start[s]:start[s] + length[s]]
        assert np.array_equal(out[s].view(np.uint32), want.view(np.uint32)), s  # tails exactly +0
    # t_seg defaults to the longest length
    o2, f2 = eng.gather_segments(torch.from_numpy(fb), src, start, length)
    assert o2.shape == (6, 64, 80) and np.array_equal(o2.cpu().numpy(), out[:, :64])
    assert eng.device_flags() == 0
    # out-of-range entries are clamped, never followed: guard bit 64
    for bad_src, bad_start, bad_len, want_len, row in (([3], [0], [5], 5, fb[2, 0:5]), ([-1], [0], [5], 5, fb[0, 0:5]),
                                                       ([1], [690], [20], 10, fb[1, 690:700]), ([1], [-4], [6], 6, fb[1, 0:6]),
                                                       ([1], [10], [80], 70, fb[1, 10:80]), ([1], [10], [-3], 0, fb[1, 0:0]),
                                                       ([1], [800], [5], 0, fb[1, 0:0])):
        o, f = eng.gather_segments(torch.from_numpy(fb), bad_src, bad_start, bad_len, t_seg=t_seg)
        assert eng.device_flags() & 64
        assert f.tolist() == [want_len]
        o = o.cpu().numpy()[0]
        assert np.array_equal(o[:want_len], row) and not o[want_len:].any()


# ---------------------------------------------------------------- 5. end to end
def _write_wav16(path, x, rate=16000):
    data = np.clip(np.rint(x * 32768.0), -32768, 32767).astype("<i2").tobytes()
    hdr = struct.pack("<HHIIHH", 1, 1, rate, rate * 2, 2, 16)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<I", 16) + hdr)
        f.write(b"data" + struct.pack("<I", len(data)) + data)


def test_transcribe_equals_per_segment_decode(tmp_path):
    """main.transcribe on the 35 s synthetic signal (and a 6 s recording in the same call): the device's
    segments are the reference's on the device's own fbank, and every segment's text and score are what
    the existing chain (Engine.features -> encode -> greedy, or beam 4) gives on a batch built on the host
    from the same slices in the same order."""
    import data as D
    import main as MN
    import model as M
    from casr.results import greedy_outputs
    paths = [str(tmp_path / "long.wav"), str(tmp_path / "short.wav")]
    _write_wav16(paths[0], R.synthetic_recording(7))
    _write_wav16(paths[1], R.synthetic_recording(8)[:6 * 16000])
    m = M.Model()
    m.load_state_dicts(*synthetic_state_dicts(CFG, peaked=True))
    ab = types.SimpleNamespace(int2word={i: f"<{i}>" for i in range(CFG.vocab)})  # text <-> tokens, one to one
    word = ab.int2word.__getitem__
    # the device's own fbank, and the reference segmentation of it
    audios = MN.read_audio(paths)
    wav = np.zeros((2, max(len(a) for a in audios)), np.float32)
    for b, a in enumerate(audios):
        wav[b, :len(a)] = a
    fe = D._engine()
    fb_d, frames_d = fe.log_mel(torch.from_numpy(wav).to(fe.device), torch.tensor([len(a) for a in audios], dtype=torch.int32))
    fb, frames = fb_d.cpu().numpy(), frames_d.cpu().numpy()
    assert frames.tolist() == [L.log_mel_frames(len(a)) for a in audios]
    details = [{}, {}]
    ref = [R.segment_fbank(fb[b], int(frames[b]), R.P(), details[b]) for b in range(2)]
    assert len(ref[0][1]) >= 4 and len(details[0]["cuts"]) >= 1 and len(details[0]["pieces"]) > len(ref[0][1])
    assert len(ref[1][1]) >= 1
    start, length, n_seg, thr = (x.cpu().numpy() for x in fe.segment(fb_d, frames_d))
    assert fe.device_flags() == 0
    for b in range(2):
        assert thr[b] == ref[b][0] and listed(start, length, n_seg, b) == ref[b][1]
    # the host-built batch of the same slices in (recording, time) order
    flat = [(b, s, l) for b in range(2) for s, l in ref[b][1]]
    assert all(l >= MN.MIN_SEGMENT_FRAMES for _, _, l in flat)
    t_seg = max(l for _, _, l in flat)
    batch = np.zeros((len(flat), t_seg, 80), np.float32)
    for i, (b, s, l) in enumerate(flat):
        batch[i, :l] = fb[b, s:s + l]
    lens = torch.tensor([l for _, _, l in flat], dtype=torch.int32, device=m.device)
    feat, flen = m.engine.features(torch.from_numpy(batch).to(m.device), lens, eps=1e-6)

    def compare(got, texts, scores, cut):
        assert [len(g) for g in got] == [len(ref[0][1]), len(ref[1][1])]
        for i, ((b, s, l), seg) in enumerate(zip(flat, got[0] + got[1])):
            assert seg.start_s == s * 0.01 and seg.end_s == (s + l) * 0.01
            assert seg.text == texts[i] and seg.score == scores[i] and seg.truncated == cut[i], i

    got = MN.transcribe(paths, m, ab)
    m.engine.encode(feat, flen)
    out = m.engine.greedy(alignment=True)
    assert m.engine.device_flags() == 0
    out_len = out["out_len"].cpu().numpy()
    toks, scores = greedy_outputs(out["tokens"].cpu().numpy(), out_len, out["finished"].cpu().numpy().astype(bool),
                                  out["accum"].cpu().numpy())
    compare(got, ["".join(map(word, t)) for t in toks], scores, (out_len >= CFG.max_len).tolist())
    assert any(len(t) for t in toks)

    got = MN.transcribe(paths, m, ab, bw=4)
    m.engine.encode(feat, flen)
    r = m.engine.beam(4, 1.5, 1.5)
    assert m.engine.device_flags() == 0
    bt, bl, bs = r["tokens"].cpu().numpy(), r["length"].cpu().numpy(), r["score"].cpu().numpy()
    none_finished = (~m.engine.beam_records()[2].cpu().numpy().reshape(len(flat), -1).any(1)).tolist()
    compare(got, ["".join(map(word, bt[i, :bl[i]].tolist())) for i in range(len(flat))], [float(x) for x in bs],
            none_finished)
    # batch_size smaller than the count: the same segments and times (the decode batches differ)
    small = MN.transcribe(paths, m, ab, batch_size=3)
    assert [[(s.start_s, s.end_s) for s in rec] for rec in small] == [[(s.start_s, s.end_s) for s in rec] for rec in got]
    # parse is untouched: the 6 s file alone gives what its own chain gives
    f1, l1 = D.log_mel_batch([audios[1]], cmvn_eps=1e-6)
    m.engine.encode(f1, l1)
    o1 = m.engine.greedy(alignment=True)
    t1, _ = greedy_outputs(o1["tokens"].cpu().numpy(), o1["out_len"].cpu().numpy(),
                           o1["finished"].cpu().numpy().astype(bool), o1["accum"].cpu().numpy())
    assert MN.parse(paths[1], m, ab, None, None) == "".join(map(word, t1[0]))
