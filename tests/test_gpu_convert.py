"""casr_convert_audio on the device (include/casr.h: downmix, polyphase Kaiser-sinc resampling to 16 kHz,
s16 quantisation, peak normalisation) against the numpy restatement of its formulas
(tests/resample_ref.py): float64 is the reference, and the float32 restatement's own distance from it
sets the device's budget (8 times, the project's rule).

Shapes: the longest signal is 0.5 s, which is 8,000 outputs = 15.6 tiles of 512, so every case spans
several tiles and ends inside one; rows are (full, about 60 % of it, 1 frame).  Each accuracy case prints
an "[acc] convert ..." line (tools/acc_lines.py turns them into profiles/convert/accuracy.json).

MEASURED on one MI355X (profiles/convert/accuracy.json): the device's largest error is
0.89 to 1.03 times the float32 restatement's (2.1e-7 to 2.8e-7); 4 to 10 of 12,800 quantised samples
differ from rint of the float64 reference, all within 0.02 LSB of a tie."""
import ctypes
import functools
import struct

import numpy as np
import pytest
import torch

import resample_ref as R
from casr import lib as L
from casr.config import CasrConfig
from casr.weights import synthetic_state_dicts

pytestmark = pytest.mark.gpu

CFG = CasrConfig()
MARGIN = 8.0
CASES = [(8000, 1), (11025, 1), (44100, 1), (48000, 1), (96000, 1), (48000, 2)]


@pytest.fixture(scope="module")
def eng():
    from casr.engine import Engine
    e = Engine(CFG)  # front end only: no weights
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def case(rate, ch):
    """Seeded noise of rms 0.2, B = 3 rows of (full, about 60 %, 1) frames, and both restatements'
    outputs per row (computed once, shared by the tests, never modified)."""
    n = rate // 2
    n_in = (n, int(0.6 * n) | 1, 1)
    rs = np.random.RandomState(rate + ch)
    pcm = (0.2 * rs.standard_normal((3, n, ch))).astype(np.float32)
    ref64 = [R.convert(pcm[b, :n_in[b]].astype(np.float64), rate, np.float64)[0] for b in range(3)]
    ref32 = [R.convert(pcm[b, :n_in[b]], rate, np.float32)[0] for b in range(3)]
    for a in [pcm] + ref64 + ref32:
        a.setflags(write=False)
    e_ref = max(float(np.abs(ref32[b].astype(np.float64) - ref64[b]).max()) for b in range(3))
    return dict(pcm=pcm, n_in=n_in, ref64=ref64, ref32=ref32, e_ref=e_ref, K=R.plan(rate)[2])


def run(eng, pcm, n_in, rate, quantize=False, norm_db=0.0, m_max=None):
    wav, n_out, gain = eng.convert_audio(torch.tensor(np.asarray(pcm)), torch.tensor(n_in, dtype=torch.int32),
                                         rate, quantize=quantize, norm_db=norm_db, m_max=m_max)
    return wav.cpu().numpy(), n_out.cpu().numpy(), gain.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- 1. accuracy budget
@pytest.mark.parametrize("rate,ch", CASES)
def test_accuracy_budget(eng, rate, ch):
    c = case(rate, ch)
    wav, n_out, _ = run(eng, c["pcm"], c["n_in"], rate)
    assert eng.device_flags() == 0
    e_dev, sq_dev, sq_ref, cnt = 0.0, 0.0, 0.0, 0
    for b in range(3):
        ref = c["ref64"][b]
        assert n_out[b] == len(ref)
        d = wav[b, :len(ref)].astype(np.float64) - ref
        e_dev = max(e_dev, float(np.abs(d).max()))
        sq_dev += float((d * d).sum())
        sq_ref += float(((c["ref32"][b].astype(np.float64) - ref) ** 2).sum())
        cnt += len(ref)
    print(f"[acc] convert {rate}x{ch} f32 wav max_ratio={e_dev / c['e_ref']:.3f} rms_ratio={np.sqrt(sq_dev / sq_ref):.3f} "
          f"e_ref_max={c['e_ref']:.3e} e_max={e_dev:.3e}")
    assert e_dev <= MARGIN * c["e_ref"], (e_dev, c["e_ref"])


# ---------------------------------------------------------------- 2. edges and padding
@pytest.mark.parametrize("rate,ch", CASES)
def test_edges_and_padding(eng, rate, ch):
    c = case(rate, ch)
    K = c["K"]
    need = L.resample_frames(c["pcm"].shape[1], rate)
    m_max = need + 700  # more than a tile of padding behind the longest row
    wav, n_out, _ = run(eng, c["pcm"], c["n_in"], rate, m_max=m_max)
    assert eng.device_flags() == 0
    assert wav.shape == (3, m_max)
    for b in range(3):
        ref = c["ref64"][b]
        assert n_out[b] == len(ref) == R.frames(c["n_in"][b], rate)
        got = wav[b, :len(ref)].astype(np.float64)
        # the first and last K outputs, where the zero extension of the signal matters
        for sl in (slice(0, K), slice(max(len(ref) - K, 0), len(ref))):
            assert np.abs(got[sl] - ref[sl]).max() <= MARGIN * c["e_ref"]
        assert not bits(wav[b, len(ref):]).any()  # exactly +0 past n_out
    # samples past n_in[b] are never read as data
    poisoned = c["pcm"].copy()
    for b in range(3):
        poisoned[b, c["n_in"][b]:] = np.nan
    wav2, n_out2, _ = run(eng, poisoned, c["n_in"], rate, m_max=m_max)
    assert eng.device_flags() == 0
    assert np.array_equal(bits(wav2), bits(wav)) and np.array_equal(n_out2, n_out)


# ---------------------------------------------------------------- 3. independence and determinism
@pytest.mark.parametrize("rate,ch", CASES)
def test_independence_and_determinism(eng, rate, ch):
    c = case(rate, ch)
    wav, n_out, _ = run(eng, c["pcm"], c["n_in"], rate)
    again, _, _ = run(eng, c["pcm"], c["n_in"], rate)
    assert np.array_equal(bits(again), bits(wav))
    n1 = c["n_in"][1]
    alone, n_alone, _ = run(eng, c["pcm"][1:2, :n1 + 3], [n1], rate, m_max=int(n_out[1]) + 1234)
    assert n_alone[0] == n_out[1]
    assert np.array_equal(bits(alone[0, :n_out[1]]), bits(wav[1, :n_out[1]]))
    assert not bits(alone[0, n_out[1]:]).any()


# ---------------------------------------------------------------- 4. pass-through
def test_pass_through_16k(eng):
    rs = np.random.RandomState(16)
    mono = (0.3 * rs.standard_normal((2, 3000, 1))).astype(np.float32)
    wav, n_out, gain = run(eng, mono, [3000, 1777], 16000)
    assert n_out.tolist() == [3000, 1777] and gain.tolist() == [1.0, 1.0]
    assert np.array_equal(bits(wav[0]), bits(mono[0, :, 0]))
    assert np.array_equal(bits(wav[1, :1777]), bits(mono[1, :1777, 0])) and not bits(wav[1, 1777:]).any()
    st = (0.3 * rs.standard_normal((2, 3000, 2))).astype(np.float32)
    wav, n_out, _ = run(eng, st, [3000, 1777], 16000)
    want = (st[..., 0] + st[..., 1]) * np.float32(0.5)
    assert np.array_equal(bits(wav[0]), bits(want[0]))
    assert np.array_equal(bits(wav[1, :1777]), bits(want[1, :1777])) and not bits(wav[1, 1777:]).any()
    assert eng.device_flags() == 0


# ---------------------------------------------------------------- 5. quantise
@pytest.mark.parametrize("rate,ch", [(8000, 1), (48000, 1), (48000, 2)])
def test_quantise(eng, rate, ch):
    """wav 32768 is integral and equals rint of the float64 reference except where the reference lies
    within 0.02 LSB of a tie; there it differs by one LSB; at most 1 % of the samples differ (a condition:
    the float32 restatement differed at 8 of 8,000 at most, all within 0.005 LSB of a tie)."""
    c = case(rate, ch)
    wav, n_out, gain = run(eng, c["pcm"], c["n_in"], rate, quantize=True)
    assert eng.device_flags() == 0 and gain.tolist() == [1.0, 1.0, 1.0]
    bad = total = 0
    for b in range(3):
        ref = c["ref64"][b] * 32768.0
        q = wav[b, :n_out[b]].astype(np.float64) * 32768.0
        assert np.array_equal(q, np.rint(q)) and np.abs(q).max() <= 32768
        want = np.clip(np.rint(ref), -32768, 32767)
        miss = q != want
        assert (np.abs(q - want)[miss] == 1).all()
        frac = ref - np.floor(ref)
        assert (np.abs(frac[miss] - 0.5) <= 0.02).all()
        bad += int(miss.sum())
        total += len(ref)
        assert not bits(wav[b, n_out[b]:]).any()
    print(f"quantise {rate}x{ch}: {bad} of {total} differ from rint(float64)")
    assert bad <= 0.01 * total


# ---------------------------------------------------------------- 6. normalise
@pytest.mark.parametrize("rate", [16000, 48000])
def test_normalise(eng, rate):
    """Given the device's own quantised output, stage (d) is the float32 evaluation of its formula bit for
    bit, and gain is that g.  Rows: noise, silence, n_in = 0, and (at 16 kHz, where the samples pass
    through) a full-scale row, whose peak becomes rint(32768 10^(-1/20)) / 32768."""
    n = rate // 4
    rs = np.random.RandomState(rate + 6)
    pcm = np.zeros((4, n, 1), np.float32)
    pcm[0] = (0.2 * rs.standard_normal((n, 1))).astype(np.float32)
    pcm[3] = (0.5 * rs.standard_normal((n, 1))).astype(np.float32).clip(-0.9, 0.9)
    pcm[3, n // 3] = -1.0  # q = -32768
    n_in = [n, n - 7, 0, n]
    q, n_out, g1 = run(eng, pcm, n_in, rate, quantize=True, norm_db=0.0)
    out, n_out2, gain = run(eng, pcm, n_in, rate, quantize=True, norm_db=-1.0)
    assert eng.device_flags() == 0
    assert np.array_equal(n_out, n_out2) and n_out[2] == 0 and g1.tolist() == [1.0] * 4
    for b in range(4):
        want, g = R.normalise_q(q[b, :n_out[b]] * np.float32(32768), -1.0)
        assert np.array_equal(bits(out[b, :n_out[b]]), bits(want)), b
        assert bits(gain[b:b + 1])[0] == bits(np.array([g]))[0], (b, gain[b], g)
        assert not bits(out[b, n_out[b]:]).any()
    assert gain[1] == 1.0 and gain[2] == 1.0 and not out[1].any() and not out[2].any()
    if rate == 16000:
        assert np.abs(q[3]).max() == 1.0  # full scale: |q| = 32768
        assert np.abs(out[3]).max() == np.float32(np.rint(32768.0 * 10.0 ** (-1.0 / 20.0)) / 32768.0)
    # without quantisation: y g with g = float32(10^(-1/20)) / peak, on the device's own y
    y, n_out, _ = run(eng, pcm, n_in, rate, quantize=False, norm_db=0.0)
    out, _, gain = run(eng, pcm, n_in, rate, quantize=False, norm_db=-1.0)
    for b in range(4):
        want, g = R.normalise_y(y[b, :n_out[b]], -1.0)
        assert np.array_equal(bits(out[b, :n_out[b]]), bits(want)), b
        assert bits(gain[b:b + 1])[0] == bits(np.array([g]))[0]
    assert eng.device_flags() == 0


# ---------------------------------------------------------------- 7. tones on the device
def test_tones_on_the_device(eng):
    """The 48 kHz cases of tests/test_convert_host.py's quality test at 1 kHz (passband) and 9 kHz
    (which 16 kHz cannot carry), with its gates, on the device's float32 output."""
    n = 24000
    pcm = np.stack([R.tone(1000, 48000, n), R.tone(9000, 48000, n)]).astype(np.float32)[..., None]
    wav, n_out, _ = run(eng, pcm, [n, n], 48000)
    assert n_out.tolist() == [8000, 8000]
    e1 = R.tone_error_db(wav[0], 1000)
    e9 = R.residual_db(wav[1])
    print(f"device 48000 tone 1000: {e1:.1f} dB, alias 9000: {e9:.1f} dB")
    assert e1 <= -85.0 and e9 <= -85.0


# ---------------------------------------------------------------- 8. guards and errors
def _raw(eng, pcm, n_in, rate, ch, m_max, wav, n_out, n_max_in=None):
    from casr.engine import _ptr, _stream
    return eng.lib.casr_convert_audio(eng.handle, _ptr(pcm), _ptr(n_in), pcm.shape[0], n_max_in or pcm.shape[1], ch, rate,
                                      m_max, 0, ctypes.c_float(0.0), _ptr(wav), _ptr(n_out), None, _stream())


def test_guards_and_errors(eng):
    c = case(48000, 1)
    n = c["pcm"].shape[1]
    eng.device_flags()
    good, n_good, _ = run(eng, c["pcm"], [n, n, 1], 48000)
    wav, n_out, _ = run(eng, c["pcm"], [n, n + 5, 1], 48000)  # clamped to n_max_in
    assert eng.device_flags() == 64
    assert eng.device_flags() == 0  # raised once, read and cleared
    assert np.array_equal(n_out, n_good) and np.array_equal(bits(wav), bits(good))
    wav, n_out, _ = run(eng, c["pcm"], [n, -3, 1], 48000)  # clamped to 0
    assert eng.device_flags() == 64
    assert n_out.tolist() == [n_good[0], 0, n_good[2]] and not bits(wav[1]).any()
    assert np.array_equal(bits(wav[0]), bits(good[0])) and np.array_equal(bits(wav[2]), bits(good[2]))
    # refusals launch nothing: a sentinel-filled output stays as it was
    dev = eng.device
    pcm = torch.from_numpy(c["pcm"][:, :3000].copy()).to(dev)
    n_in = torch.tensor([3000, 10, 1], dtype=torch.int32, device=dev)
    sent = torch.full((3, 1000), 7.5, device=dev)
    n_sent = torch.full((3,), -9, dtype=torch.int32, device=dev)
    for rate, ch, m_max, rc, word in [(48000, 1, 999, 1, b"m_max"), (48000, 9, 1000, 1, b"channels"),
                                      (44101, 1, 1000, 4, b"44101"), (3999, 1, 1000, 4, b"3999")]:
        assert _raw(eng, pcm, n_in, rate, ch, m_max, sent, n_sent) == rc, (rate, ch, m_max)
        assert word in eng.lib.casr_last_error(eng.handle)
    assert _raw(eng, pcm, n_in, 48000, 1, 1000, None, n_sent) == 1
    assert _raw(eng, pcm, n_in, 48000, 1, 0, sent, n_sent) == 1
    torch.cuda.synchronize()
    assert (sent == 7.5).all() and (n_sent == -9).all()
    assert _raw(eng, pcm, n_in, 48000, 1, 1000, sent, n_sent) == 0  # the same call with m_max just enough
    torch.cuda.synchronize()
    assert n_sent.tolist() == [1000, 4, 1] and eng.device_flags() == 0


# ---------------------------------------------------------------- 9. the chain
def _write_wav16(path, frames, rate):
    n, ch = frames.shape
    data = frames.astype("<i2").tobytes()
    hdr = struct.pack("<HHIIHH", 1, ch, rate, rate * ch * 2, ch * 2, 16)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<I", 16) + hdr)
        f.write(b"data" + struct.pack("<I", len(data)) + data)


def test_chain_file_to_decode(tmp_path):
    import data as D
    from casr.engine import Engine
    rs = np.random.RandomState(9)
    pcm16 = (3000 * rs.standard_normal((24000, 2))).clip(-32768, 32767).astype(np.int16)
    path = str(tmp_path / "st48.wav")
    _write_wav16(path, pcm16, 48000)
    eng = Engine(CFG, *synthetic_state_dicts(CFG, peaked=True))
    try:
        def decode(wav, n):
            fb, frames = eng.log_mel(wav, n)
            feat, flen = eng.features(fb, frames)
            eng.encode(feat, flen)
            out = eng.greedy()
            return frames.cpu().numpy(), out["tokens"].cpu().numpy(), out["accum"].cpu().numpy()

        frames_f32 = pcm16.astype(np.float32) / 32768.0
        audio = D.load_audio([path])[0]
        assert D._engine().device_flags() == 0
        wav, n_out, gain = eng.convert_audio(torch.from_numpy(frames_f32[None]), [24000], 48000)
        assert int(n_out[0]) == 8000 == len(audio)
        assert np.array_equal(bits(wav[0].cpu().numpy()), bits(audio))
        assert abs(np.abs(audio).max() - 10 ** (-1 / 20)) < 1e-4 and float(gain[0]) > 1
        # the 16 kHz samples as an array, before and after a conversion on the same handle
        arr = torch.from_numpy(audio[None].copy()).to(eng.device)
        f0, t0, a0 = decode(arr, [8000])
        wav, n_out, _ = eng.convert_audio(torch.from_numpy(frames_f32[None]), [24000], 48000)
        f1, t1, a1 = decode(wav, n_out)  # the converter's device outputs feed casr_log_mel directly
        assert eng.device_flags() == 0
        f2, t2, a2 = decode(arr, [8000])
        assert f0.tolist() == f1.tolist() == f2.tolist() == [L.log_mel_frames(8000)]
        assert np.array_equal(t0, t1) and np.array_equal(t0, t2)
        assert np.array_equal(bits(a0), bits(a1)) and np.array_equal(bits(a0), bits(a2))
        feat, flen = D.log_mel_batch([audio])
        assert D._engine().device_flags() == 0 and int(flen[0]) == L.log_mel_frames(8000) // 3
    finally:
        eng.close()
