"""casr_convert_audio on the host (CPU only): the resampler's plan, output length and f32 table against
the numpy restatement (tests/resample_ref.py); the filter quality of that restatement on tones, which
anchors the specification outside its own formula; the error paths that need no device; the design
header under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program; WAV reading at any
rate and channel count; and how ``data.load_audio`` routes and groups files."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import resample_ref as R
from casr import lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
INT_MAX = 2 ** 31 - 1


# ---------------------------------------------------------------- plan, frames, table
@pytest.mark.parametrize("rate", R.RATES)
def test_plan_matches_reference(rate):
    Lr, Mr, K, _, _ = R.plan(rate)
    assert L.resample_plan(rate) == (Lr, Mr, 2 * K)


@pytest.mark.parametrize("rate", R.RATES)
def test_frames_match_reference(rate):
    """n_out = ceil(n L / M) for every n of the list.  The C function returns an int: the one count
    that does not fit (2^30 frames at 8 kHz are 2^31 outputs) is answered with -1."""
    lib = L.load()
    for n in (0, 1, 2, 159, 160, 161, 12345, 2 ** 30):
        want = R.frames(n, rate)
        got = lib.casr_resample_frames(n, rate)
        assert got == (want if want <= INT_MAX else -1), (rate, n, got, want)
        if want <= INT_MAX:
            assert L.resample_frames(n, rate) == want


@pytest.mark.parametrize("rate", R.RATES)
def test_table_matches_float64_design(rate):
    """Every entry within 1.2e-7 of the float64 design (two f32 half-ulps at magnitude 1; entries are
    below 1), every row sums to 1 within 2e-6."""
    tab = L.resample_filter(rate)
    ref = R.table(rate)
    assert tab.shape == ref.shape and tab.dtype == np.float32
    assert np.abs(ref).max() < 1.0  # (0.94 before each phase is scaled to unit DC gain)
    assert np.abs(tab.astype(np.float64) - ref).max() <= 1.2e-7
    assert np.abs(tab.astype(np.float64).sum(axis=1) - 1.0).max() <= 2e-6


# ---------------------------------------------------------------- filter quality of the reference
def _ref(freq, rate):
    n = rate // 2  # 0.5 s
    return R.resample(R.tone(freq, rate, n), rate, np.float64)


@pytest.mark.parametrize("rate", [8000, 44100, 48000])
def test_reference_filter_quality(rate):
    """Tones of 0.5 s through the float64 reference, 400 output samples skipped at each edge.  Passband
    error against the analytic 16 kHz tone <= -85 dB at 1, 3 and 6 kHz; <= -40 dB at 7 kHz (inside the
    0.94 roll-off); tones at 8.5 and 12 kHz, which 16 kHz cannot carry, leave <= -85 dB; the image of a
    3 kHz tone at 8 kHz input (at 5 kHz in the output) <= -85 dB.  An 8 kHz input carries no tone above
    4 kHz, so only the 1 and 3 kHz passband cases and the image case exist for it.  (Measured: passband
    <= -95.6 dB, 7 kHz -44.7 dB, aliases <= -92.2 dB, images <= -90.4 dB; a wrong phase rule gives -20 dB.)"""
    nyq = min(rate, R.RATE_OUT) / 2
    for f in (1000, 3000, 6000):
        if f < 0.94 * nyq:
            e = R.tone_error_db(_ref(f, rate), f)
            print(f"rate {rate} tone {f}: {e:.1f} dB")
            assert e <= -85.0, (rate, f, e)
    if rate > R.RATE_OUT:
        e7 = R.tone_error_db(_ref(7000, rate), 7000)
        print(f"rate {rate} tone 7000: {e7:.1f} dB")
        assert e7 <= -40.0, (rate, e7)
        for f in (8500, 12000):
            e = R.residual_db(_ref(f, rate))
            print(f"rate {rate} alias {f}: {e:.1f} dB")
            assert e <= -85.0, (rate, f, e)
    if rate == 8000:
        y = _ref(3000, rate)
        e = R.component_db(y, 5000)
        print(f"rate {rate} image of 3000 at 5000: {e:.1f} dB")
        assert e <= -85.0, e
        assert R.tone_error_db(y, 3000) <= -85.0  # the whole residual, image included


# ---------------------------------------------------------------- error paths without a device
def test_error_paths_without_a_device():
    lib = L.load()
    a, b, c = ctypes.c_int32(-7), ctypes.c_int32(-7), ctypes.c_int32(-7)
    for rate in (3999, 384001, 0, -16000):
        assert lib.casr_resample_plan(rate, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 4
        assert lib.casr_resample_frames(100, rate) == -1
        assert lib.casr_resample_filter(rate, ctypes.c_void_p(0x10)) == 4  # refused before the buffer is touched
    assert b"[4000, 384000]" in lib.casr_last_error(None)
    # 44,101 Hz: gcd 1, so 16,000 phases x 190 taps
    assert lib.casr_resample_plan(44101, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 4
    msg = lib.casr_last_error(None)
    assert b"16000" in msg and b"65536" in msg, msg
    assert lib.casr_resample_frames(100, 44101) == -1
    assert (a.value, b.value, c.value) == (-7, -7, -7)  # nothing written on a refusal
    with pytest.raises(L.CasrError, match="44101"):
        L.resample_plan(44101)
    # NULL outputs
    assert lib.casr_resample_plan(48000, None, ctypes.byref(b), ctypes.byref(c)) == 1
    assert lib.casr_resample_plan(48000, ctypes.byref(a), None, ctypes.byref(c)) == 1
    assert lib.casr_resample_plan(48000, ctypes.byref(a), ctypes.byref(b), None) == 1
    assert lib.casr_resample_filter(48000, None) == 1
    # the device call refuses a NULL handle before anything else
    assert lib.casr_convert_audio(None, None, None, 1, 16, 1, 48000, 16, 1, ctypes.c_float(-1.0), None, None, None,
                                  None) == 1


# ---------------------------------------------------------------- the design header under sanitizers
def _fnv1a(data):
    h = 1469598103934665603
    for v in data:
        h = ((h ^ v) * 1099511628211) & (2 ** 64 - 1)
    return h


@pytest.mark.timeout(300)
def test_resample_design_under_asan_ubsan(tmp_path):
    """tests/host_resample/resample_check.cpp: a program of its own (host code only, nothing loaded
    into Python), built from resample_design.h under ASan + UBSan.  Its tables, built into exact-size
    heap buffers, must be the library's bit for bit (FNV-1a of the bytes)."""
    if not os.path.exists(CLANG):
        pytest.skip("clang++ not available")
    exe = str(tmp_path / "resample_check")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "chinese-asr_amd", "csrc"),
                    os.path.join(HERE, "host_resample", "resample_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "resample_check ok" in r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    seen = {}
    for line in r.stdout.splitlines():
        if line.startswith("table "):
            _, rate, l_, m_, taps, h = line.split()
            seen[int(rate)] = (int(l_), int(m_), int(taps), int(h, 16))
    for rate in R.RATES:
        l_, m_, taps, h = seen[rate]
        assert (l_, m_, taps) == L.resample_plan(rate)
        assert h == _fnv1a(L.resample_filter(rate).tobytes()), rate


# ---------------------------------------------------------------- WAV reading
def _write_wav(path, frames, rate, fmt):
    """frames [n, ch]: int16 (fmt 'pcm16') or float32 (fmt 'f32')."""
    frames = np.ascontiguousarray(frames)
    n, ch = frames.shape
    tag, bits = (1, 16) if fmt == "pcm16" else (3, 32)
    data = frames.astype("<i2" if fmt == "pcm16" else "<f4").tobytes()
    hdr = struct.pack("<HHIIHH", tag, ch, rate, rate * ch * bits // 8, ch * bits // 8, bits)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + 8 + len(hdr) + 8 + len(data)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<I", len(hdr)) + hdr)
        f.write(b"data" + struct.pack("<I", len(data)) + data)


def test_read_wav_any_rate_and_channels(tmp_path):
    import data as D
    rs = np.random.RandomState(5)
    st = rs.randint(-32768, 32768, size=(1234, 2)).astype(np.int16)
    _write_wav(tmp_path / "s.wav", st, 48000, "pcm16")
    frames, rate = D.read_wav(str(tmp_path / "s.wav"))
    assert rate == 48000 and frames.dtype == np.float32 and frames.shape == (1234, 2)
    np.testing.assert_array_equal(frames, st.astype(np.float32) / 32768.0)
    mono = rs.standard_normal((777, 1)).astype(np.float32)
    _write_wav(tmp_path / "m.wav", mono, 8000, "f32")
    frames, rate = D.read_wav(str(tmp_path / "m.wav"))
    assert rate == 8000 and frames.shape == (777, 1)
    np.testing.assert_array_equal(frames, mono)
    with pytest.raises(ValueError, match="channels"):  # fast_read keeps refusing stereo
        D.fast_read(str(tmp_path / "s.wav"))


# ---------------------------------------------------------------- load_audio routing
class _StubEngine:
    def __init__(self):
        self.calls = []

    def convert_audio(self, pcm, n_in, rate, channels=None, quantize=True, norm_db=-1.0, m_max=None):
        pcm, n_in = np.asarray(pcm), np.asarray(n_in)
        self.calls.append(dict(pcm=pcm.copy(), n_in=n_in.copy(), rate=rate, channels=channels, quantize=quantize,
                               norm_db=norm_db))
        n_out = np.array([R.frames(int(n), rate) for n in n_in], np.int32)
        wav = np.zeros((len(n_in), max(int(n_out.max()), 1)), np.float32)
        for b in range(len(n_in)):  # a recognisable answer: the row index + 1 over the valid outputs
            wav[b, :n_out[b]] = b + 1
        return torch.from_numpy(wav), torch.from_numpy(n_out), torch.ones(len(n_in))


def test_load_audio_routes_and_groups(tmp_path, monkeypatch):
    import shutil

    import data as D
    stub = _StubEngine()
    monkeypatch.setattr(D, "_engine", lambda: stub)
    monkeypatch.setattr(shutil, "which", lambda *_a, **_k: None)
    rs = np.random.RandomState(6)
    p16 = rs.randint(-3000, 3000, size=(2000, 1)).astype(np.int16)
    a8 = rs.randint(-3000, 3000, size=(800, 1)).astype(np.int16)
    b8 = rs.randint(-3000, 3000, size=(500, 1)).astype(np.int16)
    s48 = rs.randint(-3000, 3000, size=(4801, 2)).astype(np.int16)
    _write_wav(tmp_path / "p16.wav", p16, 16000, "pcm16")
    _write_wav(tmp_path / "a8.wav", a8, 8000, "pcm16")
    _write_wav(tmp_path / "b8.wav", b8, 8000, "pcm16")
    _write_wav(tmp_path / "s48.wav", s48, 48000, "pcm16")
    # 16 kHz mono alone: the converter is never reached, and the samples are fast_read's
    out = D.load_audio([str(tmp_path / "p16.wav")])
    assert stub.calls == []
    np.testing.assert_array_equal(out[0], D.fast_read(str(tmp_path / "p16.wav")))
    assert out[0].dtype == np.float32
    # mixed: two 8 kHz files and one 48 kHz stereo file make two calls, grouped by (rate, channels)
    out = D.load_audio([str(tmp_path / n) for n in ("a8.wav", "s48.wav", "p16.wav", "b8.wav")])
    assert len(stub.calls) == 2
    by = {(c["rate"], c["channels"]): c for c in stub.calls}
    assert set(by) == {(8000, 1), (48000, 2)}
    c8, c48 = by[(8000, 1)], by[(48000, 2)]
    assert c8["pcm"].shape == (2, 800, 1) and c8["n_in"].tolist() == [800, 500]
    np.testing.assert_array_equal(c8["pcm"][0], a8.astype(np.float32) / 32768.0)
    np.testing.assert_array_equal(c8["pcm"][1, :500], b8.astype(np.float32) / 32768.0)
    assert not c8["pcm"][1, 500:].any()
    assert c48["pcm"].shape == (1, 4801, 2) and c48["n_in"].tolist() == [4801]
    np.testing.assert_array_equal(c48["pcm"][0], s48.astype(np.float32) / 32768.0)
    for c in stub.calls:
        assert c["quantize"] is True and c["norm_db"] == -1.0
    # results come back in the order of the paths, cut to n_out, as float32 arrays
    assert [len(o) for o in out] == [1600, 1601, 2000, 1000]
    assert (out[0] == 1).all() and (out[3] == 2).all() and (out[1] == 1).all()
    np.testing.assert_array_equal(out[2], p16[:, 0].astype(np.float32) / 32768.0)
    assert all(o.dtype == np.float32 for o in out)
