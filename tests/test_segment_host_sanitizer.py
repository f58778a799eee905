"""csrc/segment_plan.h (the segmentation's decision text, which the decision kernel compiles too) under
AddressSanitizer + UndefinedBehaviorSanitizer on the CPU.

``tests/host_asan/segment_check.cpp`` is a program of its own: it includes the header, reads every
recording into a heap buffer of exactly its rows, and its segments must equal the reference's
(tests/segment_ref.py), both with whole-row runs and with runs clipped to tiles as the kernel hands them
over.  Nothing is loaded into Python, no library is preloaded, and nothing runs on a GPU."""
import os
import subprocess

import numpy as np
import pytest

import segment_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
FIELDS = ("max_frames", "min_frames", "min_pause", "min_speech", "pad", "max_gap", "pct_lo", "pct_hi", "rel_q8",
          "rise_min")


def _write_cases(path, cases, short=None):
    """cases: [(fbank [n, n_mels], P, s_max, chunk)].  short: that case's fbank is written one float
    short (the sanitizer must see the read)."""
    with open(path, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for i, (fb, p, s_max, chunk) in enumerate(cases):
            f.write(np.array([getattr(p, k) for k in FIELDS], np.int32).tobytes())
            f.write(np.array([fb.shape[0], fb.shape[1], s_max, chunk], np.int32).tobytes())
            flat = np.ascontiguousarray(fb, np.float32).ravel()
            if i == short:
                flat = flat[:-1]
            f.write(np.int64(flat.size).tobytes())
            f.write(flat.tobytes())


@pytest.mark.timeout(600)
def test_segment_plan_under_asan_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("clang++ not available")
    exe = str(tmp_path / "segment_check")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "chinese-asr_amd", "csrc"),
                    os.path.join(HERE, "host_asan", "segment_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    cases = []
    for seed, n in enumerate((0, 1, 2, 63, 64, 65, 700, 1024, 2049, 3000)):
        fb = R.fbank_from_levels(R.random_levels(n, 300 + seed), 300 + seed)
        cases.append((fb, R.SMALL, 400, (64, 7, 1024)[seed % 3]))
    cases.append((R.fbank_from_levels(R.random_levels(4000, 77, mean_on=300, mean_off=60), 77), R.P(), 3, 1024))
    nan = R.fbank_from_levels(R.random_levels(300, 78), 78)
    nan[100] = np.nan
    cases.append((nan, R.SMALL, 100, 64))
    src, out = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    _write_cases(src, cases)
    r = subprocess.run([exe, src, out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "segment_check ok" in r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    got = np.fromfile(out, np.int32).tolist()
    pos = 0
    for fb, p, s_max, _ in cases:
        thr, segs = R.segment_fbank(fb, len(fb), p)
        assert got[pos:pos + 2] == [thr, len(segs)]
        w = min(len(segs), s_max)
        assert got[pos + 2:pos + 2 + 2 * w] == [v for s in segs[:w] for v in s]
        pos += 2 + 2 * w
    assert pos == len(got)
    assert sum(len(R.segment_fbank(fb, len(fb), p)[1]) for fb, p, _, _ in cases) > 100
    # the sanitizer is live: a recording one float short is a heap-buffer-overflow read in stage (a)
    _write_cases(src, cases, short=7)
    r = subprocess.run([exe, src, out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "heap-buffer-overflow" in r.stderr, r.stderr[-2000:]
