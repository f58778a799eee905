"""csrc/align_plan.h (the weight, the recurrence, the move bits and their backtrack, the peak order
and the plan, which the kernel of csrc/align.hip compiles too) under AddressSanitizer +
UndefinedBehaviorSanitizer on the CPU.

``tests/host_asan/align_check.cpp`` is a program of its own: it includes the header, reads every
utterance's weights into a heap buffer of exactly n x T values, and its outputs must equal the
reference's (tests/align_ref.py).  Nothing is loaded into Python, no library is preloaded, and nothing
runs on a GPU."""
import os
import subprocess

import numpy as np
import pytest

import align_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _write_cases(path, cases, short=None):
    """cases: (a [L, Tp] float32, T, n); short: that case's buffer is written one value short."""
    with open(path, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for i, (a, T, n) in enumerate(cases):
            vals = np.ascontiguousarray(a[:n, :T], np.float32).reshape(-1)
            vals = vals[:-1] if i == short else vals
            f.write(np.array([a.shape[0], T, n], np.int32).tobytes())
            f.write(np.int64(vals.size).tobytes())
            f.write(vals.tobytes())


@pytest.mark.timeout(600)
def test_align_plan_under_asan_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("clang++ not available")
    exe = str(tmp_path / "align_check")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "chinese-asr_amd", "csrc"),
                    os.path.join(HERE, "host_asan", "align_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    cases = []
    for seed, (B, Lx, Tp) in enumerate([(6, 1, 1), (6, 3, 2), (8, 7, 63), (6, 40, 64), (6, 41, 65), (4, 40, 129),
                                        (4, 12, 266), (6, 9, 70), (6, 20, 7)] * 3):
        a, enc, tgt = R.seeded_case(300 + seed, B, Lx, Tp)
        cases += [(a[:, :, b], int(enc[b]), int(tgt[b])) for b in range(B)]
    src, out = str(tmp_path / "cases.bin"), str(tmp_path / "out.txt")
    _write_cases(src, cases)
    r = subprocess.run([exe, src, out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "align_check ok" in r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = open(out).read().split("\n")
    for i, (a, T, n) in enumerate(cases):
        first, last, peak, score, _ = R.path_one(a, T, n)
        assert [int(x) for x in lines[i].split()] == [score] + first.tolist() + last.tolist() + peak.tolist(), i
    # the sanitizer is live: a buffer one value short is a heap-buffer-overflow read of the last cell
    short = next(i for i, (a, T, n) in enumerate(cases) if T >= 20 and n >= 5)
    _write_cases(src, cases, short=short)
    r = subprocess.run([exe, src, out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "heap-buffer-overflow" in r.stderr, r.stderr[-2000:]
