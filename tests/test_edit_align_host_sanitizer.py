"""csrc/edit_align_plan.h (the tiles, the bit layout and its index functions, the hand-off index math, the
backtrace with its maps, both host forms and the plan, which the kernels of csrc/edit_align.hip compile
too) under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU.

``tests/host_asan/edit_align_check.cpp`` is a program of its own: it includes the header, reads every
row into a heap buffer of exactly its length and writes every map into one of exactly its row's length;
its distances, counts and maps must equal the Python restatement's (tests/edit_align_ref.py).  Nothing
is loaded into Python, no library is preloaded, and nothing runs on a GPU."""
import os
import subprocess

import numpy as np
import pytest

import edit_align_ref as A
import edit_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _write_cases(path, pairs, short=None):
    """short: that pair's first row is written one symbol short (the sanitizer must see the read)."""
    with open(path, "wb") as f:
        f.write(np.int32(len(pairs)).tobytes())
        for i, (a, b) in enumerate(pairs):
            f.write(np.array([len(a), len(b)], np.int32).tobytes())
            for row, cut in ((a, i == short), (b, False)):
                row = np.asarray(row, np.int32).reshape(-1)
                row = row[:-1] if cut else row
                f.write(np.int64(row.size).tobytes())
                f.write(row.tobytes())


@pytest.mark.timeout(600)
def test_edit_align_plan_under_asan_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("clang++ not available")
    exe = str(tmp_path / "edit_align_check")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "chinese-asr_amd", "csrc"),
                    os.path.join(HERE, "host_asan", "edit_align_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    pairs = R.hand_pairs() + R.seeded_pairs(150, 37)
    rs = np.random.RandomState(12)
    # tile boundaries in both directions: 128 rows, 64 columns
    for m, n in ((127, 64), (128, 65), (129, 63), (257, 129), (1, 193), (300, 1), (0, 70), (130, 0)):
        a, b = A.edited_copy(rs, n, 4, 12)
        pairs.append(((a + rs.randint(0, 4, size=m).tolist())[:m], b))
    src, out = str(tmp_path / "cases.bin"), str(tmp_path / "out.txt")
    _write_cases(src, pairs)
    r = subprocess.run([exe, src, out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "edit_align_check ok" in r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = open(out).read().split("\n")
    for i, (p, q) in enumerate(pairs):
        dist, ops, ba, ab = A.align(p, q)
        head, got_ba, got_ab = lines[i].split("|")
        assert [int(x) for x in head.split()[1:]] == [dist] + list(ops), i
        assert [int(x) for x in got_ba.split()] == ba and [int(x) for x in got_ab.split()] == ab, i
    # the sanitizer is live: a row one symbol short is a heap-buffer-overflow read of the cell rule
    short = next(i for i, (a, b) in enumerate(pairs) if len(a) >= 20 and len(b) >= 20)
    _write_cases(src, pairs, short=short)
    r = subprocess.run([exe, src, out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "heap-buffer-overflow" in r.stderr, r.stderr[-2000:]
