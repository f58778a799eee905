"""csrc/edit_plan.h (the cell rule, the direction bits and their backtrace, the MBR order and the plan,
which the kernels of csrc/edit.hip compile too) under AddressSanitizer + UndefinedBehaviorSanitizer on
the CPU.

``tests/host_asan/edit_check.cpp`` is a program of its own: it includes the header, reads every row into
a heap buffer of exactly its length, and its distances, counts and MBR choices must equal the
reference's (casr.results, tests/edit_ref.py).  Nothing is loaded into Python, no library is preloaded,
and nothing runs on a GPU."""
import os
import subprocess

import numpy as np
import pytest

import edit_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
L, K = 10, 4


def _write_cases(path, pairs, sets, short=None):
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
        f.write(np.int32(len(sets)).tobytes())
        for (rt, sc, va, lm), scale in sets:
            f.write(np.array([L, K], np.int32).tobytes())
            f.write(np.array([scale, 0.4, 0.7], np.float64).tobytes())
            for x in (rt, sc, va, lm):
                f.write(np.ascontiguousarray(x).tobytes())


@pytest.mark.timeout(600)
def test_edit_plan_under_asan_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("clang++ not available")
    exe = str(tmp_path / "edit_check")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "chinese-asr_amd", "csrc"),
                    os.path.join(HERE, "host_asan", "edit_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    pairs = R.hand_pairs() + R.seeded_pairs(200, 31)
    rs = np.random.RandomState(8)
    pairs.append((rs.randint(0, 3, size=513).tolist(), [1, 2, 0]))
    sets = []
    for i, n in enumerate((0, 1, 2, 9, 25, 40)):
        sets.append((R.random_record_set(np.random.RandomState(700 + i), n, L, K), (0.0, 0.3, 1e6)[i % 3]))
    src, out = str(tmp_path / "cases.bin"), str(tmp_path / "out.txt")
    _write_cases(src, pairs, sets)
    r = subprocess.run([exe, src, out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "edit_check ok" in r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = open(out).read().split("\n")
    want_d, want_o = R.reference(pairs)
    for i in range(len(pairs)):
        assert [int(x) for x in lines[i].split()[1:]] == [want_d[i], want_d[i]] + want_o[i].tolist(), i
    for j, ((rt, sc, va, lm), scale) in enumerate(sets):
        f = lines[len(pairs) + j].split()
        assert f[0] == "M"
        flat, toks, s, q = R.records_of(rt, sc, va, lm, K)
        want, wrisk, _, _ = R.mbr_utterance(toks, s, q, scale, 0.4, 0.7)
        risk = np.array([float.fromhex(x) for x in f[2:]])
        assert np.allclose(risk[flat], wrisk, rtol=1e-12, atol=0) and risk.sum() == risk[flat].sum()
        assert int(f[1]) == (-1 if want < 0 else flat[want]) or R.near_tie(wrisk, want)
    # the sanitizer is live: a row one symbol short is a heap-buffer-overflow read of the cell rule
    short = next(i for i, (a, b) in enumerate(pairs) if len(a) >= 20 and len(b) >= 20)
    _write_cases(src, pairs, sets, short=short)
    r = subprocess.run([exe, src, out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "heap-buffer-overflow" in r.stderr, r.stderr[-2000:]
