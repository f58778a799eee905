"""csrc/bias_plan.h (the phrase automaton's builder, its transition, the sentence walk and the row rule,
which the kernels of csrc/bias.hip and csrc/beam_lm.hip compile too) under AddressSanitizer +
UndefinedBehaviorSanitizer on the CPU.

``tests/host_asan/bias_check.cpp`` is a program of its own: it includes the header, reads every array
into a heap buffer of exactly its length, queries the tables from such buffers, and its full, tail and
gain rows must equal the brute force of tests/bias_ref.py.  Nothing is loaded into Python, no library is
preloaded, and nothing runs on a GPU."""
import os
import subprocess

import numpy as np
import pytest

import bias_ref as BR

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _write_cases(path, sets, short=None):
    """short = (set, sentence): that sentence is written one symbol short (the sanitizer must see the read)."""
    with open(path, "wb") as f:
        f.write(np.int32(len(sets)).tobytes())
        for i, (V, ph, bo, sents) in enumerate(sets):
            f.write(np.array([V, len(ph)], np.int32).tobytes())
            f.write(np.array([len(p) for p in ph], np.int32).tobytes())
            f.write(np.array(bo, np.int32).tobytes())
            toks = np.array([t for p in ph for t in p], np.int32)
            f.write(np.int64(toks.size).tobytes())
            f.write(toks.tobytes())
            f.write(np.int32(len(sents)).tobytes())
            for j, y in enumerate(sents):
                row = np.array(y, np.int64).astype(np.int32)
                f.write(np.int32(row.size).tobytes())
                row = row[:-1] if (i, j) == short else row
                f.write(np.int64(row.size).tobytes())
                f.write(row.tobytes())


@pytest.mark.timeout(600)
def test_bias_plan_under_asan_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("clang++ not available")
    exe = str(tmp_path / "bias_check")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "chinese-asr_amd", "csrc"),
                    os.path.join(HERE, "host_asan", "bias_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    sets = [BR.seeded_set(seed) for seed in range(200)]
    p16 = list(range(16))
    sets.append((40, [p16, p16[:15], [0], [15, 0, 1]], [4096, 4096, 1, 300], [p16 + p16, p16[:15], [], [39] * 24]))
    sets.append((5, [], [], [[], [1, 2, 3], [7, -1]]))
    sets.append((5, [[1, 2], [1, 2]], [256, 256], [[1, 2]]))  # refused: a duplicate
    src, out = str(tmp_path / "cases.bin"), str(tmp_path / "out.txt")
    _write_cases(src, sets)
    r = subprocess.run([exe, src, out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "bias_check ok" in r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = iter(open(out).read().split("\n"))
    for i, (V, ph, bo, sents) in enumerate(sets):
        head = next(lines).split()
        assert head[0] == "B"
        if i == len(sets) - 1:
            assert int(head[1]) == 1
            continue
        assert int(head[1]) == 0 and int(head[2]) >= 1
        for y in sents:
            s = next(lines).split()
            wf = BR.full(y, ph, bo)
            assert s[0] == "S" and [int(s[1]), int(s[2])] == [wf, BR.tail(y, ph, bo)], (i, y)
            row = next(lines).split()
            assert row[0] == "R" and len(row) == 1 + 2 * V
            assert [int(x) for x in row[1:1 + V]] == (BR.candidate_ints(y, ph, bo, V) - wf).tolist(), (i, y)
    # the sanitizer is live: a sentence one symbol short is a heap-buffer-overflow read of the walk
    short = next((i, j) for i, s in enumerate(sets) for j, y in enumerate(s[3]) if len(y) >= 10)
    _write_cases(src, sets, short=short)
    r = subprocess.run([exe, src, out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "heap-buffer-overflow" in r.stderr, r.stderr[-2000:]
