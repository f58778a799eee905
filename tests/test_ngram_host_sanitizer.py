"""csrc/ngram_table.h (the n-gram tables' build and query, the text the kernels run too) under
AddressSanitizer + UndefinedBehaviorSanitizer on the CPU.

``tests/host_asan/ngram_check.cpp`` is a program of its own: it includes the header, builds tables from
exact-size heap buffers (its built-in edge cases, then a random 4-gram model this test writes), scores
sentences held in exact-size rows, and its scores must equal the library's and the reference's bit for
bit.  Nothing is loaded into Python, no library is preloaded, and nothing runs on a GPU."""
import os
import subprocess

import numpy as np
import pytest

import ngram_ref as R
from casr.ngram import NgramLM

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
V = 5004


def _write_model(path, grams, tokens, lens, bos, short_order=None):
    """short_order: that order's id array is written one id short (the sanitizer must see the read)."""
    ids, prob, back = R.arrays_of(grams)
    with open(path, "wb") as f:
        f.write(np.array([len(grams), V], np.int32).tobytes())
        for n, (a, p, b) in enumerate(zip(ids, prob, back), 1):
            f.write(np.int64(len(a)).tobytes())
            flat = a.ravel()
            if n == short_order:
                flat = flat[:-1]
            for arr in (flat, p, b):
                f.write(np.int64(arr.size).tobytes())
                f.write(np.ascontiguousarray(arr).tobytes())
        f.write(np.array([tokens.shape[0], tokens.shape[1], int(bos)], np.int32).tobytes())
        for arr in (tokens.ravel(), lens):
            f.write(np.int64(arr.size).tobytes())
            f.write(np.ascontiguousarray(arr, np.int32).tobytes())


@pytest.mark.timeout(600)
def test_ngram_table_under_asan_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("clang++ not available")
    exe = str(tmp_path / "ngram_check")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "chinese-asr_amd", "csrc"),
                    os.path.join(HERE, "host_asan", "ngram_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    grams = R.random_model(4, V, 41, n_high=4096)
    tokens, lens = R.sentences_from(grams, V, 300, 40, 42)
    model, scores = str(tmp_path / "model.bin"), str(tmp_path / "scores.bin")
    ref = R.RefLM(4, V, grams)
    lm = NgramLM.from_ids(*R.arrays_of(grams), {}, V)
    for bos in (True, False):
        _write_model(model, grams, tokens, lens, bos)
        r = subprocess.run([exe, model, scores], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "ngram_check ok" in r.stdout
        assert "runtime error" not in r.stderr, r.stderr[-4000:]
        got = np.fromfile(scores, np.float32)
        want = np.array([ref.sentence(tokens[i, :lens[i]], bos) for i in range(len(lens))], np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(got.view(np.uint32), lm.score_ids(tokens, lens, bos).view(np.uint32))
    # the sanitizer is live: the 4-gram ids one id short is a heap-buffer-overflow read in the build
    _write_model(model, grams, tokens, lens, True, short_order=4)
    r = subprocess.run([exe, model, scores], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "heap-buffer-overflow" in r.stderr, r.stderr[-2000:]
