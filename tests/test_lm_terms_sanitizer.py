"""csrc/ngram_succ.h (the successor lists' build and the per-row term query, the text the kernel runs
too) under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU.

``tests/host_asan/ngram_terms_check.cpp`` is a program of its own: it includes the headers, builds
seeded random models of orders 1..4 in exact-size heap buffers, builds their successor lists, and for
hundreds of contexts compares the whole term row with the per-word query (ngram_term) bit for bit.
Nothing is loaded into Python, no library is preloaded, and nothing runs on a GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.timeout(600)
def test_successor_lists_and_term_rows_under_asan_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("clang++ not available")
    exe = str(tmp_path / "ngram_terms_check")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "chinese-asr_amd", "csrc"),
                    os.path.join(HERE, "host_asan", "ngram_terms_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for seed in ("1", "20261020"):
        r = subprocess.run([exe, seed], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "ngram_terms_check ok" in r.stdout
        assert "runtime error" not in r.stderr, r.stderr[-4000:]
