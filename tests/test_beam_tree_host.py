"""The beam tree's reading rules on the host (CPU only): ``tests/host_plan/beam_tree_check.cpp`` is a
stand-alone program built from ``chinese-asr_amd/csrc/beam_tree.h``, the text the kernels compile, under
AddressSanitizer + UndefinedBehaviorSanitizer; it checks the executed steps, the plain beam's live-row
choice, the walk over both layouts, the staging and a record's start slot on small hand-built trees in
exactly sized heap arrays, each against a literal restatement."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.timeout(300)
def test_beam_tree_rules_under_asan_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("clang++ not available")
    exe = str(tmp_path / "beam_tree_check")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(REPO, "chinese-asr_amd", "csrc"),
                    os.path.join(HERE, "host_plan", "beam_tree_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "beam_tree_check ok (1517 checks)" in r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
