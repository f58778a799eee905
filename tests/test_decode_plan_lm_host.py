"""The decode plan of the fused beam's caller on the host (CPU only): ``tests/host_plan/plan_lm_check.cpp``
is a stand-alone program built from ``chinese-asr_amd/csrc/decode_plan.h`` alone under AddressSanitizer +
UndefinedBehaviorSanitizer; over shapes, options and blobs it checks that PLAN_BEAM_LM's plan is
casr_beam's with the caller changed and the select never fused."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.timeout(300)
def test_beam_lm_plan_under_asan_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("clang++ not available")
    exe = str(tmp_path / "plan_lm_check")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "chinese-asr_amd", "csrc"),
                    os.path.join(HERE, "host_plan", "plan_lm_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "plan_lm_check ok" in r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
