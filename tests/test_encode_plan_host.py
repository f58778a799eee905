"""The encode plan on the host (CPU only, milliseconds): ``chinese-asr_amd/csrc/encode_plan.h`` decides
which kernels an encode runs (feature path, image layout, the input GEMM's form, stage counts and tail
split, the recurrence's layout, grid, pacing and per-step fallback, the keys form), sizes the encode
workspaces and gives the bytes the per-step fallback's hipGraph key is built from.
``tests/host_plan/encode_plan_check.cpp`` is a stand-alone program built from that header alone under
AddressSanitizer + UndefinedBehaviorSanitizer; it checks the plan against the decisions worked out by
hand from the launchers' rules, on both sides of every guard."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.timeout(300)
def test_encode_plan_under_asan_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("clang++ not available")
    exe = str(tmp_path / "encode_plan_check")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "chinese-asr_amd", "csrc"),
                    os.path.join(HERE, "host_plan", "encode_plan_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "encode_plan_check ok" in r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
