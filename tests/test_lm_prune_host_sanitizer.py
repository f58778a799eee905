"""csrc/lm_prune_plan.h (relative-entropy pruning: the text the kernels run too) under
AddressSanitizer + UndefinedBehaviorSanitizer on the CPU.

``tests/host_asan/lm_prune_check.cpp`` is a program of its own: it includes the header, runs its built-in
edge cases, then prunes a model this test writes from exact-size heap buffers, and what it writes must
equal the library's host entry bit for bit; its lmp_exp10 and lmp_log over two sweeps must equal the
Python restatement bit for bit and meet their accuracy bound against numpy.  Nothing is loaded into
Python, no library is preloaded, and nothing runs on a GPU."""
import os
import subprocess

import numpy as np
import pytest

import lm_estimate_ref as E
import lm_prune_ref as PR
from casr import ngram

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

XS = np.concatenate([np.linspace(-99.0, 0.0, 997), -np.logspace(-12, 2, 200), [-99.0, -1e-9, 0.0, -100.0, 0.30103]])
YS = np.concatenate([np.logspace(-99, 0, 997), 1.0 + np.linspace(-1e-9, 1e-9, 41), np.linspace(0.5, 2.0, 301),
                     [1e-99, 2.2250738585072014e-308, 1.7976931348623157e308, 5e-324]])


def _write_model(path, lm, theta, short=False):
    """short: the top order's id array is written one id short (the sanitizer must see the read)."""
    ids, prob, back = lm._arrays
    with open(path, "wb") as f:
        f.write(np.array([lm.order, lm.vocab], np.int32).tobytes())
        f.write(np.float64(theta).tobytes())
        for n in range(lm.order):
            flat = ids[n].reshape(-1)
            if short and n == lm.order - 1:
                flat = flat[:-1]
            f.write(np.int64(len(ids[n])).tobytes() + np.int64(flat.size).tobytes())
            f.write(np.ascontiguousarray(flat, np.int32).tobytes())
            f.write(np.ascontiguousarray(prob[n], np.float32).tobytes())
            f.write(np.ascontiguousarray(back[n], np.float32).tobytes())
        for a in (XS, YS):
            f.write(np.int64(a.size).tobytes() + np.ascontiguousarray(a, np.float64).tobytes())


def _read_result(path, order):
    raw = open(path, "rb").read()
    at = 0

    def take(dt, n):
        nonlocal at
        a = np.frombuffer(raw, dt, n, at)
        at += a.nbytes
        return a

    out = dict(tau=take(np.float64, 1)[0], head=take(np.int64, 2), orders=[])
    for _ in range(order):
        c = int(take(np.int64, 1)[0])
        out["orders"].append(dict(key=take(np.uint64, c), delta=take(np.float64, c), kept=take(np.uint8, c),
                                  b64=take(np.float64, c), backoff=take(np.float32, c)))
    out["exp10"], out["log"] = take(np.float64, XS.size), take(np.float64, YS.size)
    assert at == len(raw)
    return out


@pytest.mark.timeout(600)
def test_lm_prune_plan_under_asan_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("clang++ not available")
    exe = str(tmp_path / "lm_prune_check")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "chinese-asr_amd", "csrc"),
                    os.path.join(HERE, "host_asan", "lm_prune_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    lm = ngram.estimate(E.small_corpus(6, 300, 8, 6), 4, 6)
    model, out = str(tmp_path / "model.bin"), str(tmp_path / "out.bin")
    for theta in (1e-4, 1e-2):
        _write_model(model, lm, theta)
        r = subprocess.run([exe, model, out], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "lm_prune_check ok" in r.stdout
        assert "runtime error" not in r.stderr, r.stderr[-4000:]
        got = _read_result(out, 4)
        pr = lm.prune(theta).pruned
        assert got["tau"] == pr.tau and got["head"].tolist() == [1, pr.n_degenerate]
        for n, o in enumerate(got["orders"]):
            key = np.zeros(len(pr.all_ids[n]), np.uint64)
            for e in range(n + 1):  # ngram_key's packing: the last word in field 0
                key |= (pr.all_ids[n][:, n - e].astype(np.uint64) + np.uint64(1)) << np.uint64(16 * e)
            assert np.array_equal(o["key"], key)
            assert np.array_equal(o["delta"].view(np.uint64), pr.delta[n].view(np.uint64))
            kept = o["kept"].astype(bool)
            assert np.array_equal(kept, pr.kept[n])
            assert np.array_equal(o["b64"][kept].view(np.uint64), pr.backoff_f64[n].view(np.uint64))
            assert np.array_equal(o["backoff"][kept].view(np.uint32), pr.backoff[n].view(np.uint32))
    # lmp_exp10 and lmp_log: the restatement's bits, and the accuracy bound against numpy
    with np.errstate(all="ignore"):
        assert np.array_equal(got["exp10"].view(np.uint64), np.array([PR.exp10(x) for x in XS]).view(np.uint64))
        assert np.array_equal(got["log"].view(np.uint64), np.array([PR.log(y) for y in YS]).view(np.uint64))
        assert np.abs(got["exp10"] / 10.0 ** XS - 1.0).max() <= 1e-12
        assert (np.abs(got["log"] - np.log(YS)) <= 1e-12 * np.maximum(1.0, np.abs(np.log(YS)))).all()
    # the sanitizer is live: the top order's ids one short is a heap-buffer-overflow read in the build
    _write_model(model, lm, 1e-4, short=True)
    r = subprocess.run([exe, model, out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "heap-buffer-overflow" in r.stderr, r.stderr[-2000:]
    lm.close()
