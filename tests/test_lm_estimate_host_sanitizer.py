"""csrc/lm_estimate_plan.h (the Kneser-Ney estimator: the text the kernels run too) under
AddressSanitizer + UndefinedBehaviorSanitizer on the CPU.

``tests/host_asan/lm_estimate_check.cpp`` is a program of its own: it includes the header, runs its
built-in edge cases, then estimates a corpus this test writes from exact-size heap buffers, and what it
writes must equal the library's host entry bit for bit.  Nothing is loaded into Python, no library is
preloaded, and nothing runs on a GPU."""
import os
import subprocess

import numpy as np
import pytest

import lm_estimate_ref as E
from casr import ngram

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
V = 120


def _write_corpus(path, order, tokens, offsets, short=False):
    """short: the token array is written one id short (the sanitizer must see the read)."""
    with open(path, "wb") as f:
        f.write(np.array([order, V], np.int32).tobytes())
        tok = tokens[:-1] if short else tokens
        for arr, dt in ((tok, np.int32), (offsets, np.int64)):
            f.write(np.int64(arr.size).tobytes())
            f.write(np.ascontiguousarray(arr, dt).tobytes())


def _read_result(path, order):
    raw = open(path, "rb").read()
    at = 0

    def take(dt, n):
        nonlocal at
        a = np.frombuffer(raw, dt, n, at)
        at += a.nbytes
        return a

    out = dict(head=take(np.int64, 2), D=take(np.float64, 12).reshape(4, 3), fallback=take(np.int32, 4), orders=[])
    for _ in range(order):
        c = int(take(np.int64, 1)[0])
        out["orders"].append(dict(key=take(np.uint64, c), raw=take(np.uint32, c), adj=take(np.uint32, c),
                                  p=take(np.float64, c), gamma=take(np.float64, c), prob=take(np.float32, c),
                                  backoff=take(np.float32, c)))
    assert at == len(raw)
    return out


@pytest.mark.timeout(600)
def test_lm_estimate_plan_under_asan_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("clang++ not available")
    exe = str(tmp_path / "lm_estimate_check")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "chinese-asr_amd", "csrc"),
                    os.path.join(HERE, "host_asan", "lm_estimate_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    sents = E.zipf_corpus()
    sents[5] = sents[5] + [V + 2]  # <unk> as a word
    tokens, offsets = ngram.flatten(sents, V)
    corpus, out = str(tmp_path / "corpus.bin"), str(tmp_path / "out.bin")
    for order in (1, 4):
        _write_corpus(corpus, order, tokens, offsets)
        r = subprocess.run([exe, corpus, out], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "lm_estimate_check ok" in r.stdout
        assert "runtime error" not in r.stderr, r.stderr[-4000:]
        got = _read_result(out, order)
        est = ngram.estimate_host(tokens, offsets, order, V)
        assert got["head"].tolist() == [est.positions, est.n_types]
        assert np.array_equal(got["D"][:order].view(np.uint64), est.discounts.view(np.uint64))
        assert got["fallback"][:order].tolist() == est.fallback.astype(int).tolist()
        for n, o in enumerate(got["orders"]):
            key = np.zeros(len(est.ids[n]), np.uint64)
            for e in range(n + 1):  # ngram_key's packing: the last word in field 0
                key |= (est.ids[n][:, n - e].astype(np.uint64) + np.uint64(1)) << np.uint64(16 * e)
            assert np.array_equal(o["key"], key)
            assert np.array_equal(o["raw"], est.raw[n]) and np.array_equal(o["adj"], est.adjusted[n])
            assert np.array_equal(o["p"].view(np.uint64), est.p[n].view(np.uint64))
            assert np.array_equal(o["gamma"].view(np.uint64), est.gamma[n].view(np.uint64))
            assert np.array_equal(o["prob"].view(np.uint32), est.prob[n].view(np.uint32))
            assert np.array_equal(o["backoff"].view(np.uint32), est.backoff[n].view(np.uint32))
    # the sanitizer is live: the token array one id short is a heap-buffer-overflow read in the estimator
    _write_corpus(corpus, 4, tokens, offsets, short=True)
    r = subprocess.run([exe, corpus, out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "heap-buffer-overflow" in r.stderr, r.stderr[-2000:]
