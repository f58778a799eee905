"""csrc/grammar_plan.h (the acceptor's builder, its transition, the candidate rule, the sentence walk and
the row rule, which the kernels of csrc/grammar.hip and csrc/beam_lm.hip compile too) and the readers'
gate with BeamState::grammar (csrc/beam_state.h), under AddressSanitizer + UndefinedBehaviorSanitizer on
the CPU.

``tests/host_asan/grammar_check.cpp`` and ``tests/host_plan/beam_state_grammar_check.cpp`` are programs
of their own: the first includes the header, reads every array into a heap buffer of exactly its length,
queries the tables from such buffers, and its distances, walks and rows must equal the restatement of
tests/grammar_ref.py.  Nothing is loaded into Python, no library is preloaded, and nothing runs on a GPU."""
import os
import subprocess

import numpy as np
import pytest

import grammar_ref as GR

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-fno-omit-frame-pointer", "-I" + os.path.join(REPO, "include"),
         "-I" + os.path.join(REPO, "chinese-asr_amd", "csrc")]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
V, EOS = 12, 2
BUDGETS = (-1, 0, 1, 5, 10 ** 6)


def _write_cases(path, sets, short=None):
    """short = (set, sentence): that sentence is written one symbol short (the sanitizer must see the read)."""
    with open(path, "wb") as f:
        f.write(np.int32(len(sets)).tobytes())
        for i, (vocab, eos, arcs, finals, sents, rows) in enumerate(sets):
            S = len(arcs)
            f.write(np.array([vocab, eos, S], np.int32).tobytes())
            off = np.zeros(S + 1, np.int64)
            off[1:] = np.cumsum([len(r) for r in arcs])
            f.write(off.tobytes())
            f.write(np.int64(off[-1]).tobytes())
            f.write(np.array([t for r in arcs for t, _ in r], np.int32).tobytes())
            f.write(np.array([d for r in arcs for _, d in r], np.int32).tobytes())
            fin = np.zeros(S, np.uint8)
            fin[np.array(sorted(finals), np.intp)] = 1
            f.write(fin.tobytes())
            f.write(np.int32(len(sents)).tobytes())
            for j, y in enumerate(sents):
                row = np.array(y, np.int64).astype(np.int32)
                f.write(np.int32(row.size).tobytes())
                row = row[:-1] if (i, j) == short else row
                f.write(np.int64(row.size).tobytes())
                f.write(row.tobytes())
            f.write(np.int32(len(rows)).tobytes())
            f.write(np.array(rows, np.int32).reshape(-1).tobytes())


def _set(seed):
    arcs, finals, sents = GR.seeded_acceptor(seed, V, EOS)
    rows = [(s, b) for s in list(range(len(arcs))) + [-1, len(arcs), -7] for b in BUDGETS]
    return V, EOS, arcs, finals, sents, rows


@pytest.mark.timeout(600)
def test_grammar_plan_under_asan_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("clang++ not available")
    exe = str(tmp_path / "grammar_check")
    subprocess.run([CLANG] + FLAGS + [os.path.join(HERE, "host_asan", "grammar_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    sets = [_set(seed) for seed in range(200)]
    # a chain of 12 tokens (a long walk), a state with every token, and a refusal (state 1 reaches no final state)
    chain = [[(3 + (i % 9), i + 1)] for i in range(12)] + [[]]
    walk = [3 + (i % 9) for i in range(12)]
    sets.append((V, EOS, chain, [12], [walk, walk[:11], walk + [3], []], [(0, 11), (0, 12), (11, 0), (12, -1)]))
    sets.append((V, EOS, [[(3, 0), (4, 1)], []], [0], [[3, 3]], [(0, 0)]))
    src, out = str(tmp_path / "cases.bin"), str(tmp_path / "out.txt")
    _write_cases(src, sets)
    r = subprocess.run([exe, src, out], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "grammar_check ok" in r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = iter(open(out).read().split("\n"))
    for i, (vocab, eos, arcs, finals, sents, rows) in enumerate(sets):
        head = next(lines).split()
        assert head[0] == "G"
        if i == len(sets) - 1:
            assert int(head[1]) == 1
            continue
        assert int(head[1]) == 0 and int(head[2]) == len(arcs)
        acc = GR.TripleAcceptor({(s, v, d) for s, row in enumerate(arcs) for v, d in row}, finals, len(arcs))
        assert [int(x) for x in next(lines).split()[1:]] == acc.dist(), i
        for y in sents:
            s = next(lines).split()
            n, cur = acc.walk(y, vocab)
            assert s[0] == "S" and int(s[1]) == n and {int(s[2])} == cur, (i, y)
            assert int(s[3]) == acc.accepts(y, vocab), (i, y)
        for state, budget in rows:
            row = next(lines).split()
            assert row[0] == "R" and int(row[1]) == (state != -1 and not 0 <= state < len(arcs)), (i, state)
            want = acc.row(state, budget, vocab, eos)
            assert row[2] == "".join("01"[int(x)] for x in want), (i, state, budget)
    # the sanitizer is live: a sentence one symbol short is a heap-buffer-overflow read of the walk
    short = (200, 0)
    _write_cases(src, sets, short=short)
    r = subprocess.run([exe, src, out], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode != 0 and "heap-buffer-overflow" in r.stderr, r.stderr[-2000:]


@pytest.mark.timeout(300)
def test_beam_state_gate_with_the_grammar_flag_under_asan_ubsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("clang++ not available")
    exe = str(tmp_path / "beam_state_grammar_check")
    subprocess.run([CLANG] + FLAGS + [os.path.join(HERE, "host_plan", "beam_state_grammar_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "beam_state_grammar_check ok" in r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
