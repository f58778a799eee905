"""The monotone attention path on the host (include/casr.h casr_align_path_host; csrc/align_plan.h),
the span arithmetic of casr.results.token_spans and the subtitle cues of casr.subtitles, without a GPU.

The host entry must equal the numpy restatement of the formulas (tests/align_ref.py: the plain
sequential double loop) value for value."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import align_ref as R
from casr import lib as L
from casr import subtitles as S
from casr.results import EvalOutput, token_spans

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SHAPES = [(1, 1, 1), (1, 3, 2), (17, 7, 63), (16, 40, 64), (33, 41, 65), (5, 40, 129), (65, 12, 266)]
KEYS = ("first", "last", "peak", "path_score")


def same(got, want):
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), k


def test_api_exports_and_limit():
    hdr = open(os.path.join(REPO, "include", "casr.h")).read()
    assert int(re.search(r"#define CASR_ALIGN_MAX_TP (\d+)", hdr).group(1)) == L.ALIGN_MAX_TP == 1024
    for name in ("casr_align_path_host", "casr_align_path"):
        assert name in L.EXPORTS and hasattr(L.load(), name)
    assert L.OPTIONS["ALIGN_GROUP"] == 20 and L.load().casr_api_version() == 3


def test_quantiser_table():
    """One cell per utterance: its path score is the cell's weight."""
    table = [(1.0, 0), (0.5, -128), (2.0 ** -24, -3072), (2.0 ** -25, -3072), (1e-40, -3072), (0.75, -64),
             (np.nan, -3072), (0.0, -3072), (-1.0, -3072), (2.0, 0), (np.inf, 0), (-np.inf, -3072), (0.25, -256),
             (2.0 ** -23, -2944), (np.float32(1.0) - np.float32(2.0 ** -24), -1)]
    a = np.array([x for x, _ in table], np.float32).reshape(1, 1, -1)
    one = np.ones(len(table), np.int32)
    r = L.align_path_host(a, one, one)
    assert r["path_score"].tolist() == [q for _, q in table]
    assert R.quant(a).reshape(-1).tolist() == [q for _, q in table]
    assert not r["first"].any() and not r["last"].any() and not r["peak"].any()


def test_seeded_cases_equal_the_reference():
    """About 300 cases over the shapes the device test uses (the first round at their full batch, the
    others at two utterances: the host entry loops over b), every generator, lengths drawn per
    utterance with 0, 1, Tp and L among them; and the invariants on every one."""
    cases, moves = 0, set()
    for rnd in range(43):
        for i, (B, Lx, Tp) in enumerate(SHAPES):
            B = B if rnd == 0 else min(B, 2)
            a, enc, tgt = R.seeded_case(1000 * rnd + i, B, Lx, Tp)
            got, want = L.align_path_host(a, enc, tgt), R.path(a, enc, tgt)
            same(got, want)
            R.check_invariants(a, enc, tgt, got)
            cases += 1
            for b in range(B):
                f, la = got["first"][b], got["last"][b]
                for l in range(1, min(int(tgt[b]), Lx) if enc[b] > 0 else 0):
                    moves.add("vertical" if f[l] == la[l - 1] else "diagonal")
                    moves.add("stay" if la[l] > f[l] else "single")
    assert cases == 301 and moves == {"vertical", "diagonal", "stay", "single"}


def test_constant_rows_follow_the_tie_order():
    """Every cell equal: the diagonal first, then (nothing above left) the stay; with T < n the vertical."""
    a = np.full((5, 9, 2), 0.5, np.float32)
    r = L.align_path_host(a, [9, 3], [5, 5])
    same(r, R.path(a, [9, 3], [5, 5]))
    # T = 9, n = 5: the fewest cells is 9; from the end the diagonal is taken while it can be
    assert r["first"][0].tolist() == [0, 5, 6, 7, 8] and r["last"][0].tolist() == [4, 5, 6, 7, 8]
    assert r["path_score"][0] == -128 * 9
    # T = 3, n = 5: 5 cells, two vertical moves
    assert r["path_score"][1] == -128 * 5 and r["last"][1, 4] == 2 and r["first"][1, 0] == 0


def test_planted_paths_are_found():
    """alpha = 0.5 on a token's own span, 2^-10 elsewhere: every path has >= T cells of <= -128 each, and
    only the planted one has exactly T cells all at -128."""
    for seed, (B, Lx, Tp) in enumerate([(8, 7, 63), (6, 40, 64), (4, 41, 129), (3, 12, 266), (5, 3, 3)]):
        a, enc, tgt, first, last = R.planted(np.random.RandomState(50 + seed), B, Lx, Tp)
        r = L.align_path_host(a, enc, tgt)
        assert np.array_equal(r["first"], first) and np.array_equal(r["last"], last)
        assert np.array_equal(r["peak"], first)  # (equal weights on the span: the smallest frame)
        assert np.array_equal(r["path_score"], -128 * enc)
        same(r, R.path(a, enc, tgt))


def test_fewer_frames_than_tokens():
    rs = np.random.RandomState(9)
    for Lx, Tp in [(40, 9), (12, 3), (7, 1), (41, 40)]:
        a = R.softmax_rows(rs, 6, Lx, Tp)
        enc = rs.randint(1, Tp + 1, size=6).astype(np.int32)
        tgt = np.full(6, Lx, np.int32)
        r = L.align_path_host(a, enc, tgt)
        same(r, R.path(a, enc, tgt))
        R.check_invariants(a, enc, tgt, r)
        assert (r["first"] >= 0).all() and (r["last"] >= r["first"]).all()  # every token has a cell
        assert (np.diff(r["first"], axis=1) >= 0).all() and (np.diff(r["last"], axis=1) >= 0).all()
        shared = r["first"][:, 1:] == r["last"][:, :-1]
        assert shared.sum(axis=1).min() >= Lx - Tp  # adjacent spans share frames where there are too few


def test_clamps_and_values_past_the_lengths():
    a, enc, tgt = R.seeded_case(7, 6, 9, 20)
    enc2, tgt2 = enc.copy(), tgt.copy()
    enc2[0], tgt2[1], enc2[2], tgt2[3] = -1, 9 + 3, 20 + 5, -4
    r = L.align_path_host(a, enc2, tgt2)
    same(r, R.path(a, enc2, tgt2))
    assert (r["first"][0] == -1).all() and r["path_score"][0] == 0 and (r["first"][3] == -1).all()
    same(r, L.align_path_host(a, np.clip(enc2, 0, 20), np.clip(tgt2, 0, 9)))
    # nothing at t >= T or l >= n is read as data
    enc, tgt = np.array([5, 20, 1, 0, 7, 13], np.int32), np.array([9, 2, 3, 4, 0, 8], np.int32)
    want = L.align_path_host(a, enc, tgt)
    p = a.copy()
    for b in range(6):
        p[:, enc[b]:, b] = np.nan
        p[tgt[b]:, :, b] = np.nan
    same(L.align_path_host(p, enc, tgt), want)


def test_error_paths():
    lib = L.load()
    a = np.full((2, 3, 1), 0.5, np.float32)
    one = np.ones(1, np.int32)
    out = [np.full((1, 2), 77, np.int32) for _ in range(3)]
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    good = [ptr(a), ptr(one), ptr(one), 1, 3, 2] + [ptr(o) for o in out] + [None]
    assert lib.casr_align_path_host(*good) == 0 and out[0][0].tolist() == [0, -1]  # (path_score may be NULL)
    for o in out:
        o[:] = 77
    for i in (0, 1, 2, 6, 7, 8):
        bad = list(good)
        bad[i] = None
        assert lib.casr_align_path_host(*bad) == 1
    for i, v in ((3, 0), (4, 0), (5, 0), (5, 513), (3, -1)):
        bad = list(good)
        bad[i] = v
        assert lib.casr_align_path_host(*bad) == 1
    assert b"casr_align_path_host" in lib.casr_last_error(None)
    assert all((o == 77).all() for o in out)  # nothing written on an error
    # the device entry without a handle: refused before anything else
    assert lib.casr_align_path(None, *good, None) == 1
    # any Tp on the host, beyond the device entry's limit
    Tp = L.ALIGN_MAX_TP + 77
    a = R.softmax_rows(np.random.RandomState(2), 1, 3, Tp)
    r = L.align_path_host(a, [Tp], [3])
    same(r, R.path(a, [Tp], [3]))


# ---------------------------------------------------------------------------- token_spans
def test_token_spans_arithmetic():
    first = np.array([[0, 4, 9, -1], [0, 0, 1, 2]], np.int32)
    last = np.array([[3, 8, 11, -1], [0, 1, 1, 5]], np.int32)
    peak = np.array([[2, 4, 10, -1], [0, 1, 1, 3]], np.int32)
    lp = np.log(np.array([[0.5, 0.25, 1.0, 1.0], [0.125, 1.0, 0.5, 0.75]]))
    sp = token_spans(first, last, peak, lp, [3, 4], 16000, n_tokens=[2, 4])
    assert [len(x) for x in sp] == [2, 4]  # the closing eos of utterance 0 is scored, not listed
    assert sp[0][0] == pytest.approx((0.0, 0.12, 0.06, 0.5)) and sp[0][1] == pytest.approx((0.12, 0.27, 0.12, 0.25))
    assert sp[1][3] == pytest.approx((0.06, 0.18, 0.09, 0.75))
    assert len(token_spans(first, last, peak, lp, [3, 4])[0]) == 3  # by default every scored position
    assert token_spans(first, last, peak, lp, [3, 4], 8000)[0][1][0] == pytest.approx(0.24)
    assert EvalOutput(1, 2, 3, 4, 5, 6, 7, 8).timing is None and EvalOutput._fields[-1] == "timing"


# ---------------------------------------------------------------------------- subtitles
def seg(start, text, chars=True, step=0.3, gaps=()):
    t, cs = start, []
    for i, ch in enumerate(text):
        t += 1.0 if i in gaps else 0.0
        cs.append((ch, t, t + step, 0.9))
        t += step
    return SimpleNamespace(start_s=start, end_s=t, text=text, chars=cs if chars else None)


def test_cues_split_rule():
    assert S.cues([]) == [] and S.to_srt([]) == "" and S.to_vtt([]) == "WEBVTT\n\n"
    # within both limits: one cue per segment, with the characters' own times; empty segments give none
    c = S.cues([seg(1.0, "abc"), seg(5.0, ""), seg(7.0, "de", chars=False)])
    assert c == [S.Cue(1.0, pytest.approx(1.9), "abc"), S.Cue(7.0, pytest.approx(7.6), "de")]
    # over max_chars: cut at the largest gap, wherever it is
    c = S.cues([seg(0.0, "abcdefgh", step=0.1, gaps=(6,))], max_chars=6)
    assert [x.text for x in c] == ["abcdef", "gh"] and c[1].start_s == pytest.approx(1.6)
    # equal gaps: the cut nearest the middle (of two as near, the earlier), again while a part is over
    # the limit: 10 -> 5 + 5 -> (2 + 3) + (2 + 3)
    c = S.cues([seg(0.0, "abcdefghij", step=0.1)], max_chars=4)
    assert [x.text for x in c] == ["ab", "cde", "fg", "hij"]
    # over max_s only
    c = S.cues([seg(0.0, "abcd", step=2.0)], max_chars=20, max_s=6.0)
    assert [x.text for x in c] == ["ab", "cd"] and c[0].end_s == pytest.approx(4.0)
    # one character cannot be split
    assert len(S.cues([seg(0.0, "a", step=9.0)])) == 1


def test_srt_and_vtt_format():
    c = [S.Cue(0.0, 1.2345, "你好"), S.Cue(3661.0049, 3725.9996, "ab")]
    assert S.to_srt(c) == ("1\n00:00:00,000 --> 00:00:01,234\n你好\n\n"
                           "2\n01:01:01,005 --> 01:02:06,000\nab\n\n")
    assert S.to_vtt(c) == ("WEBVTT\n\n00:00:00.000 --> 00:00:01.234\n你好\n\n"
                           "01:01:01.005 --> 01:02:06.000\nab\n\n")
