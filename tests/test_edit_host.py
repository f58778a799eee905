"""Edit distance, operation counts and the MBR choice on the host (include/casr.h
casr_edit_distance_host, casr_mbr_host; csrc/edit_plan.h), without a GPU.

The distances and counts must equal casr.results.edit_distance / edit_ops value for value; the MBR
choice and risks the numpy restatement of the formulas (tests/edit_ref.py).  wer_batch without an engine
must return the Python values of the get_wer loop it replaces, and the plan is checked at every
boundary through a small program that includes the header."""
import os
import subprocess

import numpy as np
import pytest

import edit_ref as R
from casr import lib as L
from casr.results import get_wer, wer_batch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def seeded():
    pairs = R.seeded_pairs(1500, 11)
    return pairs, R.reference(pairs)


# ---------------------------------------------------------------------------- distances and ops
def test_api_exports_and_limit():
    import re
    hdr = open(os.path.join(REPO, "include", "casr.h")).read()
    assert int(re.search(r"#define CASR_EDIT_MAX_LEN (\d+)", hdr).group(1)) == L.EDIT_MAX_LEN == 512
    for name in ("casr_edit_distance_host", "casr_edit_distance", "casr_mbr_host", "casr_beam_mbr"):
        assert name in L.EXPORTS and hasattr(L.load(), name)
    assert L.OPTIONS["MBR_MAP"] == 19


def test_seeded_pairs_equal_the_python_reference(seeded):
    pairs, (want_d, want_o) = seeded
    assert max(max(len(p), len(r)) for p, r in pairs) <= 70
    a, al, b, bl = R.pad_pairs(pairs)
    dist, ops = L.edit_distance_host(a, al, b, bl, ops=True)
    assert np.array_equal(dist, want_d)
    assert np.array_equal(ops, want_o)
    assert np.array_equal(L.edit_distance_host(a, al, b, bl), want_d)
    assert np.array_equal(ops.sum(axis=1), dist)


def test_the_ops_check_is_not_vacuous(seeded):
    """Every branch of the backtrace is taken by the seeded pairs, and at least 100 of them have counts
    that another tie order (insert before delete before replace) changes."""
    pairs, (_, want_o) = seeded
    branches, changed = {}, 0
    for (p, r), o in zip(pairs, want_o.tolist()):
        assert R.backtrace(p, r, branches=branches) == tuple(o)
        changed += R.backtrace(p, r, order=("match", "insert", "delete", "replace")) != tuple(o)
    for key in ("match", "replace", "delete", "insert", "delete_edge", "insert_edge"):
        assert branches.get(key, 0) > 0, key
    assert changed >= 100, changed


def test_hand_cases():
    pairs = R.hand_pairs()
    want_d, want_o = R.reference(pairs)
    assert want_d[:5].tolist() == [0, 1, 1, 0, 1] and want_d[5] == 0 and want_d[6] == 30
    dist, ops = L.edit_distance_host(*R.pad_pairs(pairs), ops=True)
    assert np.array_equal(dist, want_d) and np.array_equal(ops, want_o)
    # the same pairs in wider arrays: nothing past a length is read as data
    dist2, ops2 = L.edit_distance_host(*R.pad_pairs(pairs, 80, 90), ops=True)
    assert np.array_equal(dist2, want_d) and np.array_equal(ops2, want_o)


def test_long_rows_past_the_device_limit():
    rs = np.random.RandomState(3)
    pairs = [R.edited_pair(rs, 512, 4, 0)]
    pairs += [(R.edited_pair(rs, 512, 4, 40)[0][:512], rs.randint(0, 4, size=512).tolist())]
    pairs += [(rs.randint(0, 3, size=513).tolist(), [1, 2, 0]), ([1, 2, 0], rs.randint(0, 3, size=513).tolist())]
    want_d, want_o = R.reference(pairs)
    dist, ops = L.edit_distance_host(*R.pad_pairs(pairs), ops=True)
    assert np.array_equal(dist, want_d) and np.array_equal(ops, want_o)


def test_host_entry_refusals():
    a = np.zeros((2, 4), np.int32)
    ok = np.array([4, 0], np.int32)
    for bad in (np.array([5, 0], np.int32), np.array([0, -1], np.int32)):
        with pytest.raises(L.CasrError, match="CASR_ERR_ARG"):
            L.edit_distance_host(a, bad, a, ok)
        with pytest.raises(L.CasrError, match="CASR_ERR_ARG"):
            L.edit_distance_host(a, ok, a, bad)
    assert L.edit_distance_host(np.zeros((0, 3), np.int32), [], np.zeros((0, 2), np.int32), []).shape == (0,)
    assert L.edit_distance_host(np.zeros((1, 0), np.int32), [0], np.ones((1, 2), np.int32), [2]).tolist() == [2]


# ---------------------------------------------------------------------------- MBR
MBR_L, MBR_K = 12, 5


def _sets(seed0, count, ns, equal_scores=False):
    out = []
    for i in range(count):
        rs = np.random.RandomState(seed0 + i)
        out.append(R.random_record_set(rs, ns[i % len(ns)], MBR_L, MBR_K, equal_scores=equal_scores))
    return [np.stack(x) for x in zip(*out)]


@pytest.mark.parametrize("scale", [0.0, 0.3, 1.0, 1e6])
def test_mbr_host_equals_the_restatement(scale):
    ns = (0, 1, 2, 3, 7, 20, 41, 60)
    rt, sc, va, lm = _sets(100, 48, ns)
    assert sc.dtype == np.float32
    best, risk = L.mbr_host(rt, sc, va, scale, rec_lm=lm, lm_weight=0.4, length_weight=0.7, risk=True)
    excused = 0
    for b in range(rt.shape[0]):
        flat, toks, s, q = R.records_of(rt[b], sc[b], va[b], lm[b], MBR_K)
        assert len(flat) == ns[b % len(ns)]
        want, wrisk, c, _ = R.mbr_utterance(toks, s, q, scale, 0.4, 0.7)
        got_risk = risk[b].reshape(-1)
        assert np.all(got_risk[np.setdiff1d(np.arange(MBR_L * MBR_K), flat)] == 0)
        assert np.allclose(got_risk[flat], wrisk, rtol=1e-12, atol=0)
        if want < 0:
            assert best[b] == -1
        elif best[b] != flat[want]:
            assert R.near_tie(wrisk, want), (b, best[b], flat[want])
            excused += 1
    assert excused <= rt.shape[0] // 100, excused


def test_mbr_host_without_lm_and_risk_outputs():
    rt, sc, va, lm = _sets(300, 12, (5, 9, 30))
    best = L.mbr_host(rt, sc, va, 0.5, length_weight=0.25)
    for b in range(rt.shape[0]):
        flat, toks, s, q = R.records_of(rt[b], sc[b], va[b], lm[b], MBR_K)
        want, wrisk, _, _ = R.mbr_utterance(toks, s, np.zeros_like(q), 0.5, 0.0, 0.25)
        assert best[b] == flat[want] or R.near_tie(wrisk, want)


def test_exactly_tied_risks_take_the_lower_index():
    """n = 2 with equal scores: both risks are w d(0, 1), bit for bit, so the first record wins."""
    rt, sc, va, lm = _sets(400, 20, (2,), equal_scores=True)
    best, risk = L.mbr_host(rt, sc, va, 0.3, risk=True)
    differ = 0
    for b in range(rt.shape[0]):
        flat, toks, _, _ = R.records_of(rt[b], sc[b], va[b], lm[b], MBR_K)
        r = risk[b].reshape(-1)[flat]
        assert r[0] == r[1] and best[b] == flat[0]
        differ += toks[0] != toks[1]
    assert differ >= 10


def test_scale_zero_is_the_medoid_and_a_large_scale_the_first_maximum():
    rt, sc, va, lm = _sets(500, 30, (3, 8, 25, 60))
    # scores on a grid of 1/64, LM off: c = s + 0.5 l is exact, so a maximum is unique or an exact tie
    sc = (np.round(sc * 64) / 64).astype(np.float32)
    med = L.mbr_host(rt, sc, va, 0.0, length_weight=0.5)
    top = L.mbr_host(rt, sc, va, 1e6, length_weight=0.5)
    differ = 0
    for b in range(rt.shape[0]):
        flat, toks, s, q = R.records_of(rt[b], sc[b], va[b], lm[b], MBR_K)
        _, _, c, dist = R.mbr_utterance(toks, s, q * 0, 0.0, 0.0, 0.5)
        sums = dist.sum(axis=1)
        assert med[b] == flat[int(np.argmin(sums))]  # (integer sums: the first minimum)
        if (c == c.max()).sum() == 1:
            # every other weight underflows to 0: risk_i = d(i, max), which only the maximum reaches 0
            # with, or an earlier record of the very same tokens (these random sets hold such twins)
            am = int(np.argmax(c))
            assert top[b] == flat[int(np.flatnonzero(dist[:, am] == 0)[0])]
            assert toks[flat.tolist().index(top[b])] == toks[am]
        differ += med[b] != top[b]
    assert differ >= 3


def test_mbr_host_refusals():
    rt, sc, va, lm = _sets(600, 2, (3,))
    for scale in (-1.0, float("inf"), float("nan")):
        with pytest.raises(L.CasrError, match="CASR_ERR_ARG"):
            L.mbr_host(rt, sc, va, scale)
    assert L.mbr_host(rt[:0], sc[:0], va[:0], 1.0).shape == (0,)


# ---------------------------------------------------------------------------- wer_batch
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("return_tuple", [False, True])
def test_wer_batch_returns_the_values_of_the_get_wer_loop(normalize, return_tuple):
    rs = np.random.RandomState(9)
    chars = "的一是不了人我在有他这为之大来以个中上们\U0001F600ab"
    words = ["的", "北京", "abc", "é", "\U0001F600x"]  # multi-character words: compared by code point
    preds, refs = [], []
    for i in range(60):
        ref = "".join(rs.choice(list(chars), size=rs.randint(1, 40)))
        pred = list(ref)
        for _ in range(rs.randint(0, 6)):
            pred[rs.randint(len(pred)):rs.randint(len(pred)) + 1] = rs.choice(words)
        preds.append("".join(pred))
        refs.append(ref)
    preds.append("")
    refs.append("的的")
    want = [get_wer(p, r, normalize, return_tuple) for p, r in zip(preds, refs)]
    got = wer_batch(preds, refs, normalize, return_tuple)
    assert got == want and [type(x) for x in got] == [type(x) for x in want]
    if return_tuple:
        assert all(type(e) is type(f) for x, y in zip(got, want) for e, f in zip(x, y))
    ids = R.seeded_pairs(80, 21, max_len=30)
    ids = [(p, r) for p, r in ids if r]
    want = [get_wer(p, r, normalize, return_tuple) for p, r in ids]
    assert wer_batch([p for p, _ in ids], [r for _, r in ids], normalize, return_tuple) == want
    assert wer_batch([], []) == []


def test_wer_batch_empty_reference_raises_as_get_wer_does():
    with pytest.raises(ZeroDivisionError):
        get_wer("ab", "")
    with pytest.raises(ZeroDivisionError):
        wer_batch(["ab"], [""])
    assert wer_batch(["ab"], [""], normalize=False) == [get_wer("ab", "", normalize=False)] == [2]
    # a row past the device limit goes to the host entry whatever engine is given
    long_ref = "的" * 600
    assert wer_batch([long_ref[:-3]], [long_ref], engine=object()) == [get_wer(long_ref[:-3], long_ref)]


# ---------------------------------------------------------------------------- the plan
PLAN_SRC = r"""
#include <cstdio>
#include "edit_plan.h"
using namespace casr;
int main() {
  // pairs: La Lb ops -> form strips lds raise
  const int L[] = {0, 1, 40, 63, 64, 65, 128, 129, 511, 512, 513};
  for (int la : L) for (int lb : L) for (int ops = 0; ops < 2; ++ops) {
    const EditPlan p = edit_plan_pairs(la, lb, 7, ops != 0);
    std::printf("P %d %d %d %d %d %d %zu %d\n", la, lb, ops, p.form, p.strips, p.grid, p.lds_bytes, (int)p.raise_lds);
  }
  const int ML[] = {0, 1, 40, 64, 65, 255, 256}, MK[] = {0, 1, 4, 16, 31, 32, 64};
  for (int l : ML) for (int k : MK) for (int map = -1; map <= 3; ++map) {
    const EditPlan p = edit_plan_mbr(l, k, map);
    std::printf("M %d %d %d %d %d %d %zu\n", l, k, map, p.form, p.strips, p.grid, p.lds_bytes);
  }
  std::printf("D %d\n", EDIT_MBR_DEFAULT_FORM);
  return 0;
}
"""


def test_plan_at_every_boundary(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("clang++ not available")
    src, exe = tmp_path / "plan.cpp", str(tmp_path / "plan")
    src.write_text(PLAN_SRC)
    subprocess.run([CLANG, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
                    "-I" + os.path.join(REPO, "chinese-asr_amd", "csrc"), str(src), "-o", exe],
                   check=True, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    default = int([ln for ln in out if ln.startswith("D ")][0].split()[1])
    assert default in (1, 2)
    seen = 0
    for ln in out:
        f = ln.split()
        if not f or f[0] == "D":
            continue
        v = [int(x) for x in f[1:]]
        seen += 1
        if f[0] == "P":
            la, lb, ops, form, strips, grid, lds, raise_lds = v
            if not (1 <= la <= 512 and 1 <= lb <= 512):
                assert form == 0, ln
                continue
            words = lb * ((la + 15) // 16)
            assert form == 1 and strips == (lb + 63) // 64 and grid == 7, ln
            assert lds == 4 * (2 * la + 1) + (4 * words if ops else 0), ln
            assert raise_lds == (lds > 65536) and lds <= 160 * 1024, ln
        else:
            l, k, mp, form, strips, grid, lds = v
            tree = 8 * l * k
            want = {1: tree + 4 * (3 * l + 1), 2: tree + 4 * l + 64 * (l + 1)}
            pick = mp if mp in (1, 2) else default
            if not (1 <= l <= 255 and k >= 1 and 0 <= mp <= 2) or want[pick] > 65536:
                assert form == 0, ln
                continue
            assert form == pick and lds == want[pick] and grid == 128 and strips == (l + 63) // 64, ln
    assert seen == 11 * 11 * 2 + 7 * 7 * 5
    # the one shape that needs more than the default LDS: 512 x 512 with ops
    assert 4 * 1025 + 4 * 512 * 32 > 65536
