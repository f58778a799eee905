"""The edit script of long pairs on the host (include/casr.h casr_edit_align_host,
casr_edit_align_tiles_host, casr_edit_align_plan; csrc/edit_align_plan.h) and the span policy of
casr.longalign, without a GPU.

Distances, counts and both maps must equal the plain Python restatement (tests/edit_align_ref.py, built
on casr.results.edit_ops' table and rules) value for value; the tile-by-tile order the device takes must
equal the rolling-row form at every tile boundary; the plan's numbers are checked against formulas
written out here."""
import numpy as np
import pytest

import edit_align_ref as A
import edit_ref as R
from casr import lib as L
from casr import longalign as LA
from casr.results import wer_batch, wer_long

TR, TC = L.EDIT_ALIGN_TILE
M_SIZES = (0, 1, 63, 64, 65, TR - 1, TR, TR + 1, 2 * TR + 1)
N_SIZES = (0, 1, 63, 64, 65, 129, 193)


@pytest.fixture(scope="module")
def seeded():
    pairs = R.seeded_pairs(1000, 23)
    return pairs, A.reference(pairs)


def test_api_exports_and_limit():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "casr.h")).read()
    assert int(re.search(r"#define CASR_EDIT_ALIGN_MAX_LEN (\d+)", hdr).group(1)) == L.EDIT_ALIGN_MAX_LEN == 32768
    for name in ("casr_edit_align_host", "casr_edit_align", "casr_edit_align_tiles_host", "casr_edit_align_plan"):
        assert name in L.EXPORTS and hasattr(L.load(), name)
    assert (TR, TC) == (128, 64) and L.load().casr_api_version() == 3


def test_hand_cases():
    pairs = R.hand_pairs() + [
        ([5], []), ([], [5]),                                    # one symbol against nothing
        ([1, 2, 3], [9, 9, 1, 2, 3]), ([1, 2, 3], [1, 2, 3, 9, 9]),  # a pure prefix / suffix insertion
        ([9, 9, 1, 2, 3], [1, 2, 3]), ([1, 2, 3, 9, 9], [1, 2, 3]),  # a pure prefix / suffix deletion
        ([1, 2, 3, 4], [1, 9, 3, 4]), ([1, 1, 1], [1, 1]), ([1, 1], [1, 1, 1])]
    want = A.reference(pairs)
    n0 = len(R.hand_pairs())
    assert want["b_of_a"][n0 + 2, :3].tolist() == [2, 3, 4] and want["a_of_b"][n0 + 2, :5].tolist() == [-1, -1, 0, 1, 2]
    assert want["b_of_a"][n0 + 4, :5].tolist() == [-1, -1, 0, 1, 2] and want["ops"][n0 + 4].tolist() == [0, 2, 0]
    assert want["b_of_a"][n0 + 6, :4].tolist() == [0, 1, 2, 3] and want["ops"][n0 + 6].tolist() == [0, 0, 1]
    assert want["b_of_a"][5, :30].tolist() == list(range(30)) and want["dist"][6] == 30
    for tiles in (False, True):
        assert A.same(L.edit_align_host(*R.pad_pairs(pairs), tiles=tiles), want)
    # the same pairs in wider arrays: nothing past a length is read as data, everything past it is -1
    got = L.edit_align_host(*R.pad_pairs(pairs, 80, 90))
    assert A.same(got, A.reference(pairs, 80, 90))


def test_seeded_pairs_equal_the_restatement(seeded):
    pairs, want = seeded
    assert max(max(len(p), len(r)) for p, r in pairs) <= 70
    a, al, b, bl = R.pad_pairs(pairs)
    got = L.edit_align_host(a, al, b, bl)
    assert A.same(got, want)
    assert A.same(L.edit_align_host(a, al, b, bl, tiles=True), want)
    dist, ops = L.edit_distance_host(a, al, b, bl, ops=True)
    assert np.array_equal(got["dist"], dist) and np.array_equal(got["ops"], ops)
    # the maps are each other's inverse and count the diagonal steps
    for k in range(0, len(pairs), 7):
        ba, ab = got["b_of_a"][k], got["a_of_b"][k]
        for i in np.nonzero(ba >= 0)[0]:
            assert ab[ba[i]] == i
        assert (ba >= 0).sum() == (ab >= 0).sum() == al[k] - ops[k, 1] == bl[k] - ops[k, 0]


def test_the_map_check_is_not_vacuous(seeded):
    """Every branch of the backtrace is taken by the seeded pairs, and at least 100 of them have maps
    that another tie order (insert before delete before replace) changes."""
    pairs, want = seeded
    branches, changed = {}, 0
    for k, (p, r) in enumerate(pairs):
        _, ops, ba, ab = A.align(p, r, branches=branches)
        assert ba == want["b_of_a"][k, :len(p)].tolist() and tuple(ops) == R.backtrace(p, r)
        other = A.align(p, r, order=("match", "insert", "delete", "replace"))
        changed += (other[2], other[3]) != (ba, ab)
    for key in ("match", "replace", "delete", "insert", "delete_edge", "insert_edge"):
        assert branches.get(key, 0) > 0, key
    assert changed >= 100, changed


def _grid_pairs(alphabet, seed):
    """One pair per size of the grid: b random, a an edited copy of it cut or filled to its length."""
    rs = np.random.RandomState(seed)
    pairs = []
    for m in M_SIZES:
        for n in N_SIZES:
            a, b = A.edited_copy(rs, n, alphabet, max(m, n) // 10 + 2)
            pairs.append(((a + rs.randint(0, alphabet, size=m).tolist())[:m], b))
    return pairs


def test_tile_order_equals_rolling_rows_at_every_boundary():
    """m over {0, 1, 63, 64, 65, TR - 1, TR, TR + 1, 2 TR + 1} crossed with n over {0, 1, 63, 64, 65, 129,
    193}: the device's order (hand-offs through colc and rowc, launch by launch) against the rolling
    row, and the rolling row against the Python restatement."""
    for alphabet, seed in ((2, 1), (5, 2), (300, 3)):
        pairs = _grid_pairs(alphabet, seed)
        assert sorted({(len(p), len(r)) for p, r in pairs}) == sorted((m, n) for m in M_SIZES for n in N_SIZES)
        args = R.pad_pairs(pairs)
        rows = L.edit_align_host(*args)
        tiles = L.edit_align_host(*args, tiles=True)
        for key in ("dist", "ops", "b_of_a", "a_of_b"):
            assert np.array_equal(rows[key], tiles[key]), (alphabet, key)
        if alphabet == 5:
            assert A.same(rows, A.reference(pairs))
        dist, ops = L.edit_distance_host(*args, ops=True)
        assert np.array_equal(rows["dist"], dist) and np.array_equal(rows["ops"], ops)


def _want_plan(La, Lb, n):
    tr, tc = -(-La // TR), -(-Lb // TC)
    bits = n * tr * tc * TR * TC // 4
    r256 = lambda x: -(-x // 256) * 256  # noqa: E731
    grid = [n * sum(1 for ti in range(tr) if 0 <= d - ti < tc) for d in range(tr + tc - 1)]
    return dict(ok=bits <= 2 ** 30, tiles_r=tr, tiles_c=tc, launches=tr + tc - 1, bits_bytes=bits,
                bytes=r256(bits) + r256(4 * n * (La + 1)) + r256(4 * n * tc * 65), grid=grid)


def test_plan_launches_grids_and_workspace():
    for La in M_SIZES[1:]:
        for Lb in N_SIZES[1:]:
            for n in (1, 3):
                got = L.edit_align_plan(La, Lb, n)
                assert got == _want_plan(La, Lb, n), (La, Lb, n)
                assert sum(got["grid"]) == n * got["tiles_r"] * got["tiles_c"]
    top = L.edit_align_plan(32768, 32768, 1)
    assert top == _want_plan(32768, 32768, 1)
    assert top["ok"] and top["bits_bytes"] == 256 * 2 ** 20 and top["launches"] == 256 + 512 - 1
    assert max(top["grid"]) == 256 and top["grid"][0] == top["grid"][-1] == 1
    assert L.edit_align_plan(32768, 65, 1) == _want_plan(32768, 65, 1)
    assert L.edit_align_plan(65, 32768, 1) == _want_plan(65, 32768, 1)
    assert L.edit_align_plan(16, 16, 7, bits=False)["bits_bytes"] == 0


def test_plan_refusals():
    for La, Lb in ((0, 5), (5, 0), (32769, 5), (5, 32769), (-1, 5)):
        assert not L.edit_align_plan(La, Lb, 1)["ok"], (La, Lb)
    # the direction bits of a call stop at 1 GiB: four pairs at the limit are exactly that
    assert L.edit_align_plan(32768, 32768, 4)["ok"] and L.edit_align_plan(32768, 32768, 4)["bits_bytes"] == 2 ** 30
    assert not L.edit_align_plan(32768, 32768, 5)["ok"]
    assert L.edit_align_plan(128, 64, 2 ** 19)["ok"] and not L.edit_align_plan(128, 64, 2 ** 19 + 1)["ok"]
    assert not L.edit_align_plan(129, 64, 2 ** 18 + 1)["ok"] and not L.edit_align_plan(128, 64, 2 ** 31 - 1)["ok"]


def test_host_entry_refusals_and_empty_calls():
    a = np.zeros((2, 4), np.int32)
    ok = np.array([4, 0], np.int32)
    for bad in (np.array([5, 0], np.int32), np.array([0, -1], np.int32)):
        for tiles in (False, True):
            with pytest.raises(L.CasrError, match="CASR_ERR_ARG"):
                L.edit_align_host(a, bad, a, ok, tiles=tiles)
            with pytest.raises(L.CasrError, match="CASR_ERR_ARG"):
                L.edit_align_host(a, ok, a, bad, tiles=tiles)
    assert L.edit_align_host(np.zeros((0, 3), np.int32), [], np.zeros((0, 2), np.int32), [])["dist"].shape == (0,)
    r = L.edit_align_host(np.zeros((1, 0), np.int32), [0], np.ones((1, 2), np.int32), [2])
    assert r["dist"].tolist() == [2] and r["ops"].tolist() == [[2, 0, 0]] and r["a_of_b"].tolist() == [[-1, -1]]


def test_wer_long_equals_wer_batch_and_takes_long_rows():
    pairs = R.seeded_pairs(60, 5)
    hyps, refs = [p for p, _ in pairs], [r for _, r in pairs]
    assert wer_long(hyps, refs) == wer_batch(hyps, refs, normalize=False, return_tuple=True)
    assert wer_long(["abcd", ""], ["abed", "xy"]) == [(1, 0, 0, 1), (2, 2, 0, 0)]
    rs = np.random.RandomState(4)
    ref = rs.randint(0, 50, size=3000).tolist()
    hyp = ref[:1000] + ref[1200:2000] + [77] * 30 + ref[2000:]
    dist, ops = L.edit_distance_host(*R.pad_pairs([(hyp, ref)]), ops=True)
    assert wer_long([hyp], [ref]) == [(int(dist[0]),) + tuple(ops[0].tolist())] and 170 <= dist[0] <= 230


# ---------------------------------------------------------------------------- casr.longalign
def test_assign_spans_rules():
    # aligned positions go to the segment that holds their hypothesis position
    assert LA.assign_spans([2, 3], [0, 1, 2, 3, 4]) == [(0, 2), (2, 5)]
    # an inserted run inside one segment stays there
    assert LA.assign_spans([3, 2], [0, -1, -1, 1, 2, 3, 4]) == [(0, 5), (5, 7)]
    # a run across a boundary goes to the earlier segment
    assert LA.assign_spans([2, 2], [0, 1, -1, -1, 2, 3]) == [(0, 4), (4, 6)]
    # a run before the first aligned position goes to the first segment that has a hypothesis
    assert LA.assign_spans([0, 2, 2], [-1, -1, 0, 1, 2, 3]) == [(0, 0), (0, 4), (4, 6)]
    assert LA.assign_spans([2, 2], [-1, 2, 3]) == [(0, 1), (1, 3)]
    # a run after the last aligned position stays with that position's segment
    assert LA.assign_spans([2, 2], [0, 1, 2, -1, -1]) == [(0, 2), (2, 5)]
    assert LA.assign_spans([2, 2], [0, 1, -1, -1]) == [(0, 4), (4, 4)]
    # a segment with an empty hypothesis between two others gets an empty span
    assert LA.assign_spans([2, 0, 2], [0, 1, -1, 2, 3]) == [(0, 3), (3, 3), (3, 5)]
    # deleted hypothesis positions leave their segment's span short or empty
    assert LA.assign_spans([2, 2, 2], [0, 1, 4, 5]) == [(0, 2), (2, 2), (2, 4)]
    # nothing aligned: everything to the first segment with a hypothesis; none has one: the first
    assert LA.assign_spans([0, 3], [-1, -1]) == [(0, 0), (0, 2)]
    assert LA.assign_spans([0, 0], [-1, -1]) == [(0, 2), (2, 2)]
    assert LA.assign_spans([1, 1], []) == [(0, 0), (0, 0)] and LA.assign_spans([], []) == []
    with pytest.raises(ValueError):
        LA.assign_spans([], [0])
    with pytest.raises(ValueError):
        LA.assign_spans([2], [0, 2])


def test_spans_are_monotone_and_cover_on_seeded_maps(seeded):
    pairs, want = seeded
    rs = np.random.RandomState(9)
    for k in range(0, len(pairs), 5):
        p, r = pairs[k]
        cuts = sorted(rs.randint(0, len(p) + 1, size=3).tolist())
        counts = [cuts[0], cuts[1] - cuts[0], cuts[2] - cuts[1], len(p) - cuts[2]]
        spans = LA.assign_spans(counts, want["a_of_b"][k, :len(r)])
        assert spans[0][0] == 0 and spans[-1][1] == len(r)
        assert all(lo <= hi for lo, hi in spans) and all(spans[s][1] == spans[s + 1][0] for s in range(3))
        ends = np.cumsum(counts)
        for s, (lo, hi) in enumerate(spans):
            for j in range(lo, hi):
                i = want["a_of_b"][k, j]
                assert i < 0 or (ends[s] - counts[s] <= i < ends[s])


def test_unaligned_characters_are_put_back():
    w2i = {"a": 10, "b": 11, "c": 12, "d": 13}
    text = '"a, b!c d.'
    ids, pos = LA.text_ids(text, w2i)
    assert ids == [10, 11, 12, 13] and pos == [1, 4, 6, 8]
    assert LA.hyp_ids("ab<", w2i) == [10, 11, LA.HYP_UNKNOWN]
    spans = [(0, 2), (2, 2), (2, 4)]
    parts = LA.span_text(text, pos, spans)
    assert parts == ['"a, b!', '', 'c d.'] and ''.join(parts) == text
    ch = LA.span_chars(text, pos, 0, 2, [(1.0, 1.5, 0.9), (1.5, 2.0, 0.8)], 0.5)
    assert ch == [('"', 0.5, 0.5, None), ('a', 1.0, 1.5, 0.9), (',', 1.5, 1.5, None), (' ', 1.5, 1.5, None),
                  ('b', 1.5, 2.0, 0.8), ('!', 2.0, 2.0, None)]
    ch = LA.span_chars(text, pos, 2, 4, [(3.0, 3.5, 0.7), (3.5, 4.0, 0.6)], 3.0)
    assert ''.join(c[0] for c in ch) == 'c d.' and ch[-1] == ('.', 4.0, 4.0, None)
    assert LA.span_chars(text, pos, 2, 2, None, 0.0) == []
    # a span that does not start the transcript begins at its first aligned character
    assert LA.span_text(text, pos, [(0, 1), (1, 4)]) == ['"a, ', 'b!c d.']
    # nothing aligned: the first segment carries the text
    assert LA.span_text("?!", [], [(0, 0), (0, 0)]) == ["?!", ""]
    assert LA.interpolate(4, 2.0, 4.0) == [(2.0, 2.5, None), (2.5, 3.0, None), (3.0, 3.5, None), (3.5, 4.0, None)]
    assert LA.interpolate(0, 2.0, 4.0) == []
