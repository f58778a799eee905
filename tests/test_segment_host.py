"""casr_segment_host (include/casr.h: segmentation of long recordings at their pauses, on the host)
against the numpy restatement of its formulas (tests/segment_ref.py), exactly: thr, the count, every
start and every length.  No GPU.

Inputs are fbank rows built from level sequences (a level plus seeded noise, spread over the 80 bins,
so stage (a) adds unequal numbers), about 200 seeds with n from 0 to 5,000 at small parameters, plus
hand-built rows; ``test_cases_cover`` asserts FROM THE REFERENCE's intermediate stages that the cases
hold every edge the operation has."""
import ctypes
import functools

import numpy as np
import pytest

import segment_ref as R
from casr import lib as L
from casr.segment import SegmentParams, segment_bound, segment_host

SMALL = R.SMALL
QUIET, LOUD = -9.0, -2.0


def params_of(p):
    return SegmentParams(**{k: getattr(p, k) for k in p.__dataclass_fields__})


def hand_levels():
    """Hand-built level sequences (name -> levels) at the SMALL parameters (min_speech 3, min_pause 6,
    pad 2, max_frames 64, min_frames 16, max_gap 10)."""
    def seq(*parts):  # (length, loud?) ...
        return np.concatenate([np.full(m, LOUD if on else QUIET) for m, on in parts])

    out = {}
    # active runs of min_speech - 1 and min_speech; quiet runs of min_pause - 1 and min_pause
    out["runs"] = seq((40, 0), (2, 1), (30, 0), (3, 1), (30, 0), (20, 1), (5, 0), (20, 1), (6, 0), (20, 1), (40, 0))
    out["island_at_0"] = seq((30, 1), (100, 0))
    out["island_at_n"] = seq((100, 0), (30, 1))
    out["long_island"] = np.concatenate([seq((20, 0)), LOUD + 0.8 * np.sin(np.arange(3 * 64 + 40) / 5.0), seq((60, 0))])
    out["tie"] = seq((30, 0), (150, 1), (120, 0))  # a constant level: every cut costs the same
    # a merge stopped by max_gap (11 quiet frames widen to a gap of 11 - 4 = 7 <= 10: merged; 20 -> 16: not)
    out["merge_gap"] = seq((20, 0), (10, 1), (11, 0), (10, 1), (20, 0), (10, 1), (60, 0))
    # and one stopped by max_frames: three islands of 24 at gaps of 4: two fit 64 frames, the third does not
    out["merge_len"] = seq((20, 0), (20, 1), (8, 0), (20, 1), (8, 0), (20, 1), (90, 0))
    out["all_quiet"] = seq((300, 0))
    out["all_active"] = seq((300, 1))
    out["n0"] = np.zeros(0)
    out["n1"] = seq((1, 1))
    out["n2"] = seq((1, 0), (1, 1))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, fbank [n, 80], P)]: computed once, shared, never modified."""
    out = []
    for i, (name, lv) in enumerate(hand_levels().items()):
        noise = 0.0 if name in ("tie", "all_quiet", "all_active") else 0.4
        # every frame is active only where thr = lo: no rise at all
        p = R.replace(SMALL, rise_min=0, rel_q8=0) if name == "all_active" else SMALL
        out.append((name, R.fbank_from_levels(lv, 1000 + i, noise=noise), p))
    rs = np.random.RandomState(5)
    for seed in range(200):
        n = int(rs.choice([0, 1, 2, 3, 17, 63, 64, 65, 300, 1023, 1024, 1025, 2500, 5000])) if seed < 60 else int(rs.randint(0, 5001))
        out.append((f"seed{seed}", R.fbank_from_levels(R.random_levels(n, seed), seed), SMALL))
    nan = R.fbank_from_levels(R.random_levels(400, 900), 900).copy()
    nan[123, 17] = np.nan
    nan[200, :] = np.nan
    nan[201, 3] = np.inf
    nan[202, 3] = -np.inf
    out.append(("nan", nan, SMALL))
    out.append(("default", R.fbank_from_levels(R.random_levels(5000, 901, mean_on=300, mean_off=60), 901), R.P()))
    for _, fb, _ in out:
        fb.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(i):
    name, fb, p = cases()[i]
    d = {}
    thr, segs = R.segment_fbank(fb, len(fb), p, d)
    return thr, segs, d


def host(fb, p, s_max=None, n=None, T=None):
    n = len(fb) if n is None else n
    T = max(len(fb), 1) if T is None else T
    buf = np.zeros((1, T, fb.shape[1]), np.float32)
    buf[0, :len(fb)] = fb
    start, length, n_seg, thr = segment_host(buf, [n], params_of(p), s_max)
    return start[0], length[0], int(n_seg[0]), int(thr[0])


def test_host_equals_reference_exactly():
    for i, (name, fb, p) in enumerate(cases()):
        thr, segs, _ = reference(i)
        start, length, n_seg, got_thr = host(fb, p)
        assert got_thr == thr, name
        assert n_seg == len(segs), name
        got = list(zip(start[:n_seg].tolist(), length[:n_seg].tolist()))
        assert got == segs, name
        assert (start[n_seg:] == -1).all() and (length[n_seg:] == -1).all(), name


def test_invariants_and_bound():
    for i, (name, fb, p) in enumerate(cases()):
        _, segs, _ = reference(i)
        n, end = len(fb), 0
        for s, l in segs:
            assert s >= end and 1 <= l <= p.max_frames and s + l <= n, name
            end = s + l
        assert segment_bound(max(n, 1), params_of(p)) >= len(segs), name
        assert segment_bound(n, params_of(p)) == R.bound(n, p)


def test_cases_cover():
    """What the cases exercise, read from the reference's intermediate stages."""
    by = {name: reference(i) for i, (name, _, _) in enumerate(cases())}
    p = SMALL

    def a0_runs(name, v):
        return [e - s for val, s, e in R.runs(by[name][2]["a0"]) if val == v]

    def inner_quiet(name):  # quiet runs of A1 with an active frame on both sides
        a1 = by[name][2]["a1"]
        return [e - s for val, s, e in R.runs(a1) if not val and s > 0 and e < len(a1)]

    act = a0_runs("runs", True)
    assert p.min_speech - 1 in act and p.min_speech in act
    assert by["runs"][2]["a1"].sum() == by["runs"][2]["a0"].sum() - (p.min_speech - 1)  # only that run is cleared
    qt = inner_quiet("runs")
    assert p.min_pause - 1 in qt and p.min_pause in qt
    a2 = by["runs"][2]["a2"]
    assert sorted(e - s for v, s, e in R.runs(a2) if not v and s > 0 and e < len(a2)).count(p.min_pause - 1) == 0
    assert by["island_at_0"][2]["islands"][0][0] == 0 and by["island_at_0"][1][0][0] == 0
    n = len(by["island_at_n"][2]["a0"])
    assert by["island_at_n"][2]["islands"][-1][1] == n and sum(by["island_at_n"][1][-1]) == n
    s, e = by["long_island"][2]["islands"][0]
    assert e - s > 3 * p.max_frames and len(by["long_island"][2]["cuts"]) >= 3
    # the tie: every candidate cut of the constant level costs the same, and the largest c wins
    d = by["tie"][2]
    (s, e), (c, ties) = d["islands"][0], d["cuts"][0]
    assert ties > 1 and c == min(s + p.max_frames, e - p.min_frames)
    assert "gap" in by["merge_gap"][2]["stops"] and len(by["merge_gap"][2]["pieces"]) > len(by["merge_gap"][1])
    assert "len" in by["merge_len"][2]["stops"] and len(by["merge_len"][2]["pieces"]) > len(by["merge_len"][1])
    assert by["all_quiet"][1] == [] or not by["all_quiet"][2]["a0"].all()
    assert by["all_active"][2]["a0"].all() and len(by["all_active"][1]) >= 4
    assert by["n0"][1] == [] and by["n0"][0] == 0
    assert len(by["n1"][2]["a0"]) == 1 and len(by["n2"][2]["a0"]) == 2
    q = R.levels(dict((nm, fb) for nm, fb, _ in cases())["nan"])
    assert q[123] == 0 and q[200] == 0 and q[201] == 511 and q[202] == 0
    assert len(by["default"][1]) >= 3 and len(by["default"][2]["cuts"]) >= 1
    # across the random cases: cuts, merges and both stops occur many times
    rnd = [v for k, v in by.items() if k.startswith("seed")]
    assert sum(len(v[2]["cuts"]) for v in rnd) > 100
    assert sum(v[2]["stops"].count("gap") for v in rnd) > 100 and sum(v[2]["stops"].count("len") for v in rnd) > 100
    assert sum(len(v[1]) for v in rnd) > 2000


def test_all_quiet_has_no_segment():
    # a constant level: lo = hi, thr = lo + rise_min is above every frame
    i = [nm for nm, _, _ in cases()].index("all_quiet")
    assert reference(i)[1] == []


def test_s_max_smaller_than_count():
    i = [nm for nm, _, _ in cases()].index("seed70")
    name, fb, p = cases()[i]
    _, segs, _ = reference(i)
    assert len(segs) > 6
    for s_max in (0, 1, 5):
        start, length, n_seg, _ = host(fb, p, s_max=s_max)
        assert n_seg == len(segs) and len(start) == s_max
        assert list(zip(start.tolist(), length.tolist())) == segs[:s_max]
    # a wider row: entries past the count keep the sentinel
    start, length, n_seg, _ = host(fb, p, s_max=len(segs) + 3)
    assert (start[n_seg:] == -1).all() and (length[n_seg:] == -1).all()


def test_independent_of_padding_and_neighbours():
    """frames < T, garbage (NaN) past frames[b], other rows beside it: the same segments."""
    sel = [i for i, (nm, fb, _) in enumerate(cases()) if nm in ("seed61", "seed75", "long_island", "n1")]
    T = max(len(cases()[i][1]) for i in sel) + 37
    buf = np.full((len(sel), T, 80), np.nan, np.float32)
    for r, i in enumerate(sel):
        buf[r, :len(cases()[i][1])] = cases()[i][1]
    frames = [len(cases()[i][1]) for i in sel]
    start, length, n_seg, thr = segment_host(buf, frames, params_of(SMALL))
    for r, i in enumerate(sel):
        rt, segs, _ = reference(i)
        assert thr[r] == rt and n_seg[r] == len(segs)
        assert list(zip(start[r, :n_seg[r]].tolist(), length[r, :n_seg[r]].tolist())) == segs


INVALID = [dict(min_speech=0), dict(pad=-1), dict(min_pause=4, pad=2), dict(min_pause=0, pad=0), dict(min_frames=0),
           dict(min_frames=33), dict(max_frames=31), dict(max_gap=-1), dict(pct_lo=-1), dict(pct_lo=96),
           dict(pct_hi=101), dict(rel_q8=-1), dict(rel_q8=257), dict(rise_min=-1)]


@pytest.mark.parametrize("bad", INVALID, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_invalid_parameters(bad):
    p = R.replace(SMALL, **bad)
    assert not R.valid(p) and not params_of(p).valid()
    with pytest.raises(ValueError):
        params_of(p).validate()
    fb = np.zeros((1, 8, 80), np.float32)
    with pytest.raises(L.CasrError, match="CASR_ERR_ARG"):
        segment_host(fb, [8], params_of(p), s_max=4)
    c = params_of(p).struct()
    assert L.load().casr_segment_bound(100, ctypes.byref(c)) == -1


def test_host_argument_errors():
    fb = np.zeros((1, 8, 80), np.float32)
    for frames in ([9], [-1]):
        with pytest.raises(L.CasrError, match="CASR_ERR_ARG"):
            segment_host(fb, frames, params_of(SMALL), s_max=4)
    with pytest.raises(L.CasrError, match="CASR_ERR_UNSUPPORTED"):
        segment_host(np.zeros((1, 8, 40), np.float32), [8], params_of(SMALL), s_max=4)
    assert L.load().casr_segment_bound(100, None) == -1
    assert L.load().casr_segment_default_params(None) == 1


def test_defaults():
    assert SegmentParams() == SegmentParams.library_defaults()
    assert params_of(R.P()) == SegmentParams()
    assert SegmentParams().validate().valid() and R.valid(R.P())
    assert segment_bound(60000) == (60000 + 20) // 25 + 60000 // 200
