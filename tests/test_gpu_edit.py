"""Edit distance on the device (include/casr.h casr_edit_distance; csrc/edit.hip) against the host entry
(casr_edit_distance_host), which tests/test_edit_host.py pins to casr.results.edit_distance / edit_ops:
distances and operation counts exactly, at the strip boundaries of the wave form and at the longest
rows; the clamp and its guard bit; the refusal past CASR_EDIT_MAX_LEN; repeatable bits."""
import numpy as np
import pytest
import torch

import edit_ref as R
from casr import lib as L
from casr.config import CasrConfig

pytestmark = pytest.mark.gpu

CFG = CasrConfig()


@pytest.fixture(scope="module")
def eng():
    from casr.engine import Engine
    e = Engine(CFG)  # no weights: the distances need none
    yield e
    e.close()


def _both(eng, a, al, b, bl):
    d1, o1 = (x.cpu().numpy() for x in eng.edit_distance(a, al, b, bl, ops=True))
    d0 = eng.edit_distance(a, al, b, bl).cpu().numpy()
    return d0, d1, o1


def _shaped_pairs(n, La, Lb, seed):
    """n pairs with rows up to (La, Lb): a reference and an edited copy over a small alphabet, cut to
    the shape; the first pair has full rows."""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        alphabet = (2, 5, 300)[i % 3]
        lb = Lb if i == 0 else int(rs.randint(0, Lb + 1))
        p, r = R.edited_pair(rs, lb, alphabet, int(rs.randint(0, 8)))
        if i == 0 or rs.rand() < 0.3:  # rows of unrelated lengths too
            p = rs.randint(0, alphabet, size=La if i == 0 else rs.randint(0, La + 1)).tolist()
        out.append((p[:La], r))
    return out


def test_hand_cases_equal_the_host_entry(eng):
    pairs = R.hand_pairs()
    a, al, b, bl = R.pad_pairs(pairs)
    want_d, want_o = L.edit_distance_host(a, al, b, bl, ops=True)
    eng.device_flags()
    d0, d1, o1 = _both(eng, a, al, b, bl)
    assert eng.device_flags() == 0
    assert np.array_equal(d1, want_d) and np.array_equal(o1, want_o) and np.array_equal(d0, want_d)


@pytest.mark.parametrize("La,Lb", [(1, 1), (40, 40), (64, 65), (130, 7), (512, 512)])
def test_seeded_pairs_equal_the_host_entry(eng, La, Lb):
    pairs = _shaped_pairs(300, La, Lb, 1000 + La + Lb)
    a, al, b, bl = R.pad_pairs(pairs, La, Lb)
    assert al.max() == La and bl.max() == Lb
    want_d, want_o = L.edit_distance_host(a, al, b, bl, ops=True)
    eng.device_flags()
    d0, d1, o1 = _both(eng, a, al, b, bl)
    assert eng.device_flags() == 0
    assert np.array_equal(d1, want_d), np.flatnonzero(d1 != want_d)[:5]
    assert np.array_equal(o1, want_o), np.flatnonzero((o1 != want_o).any(axis=1))[:5]
    assert np.array_equal(d0, d1)  # the two kernels agree
    d0b, d1b, o1b = _both(eng, a, al, b, bl)  # and a second call gives the same bits
    assert np.array_equal(d0b, d0) and np.array_equal(d1b, d1) and np.array_equal(o1b, o1)


def test_zero_and_one_pair(eng):
    e = np.zeros((0, 5), np.int32)
    d, o = eng.edit_distance(e, np.zeros(0, np.int32), e, np.zeros(0, np.int32), ops=True)
    assert d.shape == (0,) and o.shape == (0, 3)
    a, al, b, bl = R.pad_pairs([([1, 2, 3, 4], [1, 3, 4, 4, 5])])
    d, o = eng.edit_distance(a, al, b, bl, ops=True)
    wd, wo = L.edit_distance_host(a, al, b, bl, ops=True)
    assert d.cpu().numpy().tolist() == wd.tolist() and o.cpu().numpy().tolist() == wo.tolist()


def test_lengths_out_of_range_are_clamped_and_flagged(eng):
    pairs = R.seeded_pairs(8, 77, max_len=20)
    a, al, b, bl = R.pad_pairs(pairs, 20, 24)
    bad_a, bad_b = al.copy(), bl.copy()
    bad_a[2] = -1
    bad_b[5] = 25
    clamp_a, clamp_b = bad_a.copy(), bad_b.copy()
    clamp_a[2] = 0
    clamp_b[5] = 24
    want_d, want_o = L.edit_distance_host(a, clamp_a, b, clamp_b, ops=True)
    eng.device_flags()
    d, o = (x.cpu().numpy() for x in eng.edit_distance(a, bad_a, b, bad_b, ops=True))
    assert eng.device_flags() == 1
    assert np.array_equal(d, want_d) and np.array_equal(o, want_o)
    d = eng.edit_distance(a, bad_a, b, bad_b).cpu().numpy()
    assert eng.device_flags() == 1 and np.array_equal(d, want_d)
    eng.edit_distance(a, clamp_a, b, clamp_b)
    assert eng.device_flags() == 0


def test_rows_past_the_limit_are_refused_and_nothing_is_written(eng):
    n = 3
    a = torch.zeros(n, 513, dtype=torch.int32, device=eng.device)
    b = torch.zeros(n, 4, dtype=torch.int32, device=eng.device)
    al = torch.full((n,), 2, dtype=torch.int32, device=eng.device)
    dist = torch.full((n,), -5, dtype=torch.int32, device=eng.device)
    ops = torch.full((n, 3), -5, dtype=torch.int32, device=eng.device)
    p = lambda t: t.data_ptr()  # noqa: E731
    for La, Lb, pa, pb in ((513, 4, a, b), (4, 513, b, a), (0, 4, b, b)):
        rc = eng.lib.casr_edit_distance(eng.handle, p(pa), p(al), La, p(pb), p(al), Lb, n, p(dist), p(ops), None)
        assert rc == 4, (La, Lb, rc)
    torch.cuda.synchronize()
    assert (dist.cpu() == -5).all() and (ops.cpu() == -5).all()
    with pytest.raises(L.CasrError, match="CASR_ERR_UNSUPPORTED"):
        eng.edit_distance(a, al, b, al)
