"""The edit script of long pairs on the device (include/casr.h casr_edit_align; csrc/edit_align.hip)
against the host entry (casr_edit_align_host), which tests/test_edit_align_host.py pins to the Python
restatement: distance, counts and both maps exactly, at every tile boundary, through whole tiles of
deletions and insertions, at the limit's indexing; the refusals, the clamp and its guard bit; the
encode and the beam of the handle left alone."""
import numpy as np
import pytest
import torch

import edit_align_ref as A
import edit_ref as R
from casr import lib as L
from casr.config import CasrConfig
from casr.weights import synthetic_state_dicts

pytestmark = pytest.mark.gpu

CFG = CasrConfig()
TR, TC = L.EDIT_ALIGN_TILE
M_SIZES = (0, 1, 63, 64, 65, TR - 1, TR, TR + 1, 2 * TR + 1)
N_SIZES = (0, 1, 63, 64, 65, 129, 193)
KEYS = ("dist", "ops", "b_of_a", "a_of_b")


@pytest.fixture(scope="module")
def eng():
    from casr.engine import Engine
    e = Engine(CFG)  # no weights: the alignment needs none
    yield e
    e.close()


def _device(eng, a, al, b, bl):
    return {k: v.cpu().numpy() for k, v in eng.edit_align(a, al, b, bl).items()}


def _check(eng, pairs, La=None, Lb=None):
    args = R.pad_pairs(pairs, La, Lb)
    want = L.edit_align_host(*args)
    got = _device(eng, *args)
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:5].tolist())
    return got


def _copy_to(rs, m, n, alphabet, edits):
    a, b = A.edited_copy(rs, n, alphabet, edits)
    return (a + rs.randint(0, alphabet, size=m).tolist())[:m], b


@pytest.mark.parametrize("alphabet", [2, 5, 300])
def test_size_grid_equals_the_host_entry(eng, alphabet):
    rs = np.random.RandomState(alphabet)
    pairs = [_copy_to(rs, m, n, alphabet, max(m, n) // 10 + 2) for m in M_SIZES for n in N_SIZES]
    eng.device_flags()
    got = _check(eng, pairs)
    assert eng.device_flags() == 0
    # the distance alone (no bits are kept) is the same, and a second call gives the same bits
    args = R.pad_pairs(pairs)
    only = eng.edit_align(*args, ops=False, maps=False)
    assert only["ops"] is None and only["b_of_a"] is None and np.array_equal(only["dist"].cpu().numpy(), got["dist"])
    again = _device(eng, *args)
    assert all(np.array_equal(again[k], got[k]) for k in KEYS)


def test_runs_through_whole_tiles(eng):
    rs = np.random.RandomState(6)
    base = rs.randint(0, 300, size=400).tolist()
    deleted = base[:70] + rs.randint(300, 600, size=TR + 150).tolist() + base[70:]   # a vertical run
    inserted = base[:130] + rs.randint(300, 600, size=2 * TC + 90).tolist() + base[130:]  # a horizontal run
    got = _check(eng, [(deleted, base), (base, inserted), (deleted, inserted)])
    assert got["ops"][0].tolist() == [0, TR + 150, 0] and got["ops"][1].tolist() == [2 * TC + 90, 0, 0]
    assert (got["b_of_a"][0, 70:70 + TR + 150] == -1).all() and (got["a_of_b"][1, 130:130 + 2 * TC + 90] == -1).all()


def test_one_call_with_several_pairs_in_wider_arrays(eng):
    rs = np.random.RandomState(8)
    pairs = [_copy_to(rs, 300, 280, 5, 30), ([], []), _copy_to(rs, 17, 400, 2, 5), _copy_to(rs, 129, 64, 300, 9),
             _copy_to(rs, 500, 3, 5, 2)]
    _check(eng, pairs, 520, 450)


def test_larger_pairs_and_the_limit_s_indexing(eng):
    rs = np.random.RandomState(10)
    _check(eng, [_copy_to(rs, 4099, 3001, 50, 300)])
    _check(eng, [_copy_to(rs, 32768, 65, 4, 6)])
    _check(eng, [_copy_to(rs, 65, 32768, 4, 6)])


def test_refusals_leave_outputs_and_workspace_alone(eng):
    n = 2
    z = torch.zeros(n, 32769, dtype=torch.int32, device=eng.device)
    s = torch.zeros(n, 4, dtype=torch.int32, device=eng.device)
    ln = torch.full((n,), 2, dtype=torch.int32, device=eng.device)
    dist = torch.full((n,), -5, dtype=torch.int32, device=eng.device)
    ops = torch.full((n, 3), -5, dtype=torch.int32, device=eng.device)
    p = lambda t: t.data_ptr()  # noqa: E731
    _check(eng, [([1, 2], [1, 3])])
    before = eng.edit_align_workspace_bytes()
    assert before > 0
    for La, Lb, pa, pb in ((32769, 4, z, s), (4, 32769, s, z), (0, 4, s, s)):
        rc = eng.lib.casr_edit_align(eng.handle, p(pa), p(ln), La, p(pb), p(ln), Lb, n, p(dist), p(ops), None, None, None)
        assert rc == 4, (La, Lb, rc)
    # a call whose bits pass 1 GiB: 5 pairs at the limit (the arrays are never read: only their shape counts)
    rc = eng.lib.casr_edit_align(eng.handle, p(z), p(ln), 32768, p(z), p(ln), 32768, 5, p(dist), p(ops), None, None, None)
    assert rc == 4
    assert L.edit_align_plan(32768, 32768, 5)["bits_bytes"] > 2 ** 30
    torch.cuda.synchronize()
    assert eng.edit_align_workspace_bytes() == before
    assert (dist.cpu() == -5).all() and (ops.cpu() == -5).all()
    with pytest.raises(L.CasrError, match="CASR_ERR_UNSUPPORTED"):
        eng.edit_align(z, ln, s, ln)


def test_lengths_out_of_range_are_clamped_and_flagged(eng):
    pairs = R.seeded_pairs(8, 77, max_len=20)
    a, al, b, bl = R.pad_pairs(pairs, 20, 24)
    bad_a, bad_b = al.copy(), bl.copy()
    bad_a[2], bad_b[5] = -1, 25
    clamp_a, clamp_b = bad_a.copy(), bad_b.copy()
    clamp_a[2], clamp_b[5] = 0, 24
    want = L.edit_align_host(a, clamp_a, b, clamp_b)
    eng.device_flags()
    got = _device(eng, a, bad_a, b, bad_b)
    assert eng.device_flags() == 1
    assert all(np.array_equal(got[k], want[k]) for k in KEYS)
    _device(eng, a, clamp_a, b, clamp_b)
    assert eng.device_flags() == 0


def test_dist_and_ops_equal_casr_edit_distance(eng):
    pairs = R.seeded_pairs(300, 41, max_len=512)
    assert max(len(p) for p, _ in pairs) > 400
    a, al, b, bl = R.pad_pairs(pairs, 512, 512)
    d, o = (x.cpu().numpy() for x in eng.edit_distance(a, al, b, bl, ops=True))
    got = eng.edit_align(a, al, b, bl, maps=False)
    assert np.array_equal(got["dist"].cpu().numpy(), d) and np.array_equal(got["ops"].cpu().numpy(), o)


def test_encode_and_beam_are_left_alone():
    """A greedy decode after an edit_align call gives the bits it gives without one, and the records of a
    beam are still readable after one."""
    from casr.engine import Engine
    enc, dec = synthetic_state_dicts(CFG, peaked=True)
    e = Engine(CFG, enc, dec)
    try:
        rs = np.random.RandomState(2)
        feat = torch.from_numpy(rs.standard_normal((3, 90, CFG.feat_dim)).astype(np.float32)).to(e.device)
        lens = torch.tensor([90, 61, 75], dtype=torch.int32, device=e.device)
        pair = R.pad_pairs([_copy_to(rs, 300, 200, 5, 20)])
        e.encode(feat, lens)
        want = {k: v.clone() for k, v in e.greedy(alignment=True).items() if torch.is_tensor(v)}
        e.encode(feat, lens)
        e.edit_align(*pair)
        got = e.greedy(alignment=True)
        for k, v in want.items():
            assert torch.equal(got[k], v), k
        e.encode(feat, lens)
        e.beam(4, 1.5, 1.5)
        rec = [x.clone() for x in e.beam_records()]
        r = e.edit_align(*pair)
        host = L.edit_align_host(*pair)
        assert all(np.array_equal(r[k].cpu().numpy(), host[k]) for k in KEYS)
        for x, y in zip(e.beam_records(), rec):
            assert torch.equal(x, y)
        assert e.device_flags() == 0
    finally:
        e.close()
