"""Hotword biasing on the device (include/casr.h casr_bias_score, casr_bias_rows, casr_beam_bias,
casr_beam_record_bias).

Gain rows and sentence scores against the host entries exactly; a zero bias weight and an empty phrase
set against casr_beam and casr_beam_lm bit for bit (every width class, both arithmetics, the folded
step); invariants on the device's own records, where near ties of the search play no part (a record's
rec_bias is the brute-force bias_closed of its tokens, its rec_lm its sentence score, the best the first
maximum of the defined expression); the numpy restatement (tests/bias_ref.py) at the inputs whose rank
gaps tests/test_bias_host.py checked; refusals and state; Model, BeamShardDecoder and main.parse_batch."""
import numpy as np
import pytest
import torch

import bias_ref as BR
import fusion_ref as FR
import ngram_ref as R
from golden_util import fbank_for
from casr import lib as L
from casr.bias import PhraseBias
from casr.config import CasrConfig
from casr.ngram import NgramLM
from casr.results import records_by_utterance
from casr.weights import synthetic_state_dicts

pytestmark = pytest.mark.gpu

CFG = CasrConfig()
V = CFG.vocab
B, T = 6, 101
F = np.float32
I2W = {i: f"w{i}" for i in range(V)}
W2I = {w: i for i, w in I2W.items()}
_PACKED = {}


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _engine(eos_bias, cfg=CFG):
    from casr.engine import Engine
    if eos_bias not in _PACKED:
        _PACKED[eos_bias] = L.pack_weights(CFG, *synthetic_state_dicts(CFG, peaked=True, eos_bias=eos_bias))
    return Engine(cfg, packed=_PACKED[eos_bias])


def _encode(e, nb=B, t=T, ids=None):
    ids = list(range(nb)) if ids is None else ids
    fb = torch.from_numpy(np.stack([fbank_for(b, t) for b in ids])).to(e.device)
    e.encode_fbank(fb, torch.full((len(ids),), t, dtype=torch.int32, device=e.device))


def _np(d):
    return {n: (v.cpu().numpy() if v is not None else None) for n, v in d.items()}


def _phrases(seed, n=300):
    """Phrases over a 40-token alphabet inside V = 5004: lengths 1..16, shared prefixes and suffixes."""
    rs = np.random.RandomState(seed)
    seen, ph, bo = set(), [], []
    for _ in range(n):
        p = tuple(int(x) for x in 100 + rs.randint(0, int(rs.choice([3, 6, 40])), size=int(rs.choice([1, 2, 3, 4, 7, 16]))))
        if p not in seen:
            seen.add(p)
            ph.append(list(p))
            bo.append(int(rs.choice([1, 128, 256, 4096])))
    return ph, bo


# ---------------------------------------------------------------------------- 1. rows and sentences
def test_device_rows_and_scores_equal_the_host():
    from casr.engine import Engine
    ph, bo = _phrases(5)
    pb = PhraseBias(ph, {}, V, [b / 256 for b in bo])
    empty = PhraseBias([], {}, V)
    rs = np.random.RandomState(6)
    n, Ls = 64, 24
    tok = (100 + rs.randint(0, 6, size=(n, Ls))).astype(np.int32)
    lens = rs.randint(0, Ls + 1, size=n).astype(np.int32)
    lens[:2] = (0, Ls)
    for i in range(0, n, 3):  # a phrase planted, so deep states occur
        p = ph[rs.randint(len(ph))]
        at = rs.randint(0, Ls - 1)
        tok[i, at:at + len(p)] = p[:Ls - at]
    tok[5, 3], tok[7, 0] = V, -1  # ids outside the vocabulary match nothing
    e = Engine(CFG)  # no weights: the entries need none
    try:
        e.device_flags()
        for obj in (pb, empty):
            hf, ht, hs = obj.score_ids(tok, lens)
            df, dt, ds = (x.cpu().numpy() for x in e.bias_score(obj, tok, lens))
            assert np.array_equal(df, hf) and np.array_equal(dt, ht) and np.array_equal(ds, hs)
            hg, hn = obj.rows(hs, next=True)
            dg, dn = (x.cpu().numpy() for x in e.bias_rows(obj, hs, next=True))
            assert np.array_equal(dg, hg) and np.array_equal(dn, hn)
            assert np.array_equal(e.bias_rows(obj, hs).cpu().numpy(), hg)
        hf, ht, hs = pb.score_ids(tok, lens)
        assert hf.any() and ht.any() and len(set(hs.tolist())) > 8
        assert e.device_flags() == 0
        # guard bit 1: a state outside the automaton is the root's row; a length outside [0, L] is clamped
        st = hs[:4].copy()
        st[1], st[2] = -1, 10 ** 6
        got = e.bias_rows(pb, st).cpu().numpy()
        assert e.device_flags() == 1
        st[1] = st[2] = 0
        assert np.array_equal(got, pb.rows(st))
        bad = lens[:4].copy()
        bad[0], bad[3] = Ls + 3, -2
        df, dt, ds = (x.cpu().numpy() for x in e.bias_score(pb, tok[:4], bad))
        assert e.device_flags() == 1
        bad[0], bad[3] = Ls, 0
        hf, ht, hs = pb.score_ids(tok[:4], bad)
        assert np.array_equal(df, hf) and np.array_equal(dt, ht) and np.array_equal(ds, hs)
    finally:
        e.close()
        pb.close()
        empty.close()


# ---------------------------------------------------------------------------- 2. zero weight, no phrases
def _records(e):
    return [x.cpu().numpy() for x in e.beam_records()]


def _same(z, zrecs, want, recs, names):
    for n in ("tokens", "length", "steps"):
        assert np.array_equal(z[n], want[n]), n
    for n in names:
        assert np.array_equal(bits(z[n]), bits(want[n])), n
    assert np.array_equal(zrecs[0], recs[0]) and np.array_equal(bits(zrecs[1]), bits(recs[1]))
    assert np.array_equal(zrecs[2], recs[2])
    assert recs[2].any()


def _same_as_unbiased(e, k, lm, pb, empty):
    beam = _np(e.beam(k))
    recs = _records(e)
    fused = _np(e.beam_lm(lm, k, 1.5, 1.5))
    frecs, frq = _records(e), e.beam_record_lm().cpu().numpy()
    for obj, bw in ((pb, 0.0), (empty, 1.0)):
        z = _np(e.beam_bias(obj, k, bw))  # no LM, length weight 0: casr_beam's
        _same(z, _records(e), beam, recs, ("score",))
        assert not z["bias"].any() or obj is pb
        z = _np(e.beam_bias(obj, k, bw, lm, 1.5, 1.5))  # with the LM: casr_beam_lm's
        _same(z, _records(e), fused, frecs, ("score", "lm"))
        assert np.array_equal(bits(e.beam_record_lm().cpu().numpy()), bits(frq))
        if obj is empty:
            assert not z["bias"].any() and not e.beam_record_bias().cpu().numpy().any()


@pytest.mark.parametrize("k,precision", [(2, None), (4, None), (16, None), (4, "f32")])
def test_zero_bias_reproduces_beam_and_beam_lm(k, precision):
    grams = R.random_model(4, V, 61)
    lm = NgramLM.from_ids(*R.arrays_of(grams), {}, V)
    ph, bo = _phrases(7)
    pb = PhraseBias(ph + [[t] for t in range(3, 40)], {}, V, [b / 256 for b in bo] + [2.0] * 37)
    empty = PhraseBias([], {}, V)
    e = _engine(25.0)
    try:
        if precision:
            e.set_precision(precision)
        _encode(e)
        _same_as_unbiased(e, k, lm, pb, empty)
        assert e.device_flags() == 0
    finally:
        e.close()
        lm.close()
        pb.close()
        empty.close()


def test_zero_bias_reproduces_beam_on_the_folded_step():
    """B = 128, k = 8 (R = 1,024): casr_beam runs the folded step with its select inside the attention;
    the biased beam runs the same steps with its select as a launch of its own."""
    grams = R.random_model(4, V, 62)
    lm = NgramLM.from_ids(*R.arrays_of(grams), {}, V)
    ph, bo = _phrases(8)
    pb = PhraseBias(ph, {}, V, [b / 256 for b in bo])
    empty = PhraseBias([], {}, V)
    e = _engine(25.0)
    try:
        _encode(e, 128, 48)
        _same_as_unbiased(e, 8, lm, pb, empty)
        assert e.device_flags() == 0
    finally:
        e.close()
        lm.close()
        pb.close()
        empty.close()


# ---------------------------------------------------------------------------- 3. invariants
def _comb(a, q, z, l, w=1.5, bw=1.0, lw=1.5):
    return F(F(F(F(a) + F(F(w) * F(q))) + F(F(bw) * F(z))) + F(float(F(lw)) * float(l + 1)))


@pytest.mark.parametrize("k", [4, 16])
def test_invariants_on_the_devices_own_records(k):
    """fusion_ref.fusion_case()'s six utterances (B = 6, T = 101) under bias_ref.bias_case()'s weights
    (eos_bias 28.5: the search runs long enough for phrases to matter), LM and phrases."""
    case = BR.bias_case()
    ph, bo = case["phrases"], case["boosts"]
    lm = NgramLM.from_ids(*R.arrays_of(case["grams"]), W2I, V)
    ref = R.RefLM(4, V, case["grams"])
    pb = PhraseBias(ph, {}, V, [b / 256 for b in bo])
    e = _engine(BR.EOS_BIAS)
    try:
        _encode(e, ids=BR.UTTS)
        plain = _np(e.beam_lm(lm, k, 1.5, 1.5))
        e.device_flags()
        r = _np(e.beam_bias(pb, k, 1.0, lm, 1.5, 1.5))
        rt, rs, rv = _records(e)
        rq = e.beam_record_lm().cpu().numpy()
        rz = e.beam_record_bias().cpu().numpy()
        assert e.device_flags() == 0
        steps = int(r["steps"][0])
        assert rv.any() and not rv[:, steps:].any()
        assert not rz[~rv.astype(bool)].any() and not rq[~rv.astype(bool)].any()
        boosted = 0
        for b, l, c in zip(*np.nonzero(rv)):
            y = rt[b, l, c, :l].tolist()
            assert (rt[b, l, c, :l] >= 0).all() and (rt[b, l, c, l:] == -1).all()
            want = F(BR.full(y, ph, bo)) / F(256)
            assert bits(rz[b, l, c]) == bits(want), (b, l, c)
            assert bits(rq[b, l, c]) == bits(ref.sentence(y)), (b, l, c)
            boosted += want > 0
        assert boosted >= 1
        differs = 0
        for b in range(B):
            got = r["tokens"][b, :r["length"][b]].tolist()
            assert (r["tokens"][b, r["length"][b]:] == -1).all()
            idx = [(l, c) for l in range(steps) for c in range(k) if rv[b, l, c]]
            if idx:
                vals = [_comb(rs[b, l, c], rq[b, l, c], rz[b, l, c], l) for l, c in idx]
                l, c = idx[int(np.argmax(vals))]
                assert got == rt[b, l, c, :l].tolist(), b
                assert bits(r["score"][b]) == bits(rs[b, l, c]) and bits(r["lm"][b]) == bits(rq[b, l, c])
                assert bits(r["bias"][b]) == bits(rz[b, l, c])
            else:  # a live row of the last step: bias_open of its tokens
                assert r["length"][b] == steps and min(got) >= 0
                assert bits(r["bias"][b]) == bits(F(BR.full(got, ph, bo) + BR.tail(got, ph, bo)) / F(256)), b
            differs += got != plain["tokens"][b, :plain["length"][b]].tolist()
        assert differs >= 1, "the bias never changed a choice"
        r2 = _np(e.beam_bias(pb, k, 1.0, lm, 1.5, 1.5))  # two runs: the same bits
        for n in r:
            assert np.array_equal(r[n].view(np.int32), r2[n].view(np.int32)), n
        assert np.array_equal(bits(e.beam_record_bias().cpu().numpy()), bits(rz))
        assert e.device_flags() == 0
    finally:
        e.close()
        lm.close()
        pb.close()


def test_live_rows_use_bias_open_without_a_record():
    """An eos that can never win (eos_bias -60): no record, so the choice is among the live rows of the
    last step, under bias_open of their tokens."""
    ph, bo = _phrases(9)
    pb = PhraseBias(ph + [[t] for t in range(3, 60)], {}, V, [b / 256 for b in bo] + [1.0] * 57)
    ph, bo = pb.phrases, pb.boost_q
    e = _engine(-60.0)
    try:
        _encode(e, 2, 48)
        r = _np(e.beam_bias(pb, 4, 1.0))
        rt, rs, rv = _records(e)
        assert e.device_flags() == 0
        assert not rv.any() and int(r["steps"][0]) == CFG.max_len
        for b in range(2):
            y = r["tokens"][b].tolist()
            assert r["length"][b] == CFG.max_len and min(y) >= 0
            assert bits(r["bias"][b]) == bits(F(BR.full(y, ph, bo) + BR.tail(y, ph, bo)) / F(256)), b
    finally:
        e.close()
        pb.close()


# ---------------------------------------------------------------------------- 4. against bias_ref
@pytest.mark.parametrize("k,with_lm,precision", [(k, w, None) for k in BR.GPU_K for w in (True, False)] +
                         [(BR.GPU_K[0], True, "f32")])
def test_biased_beam_equals_the_numpy_restatement(k, with_lm, precision):
    """Tokens, records, am and bias at the widths of bias_ref.GPU_K, where tests/test_bias_host.py has
    asserted that the restatement's smallest gap between adjacent ranked vals is >= 1e-2.  No case tried
    reached that at k = 4 (bias_ref's note), so k = 4 and 16 rest on the bit-for-bit and invariant tests
    above."""
    case = BR.bias_case()
    want = BR.biased_case(k, with_lm)
    assert (want["gap"] >= 1e-2).all()
    ph, bo = case["phrases"], case["boosts"]
    lm = NgramLM.from_ids(*R.arrays_of(case["grams"]), W2I, V) if with_lm else None
    pb = PhraseBias(ph, {}, V, [b / 256 for b in bo])
    lw, nw = BR.WEIGHTS if with_lm else (0.0, BR.WEIGHTS[1])
    e = _engine(BR.EOS_BIAS)
    try:
        if precision:
            e.set_precision(precision)
        _encode(e, ids=BR.UTTS)
        r = _np(e.beam_bias(pb, k, BR.BIAS_WEIGHT, lm, lw, nw))
        rt, rs, rv = _records(e)
        rz = e.beam_record_bias().cpu().numpy()
        assert e.device_flags() == 0
        assert int(r["steps"][0]) == want["steps"]
        for b in range(B):
            assert r["tokens"][b, :r["length"][b]].tolist() == want["tokens"][b], b
            assert abs(r["score"][b] - want["score"][b]) <= 2e-3, b
            assert bits(r["bias"][b]) == bits(want["bias"][b]), b
            if with_lm:
                assert abs(r["lm"][b] - want["lm"][b]) <= 2e-3, b
            idx = [(l, c) for l in range(CFG.max_len) for c in range(k) if rv[b, l, c]]
            assert [rt[b, l, c, :l].tolist() for l, c in idx] == [t for t, _, _, _ in want["records"][b]], b
            for (l, c), (_, a, _, z) in zip(idx, want["records"][b]):
                assert abs(rs[b, l, c] - a) <= 2e-3 and bits(rz[b, l, c]) == bits(z), (b, l, c)
    finally:
        e.close()
        pb.close()
        if lm is not None:
            lm.close()


# ---------------------------------------------------------------------------- 5. refusals and state
def test_refusals_and_state():
    from casr.engine import Engine
    grams = R.random_model(3, V, 63)
    lm = NgramLM.from_ids(*R.arrays_of(grams), {}, V)
    pb = PhraseBias([[5, 6], [7]], {}, V)
    small = PhraseBias([[5, 6]], {}, 100)
    e = _engine(25.0)
    e2 = Engine(CFG)
    try:
        e.device_flags()
        dev = e.device
        out = dict(t=torch.full((B, CFG.max_len), 77, dtype=torch.int32, device=dev),
                   n=torch.full((B,), 77, dtype=torch.int32, device=dev), s=torch.full((B,), 77.0, device=dev),
                   q=torch.full((B,), 77.0, device=dev), z=torch.full((B,), 77.0, device=dev),
                   st=torch.full((1,), 77, dtype=torch.int32, device=dev))
        ptr = lambda x: x.data_ptr()

        def call(eng, bp, k, lmp=None, z="z"):
            return eng.lib.casr_beam_bias(eng.handle, bp, lmp, k, 1.0, 1.5, 1.5, ptr(out["t"]), ptr(out["n"]),
                                          ptr(out["s"]), ptr(out["q"]), ptr(out[z]) if z else None, ptr(out["st"]), None)

        assert call(e, pb.on(e), 4) == 3  # before an encode: CASR_ERR_STATE
        assert call(e2, pb.on(e2), 4) == 3  # before weights are bound
        _encode(e)
        assert call(e, None, 4) == 1
        assert call(e, pb._host, 4) == 1  # host-only
        assert call(e, small.on(e), 4) == 1  # vocab mismatch
        assert call(e, pb.on(e), 4, lm._host) == 1  # a host-only LM
        assert call(e, pb.on(e), 0) == 1 and call(e, pb.on(e), 17) == 1
        assert call(e, pb.on(e), 4, z=None) == 1  # a NULL output
        if torch.cuda.device_count() > 1:
            other = pb._create(e.lib, 1)
            assert call(e, other, 4) == 1  # on another device
            e.lib.casr_bias_destroy(other)
        st = torch.zeros(2, dtype=torch.int32, device=dev)
        rows = torch.full((2, V), 77, dtype=torch.int32, device=dev)
        for bp in (None, pb._host, small.on(e)):
            assert e.lib.casr_bias_rows(e.handle, bp, ptr(st), 2, ptr(rows), None, None) == 1
            assert e.lib.casr_bias_score(e.handle, bp, ptr(rows), ptr(st), 2, 8, ptr(st), None, None, None) == 1
        assert e.lib.casr_bias_rows(e.handle, pb.on(e), None, 2, ptr(rows), None, None) == 1
        for bad_l in (0, 513):
            assert e.lib.casr_bias_score(e.handle, pb.on(e), ptr(rows), ptr(st), 2, bad_l, ptr(st), None, None, None) == 4
        torch.cuda.synchronize()
        assert all(bool((x == 77).all()) for x in out.values()) and bool((rows == 77).all())
        # state: record_bias needs a biased beam; rescore and MBR refuse one; record_lm needs its LM
        e.beam(4)
        with pytest.raises(L.CasrError, match="CASR_ERR_STATE"):
            e.beam_record_bias()
        e.beam_bias(pb, 4)
        e.beam_record_bias()
        e.beam_records()
        with pytest.raises(L.CasrError, match="CASR_ERR_STATE"):
            e.beam_record_lm()
        with pytest.raises(L.CasrError, match="CASR_ERR_STATE"):
            e.beam_rescore(lm, 1.5, 1.5)
        with pytest.raises(L.CasrError, match="CASR_ERR_STATE"):
            e.beam_mbr(0.5)
        e.beam_bias(pb, 4, 1.0, lm, 1.5, 1.5)
        e.beam_record_lm()
        e.beam_record_bias()
        with pytest.raises(L.CasrError, match="CASR_ERR_STATE"):
            e.beam_rescore(lm, 1.5, 1.5)
        e.beam_lm(lm, 4, 1.5, 1.5)
        with pytest.raises(L.CasrError, match="CASR_ERR_STATE"):
            e.beam_record_bias()
        e.beam(4)
        e.beam_rescore(lm, 1.5, 1.5)
        e.beam_mbr(0.5)
        assert e.device_flags() == 0
    finally:
        e.close()
        e2.close()
        lm.close()
        pb.close()
        small.close()


# ---------------------------------------------------------------------------- 6. the Python layers
def _hot_from(recs, boost=2.0):
    """Bigrams of the second-best records: phrases the plain choice does not already spell."""
    ph = set()
    for b, v in recs.items():
        for t, _ in v[1:3]:
            ph.update(tuple(t[i:i + 2]) for i in range(len(t) - 1))
    return PhraseBias([list(p) for p in sorted(ph)], {}, V, boost)


def test_shard_decoder_runs_the_biased_beam_on_request():
    from casr.distributed import BeamShardDecoder, unpack_results
    e = _engine(25.0)
    fb = torch.from_numpy(np.stack([fbank_for(b, T) for b in range(B)])).cuda()
    fr = torch.full((B,), T, dtype=torch.int32, device=fb.device)
    try:
        _encode(e)
        e.beam(4)
        recs = records_by_utterance(*(x.cpu().numpy() for x in e.beam_records()))
        pb = _hot_from(recs)
        grams = FR.lm_grams_from_records(recs, V, 123)
        lm = NgramLM.from_ids(*R.arrays_of(grams), W2I, V)
        for fusion in (False, True):
            dec = BeamShardDecoder(e, 4, lm if fusion else None, I2W, 1.5, 1.5, max_batch=4, fusion=fusion, bias=pb,
                                   bias_weight=1.0)
            gt, gl, gs = unpack_results(dec.finish(dec.enqueue(fb, fr)), CFG.max_len)
            for c0, c1 in ((0, 4), (4, 6)):
                e.encode_fbank(fb[c0:c1], fr[c0:c1])
                r = _np(e.beam_bias(pb, 4, 1.0, lm if fusion else None, 1.5, 1.5))
                assert np.array_equal(gl[c0:c1], r["length"]) and np.array_equal(bits(gs[c0:c1]), bits(r["score"]))
                for b in range(c1 - c0):
                    assert gt[c0 + b, :gl[c0 + b]].tolist() == r["tokens"][b, :r["length"][b]].tolist()
        with pytest.raises(ValueError):
            BeamShardDecoder(e, 4, lm, I2W, 1.5, 1.5, bias=pb)
        assert e.device_flags() == 0
        lm.close()
        pb.close()
    finally:
        e.close()


def test_model_and_parse_batch_run_the_biased_beam_on_request():
    import main as MAIN
    import model as M
    case = BR.bias_case()  # (its weights and phrases: the restatement's choices change for 3 of the 6 at k = 4)
    m = M.Model()
    m.load_state_dicts(case["enc_sd"], case["dec_sd"])
    dev = m.device
    feats = [torch.from_numpy(f).to(dev) for f in case["feats"]]
    lens = torch.tensor(case["lens"])
    first = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, second_pass=False)
    pb = PhraseBias(case["phrases"], {}, V, [b / 256 for b in case["boosts"]])
    off = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, second_pass=False, bias=None, bias_weight=3.0)
    assert off.pred_text == first.pred_text and off.score == first.score  # unchanged defaults: the plain results
    kw = dict(second_pass=False, lm_weight=1.5, length_weight=1.5)
    got = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, bias=pb, **kw)
    r = _np(m.engine.beam_bias(pb, 4, 1.0, None, 1.5, 1.5))
    want = ["".join(I2W[t] for t in r["tokens"][b, :r["length"][b]]) for b in range(B)]
    assert got.pred_text == want
    assert np.array_equal(bits(np.array(got.score, np.float32)), bits(r["score"]))
    plain = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, **kw)
    assert got.pred_text != plain.pred_text, "the hotwords never changed a choice"
    with pytest.raises(ValueError):
        m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, bias=pb, mbr=0.5, **kw)

    # main.parse_batch: the same call behind the file front end (features_for and read_audio stubbed out)
    class _AB:
        int2word, word2int = I2W, W2I

    keep = MAIN.features_for, MAIN.read_audio
    MAIN.features_for, MAIN.read_audio = (lambda audios: (feats, lens)), (lambda paths: paths)
    try:
        assert MAIN.parse_batch(["a"] * B, m, _AB, bw=4) == plain.pred_text
        assert MAIN.parse_batch(["a"] * B, m, _AB, bw=4, bias=pb) == want
    finally:
        MAIN.features_for, MAIN.read_audio = keep
    pb.close()
