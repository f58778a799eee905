"""The n-gram LM fused into the beam search's first pass on the device (include/casr.h casr_lm_terms,
casr_beam_lm, casr_beam_record_lm).

Term rows against the host function bit for bit; zero weights against casr_beam bit for bit (every
width class, both arithmetics, the folded step); invariants on the device's own records, where near
ties of the search play no part (a record's rec_lm is its sentence score, bit for bit; its rec_score
the teacher-forced score of its tokens; the best the first maximum of the defined expression); the
numpy restatement (tests/fusion_ref.py) at inputs whose rank gaps the CPU test checked; that the LM
changes a choice; refusals and state; the drop-in Model."""
import numpy as np
import pytest
import torch

import fusion_ref as FR
import ngram_ref as R
from golden_util import fbank_for
from casr import lib as L
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


def _lm_from_records(recs, seed):
    grams = FR.lm_grams_from_records(recs, V, seed)
    return grams, NgramLM.from_ids(*R.arrays_of(grams), W2I, V), R.RefLM(4, V, grams)


# ---------------------------------------------------------------------------- 1. term rows
def _constructed(order):
    """The CPU test's constructed cases on V = 5004: a context (7) whose successor list holds every
    unigram id, word 11 as a 2-, 3- and 4-gram under (9 8 7), <unk> and </s> as successors."""
    grams = R.random_model(order, V, 700 + order, n_high=3000)
    f = np.float32
    extra = [{(7, w): (f(-0.5 - (w % 1024) / 1024.0), f(-0.25)) for (w,) in grams[0] if w != V},
             {(8, 7, 11): (f(-0.75), f(-0.5)), (8, 7, V + 2): (f(-1.25), f(-0.5)), (8, 7, V + 1): (f(-1.75), f(0)),
              (9, 8, 7): (f(-0.375), f(-1.5))},
             {(9, 8, 7, 11): (f(-0.125), f(0)), (9, 8, 7, V + 2): (f(-2.25), f(0)), (9, 8, 7, V + 1): (f(-2.5), f(0))}]
    for n in range(2, order + 1):
        grams[n - 1].update(extra[n - 2])
        if n == order:
            grams[n - 1] = {g: (p, f(0)) for g, (p, b) in grams[n - 1].items()}
    for i in (7, 8, 9, 11):
        grams[0].setdefault((i,), (f(-3.0), f(-0.125)))
    return grams


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_device_term_rows_equal_the_host_rows(order):
    from casr.engine import Engine
    grams = _constructed(order)
    lm = NgramLM.from_ids(*R.arrays_of(grams), {}, V)
    rs = np.random.RandomState(40 + order)
    n = 300
    ctx = rs.randint(0, V + 3, size=(n, 3)).astype(np.int32)
    nc = rs.randint(0, order, size=n).astype(np.int32)
    for i in range(0, n, 2):  # the leading words of the model's own n-grams
        if order > 1:
            g = grams[rs.randint(1, order)]
            key = list(g.keys())[rs.randint(len(g))]
            lead = list(key[:-1])[::-1]
            ctx[i, :len(lead)] = lead
            nc[i] = len(lead)
    ctx[1], nc[1] = (V, 0, 0), min(1, order - 1)
    for i, c in enumerate(range(0, min(4, order))):
        ctx[3 + 2 * i], nc[3 + 2 * i] = (7, 8, 9), c
    e = Engine(CFG)  # no weights: the rows need none
    try:
        e.device_flags()
        for eos in (CFG.eos, None):
            got = e.lm_terms(lm, ctx, nc, eos).cpu().numpy()
            assert np.array_equal(bits(got), bits(lm.terms(ctx, nc, eos))), (order, eos)
        assert e.device_flags() == 0
        # a context id outside [0, V + 3): guard bit 1 and the <unk> row; an nc out of range: clamped
        bad, unk = ctx[:4].copy(), ctx[:4].copy()
        nb = np.full(4, order - 1, np.int32)
        if order > 1:
            bad[2, 0], unk[2, 0] = V + 3, V + 2
            got = e.lm_terms(lm, bad, nb, CFG.eos).cpu().numpy()
            assert e.device_flags() == 1
            assert np.array_equal(bits(got), bits(lm.terms(unk, nb, CFG.eos)))
        got = e.lm_terms(lm, ctx[:4], nb + 7, CFG.eos).cpu().numpy()
        assert e.device_flags() == 1
        assert np.array_equal(bits(got), bits(lm.terms(ctx[:4], nb, CFG.eos)))
    finally:
        e.close()
        lm.close()


# ---------------------------------------------------------------------------- 2. zero weights
def _same_as_beam(e, k, lm):
    beam = _np(e.beam(k))
    recs = [x.cpu().numpy() for x in e.beam_records()]
    z = _np(e.beam_lm(lm, k, 0.0, 0.0))
    zrecs = [x.cpu().numpy() for x in e.beam_records()]
    for n in ("tokens", "length", "steps"):
        assert np.array_equal(z[n], beam[n]), (k, n)
    assert np.array_equal(bits(z["score"]), bits(beam["score"])), k
    assert np.array_equal(zrecs[0], recs[0]) and np.array_equal(bits(zrecs[1]), bits(recs[1]))
    assert np.array_equal(zrecs[2], recs[2])
    assert recs[2].any()


@pytest.mark.parametrize("k,precision", [(2, None), (4, None), (16, None), (4, "f32")])
def test_zero_weights_reproduce_beam(k, precision):
    grams = R.random_model(4, V, 61)
    lm = NgramLM.from_ids(*R.arrays_of(grams), {}, V)
    e = _engine(25.0)
    try:
        if precision:
            e.set_precision(precision)
        _encode(e)
        _same_as_beam(e, k, lm)
        assert e.device_flags() == 0
    finally:
        e.close()
        lm.close()


def test_zero_weights_reproduce_beam_on_the_folded_step():
    """B = 128, k = 8 (R = 1,024): casr_beam runs the folded step with its select inside the attention;
    the fused beam runs the same steps with the LM select as a launch of its own."""
    grams = R.random_model(4, V, 62)
    lm = NgramLM.from_ids(*R.arrays_of(grams), {}, V)
    e = _engine(25.0)
    try:
        _encode(e, 128, 48)
        _same_as_beam(e, 8, lm)
        assert e.device_flags() == 0
    finally:
        e.close()
        lm.close()


# ---------------------------------------------------------------------------- 3, 5. invariants
def _comb(a, q, l, w=1.5, lw=1.5):
    return F(F(F(a) + F(F(w) * F(q))) + F(float(F(lw)) * float(l + 1)))


@pytest.mark.parametrize("k", [4, 16])
def test_invariants_on_the_devices_own_records(k):
    e = _engine(25.0)
    try:
        _encode(e)
        plain = _np(e.beam(k))
        recs0 = records_by_utterance(*(x.cpu().numpy() for x in e.beam_records()))
        grams, lm, ref = _lm_from_records(recs0, 500 + k)
        e.device_flags()
        r = _np(e.beam_lm(lm, k, 1.5, 1.5))
        rt, rs, rv = (x.cpu().numpy() for x in e.beam_records())
        rq = e.beam_record_lm().cpu().numpy()
        assert e.device_flags() == 0
        steps = int(r["steps"][0])
        assert rv.any() and not rv[:, steps:].any()
        # rec_lm: the record's sentence score, bit for bit; 0 elsewhere
        where = np.nonzero(rv)
        rows = np.zeros((len(where[0]), CFG.max_len), np.int32)
        lens = np.zeros(len(where[0]), np.int32)
        for i, (b, l, c) in enumerate(zip(*where)):
            assert (rt[b, l, c, :l] >= 0).all() and (rt[b, l, c, l:] == -1).all()
            rows[i, :l], lens[i] = rt[b, l, c, :l], l
        want_q = np.zeros(rv.shape, np.float32)
        want_q[where] = lm.score_ids(rows, lens)
        assert np.array_equal(bits(rq), bits(want_q))
        for i in range(0, len(lens), 7):  # ... and the reference's
            assert bits(want_q[where][i]) == bits(ref.sentence(rows[i, :lens[i]].tolist()))
        # rec_score: the teacher-forced score of the record's tokens plus eos (a sample: B rows a call)
        pick = np.linspace(0, len(lens) - 1, 3 * B).astype(int)
        for i0 in range(0, len(pick), B):
            tg = np.full((B, CFG.max_len), CFG.eos, np.int32)
            tl = np.ones(B, np.int32)
            sel = {}
            for i in pick[i0:i0 + B]:
                b = where[0][i]
                if b not in sel and lens[i] + 1 <= CFG.max_len:
                    sel[b] = i
                    tg[b, :lens[i]] = rows[i, :lens[i]]
                    tl[b] = lens[i] + 1
            total = e.score(tg, tl)["total_logp"].cpu().numpy()
            for b, i in sel.items():
                assert abs(total[b] - rs[where][i]) <= 2e-3, (b, i, total[b], rs[where][i])
        # the best: the first maximum over the returned records; without a record a live row
        differs = 0
        for b in range(B):
            got = r["tokens"][b, :r["length"][b]].tolist()
            assert (r["tokens"][b, r["length"][b]:] == -1).all()
            idx = [(l, c) for l in range(steps) for c in range(k) if rv[b, l, c]]
            if idx:
                vals = [_comb(rs[b, l, c], rq[b, l, c], l) for l, c in idx]
                l, c = idx[int(np.argmax(vals))]
                assert got == rt[b, l, c, :l].tolist(), b
                assert bits(r["score"][b]) == bits(rs[b, l, c]) and bits(r["lm"][b]) == bits(rq[b, l, c])
            else:
                assert r["length"][b] == steps and (np.array(got) >= 0).all()
                # a live row's lm: its tokens' terms without the closing </s> (bos context)
                hist, q = [V], None
                for w in got:
                    t = ref.term([ref.lm_id(x) for x in hist], ref.lm_id(w) if w != CFG.eos else ref.lm_id(V + 1))
                    q = t if q is None else F(q + t)
                    hist.append(w)
                assert bits(r["lm"][b]) == bits(q), b
            differs += got != plain["tokens"][b, :plain["length"][b]].tolist()
        assert differs >= 1, "the LM never changed a choice"
        # two runs: the same bits
        r2 = _np(e.beam_lm(lm, k, 1.5, 1.5))
        for n in r:
            assert np.array_equal(r[n].view(np.int32), r2[n].view(np.int32)), n
        assert np.array_equal(bits(e.beam_record_lm().cpu().numpy()), bits(rq))
        # a later casr_beam: what it gives without the fused call before it
        again = _np(e.beam(k))
        for n in plain:
            assert np.array_equal(again[n].view(np.int32), plain[n].view(np.int32)), n
        assert e.device_flags() == 0
        lm.close()
    finally:
        e.close()


# ---------------------------------------------------------------------------- 4. against fusion_ref
@pytest.mark.parametrize("k,precision", [(k, None) for k in FR.GPU_K] + [(FR.GPU_K[0], "f32")])
def test_fused_beam_equals_the_numpy_restatement(k, precision):
    case = FR.fusion_case()
    want = FR.fused_case(k)
    assert (want["gap"] >= 1e-2).all()  # (tests/test_fusion_ref_host.py checks it on the CPU)
    lm = NgramLM.from_ids(*R.arrays_of(case["grams"]), W2I, V)
    e = _engine(FR.EOS_BIAS)
    try:
        if precision:
            e.set_precision(precision)
        _encode(e, ids=FR.UTTS)
        r = _np(e.beam_lm(lm, k, *FR.WEIGHTS))
        rt, rs, rv = (x.cpu().numpy() for x in e.beam_records())
        assert e.device_flags() == 0
        assert int(r["steps"][0]) == want["steps"]
        recs = records_by_utterance(rt, rs, rv)
        for b in range(B):
            assert r["tokens"][b, :r["length"][b]].tolist() == want["tokens"][b], b
            assert abs(r["score"][b] - want["score"][b]) <= 2e-3 and abs(r["lm"][b] - want["lm"][b]) <= 2e-3, b
            assert [t for t, _ in recs.get(b, [])] == [t for t, _, _ in want["records"][b]], b
    finally:
        e.close()
        lm.close()


# ---------------------------------------------------------------------------- 6. refusals and state
def test_refusals_and_state():
    from casr.engine import Engine
    grams = R.random_model(3, V, 63)
    lm = NgramLM.from_ids(*R.arrays_of(grams), {}, V)
    small = NgramLM.from_ids(*R.arrays_of(R.random_model(2, 100, 3, n_high=10)), {}, 100)
    e = _engine(25.0)
    e2 = Engine(CFG)
    try:
        e.device_flags()
        dev = e.device
        out = dict(t=torch.full((B, CFG.max_len), 77, dtype=torch.int32, device=dev),
                   n=torch.full((B,), 77, dtype=torch.int32, device=dev), s=torch.full((B,), 77.0, device=dev),
                   q=torch.full((B,), 77.0, device=dev), st=torch.full((1,), 77, dtype=torch.int32, device=dev))
        ptr = lambda x: x.data_ptr()

        def call(eng, lmp, k):
            return eng.lib.casr_beam_lm(eng.handle, lmp, k, 1.5, 1.5, ptr(out["t"]), ptr(out["n"]), ptr(out["s"]),
                                        ptr(out["q"]), ptr(out["st"]), None)

        assert call(e, lm.on(e), 4) == 3  # before an encode: CASR_ERR_STATE
        assert call(e2, lm.on(e2), 4) == 3  # before weights are bound
        _encode(e)
        assert call(e, None, 4) == 1
        assert call(e, lm._host, 4) == 1  # host-only
        assert call(e, small.on(e), 4) == 1  # vocab mismatch
        assert call(e, lm.on(e), 0) == 1 and call(e, lm.on(e), 17) == 1
        assert e.lib.casr_beam_lm(e.handle, lm.on(e), 4, 1.5, 1.5, ptr(out["t"]), ptr(out["n"]), ptr(out["s"]), None,
                                  ptr(out["st"]), None) == 1
        ctx = torch.zeros(2, 3, dtype=torch.int32, device=dev)
        nc = torch.zeros(2, dtype=torch.int32, device=dev)
        rows = torch.full((2, V), 77.0, device=dev)
        for lmp in (None, lm._host, small.on(e)):
            assert e.lib.casr_lm_terms(e.handle, lmp, ptr(ctx), ptr(nc), 2, -1, ptr(rows), None) == 1
        torch.cuda.synchronize()
        assert all(bool((x == 77).all()) for x in out.values()) and bool((rows == 77).all())
        # state: record_lm needs a fused beam; rescore refuses one
        e.beam(4)
        with pytest.raises(L.CasrError, match="CASR_ERR_STATE"):
            e.beam_record_lm()
        e.beam_rescore(lm, 1.5, 1.5)
        e.beam_lm(lm, 4, 1.5, 1.5)
        e.beam_record_lm()
        with pytest.raises(L.CasrError, match="CASR_ERR_STATE"):
            e.beam_rescore(lm, 1.5, 1.5)
        e.beam(4)
        e.beam_rescore(lm, 1.5, 1.5)
        assert e.device_flags() == 0
    finally:
        e.close()
        e2.close()
        lm.close()
        small.close()


# ---------------------------------------------------------------------------- 7. the drop-in Model
class _ScoreOnly:
    def __init__(self, lm):
        self.lm = lm

    def score(self, s, bos=True):
        return self.lm.score(s, bos=bos)


def test_shard_decoder_runs_the_fused_beam_on_request():
    """BeamShardDecoder(fusion=True) returns Engine.beam_lm's result per batch (batches of 4 + 2) and
    fetches no records; fusion with a host scorer is refused."""
    from casr.distributed import BeamShardDecoder, unpack_results
    e = _engine(25.0)
    fb = torch.from_numpy(np.stack([fbank_for(b, T) for b in range(B)])).cuda()
    fr = torch.full((B,), T, dtype=torch.int32, device=fb.device)
    try:
        _encode(e)
        e.beam(4)
        recs = records_by_utterance(*(x.cpu().numpy() for x in e.beam_records()))
        grams, lm, ref = _lm_from_records(recs, 123)
        dec = BeamShardDecoder(e, 4, lm, I2W, 1.5, 1.5, max_batch=4, fusion=True)
        gt, gl, gs = unpack_results(dec.finish(dec.enqueue(fb, fr)), CFG.max_len)
        assert dec.stats["records"] == 0
        for c0, c1 in ((0, 4), (4, 6)):
            e.encode_fbank(fb[c0:c1], fr[c0:c1])
            r = _np(e.beam_lm(lm, 4, 1.5, 1.5))
            assert np.array_equal(gl[c0:c1], r["length"]) and np.array_equal(bits(gs[c0:c1]), bits(r["score"]))
            for b in range(c1 - c0):
                assert gt[c0 + b, :gl[c0 + b]].tolist() == r["tokens"][b, :r["length"][b]].tolist()
        assert e.device_flags() == 0
        with pytest.raises(TypeError):
            BeamShardDecoder(e, 4, _ScoreOnly(lm), I2W, 1.5, 1.5, fusion=True)
        lm.close()
    finally:
        e.close()


def test_model_runs_the_fused_beam_on_request():
    import model as M
    from oracle import casr_oracle as O
    m = M.Model()
    enc_sd, dec_sd = synthetic_state_dicts(CFG, peaked=True, eos_bias=25.0)
    m.load_state_dicts(enc_sd, dec_sd)
    dev = m.device
    feats = [torch.from_numpy(O.features_from_fbank(fbank_for(b, T))).to(dev) for b in range(B)]
    lens = torch.tensor([f.shape[0] for f in feats])
    first = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, second_pass=False)
    recs = records_by_utterance(*(x.cpu().numpy() for x in m.engine.beam_records()))
    grams, lm, ref = _lm_from_records(recs, 91)
    kw = dict(second_pass=True, lm_model=lm, lm_weight=1.5, length_weight=1.5)
    second = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, **kw)
    off = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, fusion=False, **kw)
    assert off.pred_text == second.pred_text and off.score == second.score
    fused = m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, fusion=True, **kw)
    r = _np(m.engine.beam_lm(lm, 4, 1.5, 1.5))
    want = ["".join(I2W[t] for t in r["tokens"][b, :r["length"][b]]) for b in range(B)]
    assert fused.pred_text == want
    assert np.array_equal(bits(np.array(fused.score, np.float32)), bits(r["score"]))
    assert fused.pred_text != first.pred_text, "the LM never changed a choice"
    with pytest.raises(TypeError):
        m.eval_one_batch_with_beam(dev, 4, feats, lens, None, I2W, fusion=True, second_pass=True,
                                   lm_model=_ScoreOnly(lm), lm_weight=1.5, length_weight=1.5)
    lm.close()
