"""The stream-order contract of include/casr.h, as a table of cases and one fenced call that runs them
(tests/test_gpu_streams.py; tests/test_stream_cases_host.py checks that the table names every entry of
the header that takes a ``void* stream``).

A case builds a ``Work``: fully sized device buffers, a true and a decoy content for each (both valid
inputs of the same shape: a misordered read gives a well-defined wrong answer, never a fault), and
``run(engine)``, which calls the entries through their Engine wrappers on the current stream and returns
{name: device tensor | numpy array | None}.

``fenced_call`` then holds the entries to the contract on a caller's own non-blocking stream:

  1. reference   true inputs, default stream, outputs to the host, guard flags as expected (the warm-up)
  2. decoy       decoy inputs, default stream: at least one output must differ (a blind case is a test
                 bug); the wall time of this warm call, ``t_host``, sizes the delay
  3. stream run  with the decoy left in the buffers and the device idle: on the stream, a delay of
                 max(50 ms, 20 t_host) (at most 500 ms), buf.copy_(true), an event ``ready``, the call,
                 ready.query(), a clone of every output, buf.copy_(decoy), a fill of the original outputs;
                 no host synchronisation in between
  4. check       the clones equal the reference bit for bit, the guard flags read on the stream are as
                 expected, and a warm call of an entry the header does not mark as host-synchronising
                 returned while ``ready`` was pending.

The true inputs exist only after the delay, so every internal launch, copy or graph replay must be
ordered after the caller's stream; the clones show the outputs to later work on the stream; the decoy
written back afterwards shows the entry's reads ordered before later work on the stream.  Every tensor
made on the way is kept alive until the final synchronise (torch's allocator would hand a block freed
on another stream to the next taker)."""
import functools
import os
import re
import time

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "casr.h")

MIN_DELAY_MS, HOST_FACTOR, MAX_DELAY_MS = 50.0, 20.0, 500.0


def stream_entries(text=None):
    """Every prototype of include/casr.h with a ``void* stream`` parameter, in header order."""
    if text is None:
        with open(HEADER, encoding="utf-8") as f:
            text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(casr_\w+)\s*\(([^;{}()]*)\)\s*;", text)
    return [name for name, args in protos if re.search(r"\bvoid\s*\*\s*stream\b", args)]


# ---------------------------------------------------------------------------- the table
class Case:
    def __init__(self, name, entries, build, sync=None, group="stateless"):
        self.name, self.entries, self.build, self.sync, self.group = name, tuple(entries), build, sync, group

    def __repr__(self):
        return self.name


CASES = []
# Entries no case of the table calls, each with the reason.  Empty: every entry has a case.
EXEMPT = {}

SYNC_ESTIMATE = "include/casr.h casr_lm_estimate: 'synchronous (it returns with the result on the host)'"
SYNC_PRUNE = "include/casr.h casr_lm_prune: 'needs no weights and no encode; synchronous'"
SYNC_FLAGS = "include/casr.h casr_device_flags: 'Synchronises `stream`' (it returns the words to the host)"


def case(name, entries, sync=None, group="stateless"):
    def add(build):
        CASES.append(Case(name, entries, build, sync, group))
        return build
    return add


def by_group(group):
    return [c for c in CASES if c.group == group]


def named(name):
    return next(c for c in CASES if c.name == name)


class Work:
    """bufs: the fenced device buffers; true, decoy: their two contents (device tensors of the same shapes,
    made on the default stream); run(engine) -> {name: output}; flags: the guard bits the TRUE input
    raises (0 but for the one case that is about a bit); keep: whatever must outlive the enqueued work."""

    def __init__(self, bufs, true, decoy, run, flags=0, keep=()):
        assert len(bufs) == len(true) == len(decoy)
        for b, t, d in zip(bufs, true, decoy):
            assert b.shape == t.shape == d.shape and b.dtype == t.dtype == d.dtype, (b.shape, t.shape, d.shape)
        self.bufs, self.true, self.decoy, self.run, self.flags, self.keep = bufs, true, decoy, run, flags, keep


def _dev(a, dtype=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def fenced(pairs, run, **kw):
    """Work from [(true array, decoy array)]: the buffers start out holding the true content."""
    true = [_dev(t) for t, _ in pairs]
    decoy = [_dev(d) for _, d in pairs]
    return Work([t.clone() for t in true], true, decoy, run, **kw)


def flat(prefix, out):
    """{prefix.name: tensor} of a dict, a tuple or one tensor."""
    if isinstance(out, dict):
        return {f"{prefix}.{k}": v for k, v in out.items()}
    if isinstance(out, (tuple, list)):
        return {f"{prefix}.{i}": v for i, v in enumerate(out)}
    return {prefix: out}


# ---------------------------------------------------------------------------- the shared world
B, T, K = 6, 101, 4             # fusion_ref.fusion_case()'s batch and the beam width of the cases
EOS_BIAS = 25.0                 # tests/test_gpu_ngram.py's: some utterances finish many hypotheses, one none
TRUE_SEED, DECOY_SEED = 0, 50   # golden_util.fbank_for ids of the two batches
WEIGHTS = (1.5, 1.5)            # lm_weight, length_weight (fusion_ref.WEIGHTS)
RATES = (8000, 12000, 22050, 24000, 32000, 44100, 48000, 8000)  # seven rates; the eighth call re-builds the first


def batch(seed, nb=B, t=T):
    """(fbank [nb, t, 80], frames [nb]): ragged valid lengths, rows past them zero."""
    from golden_util import fbank_for
    rs = np.random.RandomState(900 + seed)
    frames = rs.randint(60, t + 1, size=nb).astype(np.int32)
    frames[rs.randint(nb)] = t
    x = np.zeros((nb, t, 80), np.float32)
    for b in range(nb):
        x[b, :frames[b]] = fbank_for(seed + b, t)[:frames[b]]
    return x, frames


class World:
    """What the cases share: the packed weights, one warm Engine, the caller's stream, the delay, and the
    tiny LM, phrase set and grammars, which are built (fusion_ref's, bias_ref's and grammar_ref's
    recipes) from the records of the device's own plain beam over the true and the decoy batch."""

    def __init__(self):
        import torch
        import bias_ref as BR
        import fusion_ref as FR
        import ngram_ref as R
        from casr import lib as L
        from casr.bias import PhraseBias
        from casr.config import CasrConfig
        from casr.engine import Engine
        from casr.grammar import Grammar
        from casr.ngram import NgramLM
        from casr.results import records_by_utterance
        from casr.weights import synthetic_state_dicts
        self.cfg = cfg = CasrConfig()
        self.V, self.EOS = cfg.vocab, cfg.eos
        self.blob = torch.from_numpy(L.pack_weights(cfg, *synthetic_state_dicts(cfg, peaked=True, eos_bias=EOS_BIAS))).cuda()
        self.engine = Engine(cfg, packed=self.blob)
        self.true, self.decoy = batch(TRUE_SEED), batch(DECOY_SEED)
        e = self.engine
        recs = {}
        for fb, fr in (self.true, self.decoy):
            e.encode_fbank(_dev(fb), _dev(fr))
            e.beam(K)
            got = records_by_utterance(*(x.cpu().numpy() for x in e.beam_records()))
            for b, v in got.items():
                recs.setdefault(b, []).extend(v)
        assert e.device_flags() == 0
        self.records = recs
        self.grams = FR.lm_grams_from_records(recs, self.V, FR.LM_SEED)
        self.lm = NgramLM.from_ids(*R.arrays_of(self.grams), {}, self.V)
        ph, bo = BR.draw_phrases(recs, np.random.RandomState(BR.PHRASE_SEED))
        keep = [i for i, p in enumerate(ph) if 1 <= len(p) <= L.BIAS_MAX_LEN]
        self.phrases, self.boosts = [ph[i] for i in keep], [bo[i] / 256 for i in keep]
        self.bias = PhraseBias(self.phrases, {}, self.V, self.boosts)
        sents = sorted({tuple(int(x) for x in t) for v in recs.values() for t, _ in v if len(t)})
        assert len(sents) >= 4 and self.phrases
        self.sentences = sents
        self.grammar = Grammar.from_phrases([list(s) for s in sents], {}, self.V, self.EOS)
        half = len(sents) // 2
        self.halves = [Grammar.from_phrases([list(s) for s in part], {}, self.V, self.EOS)
                       for part in (sents[:half], sents[half:])]
        self.union, self.starts = Grammar.union(self.halves)
        self.stream = torch.cuda.Stream()
        self.delay = Delay()
        torch.cuda.synchronize()
        c = self.delay.calibration
        print(f"[stream] delay kind={c['kind']} per_ms={c['per_ms']:.1f} sleep_ms={c['sleep_ms'][0]:.3f},"
              f"{c['sleep_ms'][1]:.3f} records={sum(len(v) for v in recs.values())} phrases={len(self.phrases)} "
              f"sentences={len(sents)}")

    def fresh_engine(self, weights=True):
        from casr.engine import Engine
        return Engine(self.cfg, packed=self.blob) if weights else Engine(self.cfg)

    def close(self):
        import torch
        torch.cuda.synchronize()
        self.engine.close()
        for o in (self.lm, self.bias, self.grammar, self.union, *self.halves):
            o.close()


@functools.lru_cache(maxsize=None)
def world():
    return World()


def close_world():
    if world.cache_info().currsize:
        world().close()
        world.cache_clear()


# ---------------------------------------------------------------------------- the delay
class Delay:
    """Ordinary device work of a chosen length on the current stream: torch.cuda._sleep where its time
    follows its argument on this device (checked once with timing events), else a chain of element-wise
    passes over a large tensor.  Calibrated once; never longer than MAX_DELAY_MS."""

    def __init__(self):
        import torch
        self.kind, self.per_ms, self.x = None, None, None
        c0 = 2_000_000
        torch.cuda._sleep(c0)  # (the first launch loads the kernel)
        t1, t2 = self._time(lambda: torch.cuda._sleep(c0)), self._time(lambda: torch.cuda._sleep(2 * c0))
        if t1 > 0.05 and 1.6 < t2 / t1 < 2.4:
            self.kind, self.per_ms = "sleep", 2 * c0 / t2
        else:
            self.x = torch.ones(1 << 26, device="cuda")  # 256 MB: a pass is far longer than its launch
            self.x.mul_(1.0)
            self.kind, self.per_ms = "passes", 16 / self._time(lambda: [self.x.mul_(1.0) for _ in range(16)])
        self.calibration = dict(kind=self.kind, per_ms=self.per_ms, sleep_ms=(t1, t2))

    @staticmethod
    def _time(fn):
        import torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def enqueue(self, ms):
        import torch
        ms = min(float(ms), MAX_DELAY_MS)
        if self.kind == "sleep":
            torch.cuda._sleep(int(ms * self.per_ms))
        else:
            for _ in range(max(1, int(np.ceil(ms * self.per_ms)))):
                self.x.mul_(1.0)


def delay_ms(t_host_s):
    return min(max(MIN_DELAY_MS, HOST_FACTOR * 1e3 * t_host_s), MAX_DELAY_MS)


# ---------------------------------------------------------------------------- the fenced call
def _tensors(out):
    import torch
    return {k: v for k, v in out.items() if torch.is_tensor(v)}


def to_host(out):
    import torch
    return {k: (v.cpu().contiguous().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def same_bits(a, b):
    """Equal bit for bit: floats are compared as their bytes."""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def differing(got, want):
    assert got.keys() == want.keys(), (sorted(got), sorted(want))
    return [k for k in want if not same_bits(got[k], want[k])]


def poison(t):
    import torch
    t.fill_(165 if t.dtype in (torch.uint8, torch.bool) else -7)


def _fill(bufs, src):
    for b, s in zip(bufs, src):
        b.copy_(s)


def _prewarm_pool(like, copies):
    """Allocate and free, on the current stream, blocks of the sizes the call and the clones will ask for,
    so that torch's allocator serves them from the stream's pool and not with a first hipMalloc."""
    import torch
    tmp = [torch.empty_like(v) for _ in range(copies) for v in like]
    del tmp


def fenced_call(name, work, engine=None, sync=None, cold=False):
    """Steps 1 to 4 of the module docstring on ``world().engine``; with ``engine`` (a fresh handle: the
    cold cases) the stream run is that handle's very first call.  Returns the report line's numbers."""
    import torch
    w = world()
    ref_engine = w.engine
    run_engine = engine if engine is not None else ref_engine
    st, keep = w.stream, []
    # 1. reference (and warm-up)
    ref_engine.device_flags()
    _fill(work.bufs, work.true)
    out = work.run(ref_engine)
    keep.append(out)
    ref = to_host(out)
    assert ref_engine.device_flags() == work.flags, name
    # 2. decoy
    _fill(work.bufs, work.decoy)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = work.run(ref_engine)
    t_host = time.perf_counter() - t0
    keep.append(out)
    dec = to_host(out)
    assert ref_engine.device_flags() == 0, name
    assert differing(dec, ref), f"{name}: the decoy gives the reference's outputs, the case is blind"
    # 3. the stream run
    ms = delay_ms(t_host)
    with torch.cuda.stream(st):
        _prewarm_pool(list(_tensors(out).values()), 2)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        t_a, t_b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t_a.record(st)
        w.delay.enqueue(ms)
        t_b.record(st)
        _fill(work.bufs, work.true)
        ready = torch.cuda.Event()
        ready.record(st)
        out = work.run(run_engine)
        pending = not ready.query()
        clones = {k: v.clone() for k, v in _tensors(out).items()}
        _fill(work.bufs, work.decoy)
        for v in _tensors(out).values():
            poison(v)
    keep += [out, clones]
    # 4. check
    st.synchronize()
    got = dict(to_host(out), **to_host(clones))
    print(f"[stream] {name} host_ms={1e3 * t_host:.3f} delay_ms={ms:.1f} (ran {t_a.elapsed_time(t_b):.1f}) "
          f"pending_at_return={pending}{' (cold)' if cold else ''}{' (sync)' if sync else ''}")
    bad = differing(got, ref)
    assert not bad, f"{name}: on the caller's stream these outputs differ from the default-stream reference: {bad}"
    with torch.cuda.stream(st):
        assert run_engine.device_flags() == work.flags, name
    if not sync and not cold:
        assert pending, (f"{name}: the call returned only after the work enqueued before it had finished "
                         f"({ms:.0f} ms of delay): a host synchronisation inside an entry that promises none")
    del keep
    return dict(host_ms=1e3 * t_host, delay_ms=ms, pending=pending)


# ---------------------------------------------------------------------------- the chain
CHAIN_ENTRIES = ("casr_encode_fbank", "casr_encoder_results", "casr_greedy", "casr_beam", "casr_beam_records",
                 "casr_beam_rescore", "casr_beam_mbr", "casr_beam_mbr_distances", "casr_beam_nbest",
                 "casr_beam_confusion", "casr_score", "casr_align_path")


def run_chain(e, fb, fr):
    """encode_fbank -> encoder_results -> greedy(alignment) -> beam(4) -> beam_records -> beam_rescore ->
    beam_mbr -> beam_mbr_distances -> beam_nbest -> beam_confusion -> score -> align_path, each stage fed
    by the device tensors of the ones before (the targets of score are greedy's tokens)."""
    w = world()
    lmw, lw = WEIGHTS
    out = {}
    flen = e.encode_fbank(fb, fr)
    out["feat_len"] = flen
    out.update(flat("enc", e.encoder_results()))
    g = e.greedy(alignment=True)
    out.update(flat("greedy", g))
    out.update(flat("beam", e.beam(K, 0.0, lw)))
    out.update(flat("records", e.beam_records()))
    rs = e.beam_rescore(w.lm, lmw, lw, records=True)
    out.update(flat("rescore", rs))
    out.update(flat("mbr", e.beam_mbr(0.5, w.lm, lmw, lw, records=True)))
    out.update(flat("mbr_dist", e.beam_mbr_distances()))
    out.update(flat("nbest", e.beam_nbest(3, lm_weight=lmw, length_weight=lw, rec_lm=rs["rec_lm"])))
    out.update(flat("cn", e.beam_confusion(4, 1.0, lm_weight=lmw, length_weight=lw, rec_lm=rs["rec_lm"], units=True)))
    targets = g["tokens"].clamp(0, w.V - 1)
    sc = e.score(targets, g["out_len"], alignment=True, best=True, mean=True)
    out.update(flat("score", sc))
    out.update(flat("path", e.align_path(sc["alignment"], flen, g["out_len"])))
    out["targets"] = targets
    return out


def chain_work():
    """The chain's Work: the only fenced inputs are the fbank and frame buffers."""
    w = world()
    wk = fenced(list(zip(w.true, w.decoy)), None)
    wk.run = lambda e: run_chain(e, *wk.bufs)
    return wk


def _chain_case(graphs, persistent, precision):
    def build():
        return chain_work()
    build.modes = (graphs, persistent, precision)
    return build


for _g in (0, 1, 2, 3):
    for _p in (1, 0):
        CASES.append(Case(f"chain-graphs{_g}-persistent{_p}-s16x3", CHAIN_ENTRIES, _chain_case(_g, _p, "s16x3"),
                          group="chain"))
CASES.append(Case("chain-graphs2-persistent1-f32", CHAIN_ENTRIES, _chain_case(2, 1, "f32"), group="chain"))


class modes:
    """set_graphs / set_persistent / set_precision on an engine for a with-block, the defaults after it."""

    def __init__(self, e, graphs=2, persistent=1, precision="s16x3"):
        self.e, self.m = e, (graphs, persistent, precision)

    def __enter__(self):
        self.e.set_graphs(int(self.m[0]))
        self.e.set_persistent(bool(self.m[1]))
        self.e.set_precision(self.m[2])

    def __exit__(self, *exc):
        self.e.set_graphs(2)
        self.e.set_persistent(True)
        self.e.set_precision("s16x3")


# ---------------------------------------------------------------------------- the fused beams
def _beam_case(name, entries, call):
    @case(name, ("casr_encode_fbank", "casr_beam_records") + entries, group="beam")
    def build():
        w = world()
        pick_t, pick_d = [0, 1, 0, 1, 1, 0], [1, 1, 0, 0, 1, 0]
        pairs = list(zip(w.true, w.decoy))
        pairs.append((np.array([w.starts[p] for p in pick_t], np.int32), np.array([w.starts[p] for p in pick_d], np.int32)))
        wk = fenced(pairs, None)

        def run(e):
            fb, fr, start = wk.bufs
            out = {"feat_len": e.encode_fbank(fb, fr)}
            out.update(call(w, e, start))
            out.update(flat("records", e.beam_records()))
            return out
        wk.run = run
        return wk
    return build


def _lm_beam(w, e, start):
    out = flat("beam", e.beam_lm(w.lm, K, *WEIGHTS))
    out["rec_lm"] = e.beam_record_lm()
    return out


def _bias_beam(with_lm):
    def call(w, e, start):
        lm = (w.lm, *WEIGHTS) if with_lm else (None, 0.0, WEIGHTS[1])
        out = flat("beam", e.beam_bias(w.bias, K, 1.0, *lm))
        out["rec_bias"] = e.beam_record_bias()
        if with_lm:
            out["rec_lm"] = e.beam_record_lm()
        return out
    return call


def _grammar_beam(with_lm, with_start):
    def call(w, e, start):
        lm = (w.lm, *WEIGHTS) if with_lm else (None, 0.0, 0.0)
        if with_start:
            return flat("beam", e.beam_grammar(w.union, K, *lm, start=start))
        return flat("beam", e.beam_grammar(w.grammar, K, *lm))
    return call


_beam_case("beam_lm", ("casr_beam_lm", "casr_beam_record_lm"), _lm_beam)
_beam_case("beam_bias", ("casr_beam_bias", "casr_beam_record_bias"), _bias_beam(False))
_beam_case("beam_bias-lm", ("casr_beam_bias", "casr_beam_record_bias", "casr_beam_record_lm"), _bias_beam(True))
_beam_case("beam_grammar", ("casr_beam_grammar",), _grammar_beam(False, False))
_beam_case("beam_grammar-lm", ("casr_beam_grammar",), _grammar_beam(True, False))
_beam_case("beam_grammar-start", ("casr_beam_grammar",), _grammar_beam(False, True))
_beam_case("beam_grammar-lm-start", ("casr_beam_grammar",), _grammar_beam(True, True))


# ---------------------------------------------------------------------------- the stateless entries
def _sentences(seed, n=64, L=24):
    import ngram_ref as R
    w = world()
    tokens, lens = R.sentences_from(w.grams, w.V, n, L, seed, lengths=(0, 1, 2, 3, L))
    return np.asarray(tokens, np.int32), np.asarray(lens, np.int32)


@case("lm_score", ("casr_lm_score",))
def _():
    w = world()
    (tt, tl), (dt, dl) = _sentences(31), _sentences(32)
    wk = fenced([(tt, dt), (tl, dl)], None)
    wk.run = lambda e: {"q": e.lm_score(w.lm, *wk.bufs)}
    return wk


@case("lm_terms", ("casr_lm_terms",))
def _():
    w = world()

    def rows(seed, n=24):
        rs = np.random.RandomState(seed)
        ctx = rs.randint(0, w.V + 3, size=(n, 3)).astype(np.int32)
        nc = rs.randint(0, 4, size=n).astype(np.int32)
        grams = [list(g.keys()) for g in w.grams[1:]]
        for i in range(0, n, 2):  # the leading words of the model's own n-grams
            g = grams[rs.randint(len(grams))]
            lead = list(g[rs.randint(len(g))][:-1])[::-1]
            ctx[i, :len(lead)], nc[i] = lead, len(lead)
        return ctx, nc
    (tc, tn), (dc, dn) = rows(41), rows(42)
    wk = fenced([(tc, dc), (tn, dn)], None)
    wk.run = lambda e: {"terms": e.lm_terms(w.lm, *wk.bufs, w.EOS)}
    return wk


def _phrase_rows(seed, n=64, L=24):
    """Rows over the phrases' own tokens with phrases planted, so deep automaton states occur."""
    w = world()
    rs = np.random.RandomState(seed)
    alphabet = np.array(sorted({t for p in w.phrases for t in p}), np.int32)
    tok = alphabet[rs.randint(len(alphabet), size=(n, L))]
    lens = rs.randint(0, L + 1, size=n).astype(np.int32)
    lens[:2] = (0, L)
    for i in range(0, n, 2):
        p = w.phrases[rs.randint(len(w.phrases))]
        at = rs.randint(0, L - 1)
        tok[i, at:at + len(p)] = p[:L - at]
    return np.ascontiguousarray(tok, np.int32), lens


@case("bias_score", ("casr_bias_score",))
def _():
    w = world()
    (tt, tl), (dt, dl) = _phrase_rows(51), _phrase_rows(52)
    wk = fenced([(tt, dt), (tl, dl)], None)
    wk.run = lambda e: flat("bias", e.bias_score(w.bias, *wk.bufs))
    return wk


@case("bias_rows", ("casr_bias_rows",))
def _():
    w = world()
    ts, ds = (w.bias.score_ids(*_phrase_rows(s))[2].astype(np.int32) for s in (53, 54))
    assert len(set(ts.tolist())) > 4 and not np.array_equal(ts, ds)
    wk = fenced([(ts, ds)], None)
    wk.run = lambda e: flat("rows", e.bias_rows(w.bias, wk.bufs[0], next=True))
    return wk


def _walks(seed, n=64, L=24):
    """Sentences of the grammar, some cut short or continued with a token that has no arc."""
    w = world()
    rs = np.random.RandomState(seed)
    tok = np.zeros((n, L), np.int32)
    lens = np.zeros(n, np.int32)
    for i in range(n):
        s = list(w.sentences[rs.randint(len(w.sentences))])[:L]
        if rs.rand() < 0.3:
            s = (s + [7, 9, 11])[:L]
        elif rs.rand() < 0.3:
            s = s[:rs.randint(len(s) + 1)]
        tok[i, :len(s)], lens[i] = s, len(s)
    return tok, lens


@case("grammar_accept", ("casr_grammar_accept",))
def _():
    w = world()
    (tt, tl), (dt, dl) = _walks(61), _walks(62)
    wk = fenced([(tt, dt), (tl, dl)], None)
    wk.run = lambda e: flat("walk", e.grammar_accept(w.grammar, *wk.bufs))
    return wk


@case("grammar_rows", ("casr_grammar_rows",))
def _():
    w = world()

    def rows(seed, n=48):
        rs = np.random.RandomState(seed)
        return (rs.randint(0, w.grammar.n_states, size=n).astype(np.int32),
                rs.choice([-1, 0, 1, 5, 10 ** 6], size=n).astype(np.int32))
    (ts, tb), (ds, db) = rows(63), rows(64)
    wk = fenced([(ts, ds), (tb, db)], None)
    wk.run = lambda e: {"mask": e.grammar_rows(w.grammar, *wk.bufs)}
    return wk


def _edit_pairs(seed):
    import edit_ref as ER
    return ER.pad_pairs(ER.seeded_pairs(8, seed, max_len=20), 20, 24)  # tests/test_gpu_edit.py's clamp case sizes


@case("edit_distance", ("casr_edit_distance",))
def _():
    wk = fenced(list(zip(_edit_pairs(77), _edit_pairs(78))), None)
    wk.run = lambda e: flat("edit", e.edit_distance(*wk.bufs, ops=True))
    return wk


@case("edit_align", ("casr_edit_align",))
def _():
    import edit_ref as ER
    # rows of up to 200 symbols: more than one 128 x 64 tile each way
    args = [ER.pad_pairs(ER.seeded_pairs(6, s, max_len=200), 200, 200) for s in (81, 82)]
    wk = fenced(list(zip(*args)), None)
    wk.run = lambda e: flat("align", e.edit_align(*wk.bufs, ops=True, maps=True))
    return wk


@case("confusion", ("casr_confusion",))
def _():
    import confusion_ref as CR
    args = [CR.seeded_cases(12, s) for s in (2024, 2025)]
    wk = fenced(list(zip(*args)), None)
    wk.run = lambda e: flat("cn", e.confusion(*wk.bufs, CR.V, 4))
    return wk


SEG_T, SEG_SMAX = 2500, 64  # 1.2 tiles of the decision kernel's 2,048 frames, 9.8 of the level kernel's 256


@case("segment-gather_segments", ("casr_segment", "casr_gather_segments"))
def _():
    import torch
    import segment_ref as SR
    from casr.segment import SegmentParams
    p = SegmentParams(**{k: getattr(SR.SMALL, k) for k in SR.SMALL.__dataclass_fields__})

    def rec(seed, ns):
        fb = np.zeros((len(ns), SEG_T, 80), np.float32)
        for b, n in enumerate(ns):
            if n:
                fb[b, :n] = SR.fbank_from_levels(SR.random_levels(n, 10 * seed + b), 10 * seed + b)
        return fb, np.array(ns, np.int32)
    true, decoy = rec(3, (SEG_T, int(0.6 * SEG_T) | 1, 1, 0)), rec(4, (int(0.8 * SEG_T), SEG_T, 0, 7))
    wk = fenced(list(zip(true, decoy)), None)
    nb = len(true[1])
    src = torch.arange(nb, dtype=torch.int32, device="cuda").repeat_interleave(SEG_SMAX).contiguous()

    def run(e):
        fb, fr = wk.bufs
        start, length, n_seg, thr = e.segment(fb, fr, p, SEG_SMAX)
        # entries past a row's count are -1: an empty segment at frame 0 for the gather (no host read)
        s, n = start.clamp(min=0).reshape(-1), length.clamp(min=0).reshape(-1)
        out, frames_out = e.gather_segments(fb, src, s, n, t_seg=p.max_frames)
        return dict(start=start, length=length, n_seg=n_seg, thr=thr, seg=out, seg_frames=frames_out)
    wk.run = run
    wk.keep = (src,)
    return wk


@case("gather", ("casr_gather_utterances",))
def _():
    w = world()
    rows = (17, 33, 5)

    def utts(seed):
        rs = np.random.RandomState(seed)
        return [rs.standard_normal((t, w.cfg.feat_dim)).astype(np.float32) for t in rows]
    pairs = list(zip(utts(91), utts(92))) + [(np.array([17, 20, 5], np.int32), np.array([9, 33, 1], np.int32))]
    wk = fenced(pairs, None)
    wk.run = lambda e: flat("gather", e.gather(list(wk.bufs[:3]), wk.bufs[3], Tp=max(rows)))
    return wk


@case("features", ("casr_features",))
def _():
    w = world()
    wk = fenced(list(zip(w.true, w.decoy)), None)
    wk.run = lambda e: flat("features", e.features(*wk.bufs))
    return wk


@case("encode", ("casr_encode", "casr_encoder_results"))
def _():
    w = world()
    feats = [tuple(x.cpu().numpy() for x in w.engine.features(_dev(fb), _dev(fr))) for fb, fr in (w.true, w.decoy)]
    wk = fenced(list(zip(*feats)), None)

    def run(e):
        e.encode(*wk.bufs)
        return flat("enc", e.encoder_results())
    wk.run = run
    return wk


# ---------------------------------------------------------------------------- the front end
FE_B, FE_N, FE_RATE, FE_CH = 3, 24000, 48000, 2  # half a second of 48 kHz stereo: 8,000 samples, 47 frames


def _pcm(seed, n_max=FE_N, ch=FE_CH, nb=FE_B):
    from golden_util import synth_wav
    rs = np.random.RandomState(seed)
    n_in = rs.randint(n_max // 2, n_max + 1, size=nb).astype(np.int32)
    n_in[rs.randint(nb)] = n_max
    pcm = np.zeros((nb, n_max, ch), np.float32)
    for b in range(nb):
        for c in range(ch):
            pcm[b, :n_in[b], c] = (0.5 + 0.25 * c) * synth_wav(n_max, 10 * seed + 3 * b + c)[:n_in[b]]
    return pcm, n_in


def run_frontend(e, pcm, n_in):
    """convert_audio (quantise and normalise on) -> log_mel -> encode_fbank -> greedy: wav and n_out go
    straight into log_mel, as include/casr.h promises."""
    wav, n_out, gain = e.convert_audio(pcm, n_in, FE_RATE, FE_CH, quantize=True, norm_db=-1.0)
    fbank, frames = e.log_mel(wav, n_out)
    out = dict(wav=wav, n_out=n_out, gain=gain, fbank=fbank, frames=frames, feat_len=e.encode_fbank(fbank, frames))
    out.update(flat("greedy", e.greedy()))
    return out


@case("frontend-chain", ("casr_convert_audio", "casr_log_mel", "casr_encode_fbank", "casr_greedy"), group="frontend")
def _():
    wk = fenced(list(zip(_pcm(5), _pcm(6))), None)
    wk.run = lambda e: run_frontend(e, *wk.bufs)
    return wk


@case("seven-rates", ("casr_convert_audio",), group="rates")
def _():
    wk = fenced(list(zip(_pcm(7, 6000, 1), _pcm(8, 6000, 1))), None)

    def run(e):
        out = {}
        for i, rate in enumerate(RATES):
            out.update(flat(f"call{i}-{rate}", e.convert_audio(*wk.bufs, rate, 1, quantize=False, norm_db=-3.0)))
        return out
    wk.run = run
    return wk


# ---------------------------------------------------------------------------- cold handles and the rest
@case("cold-edit_distance-guard-bit", ("casr_edit_distance", "casr_device_flags"), sync=SYNC_FLAGS, group="cold")
def _():
    a, al, b, bl = _edit_pairs(77)
    al, bl = al.copy(), bl.copy()
    al[2], bl[5] = -1, 25  # tests/test_gpu_edit.py test_lengths_out_of_range_are_clamped_and_flagged: bit 1
    wk = fenced(list(zip((a, al, b, bl), _edit_pairs(78))), None, flags=1)
    wk.run = lambda e: flat("edit", e.edit_distance(*wk.bufs, ops=True))
    return wk


EST_V, EST_ORDER, PRUNE_THETA = 120, 3, 1e-3


@case("lm_estimate-lm_prune", ("casr_lm_estimate", "casr_lm_prune"), sync=SYNC_ESTIMATE + "; " + SYNC_PRUNE, group="lm")
def _():
    import lm_estimate_ref as E
    from casr import ngram
    w = world()
    tok, off = ngram.flatten(E.zipf_corpus(V=EST_V, n=203, seed=9), w.V)
    rs = np.random.RandomState(10)
    dtok = tok[rs.permutation(len(tok))]
    doff = np.concatenate([[0], np.sort(rs.randint(0, len(tok) + 1, size=len(off) - 2)), [len(tok)]]).astype(np.int64)
    wk = fenced([(tok, dtok), (off, doff)], None)

    def run(e):
        est = e.lm_estimate(*wk.bufs, EST_ORDER).sorted()
        lm = ngram.NgramLM.from_ids(est.ids, est.prob, est.backoff, {}, w.V)
        try:
            pr = e.lm_prune(lm, PRUNE_THETA).sorted()
        finally:
            lm.close()
        out = {}
        for n in range(EST_ORDER):
            for what, arr in (("est.ids", est.ids), ("est.p", est.p), ("est.gamma", est.gamma), ("est.prob", est.prob),
                              ("est.backoff", est.backoff), ("pruned.ids", pr.ids), ("pruned.prob", pr.prob),
                              ("pruned.backoff", pr.backoff), ("pruned.backoff_f64", pr.backoff_f64),
                              ("pruned.delta", pr.delta), ("pruned.kept", pr.kept)):
                out[f"{what}.{n + 1}"] = arr[n]
        return out
    wk.run = run
    return wk


SHARED_ENTRIES = {"shared-bias": ("casr_beam_bias", "casr_beam_record_bias", "casr_beam_records", "casr_encode_fbank"),
                  "shared-grammar": ("casr_beam_grammar", "casr_beam_records", "casr_encode_fbank")}
for _n, _e in SHARED_ENTRIES.items():
    CASES.append(Case(_n, _e, None, group="shared"))


def covered():
    """{entry: [case names]} over the table."""
    out = {}
    for c in CASES:
        for e in c.entries:
            out.setdefault(e, []).append(c.name)
    return out
