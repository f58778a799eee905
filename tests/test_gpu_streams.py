"""Every device entry of include/casr.h on a caller's own non-blocking stream, held to the header's
stream contract (Conventions): a call's device work is ordered after everything already enqueued on
``stream``, its results are visible to everything enqueued on ``stream`` afterwards, and no entry but
casr_lm_estimate, casr_lm_prune and casr_device_flags makes the host wait.

tests/stream_cases.py has the case table and the fenced call (its docstring describes the four steps);
tests/test_stream_cases_host.py checks that the table names every entry that takes a stream.  Each test
prints one line ``[stream] <case> host_ms=.. delay_ms=.. pending_at_return=..``.

No test uses more than two caller streams at once: a handle adds up to three of its own."""
import time

import pytest
import torch

import stream_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _world():
    yield
    SC.close_world()


def _ids(group):
    return [pytest.param(c, id=c.name) for c in SC.by_group(group)]


# ---------------------------------------------------------------------------- warm handles
@pytest.mark.parametrize("case", _ids("chain"))
def test_chain_on_a_caller_stream(case):
    """The whole decode chain, with only the fbank and frame buffers fenced, in every graph mode with the
    persistent recurrence on and off, and once at f32."""
    w = SC.world()
    with SC.modes(w.engine, *case.build.modes):
        SC.fenced_call(case.name, case.build(), sync=case.sync)


@pytest.mark.parametrize("graphs", [2, 3])
def test_chains_back_to_back(graphs):
    """chain(true), chain(decoy), chain(true) enqueued on the stream with nothing in between but the copies
    that rewrite the input buffers: each result equals its own default-stream result.  A graph replayed
    on a private stream without an out-fence would still be reading the encoder state that the next
    encode overwrites."""
    w = SC.world()
    e, st = w.engine, w.stream
    wk = SC.chain_work()
    order = (wk.true, wk.decoy, wk.true)
    with SC.modes(e, graphs):
        e.device_flags()
        want, keep = [], []
        for src in (wk.true, wk.decoy):
            SC._fill(wk.bufs, src)
            out = wk.run(e)
            keep.append(out)
            want.append(SC.to_host(out))
        assert e.device_flags() == 0
        assert SC.differing(want[1], want[0])
        with torch.cuda.stream(st):
            SC._prewarm_pool(list(SC._tensors(out).values()), 6)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep.append(wk.run(e))
        t_host = time.perf_counter() - t0
        SC._fill(wk.bufs, wk.decoy)
        torch.cuda.synchronize()
        ms = SC.delay_ms(3 * t_host)
        got = []
        with torch.cuda.stream(st):
            w.delay.enqueue(ms)
            for src in order:
                SC._fill(wk.bufs, src)
                ready = torch.cuda.Event()
                ready.record(st)
                out = wk.run(e)
                pending = not ready.query()
                clones = {k: v.clone() for k, v in SC._tensors(out).items()}
                for v in SC._tensors(out).values():
                    SC.poison(v)
                keep += [out, clones]
                got.append(clones)
            SC._fill(wk.bufs, wk.decoy)
        st.synchronize()
        print(f"[stream] back-to-back-graphs{graphs} host_ms={1e3 * t_host:.3f} delay_ms={ms:.1f} "
              f"pending_at_return={pending}")
        for i, (g, ref) in enumerate(zip(got, (want[0], want[1], want[0]))):
            bad = SC.differing(SC.to_host(g), ref)
            assert not bad, (i, bad)
        with torch.cuda.stream(st):
            assert e.device_flags() == 0
        assert pending  # the third chain was enqueued while the first inputs were still not written
    del keep


@pytest.mark.parametrize("case", _ids("beam") + _ids("stateless") + _ids("frontend") + _ids("lm"))
def test_entry_on_a_caller_stream(case):
    SC.fenced_call(case.name, case.build(), sync=case.sync)


# ---------------------------------------------------------------------------- cold handles
def _cold(name, work, weights=True, precision=None):
    """The reference from the warm Engine on the default stream; a fresh Engine then makes its very first
    calls on the stream behind the delay: the guard words' zeroing, the f32 image build, graph capture,
    workspace allocation and the table upload all land in the middle of the caller's sequence."""
    w = SC.world()
    e = w.fresh_engine(weights)
    try:
        if precision:
            e.set_precision(precision)
        with SC.modes(w.engine, precision=precision or "s16x3"):
            SC.fenced_call(name, work, engine=e, cold=True)
    finally:
        torch.cuda.synchronize()
        e.close()


@pytest.mark.parametrize("precision", ["s16x3", "f32"])
def test_cold_handle_chain(precision):
    _cold(f"cold-chain-{precision}", SC.chain_work(), precision=precision)


def test_cold_handle_frontend_chain():
    _cold("cold-frontend-chain", SC.named("frontend-chain").build())


def test_seven_rates_in_flight_on_a_cold_handle():
    """Eight convert_audio calls at seven rates behind one delay on a fresh handle: the seventh rate
    evicts the first from the six-entry table cache while the first call's kernel and its table's
    upload are still queued; the eighth builds the first rate's table again."""
    _cold("seven-rates", SC.named("seven-rates").build(), weights=False)


def test_cold_handle_keeps_a_guard_bit():
    """The first call on a fresh handle clamps a length (guard bit 1): the zeroing of the guard words,
    first-use work on the null stream, must not land after the kernel that raises the bit."""
    case = SC.named("cold-edit_distance-guard-bit")
    _cold(case.name, case.build(), weights=False)


# ---------------------------------------------------------------------------- shared immutable objects
def _shared(name, call):
    """One casr_bias / casr_grammar object read by two handles on two streams at once, neither of them the
    default stream: handle 0 decodes the true batch, handle 1 the decoy batch, three rounds; each result
    equals the single-handle result of its batch."""
    from casr.pipeline import StreamPipeline
    w = SC.world()
    batches = [tuple(SC._dev(x) for x in b) for b in (w.true, w.decoy)]

    def decode(e, fb, fr):
        out = {"feat_len": e.encode_fbank(fb, fr)}
        out.update(call(w, e))
        out.update(SC.flat("records", e.beam_records()))
        return out
    w.engine.device_flags()
    want = [SC.to_host(decode(w.engine, *b)) for b in batches]
    assert w.engine.device_flags() == 0 and SC.differing(want[1], want[0])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        pipe = StreamPipeline(w.cfg, w.blob, n=2)
    try:
        assert pipe.streams[0] == side and pipe.streams[1] != torch.cuda.default_stream()
        t0 = time.perf_counter()
        got = [pipe.submit(lambda e, b=b: decode(e, *b)) for _ in range(3) for b in batches]
        t_host = time.perf_counter() - t0
        pending = not all(s.query() for s in pipe.streams)
        torch.cuda.synchronize()
        print(f"[stream] {name} host_ms={1e3 * t_host / len(got):.3f} delay_ms=0.0 pending_at_return={pending}"
              " (two handles, no delay: reported, not asserted)")
        assert pipe.device_flags() == 0
        for i, g in enumerate(got):
            bad = SC.differing(SC.to_host(g), want[i % 2])
            assert not bad, (name, i, bad)
    finally:
        torch.cuda.synchronize()
        pipe.close()


def test_one_bias_object_on_two_handles_and_streams():
    def call(w, e):
        out = SC.flat("beam", e.beam_bias(w.bias, SC.K, 1.0, w.lm, *SC.WEIGHTS))
        out["rec_bias"] = e.beam_record_bias()
        return out
    _shared("shared-bias", call)


def test_one_grammar_object_on_two_handles_and_streams():
    _shared("shared-grammar", lambda w, e: SC.flat("beam", e.beam_grammar(w.grammar, SC.K, w.lm, *SC.WEIGHTS)))
