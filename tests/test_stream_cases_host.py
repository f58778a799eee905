"""The table of tests/stream_cases.py is complete: every prototype of include/casr.h that takes a
``void* stream`` is named by at least one case (tests/test_gpu_streams.py runs them on a caller's own
stream), or stands in EXEMPT with a written reason.  An entry added later without a stream case fails
here, on the host, without a GPU or a library build."""
import stream_cases as SC


def test_the_header_parser_finds_the_entries():
    text = """
    /* int casr_commented(void* stream); */
    int casr_one(casr_handle* h, const float* x,
                 int n, void* stream);
    int casr_host_only(const float* x, int n);
    int casr_two(casr_handle* h, void *stream, casr_lm_est** est);
    void casr_three(void*stream);
    """
    assert SC.stream_entries(text) == ["casr_one", "casr_two", "casr_three"]
    entries = SC.stream_entries()
    assert len(entries) == len(set(entries)) >= 36
    for name in ("casr_features", "casr_encode", "casr_beam", "casr_lm_estimate", "casr_device_flags"):
        assert name in entries


def test_every_stream_entry_has_a_case_or_a_written_exemption():
    entries = SC.stream_entries()
    covered = SC.covered()
    missing = [e for e in entries if e not in covered and e not in SC.EXEMPT]
    assert not missing, f"no stream case (tests/stream_cases.py) for: {missing}"
    for e, reason in SC.EXEMPT.items():
        assert e in entries and e not in covered, e
        assert isinstance(reason, str) and len(reason.split()) >= 5, (e, reason)
    unknown = sorted(set(covered) - set(entries))
    assert not unknown, f"cases name entries the header does not have: {unknown}"


def test_the_synchronising_entries_are_the_ones_the_header_marks():
    """sync carries the header's words as the reason; only cases of casr_lm_estimate, casr_lm_prune and
    casr_device_flags may carry it."""
    marked = {"casr_lm_estimate", "casr_lm_prune", "casr_device_flags"}
    names = [c.name for c in SC.CASES]
    assert len(names) == len(set(names))
    for c in SC.CASES:
        if c.sync:
            assert isinstance(c.sync, str) and "include/casr.h" in c.sync
            assert marked & set(c.entries), c.name
    for e in marked:
        assert any(c.sync for c in SC.CASES if e in c.entries), e
