"""Relative-entropy pruning on the host (include/casr.h casr_lm_prune_host) against the Python
restatement tests/lm_prune_ref.py: tau, every n-gram's dH and kept flag and every float64 backoff are
EXACT (the float64 as bits); the stored f32 backoff is within 1 ulp of numpy's log10.  lmp_exp10 and
lmp_log are read through the entry itself (theta -> tau, stored value -> backoff_f64 of an unpruned
model), held bit for bit to the restatement and to their accuracy bound against numpy.  No test here
needs a GPU."""
import ctypes
import itertools

import numpy as np
import pytest

import lm_estimate_ref as E
import lm_prune_ref as PR
from casr import lib as L
from casr import ngram

THETAS6 = (1e-5, 1e-4, 1e-3)


def _u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def zipf3():
    lm = ngram.estimate(E.zipf_corpus(), 3, 120)
    yield lm
    lm.close()


@pytest.fixture(scope="module")
def zipf4():
    lm = ngram.estimate(E.zipf_corpus(), 4, 120)
    yield lm
    lm.close()


@pytest.fixture(scope="module")
def small6():
    lm = ngram.estimate(E.small_corpus(6, 300, 8, 6), 4, 6)
    yield lm
    lm.close()


@pytest.fixture(scope="module")
def hand():
    lm = ngram.NgramLM.from_ids(*PR.handmade(), {}, 136)
    yield lm
    lm.close()


def _same_as_ref(lm, theta):
    """Prune on the host and in the restatement; everything must agree.  Returns the pruned model."""
    ids, prob, back = lm._arrays
    ref = PR.prune(PR.Model(ids, prob, back, lm.vocab), theta)
    out = lm.prune(theta)
    r = out.pruned
    assert r.tau == float(ref["tau"]) and r.n_degenerate == ref["n_degenerate"]
    assert r.count_in.tolist() == [len(a) for a in ids]
    assert r.count_out.tolist() == ref["count_out"] and r.n_protected.tolist() == ref["n_protected"]
    for n in range(lm.order):
        assert [tuple(g) for g in r.all_ids[n].tolist()] == ref["keys"][n], n + 1
        d = r.delta[n]
        # the inputs' condition for a bit-exact comparison: no decision rests on a near tie
        fin = d[np.isfinite(d)]
        assert r.tau == 0.0 or not len(fin) or np.abs(fin / r.tau - 1.0).min() > 1e-9
        assert np.array_equal(_u64(d), _u64(ref["delta"][n])), n + 1
        assert np.array_equal(r.kept[n], ref["kept"][n]), n + 1
        assert np.array_equal(r.ids[n], r.all_ids[n][r.kept[n]]), n + 1
        want = ref["b64"][n][ref["kept"][n]]
        assert np.array_equal(_u64(r.backoff_f64[n]), _u64(want)), n + 1
        with np.errstate(divide="ignore"):
            stored = np.where(want > 0.0, np.log10(want), -99.0).astype(np.float32)
        assert np.abs(r.backoff[n].view(np.int32).astype(np.int64) - stored.view(np.int32)).max(initial=0) <= 1, n + 1
        # kept probabilities are the input's bits
        given = {tuple(g): p for g, p in zip(ids[n].tolist(), prob[n].view(np.uint32))}
        assert [given[tuple(g)] for g in r.ids[n].tolist()] == r.prob[n].view(np.uint32).tolist()
    return out


def _prefix_closed(r):
    """Every kept n-gram's prefix is kept (where the model as given has that prefix at all)."""
    for n in range(1, r.order):
        lower = {tuple(g) for g in r.ids[n - 1].tolist()}
        given = {tuple(g) for g in r.all_ids[n - 1].tolist()}
        assert all(tuple(g[:-1]) in lower or tuple(g[:-1]) not in given for g in r.ids[n].tolist()), n + 1


def test_zipf_model_comes_back_bit_for_bit_at_1e_7(zipf3):
    out = _same_as_ref(zipf3, 1e-7)
    r = out.pruned
    assert r.count_in.tolist() == [120, 1065, 2525] and r.count_out.tolist() == [120, 1065, 2525]
    for n in range(3):
        for got, want in zip(out._arrays, zipf3._arrays):
            assert np.array_equal(got[n].view(np.uint32), want[n].view(np.uint32))
    assert r.n_degenerate == 0
    out.close()


@pytest.mark.parametrize("theta,kept", [(1e-4, [120, 681, 412]), (1e-3, [120, 90, 20])])
def test_zipf_order_3_equals_the_restatement(zipf3, theta, kept):
    out = _same_as_ref(zipf3, theta)
    assert out.pruned.count_out.tolist() == kept and out.pruned.n_degenerate == 0
    _prefix_closed(out.pruned)
    out.close()


def test_zipf_order_4_equals_the_restatement(zipf4):
    out = _same_as_ref(zipf4, 1e-4)
    assert out.pruned.count_out.tolist() == [120, 676, 391, 127] and out.pruned.n_degenerate == 0
    assert out.pruned.n_protected[1:3].sum() > 0  # (some n-gram stays only as a prefix)
    _prefix_closed(out.pruned)
    out.close()


def test_order_1_model_is_returned_unchanged():
    lm = ngram.estimate(E.zipf_corpus(), 1, 120)
    out = _same_as_ref(lm, 1e-2)
    for got, want in zip(out._arrays, lm._arrays):
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    assert out.pruned.count_out.tolist() == [120] and np.isnan(out.pruned.delta[0]).all()
    out.close()
    lm.close()


def test_small_model_keeps_the_unigrams_only_at_1e_2(small6):
    out = _same_as_ref(small6, 1e-2)
    assert out.pruned.count_in.tolist() == [9, 49, 286, 714] and out.pruned.count_out.tolist() == [9, 0, 0, 0]
    assert out.pruned.n_degenerate == 0
    # nothing follows any word: every backoff is 1
    assert np.array_equal(out.pruned.backoff_f64[0], np.ones(9)) and not out.pruned.backoff[0].any()
    out.close()


def test_kept_sets_are_nested_and_prefix_closed_as_theta_grows(small6):
    sets = []
    for theta in THETAS6:
        out = _same_as_ref(small6, theta)
        r = out.pruned
        assert r.n_degenerate == 0
        _prefix_closed(r)
        sets.append([{tuple(g) for g in a.tolist()} for a in r.ids])
        out.close()
    for a, b in zip(sets, sets[1:]):
        assert all(x >= y for x, y in zip(a, b))
    assert sum(map(len, sets[0])) > sum(map(len, sets[1])) > sum(map(len, sets[2])) > 9


def _with_spare_id(lm):
    """The same model over a vocabulary one larger: the new ASR id has no unigram, so its column of
    NgramLM.terms is the term of <unk>."""
    V = lm.vocab
    ids, prob, back = lm._arrays
    return ngram.NgramLM.from_ids([np.where(a >= V, a + 1, a) for a in ids], prob, back, {}, V + 1)


def _mass(lm, words, ctx_oldest_first):
    """sum over the words with a unigram, <unk> (through the spare id) and </s> of 10^term after the
    context: float32 terms summed in float64."""
    c = list(ctx_oldest_first)[::-1]
    row = np.array([c + [0] * (3 - len(c))], np.int32)
    t = lm.terms(row, [len(c)])[0].astype(np.float64)
    eos = float(lm.terms(row, [len(c)], eos=0)[0, 0])
    return float(np.sum(10.0 ** t[words]) + 10.0 ** eos)


@pytest.mark.parametrize("which,theta", [("zipf3", 1e-4), ("zipf3", 1e-3), ("zipf4", 1e-4), ("small6", 1e-5),
                                         ("small6", 1e-4), ("small6", 1e-3), ("small6", 1e-2)])
def test_pruned_model_sums_to_one_after_every_context(request, which, theta):
    """The tolerance of test_lm_estimate_host.py::test_terms_sum_to_one_after_every_context: f32 storage
    of terms whose weights sum to 1."""
    src = request.getfixturevalue(which)
    out = src.prune(theta)
    V, N = src.vocab, src.order
    lm = _with_spare_id(out)
    words = [int(g[0]) for g in out._arrays[0][0].tolist() if g[0] < V] + [V]  # the spare id: <unk>
    remap = lambda g: tuple(t + 1 if t >= V else t for t in g)  # noqa: E731
    seen = [()]
    for n in range(N - 1):
        every = 1 if len(src._arrays[0][n]) < 400 else 9  # contexts of the model as given, kept or not
        seen += [remap(g) for g in src._arrays[0][n].tolist()[::every] if g[-1] != V + 1]
        seen += [remap(g) for g in out._arrays[0][n].tolist() if g[-1] != V + 1]
    known = set(seen)
    unseen = [c for c in itertools.product(words[:4], repeat=N - 1) if c not in known][:2]
    worst = max(abs(_mass(lm, words, c) - 1.0) for c in seen + unseen)
    assert worst < 1e-5, worst
    lm.close()
    out.close()


def test_handmade_edges_equal_the_restatement(hand):
    """Contexts of exactly 1, 64, 65 and 130 successors, a word without a unigram, no <unk> unigram."""
    V = hand.vocab
    ids, _, _ = hand._arrays
    sizes = {}
    for g in ids[1].tolist():
        sizes[g[0]] = sizes.get(g[0], 0) + 1
    assert [sizes[w] for w in (0, 1, 2, 3)] == [130, 65, 64, 1]
    for theta in (1e-3, 3e-2):
        out = _same_as_ref(hand, theta)
        r = out.pruned
        assert 0 < r.count_out[1] < r.count_in[1] and r.n_degenerate == 0
        assert r.count_out[0] == r.count_in[0] and V + 2 not in r.ids[0]  # <unk> is not invented
        for n, g in ((2, (5, V - 1)), (2, (V - 1, 2)), (3, (0, 3, V - 1))):
            i = r.all_ids[n - 1].tolist().index(list(g))
            assert np.isnan(r.delta[n - 1][i]) and r.kept[n - 1][i]
        # the bigram (V - 1, 2) keeps its backoff as given
        i = r.ids[1].tolist().index([V - 1, 2])
        assert r.backoff[1][i] == np.float32(-0.2)
        _prefix_closed(r)
        assert [0, 3] in r.ids[1].tolist()  # protected by the trigram that passes through
        out.close()


def test_exp10_and_log_equal_the_restatement_and_meet_their_bound():
    """lmp_log through tau = L(1 + theta); lmp_exp10 through backoff_f64 of a model nothing is removed
    from (exp10 of the stored backoff).  Bit for bit against the restatement; against numpy the
    absolute error of the log is at most 1e-12 max(1, |ln x|) and the relative error of exp10 at most
    1e-12 over [-99, 0]."""
    xs = np.concatenate([np.linspace(-99.0, 0.0, 1500), -np.logspace(-9, 1.99, 300), [-99.0, -1e-9, 0.0, -38.5]])
    xs = np.unique(xs.astype(np.float32))
    ids = [np.arange(len(xs), dtype=np.int32).reshape(-1, 1), np.zeros((0, 2), np.int32)]  # (order 2, no bigram)
    none = np.zeros(0, np.float32)
    lm = ngram.NgramLM.from_ids(ids, [np.full(len(xs), -2.0, np.float32), none], [xs, none], {}, len(xs))
    out = lm.prune(0.5)
    got = out.pruned.backoff_f64[0]
    want = np.array([PR.exp10(x) for x in xs], np.float64)
    assert np.array_equal(_u64(got), _u64(want))
    exact = 10.0 ** xs.astype(np.float64)
    assert np.abs(got / exact - 1.0).max() <= 1e-12
    assert np.array_equal(out._arrays[2][0].view(np.uint32), xs.view(np.uint32))  # (nothing removed: unchanged)
    out.close()
    lib = L.load()
    ys = np.concatenate([np.logspace(-99, 0, 400), 1.0 + np.linspace(-1e-9, 1e-9, 41), np.linspace(0.5, 2.0, 301),
                         [1e-99, 2.2250738585072014e-308, 1.7976931348623157e308, 1.0]])
    thetas = ys[ys >= 1.0] - 1.0  # what the entry can be asked: 1 + theta >= 1
    for th in thetas:
        p = ctypes.c_void_p()
        L.check(lib.casr_lm_prune_host(lm._host, ctypes.c_double(th), ctypes.byref(p)), lib=lib)
        tau = ctypes.c_double()
        L.check(lib.casr_lm_prune_info(p, None, None, None, None, ctypes.byref(tau)), lib=lib)
        lib.casr_lm_prune_destroy(p)
        assert tau.value == float(PR.log(np.float64(1.0) + np.float64(th))), th
    with np.errstate(all="ignore"):
        for y in ys:
            v = float(PR.log(y))
            assert abs(v - np.log(y)) <= 1e-12 * max(1.0, abs(np.log(y))), y
    for x in np.linspace(-99.0, 0.0, 4001):
        assert abs(float(PR.exp10(x)) / 10.0 ** x - 1.0) <= 1e-12, x
    lm.close()


def test_refusals(zipf3):
    lib = L.load()
    p = ctypes.c_void_p()
    for theta in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(L.CasrError, match="CASR_ERR_ARG"):
            zipf3.prune(theta)
    assert lib.casr_lm_prune_host(None, ctypes.c_double(1e-4), ctypes.byref(p)) != 0 and not p.value
    assert lib.casr_lm_prune_host(zipf3._host, ctypes.c_double(1e-4), None) != 0
    assert lib.casr_lm_prune_info(None, None, None, None, None, None) != 0
    assert lib.casr_lm_prune_workspace_bytes(None) == -1
    out = zipf3.prune(1e-4)
    assert zipf3.prune_workspace_bytes() > 0
    L.check(lib.casr_lm_prune_host(zipf3._host, ctypes.c_double(1e-4), ctypes.byref(p)), lib=lib)
    for n in (0, 4):
        assert lib.casr_lm_prune_arrays(p, n, None, None, None, None) != 0
        assert lib.casr_lm_prune_decisions(p, n, None, None, None) != 0
    assert lib.casr_lm_prune_timing(p, None) != 0
    lib.casr_lm_prune_destroy(p)
    lib.casr_lm_prune_destroy(None)
    out.close()


def test_arpa_round_trip_of_a_pruned_model_loads_and_scores(zipf3, tmp_path):
    out = zipf3.prune(1e-4)
    words = [str(i) for i in range(120)]
    path = str(tmp_path / "pruned.arpa")
    out.write_arpa(path, words)
    back = ngram.NgramLM(path, {w: i for i, w in enumerate(words)}, 120)
    assert [len(a) for a in back._arrays[0]] == out.pruned.count_out.tolist()
    held = E.zipf_corpus(n=32, seed=5)
    tokens = np.zeros((32, 15), np.int32)
    lens = np.array([len(s) for s in held], np.int32)
    for i, s in enumerate(held):
        tokens[i, :len(s)] = s
    a, b = out.score_ids(tokens, lens), back.score_ids(tokens, lens)
    assert np.all(np.isfinite(a)) and np.allclose(a, b, rtol=2e-6, atol=1e-5)
    assert np.all(a < 0)  # still a distribution over sentences: none is more likely than certain
    back.close()
    out.close()


def test_library_exports_the_prune_entries():
    lib = L.load()
    names = [n for n in L.EXPORTS if n.startswith("casr_lm_prune")]
    assert len(names) == 8
    for name in names:
        assert hasattr(lib, name)
