"""Backoff n-gram language model (ARPA, the text format KenLM reads) behind the casr C ABI.

``read_arpa`` parses the file; ``NgramLM`` maps its words to LM ids (0 .. V - 1 the ASR token ids,
V = <s>, V + 1 = </s>, V + 2 = <unk>), builds a host-only ``casr_lm`` and scores sentences through
``casr_lm_score_host`` (no GPU needed), with the duck-typed ``score(sentence, bos=True)`` the
second pass calls (casr.results.second_pass_arrays).  ``on(engine)`` gives the device copy that
``Engine.lm_score`` and ``Engine.beam_rescore`` take.  The query is defined in include/casr.h: the
textbook ARPA backoff query.  It should agree with KenLM to float rounding; KenLM is not available
here, so that statement is not pinned by any test.

``estimate`` builds a model from sentences (casr_lm_estimate*) and ``NgramLM.prune`` makes any model
smaller by relative-entropy pruning (casr_lm_prune*); both run on an Engine's device or, without one,
through their host entries, with the same bits either way.
"""
import ctypes
import os
import re

import numpy as np

from . import lib as _lib

BOS, EOS, UNK = "<s>", "</s>", "<unk>"
MAX_ORDER = 4


def read_arpa(path):
    """Sections of an ARPA file: a list over the orders n = 1, 2, .. of (ngrams, prob, backoff) with
    ngrams a list of n-tuples of words, prob and backoff float32 arrays (np.float32(float(text));
    backoff 0 where the line gives none).  Fields are separated by tabs or spaces.  A count that
    disagrees with ``\\data\\``, a malformed line or a non-finite value is a ValueError naming the line."""
    counts, sections = {}, []
    state, cur_n, words, prob, back = "head", 0, None, None, None

    def close(no):
        if cur_n and len(words) != counts[cur_n]:
            raise ValueError(f"{path}:{no}: \\{cur_n}-grams: has {len(words)} n-grams, \\data\\ says {counts[cur_n]}")
        if cur_n:
            sections.append((words, np.array(prob, np.float32), np.array(back, np.float32)))

    no = 0
    with open(path, "r", encoding="utf-8") as f:
        for no, line in enumerate(f, 1):
            line = line.strip()
            if not line:
                continue
            if state == "head":
                if line == "\\data\\":
                    state = "data"
                continue  # (text before \data\ is a comment)
            if state == "end":
                raise ValueError(f"{path}:{no}: text after \\end\\")
            m = re.fullmatch(r"\\(\d+)-grams:", line)
            if m or line == "\\end\\":
                close(no)
                if m:
                    n = int(m.group(1))
                    if n != cur_n + 1 or n not in counts:
                        raise ValueError(f"{path}:{no}: section {line} out of order or not in \\data\\")
                    state, cur_n, words, prob, back = "grams", n, [], [], []
                else:
                    if cur_n != len(counts):
                        raise ValueError(f"{path}:{no}: \\end\\ after {cur_n} of {len(counts)} sections")
                    state, cur_n = "end", 0
                continue
            if state == "data":
                m = re.fullmatch(r"ngram\s+(\d+)\s*=\s*(\d+)", line)
                if not m or int(m.group(1)) != len(counts) + 1:
                    raise ValueError(f"{path}:{no}: expected 'ngram {len(counts) + 1}=<count>', got {line!r}")
                counts[len(counts) + 1] = int(m.group(2))
                continue
            fields = line.split()
            if len(fields) not in (cur_n + 1, cur_n + 2):
                raise ValueError(f"{path}:{no}: a {cur_n}-gram line has {cur_n + 1} or {cur_n + 2} fields, got {line!r}")
            try:
                p = np.float32(float(fields[0]))
                b = np.float32(float(fields[cur_n + 1])) if len(fields) == cur_n + 2 else np.float32(0.0)
            except ValueError:
                raise ValueError(f"{path}:{no}: not a number in {line!r}") from None
            if not (np.isfinite(p) and np.isfinite(b)):
                raise ValueError(f"{path}:{no}: non-finite value in {line!r}")
            words.append(tuple(fields[1:cur_n + 1]))
            prob.append(p)
            back.append(b)
    if state != "end":
        raise ValueError(f"{path}:{no}: no \\end\\ (stopped in state {state!r})")
    if not sections:
        raise ValueError(f"{path}: no n-gram sections")
    return sections


def _ptr_array(arrays, ctype):
    """A C array of pointers to the given numpy arrays (None: NULL)."""
    out = (ctypes.c_void_p * len(arrays))()
    for i, a in enumerate(arrays):
        out[i] = None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    return out


class NgramLM:
    """NgramLM(path_or_sections, word2int, vocab): ``path_or_sections`` an ARPA file or read_arpa's
    result; ``word2int`` the ASR vocabulary (word -> id in [0, vocab)).  <s>, </s> and <unk> map to
    the ids vocab, vocab + 1 and vocab + 2; an n-gram with any other word outside the ASR vocabulary
    is dropped (no hypothesis can contain it).  Orders 1..4."""

    def __init__(self, path_or_sections, word2int, vocab):
        sections = read_arpa(path_or_sections) if isinstance(path_or_sections, (str, os.PathLike)) \
            else path_or_sections
        self.vocab = V = int(vocab)
        self.word2int = word2int
        special = {BOS: V, EOS: V + 1, UNK: V + 2}
        ids, prob, back = [], [], []
        for n, (grams, p, b) in enumerate(sections, 1):
            rows = np.full((len(grams), n), -1, np.int32)
            for i, g in enumerate(grams):
                for e, w in enumerate(g):
                    t = special.get(w)
                    if t is None:
                        t = word2int.get(w, -1)
                        t = t if 0 <= t < V else -1
                    rows[i, e] = t
            keep = (rows >= 0).all(axis=1)
            ids.append(np.ascontiguousarray(rows[keep]))
            prob.append(np.ascontiguousarray(np.asarray(p, np.float32)[keep]))
            back.append(np.ascontiguousarray(np.asarray(b, np.float32)[keep]))
        self._init_arrays(ids, prob, back)

    @classmethod
    def from_ids(cls, ids, prob, backoff, word2int, vocab):
        """From LM-id arrays directly: per order n, ids[n-1] int32 [count, n], prob[n-1] and
        backoff[n-1] float32 [count] (casr_lm_create's arguments)."""
        self = cls.__new__(cls)
        self.vocab, self.word2int = int(vocab), word2int
        self._init_arrays([np.ascontiguousarray(a, np.int32).reshape(-1, n) for n, a in enumerate(ids, 1)],
                          [np.ascontiguousarray(a, np.float32) for a in prob],
                          [np.ascontiguousarray(a, np.float32) for a in backoff])
        return self

    def _init_arrays(self, ids, prob, back):
        self.order = len(ids)
        self._arrays = (ids, prob, back)
        self._lib = _lib.load()
        self._host = self._create(self._lib, -1)
        self._device = {}  # (library, device index) -> casr_lm*

    def _create(self, lib, device):
        ids, prob, back = self._arrays
        count = np.array([len(a) for a in ids], np.int64)
        out = ctypes.c_void_p()
        rc = lib.casr_lm_create(int(device), self.order, self.vocab, count.ctypes.data_as(ctypes.c_void_p),
                                _ptr_array(ids, ctypes.c_int32), _ptr_array(prob, ctypes.c_float),
                                _ptr_array(back, ctypes.c_float), ctypes.byref(out))
        _lib.check(rc, lib=lib)
        return out

    def close(self):
        if getattr(self, "_host", None):
            self._lib.casr_lm_destroy(self._host)
            self._host = None
        for (lib, _), p in list(getattr(self, "_device", {}).items()):
            lib.casr_lm_destroy(p)
        self._device = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def on(self, engine):
        """The device object for an Engine's device (uploaded once per device and library, shared by
        every Engine there)."""
        key = (engine.lib, engine.device.index)
        if key not in self._device:
            self._device[key] = self._create(engine.lib, engine.device.index)
        return self._device[key]

    # ------------------------------------------------------------------ host scoring
    def score_ids(self, tokens, lens, bos=True):
        """Sentence scores float32 [n] of LM-id rows tokens [n, L] with lens [n], on the host."""
        tokens = np.ascontiguousarray(tokens, np.int32)
        lens = np.ascontiguousarray(lens, np.int32)
        n, L = tokens.shape
        q = np.empty(n, np.float32)
        rc = self._lib.casr_lm_score_host(self._host, tokens.ctypes.data_as(ctypes.c_void_p),
                                          lens.ctypes.data_as(ctypes.c_void_p), n, L, int(bool(bos)),
                                          q.ctypes.data_as(ctypes.c_void_p))
        _lib.check(rc, lib=self._lib)
        return q

    def terms(self, ctx, nc, eos=None):
        """Term rows float32 [n, V] on the host (casr_lm_terms_host): row i holds the term of every ASR
        token after the context ctx[i] ([n, 3] LM ids, nearest predecessor first, the first nc[i] of
        them read); token ``eos`` scores </s>."""
        ctx = np.ascontiguousarray(ctx, np.int32)
        nc = np.ascontiguousarray(nc, np.int32)
        if ctx.ndim != 2 or ctx.shape[1] != 3 or nc.shape != (ctx.shape[0],):
            raise ValueError("terms: ctx must be [n, 3] and nc [n]")
        out = np.empty((ctx.shape[0], self.vocab), np.float32)
        rc = self._lib.casr_lm_terms_host(self._host, ctx.ctypes.data_as(ctypes.c_void_p),
                                          nc.ctypes.data_as(ctypes.c_void_p), ctx.shape[0],
                                          -1 if eos is None else int(eos), out.ctypes.data_as(ctypes.c_void_p))
        _lib.check(rc, lib=self._lib)
        return out

    def ids_of(self, sentence):
        """LM ids of a sentence's whitespace-separated words: the ASR id, or <unk> for a word outside
        the ASR vocabulary.  (An ASR id the model has no unigram for scores as <unk> too, in the
        table.)"""
        V, w2i = self.vocab, self.word2int
        out = []
        for w in sentence.split():
            t = w2i.get(w, -1)
            out.append(t if 0 <= t < V else V + 2)
        return out

    def score(self, sentence, bos=True):
        """log10 probability of the sentence with its closing </s>: the call the host second pass
        makes (lm_model.score(s, bos=True), model.py:755)."""
        ids = self.ids_of(sentence)
        row = np.array([ids + [0] * (1 - min(len(ids), 1))], np.int32)
        return float(self.score_ids(row, [len(ids)], bos)[0])

    def write_arpa(self, path, int2word):
        """The model as an ARPA file: per order the n-grams in ascending key order (ascending id
        tuples), values with 7 significant digits (``%.7g``), no backoff column at the top order.
        ``int2word``: the word of every ASR id (a list or a dict); <s>, </s> and <unk> are written
        as such.  Reading the file back gives the same n-grams in the same order and, for every
        value x, np.float32(float('%.7g' % x)): within 5e-7 |x| of x (the 7th digit) plus one float32
        rounding; 0 and -99 come back exactly."""
        ids, prob, back = self._arrays
        V = self.vocab
        special = {V: BOS, V + 1: EOS, V + 2: UNK}
        with open(path, "w", encoding="utf-8") as f:
            f.write("\\data\\\n")
            for n, a in enumerate(ids, 1):
                f.write(f"ngram {n}={len(a)}\n")
            for n, (a, p, b) in enumerate(zip(ids, prob, back), 1):
                f.write(f"\n\\{n}-grams:\n")
                rows = a.tolist()
                for i in np.lexsort(a.T[::-1]).tolist():
                    words = " ".join(special[t] if t >= V else int2word[t] for t in rows[i])
                    line = "%.7g\t%s" % (float(p[i]), words)
                    if n < self.order:
                        line += "\t%.7g" % float(b[i])
                    f.write(line + "\n")
            f.write("\n\\end\\\n")

    def prune(self, theta, engine=None):
        """The model after relative-entropy pruning at threshold ``theta`` (casr_lm_prune; include/casr.h
        has the definition): on ``engine``'s device, or without one through the host entry, with the
        same bits either way.  The result is an NgramLM of the kept n-grams with renewed backoffs (the
        model itself, bit for bit, where nothing was removable); it carries ``.pruned``, the LmPruned
        with the counts, tau and every n-gram's decision."""
        if engine is None:
            out = ctypes.c_void_p()
            rc = self._lib.casr_lm_prune_host(self._host, ctypes.c_double(theta), ctypes.byref(out))
            _lib.check(rc, lib=self._lib)
            res = LmPruned(self._lib, out, self.order)
        else:
            res = engine.lm_prune(self, theta).sorted()
        lm = NgramLM.from_ids(res.ids, res.prob, res.backoff, self.word2int, self.vocab)
        lm.pruned = res
        return lm

    def prune_workspace_bytes(self):
        """casr_lm_prune_workspace_bytes: the device entry's workspace for this model."""
        return int(self._lib.casr_lm_prune_workspace_bytes(self._host))


class LmPruned:
    """What casr_lm_prune_host / casr_lm_prune returned, as numpy arrays: per order n the kept n-grams
    ids[n-1] int32 [count_out, n], prob and backoff float32 (the stored model), backoff_f64 (B'); every
    input n-gram's decision all_ids[n-1] [count_in, n], delta float64 (NaN: takes no part) and kept
    bool; ``count_in``, ``count_out``, ``n_protected`` [order], ``n_degenerate``, ``tau`` and
    ``timing_ms`` (the device entry's stages: linearise, decide, renew, compact, copy, -, -, all)."""

    def __init__(self, lib, ptr, order):
        try:
            cin, cout, prot = (np.zeros(4, np.int64) for _ in range(3))
            deg, tau = ctypes.c_int64(), ctypes.c_double()
            p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
            _lib.check(lib.casr_lm_prune_info(ptr, p(cin), p(cout), p(prot), ctypes.byref(deg), ctypes.byref(tau)),
                       lib=lib)
            self.order = int(order)
            self.count_in, self.count_out = cin[:self.order].copy(), cout[:self.order].copy()
            self.n_protected, self.n_degenerate, self.tau = prot[:self.order].copy(), deg.value, tau.value
            self.ids, self.prob, self.backoff, self.backoff_f64 = [], [], [], []
            self.all_ids, self.delta, self.kept = [], [], []
            for n in range(1, self.order + 1):
                c, ci = int(cout[n - 1]), int(cin[n - 1])
                ids, prob, back = np.zeros((c, n), np.int32), np.zeros(c, np.float32), np.zeros(c, np.float32)
                b64 = np.zeros(c, np.float64)
                _lib.check(lib.casr_lm_prune_arrays(ptr, n, p(ids), p(prob), p(back), p(b64)), lib=lib)
                aids, delta, kept = np.zeros((ci, n), np.int32), np.zeros(ci, np.float64), np.zeros(ci, np.uint8)
                _lib.check(lib.casr_lm_prune_decisions(ptr, n, p(aids), p(delta), p(kept)), lib=lib)
                for lst, a in zip((self.ids, self.prob, self.backoff, self.backoff_f64, self.all_ids, self.delta, self.kept),
                                  (ids, prob, back, b64, aids, delta, kept.astype(bool))):
                    lst.append(a)
            ms = np.zeros(8, np.float64)
            _lib.check(lib.casr_lm_prune_timing(ptr, p(ms)), lib=lib)
            self.timing_ms = ms
        finally:
            lib.casr_lm_prune_destroy(ptr)

    def sorted(self):
        """Every order in ascending key order (what the host entry gives; the device entry's order is
        unspecified).  Returns self."""
        for n in range(self.order):
            ix = np.lexsort(self.ids[n].T[::-1])
            for lst in (self.ids, self.prob, self.backoff, self.backoff_f64):
                lst[n] = np.ascontiguousarray(lst[n][ix])
            ix = np.lexsort(self.all_ids[n].T[::-1])
            for lst in (self.all_ids, self.delta, self.kept):
                lst[n] = np.ascontiguousarray(lst[n][ix])
        return self


# ---------------------------------------------------------------------------- estimation
class LmEstimate:
    """What casr_lm_estimate_host / casr_lm_estimate returned (include/casr.h has the definition), as
    numpy arrays: per order n, ids[n-1] int32 [count, n], prob and backoff float32 (the stored
    model), raw and adjusted int64 (c_n and a_n), p and gamma float64; ``discounts`` [order, 3],
    ``fallback`` [order] bool, ``n_types`` (|W|), ``positions`` and ``timing_ms`` (the device entry's
    stages: count, extend, stats, prob, compact, copy, -, all)."""

    def __init__(self, lib, ptr, order):
        try:
            count = np.zeros(4, np.int64)
            disc = np.zeros((4, 3), np.float64)
            fb = np.zeros(4, np.int32)
            nt, pos = ctypes.c_int64(), ctypes.c_int64()
            p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
            _lib.check(lib.casr_lm_estimate_info(ptr, p(count), p(disc), p(fb), ctypes.byref(nt), ctypes.byref(pos)),
                       lib=lib)
            self.order = int(order)
            self.discounts, self.fallback = disc[:self.order].copy(), fb[:self.order].astype(bool)
            self.n_types, self.positions = nt.value, pos.value
            self.ids, self.prob, self.backoff, self.raw, self.adjusted, self.p, self.gamma = ([] for _ in range(7))
            for n in range(1, self.order + 1):
                c = int(count[n - 1])
                ids, prob, back = np.zeros((c, n), np.int32), np.zeros(c, np.float32), np.zeros(c, np.float32)
                raw, adj = np.zeros(c, np.int64), np.zeros(c, np.int64)
                pf, gf = np.zeros(c, np.float64), np.zeros(c, np.float64)
                _lib.check(lib.casr_lm_estimate_arrays(ptr, n, p(ids), p(prob), p(back), p(adj), p(pf), p(gf)), lib=lib)
                _lib.check(lib.casr_lm_estimate_counts(ptr, n, p(raw)), lib=lib)
                for lst, a in zip((self.ids, self.prob, self.backoff, self.raw, self.adjusted, self.p, self.gamma),
                                  (ids, prob, back, raw, adj, pf, gf)):
                    lst.append(a)
            ms = np.zeros(8, np.float64)
            _lib.check(lib.casr_lm_estimate_timing(ptr, p(ms)), lib=lib)
            self.timing_ms = ms
        finally:
            lib.casr_lm_estimate_destroy(ptr)

    def sorted(self):
        """Every order in ascending key order (what the host entry gives; the device entry's order is
        unspecified).  Returns self."""
        for n in range(self.order):
            ix = np.lexsort(self.ids[n].T[::-1])
            for lst in (self.ids, self.prob, self.backoff, self.raw, self.adjusted, self.p, self.gamma):
                lst[n] = np.ascontiguousarray(lst[n][ix])
        return self


def flatten(sentences, vocab, word2int=None):
    """(tokens int32 [total], offsets int64 [n + 1]) of a list of id lists, or of strings taken one
    character at a time through ``word2int`` (a character outside the vocabulary is <unk> = vocab + 2,
    as NgramLM.ids_of gives it; spaces are skipped)."""
    V = int(vocab)
    rows = []
    for s in sentences:
        if isinstance(s, str):
            if word2int is None:
                raise ValueError("estimate: string sentences need word2int")
            row = []
            for ch in s:
                if ch.isspace():
                    continue
                t = word2int.get(ch, -1)
                row.append(t if 0 <= t < V else V + 2)
        else:
            row = [int(t) for t in s]
        rows.append(row)
    offsets = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=offsets[1:])
    tokens = np.array([t for r in rows for t in r], np.int32)
    return tokens, offsets


def estimate_host(tokens, offsets, order, vocab):
    """casr_lm_estimate_host on the flat corpus -> LmEstimate (ascending key order).  No GPU."""
    lib = _lib.load()
    tokens = np.ascontiguousarray(tokens, np.int32)
    offsets = np.ascontiguousarray(offsets, np.int64)
    out = ctypes.c_void_p()
    rc = lib.casr_lm_estimate_host(int(order), int(vocab), tokens.ctypes.data_as(ctypes.c_void_p),
                                   offsets.ctypes.data_as(ctypes.c_void_p), len(offsets) - 1, ctypes.byref(out))
    _lib.check(rc, lib=lib)
    return LmEstimate(lib, out, order)


def workspace_bytes(order, positions):
    """casr_lm_estimate_workspace_bytes: the device entry's counting tables for that many positions
    (-1 for what it refuses)."""
    return int(_lib.load().casr_lm_estimate_workspace_bytes(int(order), int(positions)))


def estimate(sentences, order, vocab, word2int=None, engine=None):
    """An interpolated modified-Kneser-Ney NgramLM of the given order (1..4) from ``sentences`` (id
    lists, or strings split per character through ``word2int``): on ``engine``'s device
    (Engine.lm_estimate), or without one through the host entry.  The model carries ``.discounts``
    [order, 3], ``.fallback`` [order] (orders that use (0.5, 1, 1.5)) and ``.estimate`` (the
    LmEstimate); ``.on(engine)``, rescoring and fusion work as for a model read from a file."""
    tokens, offsets = flatten(sentences, vocab, word2int)
    if engine is None:
        est = estimate_host(tokens, offsets, order, vocab)
    else:
        if engine.cfg.vocab != int(vocab):
            raise ValueError(f"estimate: vocab {vocab} is not the engine's {engine.cfg.vocab}")
        est = engine.lm_estimate(tokens, offsets, order).sorted()
    lm = NgramLM.from_ids(est.ids, est.prob, est.backoff, word2int if word2int is not None else {}, vocab)
    lm.discounts, lm.fallback, lm.estimate = est.discounts, est.fallback, est
    return lm
